// Pointwise (1x1x1, stride 1) convolutions = skinny GEMMs over every voxel:
//   forward  Y[M][N] = act(X[M][K] @ W^T + b)      (W: [N][K])
//   dgrad    dX[M][K] = dY[M][N] @ W               (same kernel, W passed as [K][N])
//   wgrad    dW[N][K] += dY^T @ X                  (reduction over M)
// with K, N <= 64 (the segmentation classifier is 32 -> 25, SqueezeNet squeeze /
// expand and the reference's combination projections are 1x1 as well).
//
// These are HBM-bound (two tiny matrices per voxel row), so the design goal is
// streaming: persistent workgroups walk 256-row tiles; a tile of a channels-last
// tensor is ONE contiguous run of 256*K bf16, loaded with 16-byte vectors
// regardless of K (25 is fine) and scattered into a padded LDS layout that the
// MFMA fragments read with aligned ds_read_b128; the next tile's loads are in
// flight while the current one computes.  Weights live in registers as MFMA B
// fragments for the whole kernel.  Output goes back through LDS so the global
// stores are 16-byte vectors too.
//
// Reference parity: Keras Conv2D with kernel (1,1) (model/input.py:294) and the
// combination projection (model/operation.py:179-186).
#include "common.h"

#include <type_traits>

#define PW_BM 256
#define PW_NTHR 256

__device__ __forceinline__ int pw_tiles(long long M) { return (int)((M + PW_BM - 1) / PW_BM); }
__device__ __forceinline__ int pw_rows(long long M, int t) {   // rows of tile t (the last may be ragged)
  return (int)(M - (long long)t * PW_BM < PW_BM ? M - (long long)t * PW_BM : PW_BM);
}

// dynamic LDS bytes: the A tile / output staging region of pw_fwd_kernel and pw_argmax_kernel, and
// the two transposed tiles of pw_wgrad_kernel
constexpr size_t pw_tile_lds(int KP, int NP) { return (size_t)PW_BM * ((KP > NP ? KP : NP) + 8) * 2; }
constexpr size_t pw_wgrad_lds(int KP, int NP) { return (size_t)(KP + NP) * (PW_BM + 8) * 2; }

// ---- The streaming front half, shared by pw_fwd_kernel and pw_argmax_kernel (the tile load by
// pw_wgrad_kernel too): one 256-row tile of X through LDS and the MFMAs to the bf16 output tile
// staged in LDS.  The A tile [256][KP+8] and the output staging [256][NP+8] (bf16) alias one
// dynamic LDS region.

// weights -> B fragments (k rows beyond K and n cols beyond N are zero) and the bias registers
template <int KS, int NT, bool HAS_BIAS>
__device__ __forceinline__ void pw_weights(const bf16* __restrict__ w, const float* __restrict__ bias, int K, int N,
                                           bf16x8 (&fb)[KS][NT], float (&bv)[NT]) {
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = nt * 16 + lr;
      Pack8 p;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = ks * 32 + lg * 8 + j;
        p.e[j] = (n < N && k < K) ? w[(long long)n * K + k] : f2bf(0.f);
      }
      fb[ks][nt] = __builtin_bit_cast(bf16x8, p.u);
    }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = nt * 16 + lr;
    bv[nt] = (HAS_BIAS && n < N) ? bias[n] : 0.f;
  }
}

// tile t of a channels-last [M][C] tensor: 256*C contiguous bf16 (16-B aligned: 512*C*t), CH 16-B
// chunks per thread; the chunks past the end of a ragged tile re-read chunk 0
template <int CH>
__device__ __forceinline__ void pw_load(const bf16* __restrict__ src, long long M, int C, int t, uint4 (&rb)[CH]) {
  const long long e0 = (long long)t * PW_BM * C;
  const long long nel = (M - (long long)t * PW_BM < PW_BM ? M - (long long)t * PW_BM : PW_BM) * C;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = i * PW_NTHR + tid;
    // M % 8 == 0 (host check): every tile is a whole number of 16-B chunks
    rb[i] = *(const uint4*)(src + e0 + (c * 8 < nel ? c * 8 : 0));
  }
}

// flat chunks -> padded rows of As, after zeroing its K padding (the scatter never writes it, the
// output staging does).  PRO >= 0: the input prologue x <- act(x * psv[j] + phv[j]) on the chunk (a
// BatchNorm + activation whose normalised output is never written): with K % 8 == 0 and
// 2048 % K == 0 (host check) every chunk this thread loads starts at channel (8 tid) mod K, so 8
// scale / shift pairs cover all of them; pro(psv, phv) hands them over, from wherever the kernel
// keeps them
template <int KP, int PRO, class ProFn>
__device__ __forceinline__ void pw_scatter(bf16* As, const uint4 (&rb)[KP / 8], int rows, int K, ProFn pro) {
  constexpr int LDA = KP + 8;
  const int tid = threadIdx.x;
  for (int i = tid; i < PW_BM * (LDA - K); i += PW_NTHR) As[(i / (LDA - K)) * LDA + K + i % (LDA - K)] = f2bf(0.f);
#pragma unroll
  for (int i = 0; i < KP / 8; ++i) {
    const int c = i * PW_NTHR + tid;
    if (c * 8 < rows * K) {
      int r = (c * 8) / K, k = c * 8 - r * K;     // one division per chunk, then walk
      if (K % 8 == 0) {                            // chunk inside one row: one 16-B LDS store
        if constexpr (PRO >= 0) {
          Pack8 p;
          p.u = rb[i];
          float psv[8], phv[8];
          pro(psv, phv);
#pragma unroll
          for (int j = 0; j < 8; ++j) p.e[j] = f2bf(act_fwd(bf2f(p.e[j]) * psv[j] + phv[j], PRO));
          *(uint4*)(As + r * LDA + k) = p.u;
        } else {
          *(uint4*)(As + r * LDA + k) = rb[i];
        }
      } else {
        Pack8 p;
        p.u = rb[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          As[r * LDA + k] = p.e[j];
          if (++k == K) { k = 0; ++r; }
        }
      }
    }
  }
}

// Os <- bf16(act(As W^T + bv)), Os aliasing As: each wave its 64 rows, the k-steps in order, a
// barrier between the last MFMA read of As and the first staging store and one after the staging
template <int KP, int NP, int ACT>
__device__ __forceinline__ void pw_mfma_stage(bf16* As, const bf16x8 (&fb)[KP / 32][NP / 16],
                                              const float (&bv)[NP / 16]) {
  constexpr int LDA = KP + 8, LDO = NP + 8, KS = KP / 32, NT = NP / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  bf16* Os = As;
  const bf16* arow = As + (wave * 64 + lr) * LDA + lg * 8;   // this lane's A-fragment row of m-tile 0
  f32x4 acc[4][NT];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const bf16x8 fa = *(const bf16x8*)(arow + mt * 16 * LDA + ks * 32);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[ks][nt], acc[mt][nt], 0, 0, 0);
    }
  __syncthreads();                               // all MFMA reads of As done before Os overwrites it
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Os[(wave * 64 + mt * 16 + lg * 4 + r) * LDO + nt * 16 + lr] = f2bf(act_fwd(acc[mt][nt][r] + bv[nt], ACT));
  __syncthreads();
}

// Y = act(X W^T + b).  KP / NP: K, N padded to 32 / 64.  Dynamic LDS: the A tile
// [256][KP+8] and the output staging [256][NP+8] share one region (bf16).
// PRO: -1 = plain input; ACT_NONE / ACT_RELU = input prologue x <- act(x * psc[k] + psh[k])
// BWS: ACT_NONE / ACT_RELU = the output is the gradient dz of a BN+act layer whose pre-BN input
//   sy [M][N] (scale ssc, shift ssh) is read alongside: each workgroup also sums that BN's raw
//   backward moments (sum g, sum g*y), g = dz * act'(y*ssc+ssh), into spart[block][2][N]
//   (bn_finalize MODE 2) -- the colstats pass over dz and y disappears (N % 8 == 0, 2048 % N == 0)
// XENT: the layer is a classifier head whose logits feed softmax + categorical cross-entropy against
//   int64 labels[M] (the per-voxel segmentation loss): every thread takes one row of the staged
//   logit tile, computes its log-sum-exp loss, top-1 hit and d(logits) = (softmax - target) * xscale
//   (label smoothing as softmax_xent_tile_kernel), and the tile's d(logits) -- not the logits --
//   are stored; per-workgroup (loss sum, hits) go to xpart[block][2].  The logits never reach HBM
//   and the separate loss kernel (one read of the logits + one write of d(logits)) disappears.
template <int KP, int NP, int ACT, bool HAS_BIAS, int PRO = -1, int BWS = -1, bool XENT = false>
__global__ __launch_bounds__(PW_NTHR, 2) void pw_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                           const float* __restrict__ bias, bf16* __restrict__ y,
                                                           long long M, int K, int N, const float* __restrict__ psc,
                                                           const float* __restrict__ psh,
                                                           const bf16* __restrict__ sy = nullptr,
                                                           const float* __restrict__ ssc = nullptr,
                                                           const float* __restrict__ ssh = nullptr,
                                                           float* __restrict__ spart = nullptr,
                                                           const long long* __restrict__ labels = nullptr,
                                                           float* __restrict__ xpart = nullptr, float xscale = 0.f,
                                                           float smoothing = 0.f) {
  constexpr int LDO = NP + 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char pw_dsm[];
  bf16* As = reinterpret_cast<bf16*>(pw_dsm);
  bf16* Os = As;                                 // aliased: staged only after the MFMAs have read As
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  bf16x8 fb[KP / 32][NP / 16];                   // weights live in registers for the whole kernel
  float bv[NP / 16];
  pw_weights<KP / 32, NP / 16, HAS_BIAS>(w, bias, K, N, fb, bv);
  // the input prologue's 8 scale / shift pairs of this thread (see pw_scatter), in registers
  constexpr int NPV = PRO >= 0 ? 8 : 1;
  float psv[NPV], phv[NPV];
  if constexpr (PRO >= 0) {
    const int pk0 = (tid * 8) % K;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      psv[j] = psc[pk0 + j];
      phv[j] = psh[pk0 + j];
    }
  }
  constexpr int NSV = BWS >= 0 ? 8 : 1;
  float ssv[NSV], shv[NSV], sg[NSV], sgy[NSV];
  if constexpr (BWS >= 0) {                      // this thread's output chunks start at channel 8 tid mod N
    const int sn0 = (tid * 8) % N;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ssv[j] = ssc[sn0 + j];
      shv[j] = ssh[sn0 + j];
      sg[j] = sgy[j] = 0.f;
    }
  }
  const int ntiles = pw_tiles(M);
  float xl = 0.f, xc = 0.f;                      // XENT: this thread's loss / top-1 hit sums
  auto pro = [&](float (&s)[8], float (&h)[8]) {
#pragma unroll
    for (int j = 0; j < NPV; ++j) { s[j] = psv[j]; h[j] = phv[j]; }
  };
  uint4 rb[KP / 8];
  int t = blockIdx.x;
  if (t < ntiles) pw_load(x, M, K, t, rb);
  for (; t < ntiles; t += gridDim.x) {
    const int rows = pw_rows(M, t);
    __syncthreads();                             // previous tile's Os readers are done
    pw_scatter<KP, PRO>(As, rb, rows, K, pro);
    __syncthreads();
    if (t + gridDim.x < ntiles) pw_load(x, M, K, t + gridDim.x, rb);   // next tile in flight during the MFMAs
    pw_mfma_stage<KP, NP, ACT>(As, fb, bv);
    if constexpr (XENT) {
      // one row per thread, from the stored bf16 logits (the values the unfused loss would read)
      if (tid < rows) {
        bf16* orow = Os + tid * LDO;
        const long long yl = labels[(long long)t * PW_BM + tid];
        const float off = smoothing / (float)N, on = 1.f - smoothing + off;
        float v[NP];
        float mx = -INFINITY;
        int am = 0;
#pragma unroll
        for (int c = 0; c < NP; ++c) {
          v[c] = c < N ? bf2f(orow[c]) : -INFINITY;
          if (v[c] > mx) { mx = v[c]; am = c; }
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < NP; ++c) se += c < N ? __expf(v[c] - mx) : 0.f;
        const float lse = mx + __logf(se);
        float lrow = 0.f;
#pragma unroll
        for (int c = 0; c < NP; ++c) {
          if (c < N) {
            const float lp = v[c] - lse;
            const float tgt = (c == yl) ? on : off;
            lrow -= tgt * lp;
            orow[c] = f2bf((__expf(lp) - tgt) * xscale);   // own row only: no race
          }
        }
        xl += lrow;
        xc += (am == yl) ? 1.f : 0.f;
      }
      __syncthreads();
    }
    // gather padded rows -> flat 256*N run, 16-B stores
    const long long o0 = (long long)t * PW_BM * N;
    const int nel = rows * N;
    for (int c = tid; c * 8 < nel; c += PW_NTHR) {
      Pack8 p;
      int r = (c * 8) / N, n = c * 8 - r * N;
      if (N % 8 == 0) {
        p.u = *(const uint4*)(Os + r * LDO + n);
        if constexpr (BWS >= 0) {
          Pack8 q;
          q.u = *(const uint4*)(sy + o0 + c * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float yv = bf2f(q.e[j]);
            const float gv = bf2f(p.e[j]) * act_bwd_from_out(act_fwd(yv * ssv[j] + shv[j], BWS), BWS);
            sg[j] += gv;
            sgy[j] += gv * yv;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          p.e[j] = Os[r * LDO + n];
          if (++n == N) { n = 0; ++r; }
        }
      }
      *(uint4*)(y + o0 + c * 8) = p.u;           // rows * N is a multiple of 8 (M % 8 == 0)
    }
  }
  if constexpr (XENT) {
    // (loss sum, hits) of the workgroup, fixed order: waves, then the 4 wave sums
    xl = wave_sum(xl);
    xc = wave_sum(xc);
    __syncthreads();
    float* red = reinterpret_cast<float*>(pw_dsm);
    if (lane == 0) {
      red[wave] = xl;
      red[4 + wave] = xc;
    }
    __syncthreads();
    if (tid == 0) {
      xpart[2 * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
      xpart[2 * blockIdx.x + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
  }
  if constexpr (BWS >= 0) {
    // block reduction of the BN-backward moments (fixed order): thread t holds channels
    // (8t mod N) .. +7; the dynamic LDS (>= 256 x 40 bf16) is free after the last tile
    __syncthreads();
    float* red = reinterpret_cast<float*>(pw_dsm);   // [256][16]
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[tid * 16 + j] = sg[j];
      red[tid * 16 + 8 + j] = sgy[j];
    }
    __syncthreads();
    const int cpr = N / 8;
    for (int c = tid; c < N; c += PW_NTHR) {
      float a = 0.f, b2 = 0.f;
      for (int t2 = c / 8; t2 < PW_NTHR; t2 += cpr) {
        a += red[t2 * 16 + (c & 7)];
        b2 += red[t2 * 16 + 8 + (c & 7)];
      }
      spart[(long long)blockIdx.x * 2 * N + c] = a;
      spart[(long long)blockIdx.x * 2 * N + N + c] = b2;
    }
  }
}

// Classifier head for inference: labels[row] = argmax_n (X W^T + b)[row][n] (+ optionally the top-1
// softmax probability), the per-voxel output of the segmentation model.  The kernel shares its
// front half with pw_fwd_kernel: the same pw_weights / pw_load / pw_scatter / pw_mfma_stage calls in
// the same persistent tile loop produce the bf16 logit tile staged in LDS, so the tile is what
// pw_fwd_kernel<.., ACT_NONE, ..> stores and the labels are the arg-max of pw_fwd's logits by
// construction (only where the prologue's scale / shift pairs are kept differs, see below).  Then
// every thread takes one row: a strict `>` scan from class 0 (the lowest index wins ties) and,
// when asked, 1 / sum exp(v - max) in fp32 over the bf16 logits.  The logits never reach HBM: a
// tile writes 256 label bytes (+ 512 confidence bytes) instead of 256 * N * 2.  NP: N padded to
// 16 / 32 / 64.
//
// CM (the scorer): the row's arg-max is not (only) stored but counted against truth[row] in a
// per-workgroup confusion histogram hist[N*N + 1] (uint32, in the dynamic LDS behind the tile):
// hist[t * N + am] for t < N, the out-of-range slot hist[N*N] for t >= N, nothing for t == ignore.
// Integer LDS adds only; after its last tile the workgroup stores the whole histogram to its row of
// `part` (every launched workgroup writes every slot: no memset, replayable), summed over the
// workgroups by cm_accumulate_kernel.  `labels` may be null (nothing written per row); no conf.
template <int KP, int NP, bool HAS_BIAS, int PRO = -1, bool CM = false>
__global__ __launch_bounds__(PW_NTHR, (KP <= 32 && NP <= 32) ? 4 : 2) void pw_argmax_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ w, const float* __restrict__ bias,
    uint8_t* __restrict__ labels, bf16* __restrict__ conf, long long M, int K, int N,
    const float* __restrict__ psc, const float* __restrict__ psh, const uint8_t* __restrict__ truth = nullptr,
    uint32_t* __restrict__ part = nullptr, int ignore = -1) {
  constexpr int LDO = NP + 8;
  constexpr int UR = NP >= 64 ? 2 : NP / 8;      // row scan: 16-B logit chunks in flight (VGPR budget)
  extern __shared__ __attribute__((aligned(16))) unsigned char pw_dsm[];
  bf16* As = reinterpret_cast<bf16*>(pw_dsm);
  bf16* Os = As;                                 // aliased: staged only after the MFMAs have read As
  const int tid = threadIdx.x;

  bf16x8 fb[KP / 32][NP / 16];
  float bv[NP / 16];
  pw_weights<KP / 32, NP / 16, HAS_BIAS>(w, bias, K, N, fb, bv);
  // the input prologue's 8 scale / shift pairs of this thread (see pw_scatter) stay in LDS and are
  // read per chunk -- unlike pw_fwd_kernel's, 16 fewer registers live across the MFMAs and the row scan
  __shared__ __attribute__((aligned(16))) float pss[PRO >= 0 ? 2 * KP : 4];
  const int pk0 = PRO >= 0 ? (tid * 8) % K : 0;
  if constexpr (PRO >= 0) {
    if (tid < K) {
      pss[tid] = psc[tid];
      pss[KP + tid] = psh[tid];
    }
  }
  auto pro = [&](float (&s)[8], float (&h)[8]) {
    const float4 s0 = *(const float4*)(pss + pk0), s1 = *(const float4*)(pss + pk0 + 4);
    const float4 h0 = *(const float4*)(pss + KP + pk0), h1 = *(const float4*)(pss + KP + pk0 + 4);
    s[0] = s0.x, s[1] = s0.y, s[2] = s0.z, s[3] = s0.w, s[4] = s1.x, s[5] = s1.y, s[6] = s1.z, s[7] = s1.w;
    h[0] = h0.x, h[1] = h0.y, h[2] = h0.z, h[3] = h0.w, h[4] = h1.x, h[5] = h1.y, h[6] = h1.z, h[7] = h1.w;
  };
  // CM: the workgroup's histogram, zeroed once (the tile loop's barriers order it before the adds)
  uint32_t* hist = reinterpret_cast<uint32_t*>(pw_dsm + pw_tile_lds(KP, NP));
  if constexpr (CM)
    for (int i = tid; i <= N * N; i += PW_NTHR) hist[i] = 0u;
  const int ntiles = pw_tiles(M);
  uint4 rb[KP / 8];
  int t = blockIdx.x;
  if (t < ntiles) pw_load(x, M, K, t, rb);
  for (; t < ntiles; t += gridDim.x) {
    const int rows = pw_rows(M, t);
    __syncthreads();                             // previous tile's Os readers are done
    pw_scatter<KP, PRO>(As, rb, rows, K, pro);
    __syncthreads();
    if (t + gridDim.x < ntiles) pw_load(x, M, K, t + gridDim.x, rb);   // next tile in flight during the MFMAs
    pw_mfma_stage<KP, NP, ACT_NONE>(As, fb, bv);
    // one row per thread, 16-B LDS reads of the staged bf16 logits: a running scan, no per-class
    // array (columns N .. NP are padding and never compete)
    if (tid < rows) {
      const bf16* orow = Os + tid * LDO;
      float mx = -INFINITY;
      int am = 0;
#pragma unroll UR
      for (int c8 = 0; c8 < NP / 8; ++c8) {
        Pack8 p;
        p.u = *(const uint4*)(orow + c8 * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = bf2f(p.e[j]);
          if (c8 * 8 + j < N && v > mx) { mx = v; am = c8 * 8 + j; }
        }
      }
      const long long row = (long long)t * PW_BM + tid;
      if (!CM || labels) labels[row] = (uint8_t)am;   // 64 consecutive bytes per wave
      if constexpr (CM) {
        // one integer LDS add per row.  Combining equal keys across the wave first (ballot + one add
        // of the popcount) measured the same on an all-one-bin input and 1.1-2x slower on mixed ones
        // (profiles/segment_score.md), so the plain add stays.
        const int tr = truth[row];
        if (tr != ignore) atomicAdd(&hist[tr >= N ? N * N : tr * N + am], 1u);
      }
      if (conf) {                                // (null in the CM instances)
        float se = 0.f;
#pragma unroll UR
        for (int c8 = 0; c8 < NP / 8; ++c8) {
          Pack8 p;
          p.u = *(const uint4*)(orow + c8 * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) se += c8 * 8 + j < N ? __expf(bf2f(p.e[j]) - mx) : 0.f;
        }
        conf[row] = f2bf(1.f / se);
      }
    }
  }
  if constexpr (CM) {
    __syncthreads();
    uint32_t* prow = part + (size_t)blockIdx.x * (size_t)(N * N + 1);
    for (int i = tid; i <= N * N; i += PW_NTHR) prow[i] = hist[i];
  }
}

// acc[i] += sum_b part[b][i] (b in order), i < len: the per-workgroup confusion histograms of one
// pw_argmax_kernel<.., CM> launch into the caller's int64 running matrix.  One thread per slot.
__global__ __launch_bounds__(256) void cm_accumulate_kernel(const uint32_t* __restrict__ part,
                                                            long long* __restrict__ acc, int len, int nb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= len) return;
  long long s = 0;
  int b = 0;
  for (; b + 32 <= nb; b += 32) {               // 32 independent loads in flight, added in order
    uint32_t v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = part[(size_t)(b + j) * len + i];
#pragma unroll
    for (int j = 0; j < 32; ++j) s += v[j];
  }
  for (; b < nb; ++b) s += part[(size_t)b * len + i];
  acc[i] += s;
}

// dW[N][K] += sum_rows dY[row][n] * X[row][k].  Both tiles are scattered into LDS
// TRANSPOSED ([channel][row]) so the MFMA operands (k = rows) are contiguous
// 8-row runs; per-wave fp32 accumulators over a static (strided) tile set, added across the
// waves in a fixed order and stored into the workgroup's partial row of `dw` ([gridDim.x][N][K]),
// summed by fn_part_reduce in a fixed order (bitwise repeatable).
template <int KP, int NP, int PRO = -1>
__global__ __launch_bounds__(PW_NTHR, 2) void pw_wgrad_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                                                             float* __restrict__ dw, long long M, int K, int N,
                                                             const float* __restrict__ psc,
                                                             const float* __restrict__ psh) {
  constexpr int LDR = PW_BM + 8;                 // row stride of the transposed tiles
  constexpr int NTN = NP / 16, NTK = KP / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char pw_dsm[];
  bf16* Yt = reinterpret_cast<bf16*>(pw_dsm);    // [NP][LDR]
  bf16* Xt = Yt + NP * LDR;                      // [KP][LDR]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  // padded channels (n >= N, k >= K) stay zero
  for (int i = tid; i < NP * LDR; i += PW_NTHR) Yt[i] = f2bf(0.f);
  for (int i = tid; i < KP * LDR; i += PW_NTHR) Xt[i] = f2bf(0.f);

  // each wave owns a 64-row quarter of the tile's k dimension (2 k-steps of 32 rows)
  f32x4 acc[NTN][NTK];
#pragma unroll
  for (int a = 0; a < NTN; ++a)
#pragma unroll
    for (int b = 0; b < NTK; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int ntiles = pw_tiles(M);
  constexpr int CY = NP / 8, CX = KP / 8;        // 16-B chunks per thread of the dy / x tiles
  uint4 ry[CY], rx[CX];
  // optional prologue on x (as pw_fwd_kernel): x <- act(x * psc[k] + psh[k])
  auto scatter_t = [&](bf16* dst, const uint4* rb, int C, int rows, int nch) {
#pragma unroll
    for (int i = 0; i < nch; ++i) {
      const int c = i * PW_NTHR + tid;
      if (c * 8 < rows * C) {
        Pack8 p;
        p.u = rb[i];
        int r = (c * 8) / C, k = c * 8 - r * C;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          dst[k * LDR + r] = p.e[j];
          if (++k == C) { k = 0; ++r; }
        }
      }
    }
  };
  int t = blockIdx.x;
  if (t < ntiles) { pw_load(dy, M, N, t, ry); pw_load(x, M, K, t, rx); }
  for (; t < ntiles; t += gridDim.x) {
    const int rows = pw_rows(M, t);
    __syncthreads();
    scatter_t(Yt, ry, N, rows, CY);
    scatter_t(Xt, rx, K, rows, CX);
    if (rows < PW_BM) {                          // ragged last tile: zero the unused rows
      for (int i = tid; i < NP * (PW_BM - rows); i += PW_NTHR) Yt[(i / (PW_BM - rows)) * LDR + rows + i % (PW_BM - rows)] = f2bf(0.f);
    }
    __syncthreads();
    if constexpr (PRO >= 0) {
      // input prologue x <- act(x * psc[k] + psh[k]) on the transposed tile in LDS: channel k is
      // one LDS row, so a thread takes 32 consecutive rows of one channel with two scalars
      // (no per-element parameter registers; rows past a ragged tile's end meet dy = 0)
      for (int k = tid >> 3; k < K; k += PW_NTHR / 8) {
        const float a = psc[k], c = psh[k];
        bf16* row = Xt + k * LDR + (tid & 7) * 32;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          Pack8 p;
          p.u = *(const uint4*)(row + v * 8);
#pragma unroll
          for (int j = 0; j < 8; ++j) p.e[j] = f2bf(act_fwd(bf2f(p.e[j]) * a + c, PRO));
          *(uint4*)(row + v * 8) = p.u;
        }
      }
      __syncthreads();
    }
    if (t + gridDim.x < ntiles) { pw_load(dy, M, N, t + gridDim.x, ry); pw_load(x, M, K, t + gridDim.x, rx); }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int r0 = wave * 64 + kk * 32 + lg * 8;
      bf16x8 fa[NTN], fb[NTK];
#pragma unroll
      for (int a = 0; a < NTN; ++a) fa[a] = *(const bf16x8*)(Yt + (a * 16 + lr) * LDR + r0);
#pragma unroll
      for (int b = 0; b < NTK; ++b) fb[b] = *(const bf16x8*)(Xt + (b * 16 + lr) * LDR + r0);
#pragma unroll
      for (int a = 0; a < NTN; ++a)
#pragma unroll
        for (int b = 0; b < NTK; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
  }
  // D[row = n][col = k]: lane holds n = a*16 + lg*4 + r, k = b*16 + lr.  Every wave holds a partial
  // of the WHOLE [N][K] block (its quarter of the rows): the four are added through LDS in wave
  // order (4 x NP x KP fp32 fit in the tiles' LDS), then stored as the workgroup's partial row
  __syncthreads();
  float* red = reinterpret_cast<float*>(pw_dsm);
#pragma unroll
  for (int a = 0; a < NTN; ++a)
#pragma unroll
    for (int b = 0; b < NTK; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wave * NP + a * 16 + lg * 4 + r) * KP + b * 16 + lr] = acc[a][b][r];
  __syncthreads();
  for (int i = tid; i < NP * KP; i += PW_NTHR) {
    const int n = i / KP, k = i % KP;
    if (n < N && k < K)
      dw[((long long)blockIdx.x * N + n) * K + k] =
          ((red[i] + red[NP * KP + i]) + red[2 * NP * KP + i]) + red[3 * NP * KP + i];
  }
}

static int g_pw_cus = 0;
static int pw_grid(long long M, int per_cu) {
  if (g_pw_cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&g_pw_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || g_pw_cus <= 0)
      g_pw_cus = 256;
  }
  const int tiles = (int)((M + PW_BM - 1) / PW_BM);
  const int g = g_pw_cus * per_cu;
  return tiles < g ? (tiles > 0 ? tiles : 1) : g;
}

// x: bf16 [M][K], w: bf16 [N][K] (row n = output channel), y: bf16 [M][N]; K, N <= 64
// psc / psh (optional, fp32 [K]): input prologue x <- pact(x * psc + psh); needs K % 8 == 0 and
// 2048 % K == 0
static bool pw_pro_ok(const float* psc, const float* psh, int K) {
  return !psc || (psh && K % 8 == 0 && 2048 % K == 0);
}

// The runtime (K, N, bias or not, prologue or not and its activation) as the compile-time tags
// (KP, NP, HAS_BIAS, PRO) of a kernel instance: f(KP, NP, HB, PRO) gets std::integral_constants and
// returns the entry point's status.  NP16: N <= 16 selects NP = 16 (the arg-max instances), else 32.
template <int V>
using pw_int = std::integral_constant<int, V>;

template <bool NP16 = false, class F>
static int pw_dispatch(int K, int N, bool hb, bool pro, int pact, F f) {
  auto with_pro = [&](auto KP, auto NP, auto HB) {
    if (!pro) return f(KP, NP, HB, pw_int<-1>{});
    if (pact == ACT_RELU) return f(KP, NP, HB, pw_int<ACT_RELU>{});
    return f(KP, NP, HB, pw_int<ACT_NONE>{});
  };
  auto with_hb = [&](auto KP, auto NP) {
    return hb ? with_pro(KP, NP, std::true_type{}) : with_pro(KP, NP, std::false_type{});
  };
  auto with_np = [&](auto KP) {
    if constexpr (NP16) {
      if (N <= 16) return with_hb(KP, pw_int<16>{});
    }
    return N <= 32 ? with_hb(KP, pw_int<32>{}) : with_hb(KP, pw_int<64>{});
  };
  return K <= 32 ? with_np(pw_int<32>{}) : with_np(pw_int<64>{});
}

// grid of the BWS (dgrad + BN-backward moments) launch = rows of its spart slab: 3 workgroups per
// CU (165 VGPRs: occupancy 3, so a 4-per-CU persistent grid would leave a serial tail)
extern "C" int fn_pw_fwd_blocks(long long M, int K, int N) {
  (void)K; (void)N;
  return pw_grid(M, 3);
}

extern "C" int fn_pw_fwd(const void* x, const void* w, const float* bias, void* y, long long M, int K, int N, int act,
                         hipStream_t st, const float* psc, const float* psh, int pact, const void* sy,
                         const float* ssc, const float* ssh, float* spart, int sact) {
  if (K < 1 || K > 64 || N < 1 || N > 64 || M < 8 || M % 8) return -2;
  if (!pw_pro_ok(psc, psh, K)) return -2;
  if (sy) {                                      // dgrad + BN-backward moments (see BWS): 32 x 32 only
    if (psc || bias || act != ACT_NONE || !ssc || !ssh || !spart || N % 8 || 2048 % N ||
        (sact != ACT_NONE && sact != ACT_RELU) || K > 32 || N > 32)
      return -2;
    auto bws = [&](auto SA) {
      hipLaunchKernelGGL((pw_fwd_kernel<32, 32, ACT_NONE, false, -1, decltype(SA)::value>),
                         dim3((unsigned)fn_pw_fwd_blocks(M, K, N)), dim3(PW_NTHR), pw_tile_lds(32, 32), st,
                         (const bf16*)x, (const bf16*)w, nullptr, (bf16*)y, M, K, N, nullptr, nullptr, (const bf16*)sy,
                         ssc, ssh, spart);
    };
    if (sact == ACT_RELU) bws(pw_int<ACT_RELU>{}); else bws(pw_int<ACT_NONE>{});
    FN_CHECK_LAUNCH();
    return 0;
  }
  if (psc) {
    if (act != ACT_NONE || (pact != ACT_NONE && pact != ACT_RELU)) return -2;
  } else if ((act == ACT_TANH || act == ACT_SIGMOID) && !bias) {
    return -5;
  }
  // ~110-200 VGPRs and <= 37 KB LDS: 4 workgroups per CU for the 32-channel variants
  const dim3 grid((unsigned)pw_grid(M, (K <= 32 && N <= 32) ? 4 : 2));
  // instances: the prologue (the BN + act of the producing layer) has the identity output only;
  // tanh and sigmoid exist with a bias only
  const int rc = pw_dispatch(K, N, bias != nullptr, psc != nullptr, pact, [&](auto KP, auto NP, auto HB, auto PRO) {
    constexpr int kp = decltype(KP)::value, np = decltype(NP)::value, pro = decltype(PRO)::value;
    constexpr bool hb = decltype(HB)::value;
    auto go = [&](auto ACT) {
      constexpr size_t lds = pw_tile_lds(kp, np);
      if (lds > 64 * 1024 &&
          hipFuncSetAttribute((const void*)pw_fwd_kernel<kp, np, decltype(ACT)::value, hb, pro>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -4;
      hipLaunchKernelGGL((pw_fwd_kernel<kp, np, decltype(ACT)::value, hb, pro>), grid, dim3(PW_NTHR), lds, st,
                         (const bf16*)x, (const bf16*)w, bias, (bf16*)y, M, K, N, psc, psh);
      return 0;
    };
    if constexpr (pro >= 0) return go(pw_int<ACT_NONE>{});
    else if (act == ACT_RELU) return go(pw_int<ACT_RELU>{});
    else if (act == ACT_NONE) return go(pw_int<ACT_NONE>{});
    else if constexpr (hb) return act == ACT_TANH ? go(pw_int<ACT_TANH>{}) : go(pw_int<ACT_SIGMOID>{});
    else return -5;
  });
  if (rc) return rc;
  FN_CHECK_LAUNCH();
  return 0;
}

// Classifier head + softmax cross-entropy (XENT instances): dlog [M][N] bf16 = d(mean loss)/d(logits)
// with xscale = 1/M folded in (the unscaled loss is sum(xpart[:, 0]) * xscale ... / M), labels
// int64 [M] (no ignore index), xpart fp32 [fn_pw_xent_blocks(M)][2] = per-workgroup (loss sum, top-1
// hits).  K, N <= 32, identity activation; psc / psh: the optional BN + act input prologue.
extern "C" int fn_pw_xent_blocks(long long M) { return pw_grid(M, 3); }   // (143-159 VGPRs: 3 per CU)

extern "C" int fn_pw_fwd_xent(const void* x, const void* w, const float* bias, void* dlog, long long M, int K, int N,
                              const float* psc, const float* psh, int pact, const long long* labels, float* xpart,
                              float xscale, float smoothing, hipStream_t st) {
  if (K < 1 || K > 32 || N < 2 || N > 32 || M < 8 || M % 8 || !labels || !xpart) return -2;
  if (!pw_pro_ok(psc, psh, K) || (psc && pact != ACT_NONE && pact != ACT_RELU)) return -2;
  const dim3 grid((unsigned)fn_pw_xent_blocks(M));
  pw_dispatch(K, N, bias != nullptr, psc != nullptr, pact, [&](auto KP, auto NP, auto HB, auto PRO) {
    if constexpr (decltype(KP)::value == 32 && decltype(NP)::value == 32)   // (K, N <= 32 above)
      hipLaunchKernelGGL((pw_fwd_kernel<32, 32, ACT_NONE, decltype(HB)::value, decltype(PRO)::value, -1, true>), grid,
                         dim3(PW_NTHR), pw_tile_lds(32, 32), st, (const bf16*)x, (const bf16*)w, bias, (bf16*)dlog, M, K,
                         N, psc, psh, nullptr, nullptr, nullptr, nullptr, labels, xpart, xscale, smoothing);
    return 0;
  });
  FN_CHECK_LAUNCH();
  return 0;
}

// rows of the partial slab fn_pw_wgrad needs ([rows][N][K] fp32)
extern "C" int fn_pw_wgrad_blocks(long long M, int K, int N) { return pw_grid(M, (K <= 32 && N <= 32) ? 3 : 2); }

// dw: fp32 [N][K], accumulated into (zero it for a fresh gradient); part: fp32 scratch
// [fn_pw_wgrad_blocks][N][K]
extern "C" int fn_pw_wgrad(const void* dy, const void* x, float* dw, long long M, int K, int N, hipStream_t st,
                           const float* psc, const float* psh, int pact, float* part) {
  if (K < 1 || K > 64 || N < 1 || N > 64 || M < 8 || M % 8) return -2;
  if (!pw_pro_ok(psc, psh, K)) return -2;
  if (!part) return -6;
  if (psc && pact != ACT_NONE && pact != ACT_RELU) return -2;
  const dim3 grid((unsigned)fn_pw_wgrad_blocks(M, K, N));
  const int rc = pw_dispatch(K, N, false, psc != nullptr, pact, [&](auto KP, auto NP, auto, auto PRO) {
    constexpr int kp = decltype(KP)::value, np = decltype(NP)::value;
    constexpr size_t lds = pw_wgrad_lds(kp, np);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)pw_wgrad_kernel<kp, np>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
      return -4;
    hipLaunchKernelGGL((pw_wgrad_kernel<kp, np, decltype(PRO)::value>), grid, dim3(PW_NTHR), lds, st, (const bf16*)dy,
                       (const bf16*)x, part, M, K, N, psc, psh);
    return 0;
  });
  if (rc) return rc;
  FN_CHECK_LAUNCH();
  return fn_part_reduce(part, dw, (long long)N * K, (int)grid.x, 1, st);
}

// Classifier head -> labels (pw_argmax_kernel): x bf16 [M][K], w bf16 [N][K], labels uint8 [M], conf
// bf16 [M] or null (the softmax pass is skipped); K, N <= 64; psc / psh / pact: the optional BN + act
// input prologue, as fn_pw_fwd.  Grid: the 32-channel instances stay under 128 VGPRs (4 workgroups
// per CU), the 64-wide ones take 2 -- as fn_pw_fwd.
extern "C" int fn_pw_argmax_blocks(long long M, int K, int N) {
  return pw_grid(M, (K <= 32 && N <= 32) ? 4 : 2);
}

extern "C" int fn_pw_argmax(const void* x, const void* w, const float* bias, void* labels, void* conf, long long M,
                            int K, int N, const float* psc, const float* psh, int pact, hipStream_t st) {
  if (K < 1 || K > 64 || N < 1 || N > 64 || M < 8 || M % 8 || !labels) return -2;
  if (!pw_pro_ok(psc, psh, K) || (psc && pact != ACT_NONE && pact != ACT_RELU)) return -2;
  const dim3 grid((unsigned)fn_pw_argmax_blocks(M, K, N));
  pw_dispatch<true>(K, N, bias != nullptr, psc != nullptr, pact, [&](auto KP, auto NP, auto HB, auto PRO) {
    constexpr int kp = decltype(KP)::value, np = decltype(NP)::value;
    hipLaunchKernelGGL((pw_argmax_kernel<kp, np, decltype(HB)::value, decltype(PRO)::value>), grid, dim3(PW_NTHR),
                       pw_tile_lds(kp, np), st, (const bf16*)x, (const bf16*)w, bias, (uint8_t*)labels, (bf16*)conf, M,
                       K, N, psc, psh);
    return 0;
  });
  FN_CHECK_LAUNCH();
  return 0;
}

// Classifier head -> confusion matrix (pw_argmax_kernel<.., CM> + cm_accumulate_kernel): operands as
// fn_pw_argmax, plus truth uint8 [M]; rows whose truth == ignore (-1: none) are skipped.  labels
// uint8 [M] or null (nothing is written per row).  part: uint32 scratch [fn_pw_argmax_cm_blocks]
// [N*N + 1], fully rewritten by every launch; acc: int64 [N*N + 1], ADDED to (rows = truth, columns =
// prediction, slot N*N = rows whose truth is >= N).  M < 2^32: a workgroup's uint32 counters cannot wrap.
extern "C" int fn_pw_argmax_cm_blocks(long long M, int K, int N) { return fn_pw_argmax_blocks(M, K, N); }

extern "C" int fn_pw_argmax_cm(const void* x, const void* w, const float* bias, const void* truth, void* labels,
                               void* part, void* acc, long long M, int K, int N, int ignore, const float* psc,
                               const float* psh, int pact, hipStream_t st) {
  if (K < 1 || K > 64 || N < 1 || N > 64 || M < 8 || M % 8 || M >= (1LL << 32)) return -2;
  if (!truth || !part || !acc || ignore < -1 || ignore > 255) return -2;
  if (!pw_pro_ok(psc, psh, K) || (psc && pact != ACT_NONE && pact != ACT_RELU)) return -2;
  const int nb = fn_pw_argmax_cm_blocks(M, K, N), len = N * N + 1;
  const dim3 grid((unsigned)nb);
  pw_dispatch<true>(K, N, bias != nullptr, psc != nullptr, pact, [&](auto KP, auto NP, auto HB, auto PRO) {
    constexpr int kp = decltype(KP)::value, np = decltype(NP)::value;
    hipLaunchKernelGGL((pw_argmax_kernel<kp, np, decltype(HB)::value, decltype(PRO)::value, true>), grid,
                       dim3(PW_NTHR), pw_tile_lds(kp, np) + (size_t)len * 4, st, (const bf16*)x, (const bf16*)w, bias,
                       (uint8_t*)labels, (bf16*)nullptr, M, K, N, psc, psh, (const uint8_t*)truth, (uint32_t*)part,
                       ignore);
    return 0;
  });
  FN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cm_accumulate_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st,
                     (const uint32_t*)part, (long long*)acc, len, nb);
  FN_CHECK_LAUNCH();
  return 0;
}
