// Walls between feature instances: for every voxel the nearest and the nearest other label of an id
// volume with their exact squared Euclidean distances (a labelled distance transform), and per
// instance the smallest distance to another instance, where it is attained, and the voxels that have
// another instance within a limit (the step beside edt.hip).
//
// ids int32 [N][D][H][W], indexed [n][z][y][x]: a voxel is a seed of label ids when ids > 0.  A key is
// d2 << 32 | label; NN_NONE = NN_INF << 32 | 0 is "no such label".  Per voxel a pair of keys: rank 0,
// the smallest key over the labels of the sample, and rank 1, the smallest key over the other labels.
// D, H, W <= NN_MAX_S, so every finite d2 is at most 3 * 127^2.
//   1  nn_xy_kernel      t uint64 [N][2][D][H][W]: the pair over the seeds of the voxel's own plane
//   2  nn_z_kernel       nn [n][.][z][y][x] = the two smallest keys with distinct labels over z' and both
//                        ranks of t[n][.][z'][y][x] + ((z-z')^2 << 32)
//   3  wall_stats_kernel raw uint64 [T][3], one row per row of the instance table: the smallest key
//                        rank-1 d2 << 32 | index in the sample over the instance's voxels (all ones:
//                        no voxel carries the row), the voxels with rank-1 d2 <= limit2, the voxels
// The passes are separable because adding one offset to two keys keeps their order: a label that is
// not among the two best distinct ones at the intermediate position is not among them at the target.
// Integers only; every result is independent of the order of execution.
#include "instance_pass.h"

constexpr int NN_NTHR = 256;                    // the transform kernels
constexpr int NN_NWAVE = NN_NTHR / FN_WAVE;
constexpr int NN_MAX_S = 128;                   // longest axis: 128 * 64 pairs are 128 KB of the CU's 160 KB of LDS
constexpr int NN_INF = 1 << 30;
constexpr int NN_NCOL = 3;                      // key thin voxels
constexpr unsigned long long NN_NONE = (unsigned long long)NN_INF << 32;
static_assert(NN_NTHR % FN_WAVE == 0 && NN_MAX_S == 2 * FN_WAVE, "a row is two 64-wide pieces");

struct __attribute__((aligned(16))) NnPair {    // a < b, of distinct labels (or b == NN_NONE)
  unsigned long long a, b;
};

// ---------------------------------------------------------------------------------------------
// Transform
// ---------------------------------------------------------------------------------------------

// The pair after key k has been seen too.  k's label is rank 0's: it can only improve rank 0, and
// rank 1 (the best of the OTHER labels) stands.  Otherwise a k below rank 0 takes its place and the
// old rank 0, the best of the labels that are not k's, becomes rank 1; else k competes for rank 1
// (against its own label there too: the minimum).  NN_NONE plus an offset never wins anything.  A k
// that is not below rank 1 changes neither rank in any of the three cases, which is most of them once
// both ranks are near: one comparison tells.
__device__ __forceinline__ void nn_put(NnPair& p, unsigned long long k) {
  if (k >= p.b) return;
  if ((unsigned)k == (unsigned)p.a) {
    p.a = min(p.a, k);
  } else if (k < p.a) {
    p.b = p.a;
    p.a = k;
  } else {
    p.b = min(p.b, k);
  }
}

// The two best distinct keys over i' in [0, L) and both ranks of g(i') + ((i - i')^2 << 32): outward
// from i, both sides at once, while the step alone (k^2) does not exceed rank 1's distance -- at
// k^2 == that distance a seed of a smaller label still wins the tie.  With rank 1 missing (NN_INF)
// the loop runs to L - 1.
template <typename G>
__device__ __forceinline__ NnPair nn_scan(G g, int i, int L) {
  NnPair p = g(i);
  for (int k = 1; k < L && (unsigned)(k * k) <= (unsigned)(p.b >> 32); ++k) {
    const unsigned long long kk = (unsigned long long)(k * k) << 32;
    if (i - k >= 0) {
      const NnPair q = g(i - k);
      nn_put(p, q.a + kk);
      nn_put(p, q.b + kk);
    }
    if (i + k < L) {
      const NnPair q = g(i + k);
      nn_put(p, q.a + kk);
      nn_put(p, q.b + kk);
    }
  }
  return p;
}

// The highest set bit at or below position q / the lowest at or above q of the 128-bit row mask
// (lo: positions 0..63, hi: 64..127); -1: none, or q outside [0, 127] on that side.
__device__ __forceinline__ int nn_le(unsigned long long lo, unsigned long long hi, int q) {
  if (q < 0) return -1;
  if (q >= FN_WAVE) {
    const unsigned long long h = hi & (~0ull >> (2 * FN_WAVE - 1 - min(q, 2 * FN_WAVE - 1)));
    if (h) return 2 * FN_WAVE - 1 - __builtin_clzll(h);
    return lo ? FN_WAVE - 1 - __builtin_clzll(lo) : -1;
  }
  const unsigned long long l = lo & (~0ull >> (FN_WAVE - 1 - q));
  return l ? FN_WAVE - 1 - __builtin_clzll(l) : -1;
}
__device__ __forceinline__ int nn_ge(unsigned long long lo, unsigned long long hi, int q) {
  if (q >= 2 * FN_WAVE) return -1;
  q = max(q, 0);
  if (q < FN_WAVE) {
    const unsigned long long l = lo & (~0ull << q);
    if (l) return __builtin_ctzll(l);
    return hi ? FN_WAVE + __builtin_ctzll(hi) : -1;
  }
  const unsigned long long h = hi & (~0ull << (q - FN_WAVE));
  return h ? FN_WAVE + __builtin_ctzll(h) : -1;
}

// The id at position q (clamped into the row) of a row held as one register per 64-wide piece.
// Every lane of the wave calls it.
__device__ __forceinline__ int nn_id_at(int id0, int id1, int q) {
  q = min(max(q, 0), 2 * FN_WAVE - 1);
  const int v0 = __shfl(id0, q & (FN_WAVE - 1), FN_WAVE), v1 = __shfl(id1, q & (FN_WAVE - 1), FN_WAVE);
  return q < FN_WAVE ? v0 : v1;
}

// Grid: (N*D) * ceil(W/64) workgroups, one per (n, z) plane and 64-column strip.  Dynamic LDS: H * 64
// pairs.  Wave w takes rows y = w, w + 4, ..: it holds the whole row's ids, one register per 64-wide
// piece, and two masks of it, one ballot per piece each: "seed here" and "seed whose previous seed in
// the row has another id".  A lane's two best distinct labels along x are among four seeds: the nearest
// at or left of it, the nearest left of that with another id -- the seed before the last change at or
// below the first -- and the same two on the right -- the first change above the nearest is the first
// seed of another id.  After the barrier the lanes scan their column.
__global__ __launch_bounds__(NN_NTHR) void nn_xy_kernel(const int* __restrict__ ids, unsigned long long* __restrict__ t,
                                                        int D, int H, int W, int strips) {
  extern __shared__ __attribute__((aligned(16))) NnPair s_row[];       // [H][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int plane = blockIdx.x / strips, s = blockIdx.x - plane * strips;
  const int x = s * FN_WAVE + lane;
  const int* src = ids + (long long)plane * H * W;
  for (int y = wave; y < H; y += NN_NWAVE) {
    const int* row = src + (long long)y * W;
    const int x1 = FN_WAVE + lane;
    const int r0 = row[min(lane, W - 1)], r1 = row[min(x1, W - 1)];
    const int id0 = lane < W && r0 > 0 ? r0 : 0, id1 = x1 < W && r1 > 0 ? r1 : 0;     // 0: no seed
    const unsigned long long m0 = __ballot(id0 > 0), m1 = __ballot(id1 > 0);
    const int p0 = nn_le(m0, m1, lane - 1), p1 = nn_le(m0, m1, x1 - 1);                // the previous seed
    const int pid0 = nn_id_at(id0, id1, p0), pid1 = nn_id_at(id0, id1, p1);
    const unsigned long long c0 = __ballot(id0 > 0 && p0 >= 0 && pid0 != id0),
                             c1 = __ballot(id1 > 0 && p1 >= 0 && pid1 != id1);
    const int l1 = nn_le(m0, m1, x);
    const int lc = nn_le(c0, c1, l1);
    const int l2 = lc >= 0 ? nn_le(m0, m1, lc - 1) : -1;
    const int g1 = nn_ge(m0, m1, x);
    const int g2 = g1 >= 0 ? nn_ge(c0, c1, g1 + 1) : -1;
    NnPair p = {NN_NONE, NN_NONE};
    const int at[4] = {l1, l2, g1, g2};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int id = nn_id_at(id0, id1, at[c]), dx = x - at[c];
      if (at[c] >= 0) nn_put(p, (unsigned long long)(dx * dx) << 32 | (unsigned)id);
    }
    s_row[y * FN_WAVE + lane] = p;
  }
  __syncthreads();
  const int n = plane / D, z = plane - n * D;
  const long long V = (long long)D * H * W;
  unsigned long long* dst = t + (long long)n * 2 * V + (long long)z * H * W;
  for (int y = wave; y < H; y += NN_NWAVE) {
    const NnPair p = nn_scan([&](int i) { return s_row[i * FN_WAVE + lane]; }, y, H);
    if (x < W) {
      dst[(long long)y * W + x] = p.a;
      dst[V + (long long)y * W + x] = p.b;
    }
  }
}

// Grid: (N*H) * ceil(W/64) workgroups, one per (n, y) and 64-column strip.  Dynamic LDS: D * 64 pairs
// (128 KB at D = 128), the strip's pairs of every z; the same scan along z.  A workgroup reads exactly
// the elements it writes, and reads them all before the barrier, so nn may be t.
__global__ __launch_bounds__(NN_NTHR) void nn_z_kernel(const unsigned long long* t, unsigned long long* nn, int D,
                                                       int H, int W, int strips) {
  extern __shared__ __attribute__((aligned(16))) NnPair s_col[];       // [D][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x / strips, s = blockIdx.x - r * strips;      // r = n*H + y
  const int n = r / H, y = r - n * H;
  const int x = s * FN_WAVE + lane;
  const long long step = (long long)H * W, V = step * D;
  const long long base = (long long)n * 2 * V + (long long)y * W;
  for (int z = wave; z < D; z += NN_NWAVE) {
    const long long e = base + z * step + min(x, W - 1);
    s_col[z * FN_WAVE + lane] = {t[e], t[e + V]};
  }
  __syncthreads();
  for (int z = wave; z < D; z += NN_NWAVE) {
    const NnPair p = nn_scan([&](int i) { return s_col[i * FN_WAVE + lane]; }, z, D);
    if (x < W) {
      nn[base + z * step + x] = p.a;
      nn[base + z * step + x + V] = p.b;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Per-instance statistics
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NN_NTHR) void wall_init_kernel(unsigned long long* __restrict__ raw, long long T) {
  const long long i = (long long)blockIdx.x * NN_NTHR + threadIdx.x;
  if (i < T * NN_NCOL) raw[i] = i % NN_NCOL == 0 ? ~0ull : 0ull;
}

// The instance pass of instance_pass.h.  ids int32 [N*V]: per-sample ids from 1, 0 = none; offsets
// int64 [N+1]: the rows of each sample (ip_row); nn as nn_z_kernel writes it, of which rank 1 is read.
// A voxel's key d2 << 32 | index in the sample is below all ones, and the smallest key of an instance
// names its smallest d2 and, among the voxels that attain it, the smallest index, whatever the order
// of the updates: EVERY voxel of a row sends its key; the run's first lane adds the voxel and thin
// counts as well.
__global__ __launch_bounds__(IP_NTHR) void wall_stats_kernel(const int* __restrict__ ids,
                                                             const long long* __restrict__ offsets,
                                                             const unsigned long long* __restrict__ nn,
                                                             unsigned long long* raw, int total, int V, int T,
                                                             unsigned rV, int limit2) {
  __shared__ int s_gid[IP_SLOTS];
  __shared__ unsigned long long s_key[IP_SLOTS];
  __shared__ unsigned s_cnt[IP_SLOTS][2];
  const int tid = threadIdx.x;
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) s_gid[s] = 0, s_key[s] = ~0ull, s_cnt[s][0] = 0, s_cnt[s][1] = 0;
  __syncthreads();
  for (int it = 0; it < IP_CHUNK / IP_NTHR; ++it) {
    const auto [g, valid] = ip_voxel(it, total);
    const int n = ip_div(g, V, rV);
    const int gid = ip_row(offsets, n, ids[g], valid, T);
    const int d = (int)(nn[((long long)n * 2 + 1) * V + (g - n * V)] >> 32);
    const unsigned long long key = (unsigned long long)(unsigned)d << 32 | (unsigned)(g - n * V);
    const unsigned long long b_thin = __ballot(d <= limit2);
    // no break at x == 0: the counts need no coordinate (edt_stats_kernel)
    const auto [head, len, run] = ip_run(gid, false);
    if (gid > 0) {
      const unsigned thin = head ? (unsigned)__popcll(b_thin & run) : 0u, vox = head ? (unsigned)len : 0u;
      const int slot = ip_claim(s_gid, gid);
      if (slot >= 0) {
        atomicMin(&s_key[slot], key);
        if (thin) atomicAdd(&s_cnt[slot][0], thin);
        if (vox) atomicAdd(&s_cnt[slot][1], vox);
      } else {
        unsigned long long* dst = raw + (long long)(gid - 1) * NN_NCOL;
        __hip_atomic_fetch_min(&dst[0], key, IP_RLX_AGENT);
        if (thin) __hip_atomic_fetch_add(&dst[1], (unsigned long long)thin, IP_RLX_AGENT);
        if (vox) __hip_atomic_fetch_add(&dst[2], (unsigned long long)vox, IP_RLX_AGENT);
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) {
    const int gid = s_gid[s];
    if (gid <= 0) continue;
    unsigned long long* dst = raw + (long long)(gid - 1) * NN_NCOL;
    __hip_atomic_fetch_min(&dst[0], s_key[s], IP_RLX_AGENT);
    if (s_cnt[s][0]) __hip_atomic_fetch_add(&dst[1], (unsigned long long)s_cnt[s][0], IP_RLX_AGENT);
    if (s_cnt[s][1]) __hip_atomic_fetch_add(&dst[2], (unsigned long long)s_cnt[s][1], IP_RLX_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------
// Entry points
// ---------------------------------------------------------------------------------------------

static bool nn_shape_ok(int N, int D, int H, int W) {
  return ip_shape_ok(N, D, H, W) && D <= NN_MAX_S && H <= NN_MAX_S && W <= NN_MAX_S;
}

// Above 64 KB of dynamic LDS a kernel has to be told once.
template <typename K>
static int nn_allow_lds(K kernel, size_t lds) {
  if (lds <= 64 * 1024) return 0;
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess
             ? 0
             : -5;
}

extern "C" void fn_nn_chunk(int* t) { t[0] = IP_CHUNK, t[1] = IP_SLOTS; }

// ids int32 [N][D][H][W]; t, nn uint64 [N][2][D][H][W] (8-byte aligned; they may be one buffer).  passes: bit 0 runs
// nn_xy_kernel (ids -> t), bit 1 nn_z_kernel (t -> nn); each writes its output in full.
extern "C" int fn_nn_transform(const void* ids, void* t, void* nn, int N, int D, int H, int W, int passes,
                               hipStream_t st) {
  if (!nn_shape_ok(N, D, H, W) || !ids || !t || !nn || passes < 1 || passes > 3) return -2;
  if ((uintptr_t)ids % 4 != 0 || ((uintptr_t)t | (uintptr_t)nn) % 8 != 0) return -2;
  const int strips = (W + FN_WAVE - 1) / FN_WAVE;
  if (passes & 1) {
    const size_t lds = (size_t)H * FN_WAVE * sizeof(NnPair);
    if (nn_allow_lds(nn_xy_kernel, lds)) return -5;
    hipLaunchKernelGGL(nn_xy_kernel, dim3((unsigned)(N * D * strips)), dim3(NN_NTHR), lds, st, (const int*)ids,
                       (unsigned long long*)t, D, H, W, strips);
    FN_CHECK_LAUNCH();
  }
  if (passes & 2) {
    const size_t lds = (size_t)D * FN_WAVE * sizeof(NnPair);
    if (nn_allow_lds(nn_z_kernel, lds)) return -5;
    hipLaunchKernelGGL(nn_z_kernel, dim3((unsigned)(N * H * strips)), dim3(NN_NTHR), lds, st,
                       (const unsigned long long*)t, (unsigned long long*)nn, D, H, W, strips);
    FN_CHECK_LAUNCH();
  }
  return 0;
}

// ids int32 [N*V], offsets int64 [N+1], nn uint64 [N][2][V]; raw int64 [T][3] (8-byte aligned), fully rewritten: key,
// thin, voxels.  0 <= limit2 < NN_INF.
extern "C" int fn_wall_stats(const void* ids, const void* offsets, const void* nn, void* raw, int N, int D, int H,
                             int W, long long T, int limit2, hipStream_t st) {
  if (!nn_shape_ok(N, D, H, W) || !ids || !offsets || !nn || limit2 < 0 || limit2 >= NN_INF) return -2;
  if ((uintptr_t)ids % 4 != 0 || ((uintptr_t)offsets | (uintptr_t)nn | (uintptr_t)raw) % 8 != 0) return -2;
  const long long V = (long long)D * H * W, total = V * N;
  if (T < 0 || T > total || (T > 0 && !raw)) return -2;
  if (T > 0) {
    hipLaunchKernelGGL(wall_init_kernel, dim3((unsigned)((T * NN_NCOL + NN_NTHR - 1) / NN_NTHR)), dim3(NN_NTHR), 0,
                       st, (unsigned long long*)raw, T);
    FN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(wall_stats_kernel, dim3((unsigned)((total + IP_CHUNK - 1) / IP_CHUNK)), dim3(IP_NTHR), 0, st,
                     (const int*)ids, (const long long*)offsets, (const unsigned long long*)nn,
                     (unsigned long long*)raw, (int)total, (int)V, (int)T, ip_recip((int)V), limit2);
  FN_CHECK_LAUNCH();
  return 0;
}
