// Mesh labels: which value of a voxel volume lies against each triangle of the mesh the volume was
// made from (../shared/voxelize.h has the lattice, the cover test, the crossing and the turn to the
// dominant axis): the way back from the voxel grid to the faces of the user's model.
//
// tris int32 [T][9], offsets int32 [N + 1] (as voxelize.hip), vol V [N][S][S][S] (V = int32 or
// uint8, x fastest, 0 = nothing) -> votes int32 [T][3] = winner, votes, covered.  A triangle is
// turned so that its normal's dominant axis m carries the rays; every column (iu, iv) whose centre
// it covers is crossed at k = vx_kcross, and the voxels k - 1 and k of that column, one on each side
// of the surface, vote with their value if they lie in the grid and hold one.  A triangle that
// covers no column centre votes once at its centroid (covered stays 0).  The winner is the value
// with the most votes, the lowest on a tie.  Integers only: bit for bit what the host path (the
// same header) and the torch oracle (reference.mesh_votes) give.
//
// Two launches; a workgroup is one wave in both.
//   Thread form (pass 1): a wave owns 64 consecutive triangles, one per lane.  A lane whose
//   triangle's box of column centres holds at most `thr` columns (<= ML_THREAD_COLS) gathers its
//   votes alone and keeps them in registers: 2 ML_THREAD_COLS values, counted against each other in
//   unrolled loops (no runtime-indexed array).  The other triangles are appended to a list.
//   Wave form (pass 2): a fixed grid of waves strides that list, so that a few large triangles
//   spread over the chip wherever they stand in the mesh; the wave takes one triangle at a time,
//   lanes striding the box.  Votes go to a table of ML_SLOTS (value, count) pairs in
//   LDS, open addressing; the votes that agree with the first voting lane's -- all of them under
//   a planar face of one feature -- are counted by ballot and added once.  A triangle with more
//   distinct values under it than the table takes is finished exactly, not capped: the scan is
//   repeated in P = 2, 4, 8 ... passes, pass p counting only the values whose hash ends in p, and
//   the passes' winners are merged; at P = 2^(32 - ML_SLOT_BITS) the values of a pass have
//   different home slots, so the doubling ends.
// One global atomic add per wave of pass 1 that has triangles for the list, none elsewhere; plain
// vector stores; every gather's three indices are tested against [0, S) first and the mesh number
// is clamped to [0, N).
#include "common.h"
#include "../shared/voxelize.h"

constexpr int ML_THREAD_COLS = 8;                // the largest box the thread form takes
constexpr int ML_SLOT_BITS = 7;
constexpr int ML_SLOTS = 1 << ML_SLOT_BITS;      // (value, count) pairs of the wave form's table
constexpr int ML_PROBES = 16;                    // slots tried before a value counts as not fitting
static_assert(ML_SLOTS == 2 * FN_WAVE, "the table is read out two slots per lane");

__device__ __forceinline__ unsigned ml_hash(int v) {
  unsigned h = (unsigned)v * 0x9E3779B1u;        // odd multiplier, xor-shift: a bijection of 32 bits
  return h ^ (h >> 15);
}

// One triangle, turned: its mesh's volume, the strides of the axes m, u, v in it, the set-up
// triangle (live: the box holds a column) and the permuted vertices for the centroid vote.
template <typename V>
struct MlTri {
  const V* vol;
  int sm, su, sv;
  int q[9];
  VxTri t;
  bool ok, live;                                 // ok: the normal is not zero
};

template <typename V>
__device__ __forceinline__ void ml_setup(MlTri<V>& r, const int* tris, const int* offsets, const V* vol, int idx,
                                         int N, int S) {
  int lo = 0, hi = N;                            // the mesh of triangle idx: the last n with offsets[n] <= idx
  while (hi - lo > 1) {                          // (at most 31 turns; n stays in [0, N) whatever offsets holds)
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= idx) lo = mid;
    else hi = mid;
  }
  r.vol = vol + (size_t)lo * S * S * S;
  const int m = vx_dominant(tris + (size_t)idx * 9, r.q);
  r.ok = m >= 0;
  r.live = r.ok && vx_setup(r.q, S, 0, S - 1, r.t);
  const int sx = 1, sy = S, sz = S * S;          // (m, u, v) is (x, y, z), (y, z, x) or (z, x, y)
  r.sm = m == 1 ? sy : m == 2 ? sz : sx;
  r.su = m == 1 ? sz : m == 2 ? sx : sy;
  r.sv = m == 1 ? sx : m == 2 ? sy : sz;
}

// the value of voxel k of column (iu, iv), 0 outside the grid
template <typename V>
__device__ __forceinline__ int ml_at(const MlTri<V>& r, int S, int k, int iu, int iv) {
  if ((unsigned)k >= (unsigned)S || (unsigned)iu >= (unsigned)S || (unsigned)iv >= (unsigned)S) return 0;
  return (int)r.vol[k * r.sm + iu * r.su + iv * r.sv];       // (< S^3 <= 2^24)
}

// the row of a triangle with at most two votes
__device__ __forceinline__ void ml_store_pair(int* row, int a, int b, int covered) {
  int w = 0, c = 0;
  if (a != 0 && a == b) w = a, c = 2;
  else if (a != 0 && b != 0) w = a < b ? a : b, c = 1;
  else if ((a | b) != 0) w = a | b, c = 1;
  row[0] = w, row[1] = c, row[2] = covered;
}

template <typename V>
__device__ __forceinline__ void ml_centroid_row(const MlTri<V>& r, int S, int* row) {
  int k, iu, iv;
  vx_centroid(r.q, k, iu, iv);
  ml_store_pair(row, ml_at(r, S, k - 1, iu, iv), ml_at(r, S, k, iu, iv), 0);
}

// ---- thread form: the box holds at most ML_THREAD_COLS columns -------------------------------
template <typename V>
__device__ __forceinline__ void ml_thread(const MlTri<V>& r, int S, int* row) {
  int val[2 * ML_THREAD_COLS];
  int covered = 0, iu = r.t.y0, iv = r.t.z0;     // the box row by row; past it iv > z1
#pragma unroll
  for (int c = 0; c < ML_THREAD_COLS; ++c) {
    int a = 0, b = 0;
    if (iv <= r.t.z1 && vx_covers(r.t, iu, iv)) {
      const int k = vx_kcross(r.t, S, iu, iv);
      a = ml_at(r, S, k - 1, iu, iv), b = ml_at(r, S, k, iu, iv);
      ++covered;
    }
    val[2 * c] = a, val[2 * c + 1] = b;
    if (++iu > r.t.y1) iu = r.t.y0, ++iv;
  }
  if (covered == 0) {
    ml_centroid_row(r, S, row);
    return;
  }
  int best = 0, votes = 0;
#pragma unroll
  for (int i = 0; i < 2 * ML_THREAD_COLS; ++i) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < 2 * ML_THREAD_COLS; ++j) n += val[j] == val[i];
    n = val[i] != 0 ? n : 0;
    if (vx_beats(val[i], n, best, votes)) best = val[i], votes = n;
  }
  row[0] = best, row[1] = votes, row[2] = covered;
}

// ---- wave form -------------------------------------------------------------------------------
// n votes for value v != 0 -> false when no slot within ML_PROBES of its home takes it
__device__ __forceinline__ bool ml_insert(int* s_key, int* s_cnt, int v, int n) {
  unsigned slot = ml_hash(v) >> (32 - ML_SLOT_BITS);
  for (int i = 0; i < ML_PROBES; ++i, slot = (slot + 1) & (ML_SLOTS - 1)) {
    const int old = atomicCAS(&s_key[slot], 0, v);
    if (old == 0 || old == v) {
      atomicAdd(&s_cnt[slot], n);
      return true;
    }
  }
  return false;
}

// the votes of one value per lane: those equal to the first voting lane's go in as one add
__device__ __forceinline__ bool ml_vote(int* s_key, int* s_cnt, int v, int lane) {
  const unsigned long long voting = __ballot(v != 0);
  if (!voting) return true;
  const int first = __ffsll((long long)voting) - 1;
  const int lead = __shfl(v, first, FN_WAVE);
  const unsigned long long same = __ballot(v == lead);
  if (lane == first) return ml_insert(s_key, s_cnt, lead, __popcll(same));
  if (v != 0 && v != lead) return ml_insert(s_key, s_cnt, v, 1);
  return true;
}

// the whole wave on triangle r (the same in every lane); lane 0 stores the row
template <typename V>
__device__ __forceinline__ void ml_wave(const MlTri<V>& r, int S, int lane, int* s_key, int* s_cnt, int* row) {
  if (!r.ok) {
    if (lane == 0) row[0] = 0, row[1] = 0, row[2] = 0;
    return;
  }
  const int wy = r.live ? r.t.y1 - r.t.y0 + 1 : 0, wn = r.live ? wy * (r.t.z1 - r.t.z0 + 1) : 0;      // <= S * S
  int best = 0, votes = 0, covered = 0;
  for (unsigned P = 1;; P <<= 1) {               // passes; P = 2^(32 - ML_SLOT_BITS) always fits
    bool fits = true;
    best = 0, votes = 0;
    for (unsigned p = 0; p < P && fits; ++p) {
      s_key[lane] = 0, s_key[lane + FN_WAVE] = 0, s_cnt[lane] = 0, s_cnt[lane + FN_WAVE] = 0;
      __syncthreads();                           // (the workgroup is this wave: every lane is here)
      bool mine = true;
      int cov = 0;
      for (int base = 0; base < wn; base += FN_WAVE) {
        const int c = base + lane, dz = c / wy, iu = r.t.y0 + (c - dz * wy), iv = r.t.z0 + dz;
        int a = 0, b = 0;
        if (c < wn && vx_covers(r.t, iu, iv)) {
          const int k = vx_kcross(r.t, S, iu, iv);
          a = ml_at(r, S, k - 1, iu, iv), b = ml_at(r, S, k, iu, iv);
          ++cov;
        }
        if (P > 1) {                             // this pass's share of the values
          a = (ml_hash(a) & (P - 1)) == p ? a : 0;
          b = (ml_hash(b) & (P - 1)) == p ? b : 0;
        }
        mine &= ml_vote(s_key, s_cnt, a, lane);
        mine &= ml_vote(s_key, s_cnt, b, lane);
      }
      __syncthreads();
      fits = __ballot(!mine) == 0ull;
      if (p == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cov += __shfl_xor(cov, o, FN_WAVE);
        covered = cov;
      }
      // the pass's winner: two slots per lane, then across the wave
      int bv = s_key[lane], bn = s_cnt[lane];
      if (vx_beats(s_key[lane + FN_WAVE], s_cnt[lane + FN_WAVE], bv, bn)) bv = s_key[lane + FN_WAVE], bn = s_cnt[lane + FN_WAVE];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int ov = __shfl_xor(bv, o, FN_WAVE), on = __shfl_xor(bn, o, FN_WAVE);
        if (vx_beats(ov, on, bv, bn)) bv = ov, bn = on;
      }
      if (vx_beats(bv, bn, best, votes)) best = bv, votes = bn;
      __syncthreads();                           // the table is read before the next pass clears it
    }
    if (fits || P >= (1u << (32 - ML_SLOT_BITS))) break;
  }
  if (covered == 0) {
    if (lane == 0) ml_centroid_row(r, S, row);
    return;
  }
  if (lane == 0) row[0] = votes ? best : 0, row[1] = votes, row[2] = covered;
}

// Pass 1, a lane per triangle: the thread form where the box allows it; the others are appended to
// `wide` (wide[0] counts them, one atomic add per wave that has any; their order does not matter:
// every row is addressed by its triangle).
template <typename V>
__global__ __launch_bounds__(FN_WAVE) void mesh_votes_kernel(const int* __restrict__ tris, const int* __restrict__ offsets,
                                                             const V* __restrict__ vol, int* __restrict__ votes,
                                                             int* __restrict__ wide, int N, int T, int S, int thr) {
  const int lane = threadIdx.x;
  const int mine = blockIdx.x * FN_WAVE + lane;
  bool later = false;
  if (mine < T) {
    MlTri<V> r;
    ml_setup(r, tris, offsets, vol, mine, N, S);
    const int cols = r.live ? (r.t.y1 - r.t.y0 + 1) * (r.t.z1 - r.t.z0 + 1) : 0;
    int* row = votes + (size_t)mine * 3;
    if (cols > thr) later = true;                // (thr < 0: every triangle)
    else if (!r.ok) row[0] = 0, row[1] = 0, row[2] = 0;
    else if (!r.live) ml_centroid_row(r, S, row);
    else ml_thread(r, S, row);
  }
  const unsigned long long todo = __ballot(later);
  if (todo) {                                    // (the same in every lane)
    int base = 0;
    if (lane == 0) base = atomicAdd(&wide[0], __popcll(todo));
    base = __shfl(base, 0, FN_WAVE);
    const int at = base + __popcll(todo & ((1ull << lane) - 1ull));
    if (later && at >= 0 && at < T) wide[1 + at] = mine;     // (always: at most T triangles are ever appended)
  }
}

// Pass 2, a wave per listed triangle: the wave form.  The grid is fixed (the host does not know the
// count); a workgroup, one wave, strides the list.
template <typename V>
__global__ __launch_bounds__(FN_WAVE) void mesh_votes_wide_kernel(const int* __restrict__ tris,
                                                                  const int* __restrict__ offsets,
                                                                  const V* __restrict__ vol, int* __restrict__ votes,
                                                                  const int* __restrict__ wide, int N, int T, int S) {
  __shared__ int s_key[ML_SLOTS], s_cnt[ML_SLOTS];
  const int lane = threadIdx.x;
  int count = wide[0];
  count = count < 0 ? 0 : count > T ? T : count;
  for (int i = blockIdx.x; i < count; i += gridDim.x) {     // (uniform over the wave)
    const int idx = wide[1 + i];
    if (idx < 0 || idx >= T) continue;                       // (never: pass 1 wrote it)
    MlTri<V> w;
    ml_setup(w, tris, offsets, vol, idx, N, S);
    ml_wave(w, S, lane, s_key, s_cnt, votes + (size_t)idx * 3);
  }
}

constexpr int ML_WIDE_GRID = 256 * 16;           // waves of pass 2: 16 per CU

extern "C" int fn_mesh_votes_thread_cols() { return ML_THREAD_COLS; }

template <typename V>
static int ml_launch(const void* tris, const void* offsets, const void* vol, void* votes, void* wide, int N, int T, int S,
                     int thr, hipStream_t st) {
  hipError_t e = hipMemsetAsync(wide, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const unsigned blocks = (unsigned)((T + FN_WAVE - 1) / FN_WAVE);
  hipLaunchKernelGGL(mesh_votes_kernel<V>, dim3(blocks), dim3(FN_WAVE), 0, st, (const int*)tris, (const int*)offsets,
                     (const V*)vol, (int*)votes, (int*)wide, N, T, S, thr);
  FN_CHECK_LAUNCH();
  const unsigned waves = (unsigned)(T < ML_WIDE_GRID ? T : ML_WIDE_GRID);
  hipLaunchKernelGGL(mesh_votes_wide_kernel<V>, dim3(waves), dim3(FN_WAVE), 0, st, (const int*)tris, (const int*)offsets,
                     (const V*)vol, (int*)votes, (const int*)wide, N, T, S);
  FN_CHECK_LAUNCH();
  return 0;
}

// vol: elem = 4 (int32) or 1 (uint8).  thr: triangles whose box holds more than thr columns take
// the wave form; -1: all of them, at most ML_THREAD_COLS.  wide: scratch of T + 1 int32 (the count
// and the list of the wave form's triangles).  tris / offsets / votes / wide (and an int32 vol)
// 4-byte aligned; S % 8 == 0, 8 <= S <= 256; offsets must run from 0 to T without a decrease (a
// table that does not is still read safely).
extern "C" int fn_mesh_votes(const void* tris, const void* offsets, const void* vol, void* votes, void* wide, int N,
                             int T, int S, int elem, int thr, hipStream_t st) {
  if (N < 0 || T < 0 || S < 8 || S > VX_MAX_S || S % 8 != 0 || (elem != 1 && elem != 4)) return -2;
  if (thr < -1 || thr > ML_THREAD_COLS) return -2;
  if (((uintptr_t)tris | (uintptr_t)offsets | (uintptr_t)votes | (uintptr_t)wide) & 3) return -2;
  if (elem == 4 && ((uintptr_t)vol & 3)) return -2;
  if (T == 0) return 0;
  if (N == 0 || !tris || !offsets || !vol || !votes || !wide) return -2;
  return elem == 4 ? ml_launch<int>(tris, offsets, vol, votes, wide, N, T, S, thr, st)
                   : ml_launch<unsigned char>(tris, offsets, vol, votes, wide, N, T, S, thr, st);
}
