// Dimensions of feature instances: the exact squared Euclidean distance from every voxel to the
// nearest seed (material, in the feature pipeline), and per instance its largest value, where it is
// attained, and the voxels that touch a seed (the step beside access.hip).
//
// seeds uint8 [N][D][H][W], indexed [n][z][y][x]: a voxel is a seed when seeds != 0; with border
// every position just outside the grid is one too.  D, H, W <= EDT_MAX_S, so every finite result is
// at most 3 * 255^2; EDT_INF marks a sample without a seed.
//   1  edt_xy_kernel     t int32 [N][D][H][W]: min over the seeds (y', x') of the voxel's own plane
//                        of (y-y')^2 + (x-x')^2 (EDT_INF: the plane has none)
//   2  edt_z_kernel      d2 [n][z][y][x] = min over z' of t[n][z'][y][x] + (z-z')^2, at most EDT_INF
//   3  edt_stats_kernel  raw int64 [T][3], one row per row of the instance table: the largest key
//                        d2 << 32 | (0xFFFFFFFF - index in the sample) over the instance's voxels,
//                        the voxels with d2 == 1, the voxels (all 0: no voxel carries the row)
// Integers only; every result is independent of the order of execution.
#include "instance_pass.h"

constexpr int EDT_NTHR = 256;                   // the transform kernels
constexpr int EDT_NWAVE = EDT_NTHR / FN_WAVE;
constexpr int EDT_MAX_S = 256;                  // longest axis
constexpr int EDT_PIECES = EDT_MAX_S / FN_WAVE; // 64-wide pieces of a row
constexpr int EDT_INF = 1 << 30;
constexpr int EDT_NONE16 = 0xFFFF;              // "no seed in this row" among the uint16 row distances (255^2 < it)
constexpr int EDT_NCOL = 3;                     // key wall voxels
static_assert(EDT_NTHR % FN_WAVE == 0 && EDT_MAX_S % FN_WAVE == 0, "shape");
static_assert((EDT_MAX_S - 1) * (EDT_MAX_S - 1) < EDT_NONE16, "a squared row distance fits uint16");

// ---------------------------------------------------------------------------------------------
// Transform
// ---------------------------------------------------------------------------------------------

// min over i' in [0, L) of g(i') + (i - i')^2 given g >= 0: outward from i, both sides at once, until
// the step alone (k^2) is no better than the best so far.  At most L - 1 steps.
template <typename G>
__device__ __forceinline__ int edt_scan(G g, int i, int L) {
  int best = g(i);
  for (int k = 1; k < L && k * k < best; ++k) {
    const int kk = k * k;
    if (i - k >= 0) best = min(best, g(i - k) + kk);
    if (i + k < L) best = min(best, g(i + k) + kk);
  }
  return best;
}

__device__ __forceinline__ int edt_border(int i, int L) {     // the squared distance to the nearer end's outside
  const int b = min(i + 1, L - i);
  return b * b;
}

// Grid: (N*D) * ceil(W/64) workgroups, one per (n, z) plane and 64-column strip.  Dynamic LDS: H * 64
// uint16.  Wave w takes rows y = w, w + 4, ..: the seed bits of the whole row are one ballot per
// 64-wide piece, and a lane's distance along x comes from the bit positions on either side of it,
// in its own piece or in another.  After the barrier the lanes run along x and scan their column.
__global__ __launch_bounds__(EDT_NTHR) void edt_xy_kernel(const uint8_t* __restrict__ seeds, int* __restrict__ t,
                                                          int H, int W, int strips, int border) {
  extern __shared__ uint16_t s_g[];              // [H][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int plane = blockIdx.x / strips, s = blockIdx.x - plane * strips;
  const int x = s * FN_WAVE + lane;
  const uint8_t* src = seeds + (long long)plane * H * W;
  for (int y = wave; y < H; y += EDT_NWAVE) {
    const uint8_t* row = src + (long long)y * W;
    int best = EDT_MAX_S;                        // (a real distance is at most 255)
#pragma unroll
    for (int p = 0; p < EDT_PIECES; ++p) {
      const int xp = p * FN_WAVE + lane;
      const unsigned long long m = p * FN_WAVE < W ? __ballot(xp < W && row[min(xp, W - 1)] != 0) : 0ull;
      if (p == s) {
        const unsigned long long left = m & (~0ull >> (63 - lane)), right = m & (~0ull << lane);
        if (left) best = min(best, lane - (63 - __builtin_clzll(left)));
        if (right) best = min(best, __builtin_ctzll(right) - lane);
      } else if (m) {
        best = min(best, p < s ? x - (p * FN_WAVE + 63 - __builtin_clzll(m)) : p * FN_WAVE + __builtin_ctzll(m) - x);
      }
    }
    if (border) best = min(best, min(x + 1, max(W - x, 1)));
    s_g[y * FN_WAVE + lane] = (uint16_t)(best < EDT_MAX_S ? best * best : EDT_NONE16);
  }
  __syncthreads();
  int* dst = t + (long long)plane * H * W;
  for (int y = wave; y < H; y += EDT_NWAVE) {
    int best = edt_scan(
        [&](int i) {
          const int v = s_g[i * FN_WAVE + lane];
          return v == EDT_NONE16 ? EDT_INF : v;
        },
        y, H);
    if (border) best = min(best, edt_border(y, H));
    if (x < W) dst[(long long)y * W + x] = best;
  }
}

// Grid: (N*H) * ceil(W/64) workgroups, one per (n, y) and 64-column strip.  Dynamic LDS: D * 64 int32
// (64 KB at D = 256), the strip's t values of every z; the same scan along z.  A workgroup reads
// exactly the elements it writes, and reads them all before the barrier, so d2 may be t.
__global__ __launch_bounds__(EDT_NTHR) void edt_z_kernel(const int* t, int* d2, int D, int H, int W, int strips,
                                                         int border) {
  extern __shared__ int s_t[];                   // [D][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x / strips, s = blockIdx.x - r * strips;          // r = n*H + y
  const int n = r / H, y = r - n * H;
  const int x = s * FN_WAVE + lane;
  const long long base = ((long long)n * D * H + y) * W, step = (long long)H * W;
  for (int z = wave; z < D; z += EDT_NWAVE) s_t[z * FN_WAVE + lane] = t[base + z * step + min(x, W - 1)];
  __syncthreads();
  for (int z = wave; z < D; z += EDT_NWAVE) {
    int best = edt_scan([&](int i) { return s_t[i * FN_WAVE + lane]; }, z, D);
    if (border) best = min(best, edt_border(z, D));
    if (x < W) d2[base + z * step + x] = min(best, EDT_INF);
  }
}

// ---------------------------------------------------------------------------------------------
// Per-instance statistics
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(EDT_NTHR) void edt_init_kernel(unsigned long long* __restrict__ raw, long long T) {
  const long long i = (long long)blockIdx.x * EDT_NTHR + threadIdx.x;
  if (i < T * EDT_NCOL) raw[i] = 0;
}

// The instance pass of instance_pass.h.  ids int32 [N*V]: per-sample ids from 1, 0 = none; offsets
// int64 [N+1]: the rows of each sample (ip_row).  A voxel's key d2 << 32 | (0xFFFFFFFF - index in
// the sample) is positive, and the largest key of an instance names its largest d2 and, among the
// voxels that attain it, the smallest index, whatever the order of the updates: EVERY voxel of a
// row sends its key; the run's first lane adds the voxel and wall counts as well.
__global__ __launch_bounds__(IP_NTHR) void edt_stats_kernel(const int* __restrict__ ids,
                                                            const long long* __restrict__ offsets,
                                                            const int* __restrict__ d2, unsigned long long* raw,
                                                            int total, int V, int T, unsigned rV) {
  __shared__ int s_gid[IP_SLOTS];
  __shared__ unsigned long long s_key[IP_SLOTS];
  __shared__ unsigned s_cnt[IP_SLOTS][2];
  const int tid = threadIdx.x;
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) s_gid[s] = 0, s_key[s] = 0, s_cnt[s][0] = 0, s_cnt[s][1] = 0;
  __syncthreads();
  for (int it = 0; it < IP_CHUNK / IP_NTHR; ++it) {
    const auto [g, valid] = ip_voxel(it, total);
    const int n = ip_div(g, V, rV);
    const int gid = ip_row(offsets, n, ids[g], valid, T);
    const int d = d2[g];
    const unsigned long long key = (unsigned long long)(unsigned)d << 32 | (0xFFFFFFFFu - (unsigned)(g - n * V));
    const unsigned long long b_wall = __ballot(d == 1);
    // no break at x == 0: the counts need no coordinate, so a run may go on into the next row of W
    // (into the next sample it cannot: the row number changes), and x is never computed
    const auto [head, len, run] = ip_run(gid, false);
    if (gid > 0) {
      const unsigned wall = head ? (unsigned)__popcll(b_wall & run) : 0u, vox = head ? (unsigned)len : 0u;
      const int slot = ip_claim(s_gid, gid);
      if (slot >= 0) {
        atomicMax(&s_key[slot], key);
        if (wall) atomicAdd(&s_cnt[slot][0], wall);
        if (vox) atomicAdd(&s_cnt[slot][1], vox);
      } else {
        unsigned long long* dst = raw + (long long)(gid - 1) * EDT_NCOL;
        __hip_atomic_fetch_max(&dst[0], key, IP_RLX_AGENT);
        if (wall) __hip_atomic_fetch_add(&dst[1], (unsigned long long)wall, IP_RLX_AGENT);
        if (vox) __hip_atomic_fetch_add(&dst[2], (unsigned long long)vox, IP_RLX_AGENT);
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) {
    const int gid = s_gid[s];
    if (gid <= 0) continue;
    unsigned long long* dst = raw + (long long)(gid - 1) * EDT_NCOL;
    __hip_atomic_fetch_max(&dst[0], s_key[s], IP_RLX_AGENT);
    if (s_cnt[s][0]) __hip_atomic_fetch_add(&dst[1], (unsigned long long)s_cnt[s][0], IP_RLX_AGENT);
    if (s_cnt[s][1]) __hip_atomic_fetch_add(&dst[2], (unsigned long long)s_cnt[s][1], IP_RLX_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------
// Entry points
// ---------------------------------------------------------------------------------------------

static bool edt_shape_ok(int N, int D, int H, int W) {
  return ip_shape_ok(N, D, H, W) && D <= EDT_MAX_S && H <= EDT_MAX_S && W <= EDT_MAX_S;
}

extern "C" void fn_edt_chunk(int* t) { t[0] = IP_CHUNK, t[1] = IP_SLOTS; }

// seeds uint8 [N][D][H][W]; t, d2 int32 [N][D][H][W] (4-byte aligned; they may be one buffer).  passes: bit 0 runs
// edt_xy_kernel (seeds -> t), bit 1 edt_z_kernel (t -> d2); each writes its output in full.
extern "C" int fn_edt_transform(const void* seeds, void* t, void* d2, int N, int D, int H, int W, int border,
                                int passes, hipStream_t st) {
  if (!edt_shape_ok(N, D, H, W) || !seeds || !t || !d2 || passes < 1 || passes > 3) return -2;
  if (((uintptr_t)t | (uintptr_t)d2) % 4 != 0) return -2;
  const int strips = (W + FN_WAVE - 1) / FN_WAVE;
  if (passes & 1) {
    hipLaunchKernelGGL(edt_xy_kernel, dim3((unsigned)(N * D * strips)), dim3(EDT_NTHR),
                       (size_t)H * FN_WAVE * sizeof(uint16_t), st, (const uint8_t*)seeds, (int*)t, H, W, strips,
                       border != 0);
    FN_CHECK_LAUNCH();
  }
  if (passes & 2) {
    hipLaunchKernelGGL(edt_z_kernel, dim3((unsigned)(N * H * strips)), dim3(EDT_NTHR),
                       (size_t)D * FN_WAVE * sizeof(int), st, (const int*)t, (int*)d2, D, H, W, strips, border != 0);
    FN_CHECK_LAUNCH();
  }
  return 0;
}

// ids, d2 int32 [N*V], offsets int64 [N+1]; raw int64 [T][3] (8-byte aligned), fully rewritten: key, wall, voxels.
extern "C" int fn_edt_stats(const void* ids, const void* offsets, const void* d2, void* raw, int N, int D, int H,
                            int W, long long T, hipStream_t st) {
  if (!edt_shape_ok(N, D, H, W) || !ids || !offsets || !d2) return -2;
  if (((uintptr_t)ids | (uintptr_t)d2) % 4 != 0 || ((uintptr_t)offsets | (uintptr_t)raw) % 8 != 0) return -2;
  const long long V = (long long)D * H * W, total = V * N;
  if (T < 0 || T > total || (T > 0 && !raw)) return -2;
  if (T > 0) {
    hipLaunchKernelGGL(edt_init_kernel, dim3((unsigned)((T * EDT_NCOL + EDT_NTHR - 1) / EDT_NTHR)), dim3(EDT_NTHR), 0,
                       st, (unsigned long long*)raw, T);
    FN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(edt_stats_kernel, dim3((unsigned)((total + IP_CHUNK - 1) / IP_CHUNK)), dim3(IP_NTHR), 0, st,
                     (const int*)ids, (const long long*)offsets, (const int*)d2, (unsigned long long*)raw, (int)total,
                     (int)V, (int)T, ip_recip((int)V));
  FN_CHECK_LAUNCH();
  return 0;
}
