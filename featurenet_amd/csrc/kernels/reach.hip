// Tool reach of feature instances: how large a ball can travel in a straight line from outside each
// face of the grid to every voxel, and per instance what a given tool reaches and clears (the step
// that joins access.hip and edt.hip).
//
// vol int32 [N][D][H][W], indexed [n][z][y][x] (in the feature pipeline the d2 of edt.hip, >= 0).
// Faces in the order +z -z +x -x +y -y, +z the high-index end of z.
//   1  reach_scan_kernel   r6 int32 [N][6][D][H][W]: r6[n][k][v] = the minimum of vol[n] over the voxels
//                          from v to face k of the grid along that face's axis, v included: a running
//                          minimum from the face inward
//   2  reach_stats_kernel  raw int64 [T][15], one row per row of the instance table: the largest r6[k]
//                          over the instance's voxels (0..5; -1: no voxel carries the row), the voxels
//                          with r6[k] >= need2 (6..11), with no such k (12), with dc2 <= cut2 (13), the
//                          voxels (14)
// Integers only; every result is independent of the order of execution.
#include <limits.h>

#include "instance_pass.h"

constexpr int RCH_NTHR = 256;                   // the scan kernel
constexpr int RCH_NWAVE = RCH_NTHR / FN_WAVE;
constexpr int RCH_MAX_S = 256;                  // longest axis (EDT_MAX_S of edt.hip)
constexpr int RCH_PIECES = RCH_MAX_S / FN_WAVE; // 64-wide pieces of a row
constexpr int RCH_NMAX = 6;                     // entry2 of the six faces
constexpr int RCH_NCNT = 9;                     // reached from each face, from none, machinable, voxels
constexpr int RCH_NCOL = RCH_NMAX + RCH_NCNT;
static_assert(RCH_NTHR % FN_WAVE == 0 && RCH_MAX_S % FN_WAVE == 0, "shape");

// ---------------------------------------------------------------------------------------------
// Directional scan
// ---------------------------------------------------------------------------------------------

// Inclusive minimum over the lanes at or below (prefix) / at or above (suffix) this one.
__device__ __forceinline__ int rch_prefix_min(int v, int lane) {
#pragma unroll
  for (int o = 1; o < FN_WAVE; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v = min(v, t);
  }
  return v;
}
__device__ __forceinline__ int rch_suffix_min(int v, int lane) {
#pragma unroll
  for (int o = 1; o < FN_WAVE; o <<= 1) {
    const int t = __shfl_down(v, o, 64);
    if (lane + o < FN_WAVE) v = min(v, t);
  }
  return v;
}

// The two running minima of 64 of the W columns that run along one axis of a slab, those from x0:
// column x holds the L voxels src[i * stride + x], and hi[i * stride + x] = min over i' >= i, lo[..]
// = min over i' <= i.  Lanes along x.  Wave w takes the segment [w * seg, (w + 1) * seg) of every
// column: its minimum goes to LDS, the minimum of the segments before (behind) it is the carry of its
// walk up (down).  The loads depend on no minimum, so the unrolled loops keep eight in flight.
__device__ __forceinline__ void rch_walk(const int* __restrict__ src, int L, long long stride, int W, int x0,
                                         int* __restrict__ hi, int* __restrict__ lo, int (*s_min)[FN_WAVE]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = (L + RCH_NWAVE - 1) / RCH_NWAVE;
  const int i0 = min(wave * seg, L), i1 = min(i0 + seg, L);
  const int x = x0 + lane;
  const bool inx = x < W;
  const int* col = src + min(x, W - 1);         // (lanes past the row read a clamped address)
  int m = INT_MAX;
#pragma unroll 8
  for (int i = i0; i < i1; ++i) m = min(m, col[i * stride]);
  s_min[wave][lane] = m;
  __syncthreads();
  int below = INT_MAX, above = INT_MAX;
#pragma unroll
  for (int w = 0; w < RCH_NWAVE; ++w) {
    const int o = s_min[w][lane];
    if (w < wave) below = min(below, o);
    if (w > wave) above = min(above, o);
  }
#pragma unroll 8
  for (int i = i0; i < i1; ++i) {
    below = min(below, col[i * stride]);
    if (inx) lo[i * stride + x] = below;
  }
#pragma unroll 8
  for (int i = i1 - 1; i >= i0; --i) {
    above = min(above, col[i * stride]);
    if (inx) hi[i * stride + x] = above;
  }
}

// Grid: N*D * strips workgroups (strips = ceil(W / 64)), one per (n, z) plane and 64-column strip,
// write that strip of the plane's y faces and, of its x faces, every strips-th group of four rows;
// N*H * strips more, one per (n, y) and strip, write that strip of the z faces.  Every element of r6
// is written by exactly one workgroup; no atomics.  A row's x minima are a prefix and a suffix
// minimum across the wave, carried across the 64-wide pieces of the row, which the wave holds in
// registers.
__global__ __launch_bounds__(RCH_NTHR) void reach_scan_kernel(const int* __restrict__ vol, int* __restrict__ r6,
                                                              int N, int D, int H, int W, int strips) {
  __shared__ int s_min[RCH_NWAVE][FN_WAVE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x / strips, s = blockIdx.x - q * strips;
  const long long V = (long long)D * H * W;
  if (q < N * D) {                               // (uniform) plane q = n*D + z
    const int n = q / D, z = q - n * D;
    const long long in_sample = (long long)z * H * W;
    const int* plane = vol + n * V + in_sample;
    int* out = r6 + (long long)n * 6 * V + in_sample;          // face k of this plane: out + k * V
    for (int y = s * RCH_NWAVE + wave; y < H; y += strips * RCH_NWAVE) {
      const int* row = plane + (long long)y * W;
      int *px = out + 2 * V + (long long)y * W, *mx = out + 3 * V + (long long)y * W;
      int v[RCH_PIECES];
#pragma unroll
      for (int p = 0; p < RCH_PIECES; ++p) {
        const int xp = p * FN_WAVE + lane;
        v[p] = xp < W ? row[min(xp, W - 1)] : INT_MAX;
      }
      int carry = INT_MAX;
#pragma unroll
      for (int p = 0; p < RCH_PIECES; ++p) {
        if (p * FN_WAVE < W) {                   // (uniform)
          const int xp = p * FN_WAVE + lane;
          const int m = min(rch_prefix_min(v[p], lane), carry);
          if (xp < W) mx[xp] = m;
          carry = __shfl(m, FN_WAVE - 1, 64);
        }
      }
      carry = INT_MAX;
#pragma unroll
      for (int p = RCH_PIECES - 1; p >= 0; --p) {
        if (p * FN_WAVE < W) {
          const int xp = p * FN_WAVE + lane;
          const int m = min(rch_suffix_min(v[p], lane), carry);
          if (xp < W) px[xp] = m;
          carry = __shfl(m, 0, 64);
        }
      }
    }
    rch_walk(plane, H, W, W, s * FN_WAVE, out + 4 * V, out + 5 * V, s_min);
  } else {
    const int r = q - N * D, n = r / H, y = r - n * H;
    const long long in_sample = (long long)y * W;
    rch_walk(vol + n * V + in_sample, D, (long long)H * W, W, s * FN_WAVE, r6 + (long long)n * 6 * V + in_sample,
             r6 + ((long long)n * 6 + 1) * V + in_sample, s_min);
  }
}

// ---------------------------------------------------------------------------------------------
// Reach table
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(RCH_NTHR) void reach_init_kernel(long long* __restrict__ raw, long long T) {
  const long long i = (long long)blockIdx.x * RCH_NTHR + threadIdx.x;
  if (i < T * RCH_NCOL) raw[i] = i % RCH_NCOL < RCH_NMAX ? -1 : 0;
}

// The instance pass of instance_pass.h.  ids int32 [N*V]: per-sample ids from 1, 0 = none; offsets
// int64 [N+1]: the rows of each sample (ip_row); r6 int32 [N][6][V], >= 0; dc2 int32 [N*V].  The nine
// counts are added once per run, by its first lane, as popcounts of the ballots under the run's
// lanes.  A maximum does not care how often it is offered: every voxel of a row offers its six
// values to the row's slot, and only where one exceeds what the slot already holds does it cost an
// atomic (the value read may be stale, but a slot only grows, so nothing larger is ever dropped).
__global__ __launch_bounds__(IP_NTHR) void reach_stats_kernel(const int* __restrict__ ids,
                                                             const long long* __restrict__ offsets,
                                                             const int* __restrict__ r6,
                                                             const int* __restrict__ dc2, long long* raw, int total,
                                                             int V, int T, unsigned rV, int need2, int cut2) {
  __shared__ int s_gid[IP_SLOTS];
  __shared__ int s_max[IP_SLOTS][RCH_NMAX];
  __shared__ unsigned s_cnt[IP_SLOTS][RCH_NCNT];
  const int tid = threadIdx.x;
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) {
    s_gid[s] = 0;
#pragma unroll
    for (int k = 0; k < RCH_NMAX; ++k) s_max[s][k] = -1;
#pragma unroll
    for (int k = 0; k < RCH_NCNT; ++k) s_cnt[s][k] = 0;
  }
  __syncthreads();
  for (int it = 0; it < IP_CHUNK / IP_NTHR; ++it) {
    const auto [g, valid] = ip_voxel(it, total);
    const int n = ip_div(g, V, rV);
    const int gid = ip_row(offsets, n, ids[g], valid, T);
    const int* rv = r6 + (long long)n * 5 * V + g;             // (n*6 + k)*V + (g - n*V) = n*5*V + g + k*V
    int e[RCH_NMAX];
    unsigned long long b[RCH_NCNT];
    bool any = false;
#pragma unroll
    for (int k = 0; k < RCH_NMAX; ++k) {
      e[k] = rv[(long long)k * V];
      const bool in = e[k] >= need2;
      any |= in;
      b[k] = __ballot(in);
    }
    b[6] = __ballot(!any);
    b[7] = __ballot(dc2[g] <= cut2);
    // no break at x == 0: nothing here needs a coordinate (edt_stats_kernel)
    const auto [head, len, run] = ip_run(gid, false);
    if (gid > 0) {
      const int slot = ip_claim(s_gid, gid);
      long long* dst = raw + (long long)(gid - 1) * RCH_NCOL;
      if (slot >= 0) {
#pragma unroll
        for (int k = 0; k < RCH_NMAX; ++k)
          if (e[k] > s_max[slot][k]) atomicMax(&s_max[slot][k], e[k]);
      } else {
#pragma unroll
        for (int k = 0; k < RCH_NMAX; ++k)
          if (e[k] >= 0) __hip_atomic_fetch_max(&dst[k], (long long)e[k], IP_RLX_AGENT);
      }
      if (head) {
        unsigned c[RCH_NCNT];
#pragma unroll
        for (int k = 0; k < RCH_NCNT - 1; ++k) c[k] = (unsigned)__popcll(b[k] & run);
        c[RCH_NCNT - 1] = (unsigned)len;
        if (slot >= 0) {
#pragma unroll
          for (int k = 0; k < RCH_NCNT; ++k)
            if (c[k]) atomicAdd(&s_cnt[slot][k], c[k]);
        } else {
#pragma unroll
          for (int k = 0; k < RCH_NCNT; ++k)
            if (c[k]) __hip_atomic_fetch_add(&dst[RCH_NMAX + k], (long long)c[k], IP_RLX_AGENT);
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < IP_SLOTS * RCH_NCOL; i += IP_NTHR) {
    const int s = i / RCH_NCOL, k = i - s * RCH_NCOL, gid = s_gid[s];
    if (gid <= 0) continue;
    long long* dst = raw + (long long)(gid - 1) * RCH_NCOL + k;
    if (k < RCH_NMAX) {
      const int m = s_max[s][k];
      if (m >= 0) __hip_atomic_fetch_max(dst, (long long)m, IP_RLX_AGENT);
    } else {
      const unsigned cnt = s_cnt[s][k - RCH_NMAX];
      if (cnt) __hip_atomic_fetch_add(dst, (long long)cnt, IP_RLX_AGENT);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Entry points
// ---------------------------------------------------------------------------------------------

static bool rch_shape_ok(int N, int D, int H, int W) {
  return ip_shape_ok(N, D, H, W) && D <= RCH_MAX_S && H <= RCH_MAX_S && W <= RCH_MAX_S;
}

extern "C" void fn_reach_chunk(int* t) { t[0] = IP_CHUNK, t[1] = IP_SLOTS; }

// vol int32 [N][D][H][W]; r6 int32 [N][6][D][H][W] (4-byte aligned), written in full.
extern "C" int fn_reach_scan(const void* vol, void* r6, int N, int D, int H, int W, hipStream_t st) {
  if (!rch_shape_ok(N, D, H, W) || !vol || !r6) return -2;
  if (((uintptr_t)vol | (uintptr_t)r6) % 4 != 0) return -2;
  const int strips = (W + FN_WAVE - 1) / FN_WAVE;
  const long long nblk = ((long long)N * D + (long long)N * H) * strips;
  if (nblk >= (1LL << 31)) return -2;
  hipLaunchKernelGGL(reach_scan_kernel, dim3((unsigned)nblk), dim3(RCH_NTHR), 0, st, (const int*)vol, (int*)r6, N, D,
                     H, W, strips);
  FN_CHECK_LAUNCH();
  return 0;
}

// ids, dc2 int32 [N*V], offsets int64 [N+1], r6 int32 [N][6][V] with values >= 0; raw int64 [T][15] (8-byte
// aligned), fully rewritten.  need2 >= 1, cut2 >= 0.
extern "C" int fn_reach_stats(const void* ids, const void* offsets, const void* r6, const void* dc2, void* raw, int N,
                              int D, int H, int W, long long T, int need2, int cut2, hipStream_t st) {
  if (!rch_shape_ok(N, D, H, W) || !ids || !offsets || !r6 || !dc2 || need2 < 1 || cut2 < 0) return -2;
  if (((uintptr_t)ids | (uintptr_t)r6 | (uintptr_t)dc2) % 4 != 0 || ((uintptr_t)offsets | (uintptr_t)raw) % 8 != 0)
    return -2;
  const long long V = (long long)D * H * W, total = V * N;
  if (T < 0 || T > total || (T > 0 && !raw)) return -2;
  if (T > 0) {
    hipLaunchKernelGGL(reach_init_kernel, dim3((unsigned)((T * RCH_NCOL + RCH_NTHR - 1) / RCH_NTHR)), dim3(RCH_NTHR), 0,
                       st, (long long*)raw, T);
    FN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(reach_stats_kernel, dim3((unsigned)((total + IP_CHUNK - 1) / IP_CHUNK)), dim3(IP_NTHR), 0, st,
                     (const int*)ids, (const long long*)offsets, (const int*)r6, (const int*)dc2, (long long*)raw,
                     (int)total, (int)V, (int)T, ip_recip((int)V), need2, cut2);
  FN_CHECK_LAUNCH();
  return 0;
}
