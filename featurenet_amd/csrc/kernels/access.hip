// Access directions of feature instances: from which of the six faces of the grid a tool reaches
// the voxels of each instance (the step after the instance table of ccl.hip).
//
// occ uint8 [N][D][H][W], indexed [n][z][y][x]: a voxel is material when occ != 0.  Faces in the
// order +z -z +x -x +y -y (bit k of a voxel's mask = face k), +z the high-index end of z.
//   1  access_extents_kernel  column extents: ex int32 [N][D][H][2], ey [N][D][W][2], ez [N][H][W][2];
//                             [..][0] = lo, the smallest index along the axis that holds material
//                             (the axis length when the column has none), [..][1] = hi, the largest
//                             (-1 when none)
//   2  access_stats_kernel    a voxel (z, y, x) is open toward +x iff ex hi <= x and toward -x iff
//                             ex lo >= x (its own occupancy does not enter), likewise y and z; acc
//                             int64 [T][8], one row per row of the instance table: voxels open toward
//                             each face, voxels open toward none, voxels
// Every result is an integer that does not depend on the order of the atomics.
#include "instance_pass.h"

constexpr int ACC_NTHR = 256;                   // the extents kernel
constexpr int ACC_NWAVE = ACC_NTHR / FN_WAVE;
constexpr int ACC_NCOL = 8;                     // +z -z +x -x +y -y none voxels

// ---------------------------------------------------------------------------------------------
// Column extents
// ---------------------------------------------------------------------------------------------

// Extents of the W columns that run along one axis of a slab: column x holds the L voxels
// src[i * stride + x].  Lanes along x, 64 columns at a time; wave w walks i = w, w + 4, ..; the four
// waves' extents of a column meet in LDS and wave 0 writes out[x] = (lo, hi).
__device__ __forceinline__ void acc_walk_extents(const uint8_t* __restrict__ src, int L, long long stride, int W,
                                                 int2* __restrict__ out, int (*s_lo)[FN_WAVE], int (*s_hi)[FN_WAVE]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int x0 = 0; x0 < W; x0 += FN_WAVE) {
    const int x = x0 + lane;
    const bool inx = x < W;
    const uint8_t* col = src + min(x, W - 1);   // (lanes past the row read a clamped address)
    int lo = L, hi = -1;
    for (int i = wave; i < L; i += ACC_NWAVE)
      if (col[i * stride] != 0) lo = min(lo, i), hi = i;
    s_lo[wave][lane] = lo, s_hi[wave][lane] = hi;
    __syncthreads();
    if (wave == 0 && inx) {
#pragma unroll
      for (int w = 1; w < ACC_NWAVE; ++w) lo = min(lo, s_lo[w][lane]), hi = max(hi, s_hi[w][lane]);
      out[x] = make_int2(lo, hi);
    }
    __syncthreads();
  }
}

// Grid: N*D workgroups, one per (n, z) plane, write that plane's ex rows and ey columns; N*H more,
// one per (n, y), write ez.  Every table element is written by exactly one workgroup; no atomics.
// The x extents of a row are one ballot per 64 voxels, met in the wave's registers.
__global__ __launch_bounds__(ACC_NTHR) void access_extents_kernel(const uint8_t* __restrict__ occ,
                                                                  int2* __restrict__ ex, int2* __restrict__ ey,
                                                                  int2* __restrict__ ez, int N, int D, int H, int W) {
  __shared__ int s_lo[ACC_NWAVE][FN_WAVE];
  __shared__ int s_hi[ACC_NWAVE][FN_WAVE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  if (b < N * D) {                               // (uniform) plane b = n*D + z
    const uint8_t* plane = occ + (long long)b * H * W;
    for (int y = wave; y < H; y += ACC_NWAVE) {
      const uint8_t* row = plane + (long long)y * W;
      int lo = W, hi = -1;
      for (int x0 = 0; x0 < W; x0 += FN_WAVE) {
        const int x = x0 + lane;
        const unsigned long long m = __ballot(x < W && row[min(x, W - 1)] != 0);
        if (m) lo = min(lo, x0 + __builtin_ctzll(m)), hi = x0 + 63 - __builtin_clzll(m);
      }
      if (lane == 0) ex[(long long)b * H + y] = make_int2(lo, hi);
    }
    acc_walk_extents(plane, H, W, W, ey + (long long)b * W, s_lo, s_hi);
  } else {
    const int r = b - N * D, n = r / H, y = r % H;
    acc_walk_extents(occ + ((long long)n * D * H + y) * W, D, (long long)H * W, W, ez + (long long)r * W, s_lo, s_hi);
  }
}

// ---------------------------------------------------------------------------------------------
// Access table
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(ACC_NTHR) void access_init_kernel(long long* __restrict__ acc, long long T) {
  const long long i = (long long)blockIdx.x * ACC_NTHR + threadIdx.x;
  if (i < T * ACC_NCOL) acc[i] = 0;
}

// The instance pass of instance_pass.h.  ids int32 [N*V]: per-sample ids from 1, 0 = none; offsets
// int64 [N+1]: the rows of each sample (ip_row).  A run of one row number along a row of W takes its
// x counts from the run's ends and the row's extents, the others as popcounts of the bits' ballots
// under the run's lanes; each occupied slot adds its non-zero counters to acc.  mask uint8 [N*V] or
// null: the six bits of every voxel, 0 where it counts nowhere.
__global__ __launch_bounds__(IP_NTHR) void access_stats_kernel(const int* __restrict__ ids,
                                                              const long long* __restrict__ offsets,
                                                              const int2* __restrict__ ex,
                                                              const int2* __restrict__ ey,
                                                              const int2* __restrict__ ez, uint8_t* __restrict__ mask,
                                                              long long* acc, int total, int V, int D, int H, int W,
                                                              int T, unsigned rV, unsigned rH, unsigned rW) {
  __shared__ int s_gid[IP_SLOTS];
  __shared__ unsigned s_cnt[IP_SLOTS][ACC_NCOL];
  const int tid = threadIdx.x;
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) {
    s_gid[s] = 0;
#pragma unroll
    for (int k = 0; k < ACC_NCOL; ++k) s_cnt[s][k] = 0;
  }
  __syncthreads();
  for (int it = 0; it < IP_CHUNK / IP_NTHR; ++it) {
    const auto [g, valid] = ip_voxel(it, total);
    const int n = ip_div(g, V, rV), zy = ip_div(g, W, rW), x = g - zy * W;      // zy = (n*D + z)*H + y
    const int nz = ip_div(zy, H, rH), y = zy - nz * H, z = nz - n * D;          // nz = n*D + z
    const int gid = ip_row(offsets, n, ids[g], valid, T);
    const int2 cx = ex[zy], cy = ey[(long long)nz * W + x], cz = ez[(long long)(n * H + y) * W + x];
    const bool pz = cz.y <= z, mz = cz.x >= z, px = cx.y <= x, mx = cx.x >= x, py = cy.y <= y, my = cy.x >= y;
    const unsigned bits = pz | mz << 1 | px << 2 | mx << 3 | py << 4 | my << 5;
    if (mask && valid) mask[g] = gid > 0 ? (uint8_t)bits : (uint8_t)0;
    const unsigned long long b_pz = __ballot(pz), b_mz = __ballot(mz), b_py = __ballot(py), b_my = __ballot(my),
                             b_none = __ballot(bits == 0);
    const auto [head, len, run] = ip_run(gid, x == 0);
    if (head && gid > 0) {
      const int x1 = x + len - 1;                // the run is x .. x1 of one row: one (lo, hi) for all of it
      unsigned c[ACC_NCOL];
      c[0] = __popcll(b_pz & run), c[1] = __popcll(b_mz & run);
      c[2] = (unsigned)max(0, x1 - max(x, cx.y) + 1), c[3] = (unsigned)max(0, min(x1, cx.x) - x + 1);
      c[4] = __popcll(b_py & run), c[5] = __popcll(b_my & run);
      c[6] = __popcll(b_none & run), c[7] = (unsigned)len;
      const int slot = ip_claim(s_gid, gid);
      if (slot >= 0) {
#pragma unroll
        for (int k = 0; k < ACC_NCOL; ++k)
          if (c[k]) atomicAdd(&s_cnt[slot][k], c[k]);
      } else {
        long long* dst = acc + (long long)(gid - 1) * ACC_NCOL;
#pragma unroll
        for (int k = 0; k < ACC_NCOL; ++k)
          if (c[k]) __hip_atomic_fetch_add(&dst[k], (long long)c[k], IP_RLX_AGENT);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < IP_SLOTS * ACC_NCOL; i += IP_NTHR) {
    const int s = i / ACC_NCOL, k = i % ACC_NCOL, gid = s_gid[s];
    const unsigned cnt = s_cnt[s][k];
    if (gid > 0 && cnt)
      __hip_atomic_fetch_add(&acc[(long long)(gid - 1) * ACC_NCOL + k], (long long)cnt, IP_RLX_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------
// Entry points
// ---------------------------------------------------------------------------------------------

extern "C" void fn_access_chunk(int* t) { t[0] = IP_CHUNK, t[1] = IP_SLOTS; }

// occ uint8 [N][D][H][W]; ex int32 [N][D][H][2], ey [N][D][W][2], ez [N][H][W][2] (8-byte aligned), all
// three written in full.
extern "C" int fn_access_extents(const void* occ, void* ex, void* ey, void* ez, int N, int D, int H, int W,
                                 hipStream_t st) {
  if (!ip_shape_ok(N, D, H, W) || !occ || !ex || !ey || !ez) return -2;
  if (((uintptr_t)ex | (uintptr_t)ey | (uintptr_t)ez) % 8 != 0) return -2;
  const long long nblk = (long long)N * D + (long long)N * H;   // (< 2^32: N*D*H < 2^31)
  if (nblk >= (1LL << 31)) return -2;
  hipLaunchKernelGGL(access_extents_kernel, dim3((unsigned)nblk), dim3(ACC_NTHR), 0, st, (const uint8_t*)occ,
                     (int2*)ex, (int2*)ey, (int2*)ez, N, D, H, W);
  FN_CHECK_LAUNCH();
  return 0;
}

// ids int32 [N*V], offsets int64 [N+1], ex / ey / ez as fn_access_extents writes them; mask uint8 [N*V]
// or null; acc int64 [T][8], fully rewritten.
extern "C" int fn_access_stats(const void* ids, const void* offsets, const void* ex, const void* ey, const void* ez,
                               void* mask, void* acc, int N, int D, int H, int W, long long T, hipStream_t st) {
  if (!ip_shape_ok(N, D, H, W) || !ids || !offsets || !ex || !ey || !ez) return -2;
  if (((uintptr_t)ex | (uintptr_t)ey | (uintptr_t)ez) % 8 != 0) return -2;
  const long long V = (long long)D * H * W, total = V * N;
  if (T < 0 || T > total || (T > 0 && !acc)) return -2;
  if (T > 0) {
    hipLaunchKernelGGL(access_init_kernel, dim3((unsigned)((T * ACC_NCOL + ACC_NTHR - 1) / ACC_NTHR)), dim3(ACC_NTHR),
                       0, st, (long long*)acc, T);
    FN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(access_stats_kernel, dim3((unsigned)((total + IP_CHUNK - 1) / IP_CHUNK)), dim3(IP_NTHR), 0, st,
                     (const int*)ids, (const long long*)offsets, (const int2*)ex, (const int2*)ey, (const int2*)ez,
                     (uint8_t*)mask, (long long*)acc, (int)total, (int)V, D, H, W, (int)T, ip_recip((int)V),
                     ip_recip(H), ip_recip(W));
  FN_CHECK_LAUNCH();
  return 0;
}
