// 3-D connected-component labelling of a uint8 label volume [N][D][H][W], and the per-component
// instance table (the last stage of the segmentation pipeline: labels -> the list of features).
//
// roots int32 [N][D][H][W] holds, for every voxel, 1 + the C-order linear index (within its
// sample) of a voxel of the same component with a SMALLER OR EQUAL index -- a parent pointer, 0 for
// background -- and, once flattened, 1 + the smallest index of the component.  Phases, one launch
// each (no kernel waits on another workgroup: launch boundaries order the phases):
//   1  ccl_local_kernel    one workgroup labels one CCL_TD x CCL_TH x CCL_TW tile in LDS (union-find
//                          with min-index roots, LDS atomic-min) and writes the tile-local roots
//   2  ccl_merge_kernel    unions across tile faces in the global array (agent-scope atomic-min)
//   3  ccl_flatten_kernel  every voxel -> its root, plus the root flag roots[v] == v + 1
//   4  (caller)            rank = inclusive prefix sum of the flags = 1-based table row of each root
//   5  ccl_stats_kernel    dense ids + the table: runs of one component along W are combined in
//                          the wave (ballot), then in an LDS run table, then added to the table
// Every result is an integer that does not depend on the order of the merges or of the atomics.
#include "instance_pass.h"

constexpr int CCL_TD = 8, CCL_TH = 8, CCL_TW = 64;      // tile: 4096 voxels, one wave lane per x
constexpr int CCL_TV = CCL_TD * CCL_TH * CCL_TW;
constexpr int CCL_ROWS = CCL_TD * CCL_TH;
constexpr int CCL_NTHR = 256;
static_assert(CCL_TW == FN_WAVE && CCL_TV == CCL_NTHR * 16 && CCL_ROWS % (CCL_NTHR / FN_WAVE) == 0, "tile shape");

#define CCL_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP
#define CCL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---------------------------------------------------------------------------------------------
// Phase 1
// ---------------------------------------------------------------------------------------------

// Union of the sets of a and b in the LDS parent array (par[i] <= i, a root has par[i] == i): the
// larger root is hung under the smaller node by a returning atomic-min; when the word was not a
// root any more, the value it held is merged on.  Lanes with a == b (masked links) do nothing.
__device__ __forceinline__ void ccl_lds_union(int* par, int a, int b) {
  if (a == b) return;
  for (int p; (p = __hip_atomic_load(&par[a], CCL_RLX_WG)) != a;) a = p;
  for (int p; (p = __hip_atomic_load(&par[b], CCL_RLX_WG)) != b;) b = p;
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&par[a], b, CCL_RLX_WG);
    if (old == a) break;
    a = old;
  }
}

// CONN: 6 or 26.  Grid: N * tiles workgroups (x tiles fastest).  bg: the background class, -1 = none.
// vec: W % 16 == 0 and a 16-byte aligned base -- the tile's rows are read as one uint4 per thread.
template <int CONN>
__global__ __launch_bounds__(CCL_NTHR) void ccl_local_kernel(const uint8_t* __restrict__ labels,
                                                             int* __restrict__ roots, int D, int H, int W, int ntz,
                                                             int nty, int ntx, int bg, int vec) {
  __shared__ short lab[CCL_TV];                 // class, -1 = background or outside the volume
  __shared__ int par[CCL_TV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = ntz * nty * ntx;
  const int n = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int x0 = (t % ntx) * CCL_TW, y0 = (t / ntx % nty) * CCL_TH, z0 = (t / (ntx * nty)) * CCL_TD;
  const long long nb = (long long)n * D * H * W;

  {                                             // 16 voxels of one row per thread
    const int row = tid >> 2, q = (tid & 3) * 16;
    const int gz = z0 + row / CCL_TH, gy = y0 + row % CCL_TH, gx = x0 + q;
    const bool rowok = gz < D && gy < H;
    const uint8_t* src = labels + nb + (long long)(min(gz, D - 1) * H + min(gy, H - 1)) * W;
    uint8_t b[16];
    if (vec) {                                  // (uniform) clipped vectors read a clamped address
      const uint4 v = *(const uint4*)(src + min(gx, W - 16));
      __builtin_memcpy(b, &v, 16);
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) b[k] = src[min(gx + k, W - 1)];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const bool ok = rowok && gx + k < W && (int)b[k] != bg;
      lab[row * CCL_TW + q + k] = ok ? (short)b[k] : (short)-1;
    }
  }
  __syncthreads();
  // runs along x: every voxel starts under the first voxel of its run (one ballot per row)
#pragma unroll 4
  for (int r = wave; r < CCL_ROWS; r += CCL_NTHR / FN_WAVE) {
    const int i = r * CCL_TW + lane;
    const int l = lab[i], ll = lab[i - (lane > 0)];
    const unsigned long long heads = __ballot(lane == 0 || l != ll || l < 0);
    par[i] = r * CCL_TW + 63 - __clzll(heads & (~0ull >> (63 - lane)));
  }
  __syncthreads();
  // links to the earlier rows: (dz, dy) = (0,-1), (-1,0) and, for 26, (-1,-1), (-1,+1), x-1 .. x+1
  // each.  Out-of-tile rows and columns read a clamped address and are masked.  A voxel whose
  // left neighbour is in its run repeats none of the links that neighbour (or one further left)
  // already makes: see the op layer's notes.
  constexpr int NOFF = CONN == 26 ? 4 : 2;
  for (int r = wave; r < CCL_ROWS; r += CCL_NTHR / FN_WAVE) {
    const int i = r * CCL_TW + lane, lz = r / CCL_TH, ly = r % CCL_TH;
    const int l = lab[i];
    const bool L = lane > 0 && l >= 0 && lab[i - (lane > 0)] == l;
#pragma unroll
    for (int o = 0; o < NOFF; ++o) {
      const int dz = o == 0 ? 0 : -1, dy = o == 0 ? -1 : o == 1 ? 0 : o == 2 ? -1 : 1;
      const int nz = lz + dz, ny = ly + dy;
      const bool inb = nz >= 0 && ny >= 0 && ny < CCL_TH && l >= 0;
      const int j = (inb ? nz * CCL_TH + ny : r) * CCL_TW + lane;
      const bool cm = inb && lane > 0 && lab[j - (lane > 0)] == l;
      const bool c0 = inb && lab[j] == l;
      if (CONN == 26) {
        const bool cp = inb && lane < 63 && lab[j + (lane < 63)] == l;
        ccl_lds_union(par, i, c0 && !L ? j : i);
        ccl_lds_union(par, i, cm && !c0 && !L ? j - 1 : i);
        ccl_lds_union(par, i, cp && !c0 ? j + 1 : i);
      } else {
        ccl_lds_union(par, i, c0 && !(L && cm) ? j : i);
      }
    }
  }
  __syncthreads();
  for (int r = wave; r < CCL_ROWS; r += CCL_NTHR / FN_WAVE) {
    const int i = r * CCL_TW + lane;
    int a = i;
    for (int p; (p = par[a]) != a;) a = p;
    const int gz = z0 + r / CCL_TH, gy = y0 + r % CCL_TH, gx = x0 + lane;
    const int rz = z0 + a / (CCL_TH * CCL_TW), ry = y0 + a / CCL_TW % CCL_TH, rx = x0 + a % CCL_TW;
    if (gz < D && gy < H && gx < W)
      roots[nb + (long long)(gz * H + gy) * W + gx] = lab[i] >= 0 ? (rz * H + ry) * W + rx + 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------
// Phase 2
// ---------------------------------------------------------------------------------------------

// Root of voxel a in one sample's parent array R (values are index + 1), read with relaxed
// agent-scope loads: a stale parent is an older ancestor, which costs another step only.  A word
// that is no smaller parent (a root, or not a parent pointer at all) ends the walk: it cannot
// leave [0, a] or loop.
__device__ __forceinline__ int ccl_find_agent(int* R, int a) {
  for (;;) {
    const int p = __hip_atomic_load(&R[a], CCL_RLX_AGENT) - 1;
    if (p < 0 || p >= a) return a;
    a = p;
  }
}

__device__ __forceinline__ void ccl_global_union(int* R, int a, int b) {
  a = ccl_find_agent(R, a);
  b = ccl_find_agent(R, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&R[a], b + 1, CCL_RLX_AGENT) - 1;
    if (old == a || old < 0) break;
    a = old;
  }
}

// One thread per voxel of a tile face's upper side: per sample fx voxels with x = k*TW, then fy with
// y = k*TH, then fz with z = k*TD (k >= 1), each facing 1 (CONN 6) or 9 (CONN 26) neighbours on the
// other side of that face.  A pair that straddles two faces is visited from both: harmless.
// The face is walked in rows along its run axis (x; y on an x face), and ccl_local's rule drops the
// unions a run makes twice: with the previous voxel of the row in this voxel's class AND tile (L),
// and the facing row's cm / c0 / cp as there, a union is left out only where links inside one tile
// and the unions of earlier voxels of the same row imply it (lm / rm: the facing row's previous /
// next voxel is in the facing voxel's tile).  A solid face makes one union per tile row, not one per
// voxel, all onto one root word.
template <int CONN>
__global__ __launch_bounds__(CCL_NTHR) void ccl_merge_kernel(const uint8_t* __restrict__ labels, int* roots, int N,
                                                             int D, int H, int W, int bg, long long fx, long long fy,
                                                             long long fz) {
  const long long per = fx + fy + fz, t = (long long)blockIdx.x * CCL_NTHR + threadIdx.x;
  if (t >= per * N) return;
  const int n = (int)(t / per);
  long long f = t % per;
  int dir, z, y, x;
  if (f < fx) {
    dir = 0;
    const int k = (int)(f / ((long long)D * H)), rem = (int)(f % ((long long)D * H));
    x = (k + 1) * CCL_TW, z = rem / H, y = rem % H;
  } else if (f < fx + fy) {
    dir = 1, f -= fx;
    const int k = (int)(f / ((long long)D * W)), rem = (int)(f % ((long long)D * W));
    y = (k + 1) * CCL_TH, z = rem / W, x = rem % W;
  } else {
    dir = 2, f -= fx + fy;
    const int k = (int)(f / ((long long)H * W)), rem = (int)(f % ((long long)H * W));
    z = (k + 1) * CCL_TD, y = rem / W, x = rem % W;
  }
  const long long nb = (long long)n * D * H * W;
  const uint8_t* lab = labels + nb;
  int* R = roots + nb;
  const int v = (z * H + y) * W + x, me = lab[v];
  const bool fg = me != bg;
  // run axis (coordinate, extent, tile extent, stride), the third axis, the stride across the face
  const int cr = dir == 0 ? y : x, nr = dir == 0 ? H : W, tr = dir == 0 ? CCL_TH : CCL_TW, sr = dir == 0 ? W : 1;
  const int ca = dir == 2 ? y : z, na = dir == 2 ? H : D, sa = dir == 2 ? W : H * W;
  const int sd = dir == 0 ? 1 : dir == 1 ? W : H * W;
  const bool hasl = cr > 0, hasr = cr + 1 < nr, lm = cr % tr != 0, rm = (cr + 1) % tr != 0;
  const bool L = fg && lm && (int)lab[v - (hasl ? sr : 0)] == me;
  constexpr int SPAN = CONN == 26 ? 1 : 0;
#pragma unroll
  for (int a = -SPAN; a <= SPAN; ++a) {
    const bool aok = fg && ca + a >= 0 && ca + a < na;
    const int u = v - sd + (aok ? a * sa : 0);  // (masked rows and columns read a clamped address)
    const bool cm = aok && hasl && (int)lab[u - (hasl ? sr : 0)] == me;
    const bool c0 = aok && (int)lab[u] == me;
    if (CONN == 26) {
      const bool cp = aok && hasr && (int)lab[u + (hasr ? sr : 0)] == me;
      if (c0 && !L) ccl_global_union(R, v, u);
      if (cm && !L && !(c0 && lm)) ccl_global_union(R, v, u - sr);
      if (cp && !(c0 && rm)) ccl_global_union(R, v, u + sr);
    } else {
      if (c0 && !(L && cm)) ccl_global_union(R, v, u);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Phase 3
// ---------------------------------------------------------------------------------------------

// roots[v] <- root of v, flags[v] <- roots[v] == v + 1.  Plain loads: the merges ended with the
// previous launch, and a word another thread of this launch has already flattened holds its root.
__global__ __launch_bounds__(CCL_NTHR) void ccl_flatten_kernel(int* roots, int* __restrict__ flags, long long total,
                                                               int V) {
  const long long g0 = (long long)blockIdx.x * CCL_NTHR;
  const long long g = g0 + threadIdx.x;
  if (g >= total) return;
  const long long nb0 = g0 / V * V;             // (uniform) sample base of the workgroup's first voxel
  long long nb = nb0;
  while (g - nb >= V) nb += V;
  const int v = (int)(g - nb);
  int* R = roots + nb;
  int r = R[v];
  if (r < 0 || r > v + 1) r = v + 1;            // (not a parent pointer: its own root)
  if (r > 0) {
    int a = r - 1;
    for (;;) {
      const int p = R[a] - 1;
      if (p < 0 || p >= a) break;
      a = p;
    }
    r = a + 1;
  }
  R[v] = r;
  flags[g] = r == v + 1;
}

// ---------------------------------------------------------------------------------------------
// Phase 5
// ---------------------------------------------------------------------------------------------

constexpr int CCL_NCOL = 13;                    // sample class voxels root z0 y0 x0 z1 y1 x1 sum_z sum_y sum_x

__global__ __launch_bounds__(CCL_NTHR) void ccl_table_init_kernel(long long* __restrict__ table, long long T) {
  const long long i = (long long)blockIdx.x * CCL_NTHR + threadIdx.x;
  if (i >= T * CCL_NCOL) return;
  const int c = (int)(i % CCL_NCOL);
  table[i] = c >= 4 && c <= 6 ? 0x7fffffffLL : c >= 7 && c <= 9 ? -1LL : 0LL;
}

__device__ __forceinline__ void ccl_row_add(long long* row, long long cnt, int z0, int y0, int x0, int z1, int y1,
                                            int x1, long long sz, long long sy, long long sx) {
  __hip_atomic_fetch_add(&row[2], cnt, CCL_RLX_AGENT);
  __hip_atomic_fetch_min(&row[4], (long long)z0, CCL_RLX_AGENT);
  __hip_atomic_fetch_min(&row[5], (long long)y0, CCL_RLX_AGENT);
  __hip_atomic_fetch_min(&row[6], (long long)x0, CCL_RLX_AGENT);
  __hip_atomic_fetch_max(&row[7], (long long)z1, CCL_RLX_AGENT);
  __hip_atomic_fetch_max(&row[8], (long long)y1, CCL_RLX_AGENT);
  __hip_atomic_fetch_max(&row[9], (long long)x1, CCL_RLX_AGENT);
  __hip_atomic_fetch_add(&row[10], sz, CCL_RLX_AGENT);
  __hip_atomic_fetch_add(&row[11], sy, CCL_RLX_AGENT);
  __hip_atomic_fetch_add(&row[12], sx, CCL_RLX_AGENT);
}

// The instance pass of instance_pass.h.  rank[g]: inclusive prefix sum of the root flags = 1-based
// table row of root g, so a voxel's row is rank[its root], checked against [1, T].  A run of one
// component along a row of W is one table update from the run's start and length alone, so a
// large component issues one set of global atomics per workgroup, not per voxel.
__global__ __launch_bounds__(IP_NTHR) void ccl_stats_kernel(const uint8_t* __restrict__ labels,
                                                            const int* __restrict__ roots,
                                                            const int* __restrict__ rank, int* __restrict__ ids,
                                                            long long* __restrict__ table, int total, int V, int H,
                                                            int W, int T, unsigned rV, unsigned rH, unsigned rW) {
  __shared__ int s_gid[IP_SLOTS];
  __shared__ int s_mm[IP_SLOTS][6];
  __shared__ unsigned long long s_sum[IP_SLOTS][4];
  const int tid = threadIdx.x;
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) {
    s_gid[s] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) s_mm[s][k] = 0x7fffffff, s_mm[s][3 + k] = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) s_sum[s][k] = 0;
  }
  __syncthreads();
  for (int it = 0; it < IP_CHUNK / IP_NTHR; ++it) {
    const auto [g, valid] = ip_voxel(it, total);
    const int n = ip_div(g, V, rV), v = g - n * V;
    const int zy = ip_div(v, W, rW), x = v - zy * W, z = ip_div(zy, H, rH), y = zy - z * H;
    const int r = roots[g];
    const bool fg = valid && r > 0 && r <= V;
    const int gid0 = rank[fg ? n * V + r - 1 : g];
    const bool on = fg && gid0 >= 1 && gid0 <= T;
    const int gid = on ? gid0 : 0;
    const int base = n > 0 ? rank[n * V - 1] : 0;          // rows of the samples before this one
    if (ids && valid) ids[g] = on ? gid - base : 0;
    if (on && r == v + 1) {                      // the root voxel: the columns nobody accumulates
      long long* row = table + (long long)(gid - 1) * CCL_NCOL;
      row[0] = n, row[1] = labels[g], row[3] = r;
    }
    const IpRun run = ip_run(gid, x == 0);
    if (run.head && gid > 0) {
      const int len = run.len, x1 = x + len - 1, slot = ip_claim(s_gid, gid);
      const long long cnt = len, sx = (long long)len * x + (long long)len * (len - 1) / 2;
      if (slot >= 0) {
        atomicMin(&s_mm[slot][0], z), atomicMin(&s_mm[slot][1], y), atomicMin(&s_mm[slot][2], x);
        atomicMax(&s_mm[slot][3], z), atomicMax(&s_mm[slot][4], y), atomicMax(&s_mm[slot][5], x1);
        atomicAdd(&s_sum[slot][0], (unsigned long long)cnt);
        atomicAdd(&s_sum[slot][1], (unsigned long long)(cnt * z));
        atomicAdd(&s_sum[slot][2], (unsigned long long)(cnt * y));
        atomicAdd(&s_sum[slot][3], (unsigned long long)sx);
      } else {
        ccl_row_add(table + (long long)(gid - 1) * CCL_NCOL, cnt, z, y, x, z, y, x1, cnt * z, cnt * y, sx);
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR)
    if (s_gid[s] > 0)
      ccl_row_add(table + (long long)(s_gid[s] - 1) * CCL_NCOL, (long long)s_sum[s][0], s_mm[s][0], s_mm[s][1],
                  s_mm[s][2], s_mm[s][3], s_mm[s][4], s_mm[s][5], (long long)s_sum[s][1], (long long)s_sum[s][2],
                  (long long)s_sum[s][3]);
}

// ---------------------------------------------------------------------------------------------
// Entry points.  labels uint8 [N][D][H][W]; roots, flags, rank, ids int32 of the same shape;
// background: the class that forms no component, -1 = none; connectivity 6 or 26.
// ---------------------------------------------------------------------------------------------

static bool ccl_shape_ok(int N, int D, int H, int W) {
  return N >= 1 && D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W < (1LL << 31);
}
static long long ccl_ntiles(int D, int H, int W) {
  return (long long)((D + CCL_TD - 1) / CCL_TD) * ((H + CCL_TH - 1) / CCL_TH) * ((W + CCL_TW - 1) / CCL_TW);
}

extern "C" void fn_ccl_tile(int* t) { t[0] = CCL_TD, t[1] = CCL_TH, t[2] = CCL_TW; }

extern "C" int fn_ccl_local(const void* labels, void* roots, int N, int D, int H, int W, int background,
                            int connectivity, hipStream_t st) {
  if (!ccl_shape_ok(N, D, H, W) || !labels || !roots || background < -1 || background > 255) return -2;
  if (connectivity != 6 && connectivity != 26) return -2;
  const long long nblk = ccl_ntiles(D, H, W) * N;
  if (nblk >= (1LL << 31)) return -2;
  const int vec = W % 16 == 0 && (uintptr_t)labels % 16 == 0;
  const int ntz = (D + CCL_TD - 1) / CCL_TD, nty = (H + CCL_TH - 1) / CCL_TH, ntx = (W + CCL_TW - 1) / CCL_TW;
  if (connectivity == 6)
    hipLaunchKernelGGL(ccl_local_kernel<6>, dim3((unsigned)nblk), dim3(CCL_NTHR), 0, st, (const uint8_t*)labels,
                       (int*)roots, D, H, W, ntz, nty, ntx, background, vec);
  else
    hipLaunchKernelGGL(ccl_local_kernel<26>, dim3((unsigned)nblk), dim3(CCL_NTHR), 0, st, (const uint8_t*)labels,
                       (int*)roots, D, H, W, ntz, nty, ntx, background, vec);
  FN_CHECK_LAUNCH();
  return 0;
}

extern "C" int fn_ccl_merge(const void* labels, void* roots, int N, int D, int H, int W, int background,
                            int connectivity, hipStream_t st) {
  if (!ccl_shape_ok(N, D, H, W) || !labels || !roots || background < -1 || background > 255) return -2;
  if (connectivity != 6 && connectivity != 26) return -2;
  const long long fx = (long long)((W - 1) / CCL_TW) * D * H, fy = (long long)((H - 1) / CCL_TH) * D * W,
                  fz = (long long)((D - 1) / CCL_TD) * H * W;
  const long long nblk = ((fx + fy + fz) * N + CCL_NTHR - 1) / CCL_NTHR;
  if (nblk >= (1LL << 31)) return -2;
  if (nblk == 0) return 0;                      // one tile per sample: nothing to merge
  if (connectivity == 6)
    hipLaunchKernelGGL(ccl_merge_kernel<6>, dim3((unsigned)nblk), dim3(CCL_NTHR), 0, st, (const uint8_t*)labels,
                       (int*)roots, N, D, H, W, background, fx, fy, fz);
  else
    hipLaunchKernelGGL(ccl_merge_kernel<26>, dim3((unsigned)nblk), dim3(CCL_NTHR), 0, st, (const uint8_t*)labels,
                       (int*)roots, N, D, H, W, background, fx, fy, fz);
  FN_CHECK_LAUNCH();
  return 0;
}

extern "C" int fn_ccl_flatten(void* roots, void* flags, int N, int D, int H, int W, hipStream_t st) {
  if (!ccl_shape_ok(N, D, H, W) || !roots || !flags) return -2;
  const long long V = (long long)D * H * W, total = V * N, nblk = (total + CCL_NTHR - 1) / CCL_NTHR;
  if (nblk >= (1LL << 31)) return -2;
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3((unsigned)nblk), dim3(CCL_NTHR), 0, st, (int*)roots, (int*)flags, total,
                     (int)V);
  FN_CHECK_LAUNCH();
  return 0;
}

// rank int32 [N*V]: the inclusive prefix sum of fn_ccl_flatten's flags over the whole batch (N*V <
// 2^31); T = rank[N*V - 1] rows; table int64 [T][13], fully rewritten; ids int32 [N*V] or null.
extern "C" int fn_ccl_stats(const void* labels, const void* roots, const void* rank, void* ids, void* table, int N,
                            int D, int H, int W, long long T, hipStream_t st) {
  if (!ip_shape_ok(N, D, H, W) || !labels || !roots || !rank) return -2;
  const long long V = (long long)D * H * W, total = V * N;
  if (T < 0 || T > total || (T > 0 && !table)) return -2;
  if (T > 0) {
    hipLaunchKernelGGL(ccl_table_init_kernel, dim3((unsigned)((T * CCL_NCOL + CCL_NTHR - 1) / CCL_NTHR)),
                       dim3(CCL_NTHR), 0, st, (long long*)table, T);
    FN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ccl_stats_kernel, dim3((unsigned)((total + IP_CHUNK - 1) / IP_CHUNK)), dim3(IP_NTHR), 0, st,
                     (const uint8_t*)labels, (const int*)roots, (const int*)rank, (int*)ids, (long long*)table,
                     (int)total, (int)V, H, W, (int)T, ip_recip((int)V), ip_recip(H), ip_recip(W));
  FN_CHECK_LAUNCH();
  return 0;
}
