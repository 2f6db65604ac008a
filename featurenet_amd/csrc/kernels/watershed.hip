// Watershed split of touching feature instances: steepest ascent on a height volume inside each component, and
// the saddles between the basins it makes (the seventh instance pass).
//
// ids int32 [N][D][H][W], indexed [n][z][y][x]: a voxel with ids > 0 belongs to that component of its sample;
// height int32 of the same shape, h(v) = max(height[v], 0) (in the pipeline the squared distance to the material).
// key(v) = h(v) << 32 | (0xFFFFFFFF - index of v in its sample): higher wins, then the lower index.  u is a
// neighbour of v when it is one of its 26 neighbours in the grid and the sample with ids[u] == ids[v];
// parent(v) is the neighbour of the largest key when that key exceeds key(v), else v.  Keys are distinct and
// grow along the parents: the chains end, at a root, after fewer than V steps.  One launch each:
//   1  ws_ascend_kernel    parent int32 (1 + index in the sample, 0 where ids <= 0)
//   2  ws_resolve_kernel   roots (1 + the index of the chain's end) and the root flags roots[v] == v + 1
//   3  (caller)            ccl_stats over roots and flags: basin ids, the basin table, offsets
//   4  ws_saddle_kernel    per pair of basins of one component that touch, the largest min(h(u), h(v)) over
//                          their 26-adjacent voxel pairs (u, v), in the pair table of pair_table.h
// Every result is an integer that does not depend on execution order.
#include "pair_table.h"

constexpr int WS_MAX_S = 256;                   // longest axis
constexpr int WS_TD = 8, WS_TH = 8, WS_TW = 64; // tile: 4096 voxels, one wave lane per x
constexpr int WS_NTHR = 256;
constexpr int WS_ROWS = WS_TD * WS_TH;
constexpr int WS_HD = WS_TD + 2, WS_HH = WS_TH + 2, WS_HW = WS_TW + 2;      // the tile and a one-voxel halo
constexpr int WS_HV = WS_HD * WS_HH * WS_HW;
static_assert(WS_TW == FN_WAVE && WS_ROWS % (WS_NTHR / FN_WAVE) == 0, "tile shape");
static_assert(2 * WS_HV * sizeof(int) <= 64 * 1024, "the staged tile fits the LDS of a workgroup");

// ---------------------------------------------------------------------------------------------
// Phase 1
// ---------------------------------------------------------------------------------------------

// The 27 positions round a voxel in ascending order of their index (the voxel itself in the middle), each one
// taken only when its height is strictly above the best so far: the first of the highest wins, which is the
// largest (h, ~index) without a 64-bit key, and the voxel keeps itself unless a higher one, or an equally high
// one of a lower index, is its neighbour.  ok(j) / h(j): position j = (dz + 1) * 9 + (dy + 1) * 3 + dx + 1 is a
// neighbour (or the voxel), and its height.  -> the index offset (dz * H + dy) * W + dx of the winner.
template <typename OK, typename HT>
__device__ __forceinline__ int ws_steepest(OK ok, HT h, int H, int W) {
  int best_h = -1, best_o = 0;
#pragma unroll
  for (int j = 0; j < 27; ++j) {
    const int dz = j / 9 - 1, dy = j / 3 % 3 - 1, dx = j % 3 - 1;
    if (!ok(j)) continue;
    const int hu = h(j);
    if (hu > best_h) best_h = hu, best_o = (dz * H + dy) * W + dx;
  }
  return best_o;
}

// Grid: N * tiles workgroups (x tiles fastest).  The heights (clamped at 0) and ids of the tile and its halo
// are staged in LDS: a halo voxel's address is formed from clamped coordinates, and outside the grid its id
// is 0, which no voxel that ascends carries -- so the grid's edge, the sample's end and another component
// all fail one comparison.  A voxel is read from global memory once per tile whose halo holds it (1.6 times on
// average), not 27 times, and every parent is written by one lane: no atomics, no initialising launch.
__global__ __launch_bounds__(WS_NTHR) void ws_ascend_kernel(const int* __restrict__ ids,
                                                            const int* __restrict__ height,
                                                            int* __restrict__ parent, int D, int H, int W, int ntz,
                                                            int nty, int ntx) {
  __shared__ int s_h[WS_HV];
  __shared__ int s_id[WS_HV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = ntz * nty * ntx;
  const int n = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int x0 = (t % ntx) * WS_TW, y0 = (t / ntx % nty) * WS_TH, z0 = (t / (ntx * nty)) * WS_TD;
  const long long nb = (long long)n * D * H * W;
  const auto halo = [&](int i, bool& in) {       // the address of halo position i, from clamped coordinates
    const int lx = i % WS_HW, r = i / WS_HW, ly = r % WS_HH, lz = r / WS_HH;
    const int gz = z0 - 1 + lz, gy = y0 - 1 + ly, gx = x0 - 1 + lx;
    in = gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W;
    return nb + (min(max(gz, 0), D - 1) * H + min(max(gy, 0), H - 1)) * W + min(max(gx, 0), W - 1);
  };
  bool any = false;
  for (int i = tid; i < WS_HV; i += WS_NTHR) {
    bool in;
    const int id = ids[halo(i, in)];
    s_id[i] = in ? id : 0;
    any = any || (in && id > 0);
  }
  // A tile without an id (most of a part is material) writes its zeros and is done: no height is read.  The
  // barrier's result is the same on every lane, so the workgroup leaves or stays as one.
  const bool work = __syncthreads_or(any);
  if (work) {
    for (int i = tid; i < WS_HV; i += WS_NTHR) {
      bool in;
      s_h[i] = max(height[halo(i, in)], 0);
    }
    __syncthreads();
  }
  for (int r = wave; r < WS_ROWS; r += WS_NTHR / FN_WAVE) {
    const int lz = r / WS_TH, ly = r % WS_TH;
    const int gz = z0 + lz, gy = y0 + ly, gx = x0 + lane;
    if (gz >= D || gy >= H || gx >= W) continue;
    const int c = ((lz + 1) * WS_HH + ly + 1) * WS_HW + lane + 1;
    const int id = s_id[c], v = (gz * H + gy) * W + gx;
    int o = 0;
    if (work && id > 0) {
      const auto at = [&](int j) { return c + ((j / 9 - 1) * WS_HH + j / 3 % 3 - 1) * WS_HW + j % 3 - 1; };
      o = ws_steepest([&](int j) { return s_id[at(j)] == id; }, [&](int j) { return s_h[at(j)]; }, H, W);
    }
    parent[nb + v] = id > 0 ? v + o + 1 : 0;
  }
}

// The same parents from global memory alone, one lane per voxel of the flat range and 27 reads of each array
// (through the caches): what ws_ascend_kernel is measured against (profiles/feature_split.md).  A neighbour's
// address is the voxel's own plus a stride that is taken only where the voxel's coordinates say the neighbour
// lies in the grid.
__global__ __launch_bounds__(WS_NTHR) void ws_ascend_plain_kernel(const int* __restrict__ ids,
                                                                  const int* __restrict__ height,
                                                                  int* __restrict__ parent, long long total, int V,
                                                                  int D, int H, int W) {
  const long long g = (long long)blockIdx.x * WS_NTHR + threadIdx.x;
  if (g >= total) return;
  const int v = (int)(g % V), x = v % W, y = v / W % H, z = v / (W * H);
  const int id = ids[g];
  if (id <= 0) {
    parent[g] = 0;
    return;
  }
  const auto in = [&](int j) {
    const int uz = z + j / 9 - 1, uy = y + j / 3 % 3 - 1, ux = x + j % 3 - 1;
    return uz >= 0 && uz < D && uy >= 0 && uy < H && ux >= 0 && ux < W;
  };
  const auto at = [&](int j) { return g + (in(j) ? ((j / 9 - 1) * H + j / 3 % 3 - 1) * W + j % 3 - 1 : 0); };
  const int o = ws_steepest([&](int j) { return in(j) && ids[at(j)] == id; },
                            [&](int j) { return max(height[at(j)], 0); }, H, W);
  parent[g] = v + o + 1;
}

// ---------------------------------------------------------------------------------------------
// Phase 2
// ---------------------------------------------------------------------------------------------

// roots[v] <- 1 + the end of v's chain of parents, flags[v] <- roots[v] == v + 1.  parent is only read and
// roots / flags are buffers of their own: no races.  A word outside [1, V] is no parent pointer: it ends the
// walk with root 0 (as the 0 of a voxel without id does) and is never used as an address; a walk of V reads
// without an end (chains of real parents are shorter) gives root 0 too.
__global__ __launch_bounds__(WS_NTHR) void ws_resolve_kernel(const int* __restrict__ parent, int* __restrict__ roots,
                                                             int* __restrict__ flags, long long total, int V) {
  const long long g = (long long)blockIdx.x * WS_NTHR + threadIdx.x;
  if (g >= total) return;
  const long long nb = g / V * V;
  const int v = (int)(g - nb);
  const int* P = parent + nb;
  int a = v, r = 0;
  for (int step = 0; step < V; ++step) {
    const int p = P[a];
    if (p < 1 || p > V) break;
    if (p - 1 == a) {
      r = p;
      break;
    }
    a = p - 1;
  }
  roots[g] = r;
  flags[g] = r == v + 1;
}

// ---------------------------------------------------------------------------------------------
// Phase 4
// ---------------------------------------------------------------------------------------------

// The instance pass of instance_pass.h, over bids (the basin ids ccl_stats wrote) and the basin table's offsets.
// A voxel v with ids[v] > 0 whose basin row lies in [1, T] looks at its 13 forward neighbours u, (dz, dy, dx) >
// (0, 0, 0), so each adjacent pair is seen once: in the grid (the address is formed only then), of another
// basin, of the same component, the basin's row in [1, T] too.  Such a pair puts min(h(u), h(v)) under the key
// row_lo << 32 | row_hi (1-based rows, below 2^31: the key is not 0 and below 2^63) with a maximum, in the
// workgroup's LDS stage first.  Most voxels have every neighbour in their own basin and stop at the first
// comparison; nothing here is a ballot, so lanes leave early.
__global__ __launch_bounds__(IP_NTHR) void ws_saddle_kernel(const int* __restrict__ ids, const int* __restrict__ bids,
                                                            const long long* __restrict__ offsets,
                                                            const int* __restrict__ height, unsigned long long* keys,
                                                            long long* counts, long long* lost, int total, int V,
                                                            int D, int H, int W, int T, unsigned long long mask,
                                                            long long bound, unsigned rV, unsigned rH, unsigned rW) {
  __shared__ unsigned long long s_key[IP_SLOTS];
  __shared__ unsigned long long s_val[IP_SLOTS];
  const int tid = threadIdx.x;
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) s_key[s] = 0, s_val[s] = 0;
  __syncthreads();
  for (int it = 0; it < IP_CHUNK / IP_NTHR; ++it) {
    const auto [g, valid] = ip_voxel(it, total);
    const int id = ids[g];
    if (!valid || id <= 0) continue;             // (material, most of a part: nothing else is read or divided)
    const int n = ip_div(g, V, rV), zy = ip_div(g, W, rW), x = g - zy * W;      // zy = (n*D + z)*H + y
    const int nz = ip_div(zy, H, rH), y = zy - nz * H, z = nz - n * D;          // nz = n*D + z
    const int bid = bids[g];
    const int gid = ip_row(offsets, n, bid, valid, T);
    if (gid == 0) continue;
    const long long off = offsets[n];
    const int hv = max(height[g], 0);
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      const int dz = k >= 4, dy = k == 0 ? 0 : k < 4 ? 1 : (k - 4) / 3 - 1, dx = k == 0 ? 1 : k < 4 ? k - 2 : (k - 4) % 3 - 1;
      if (z + dz >= D || y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W) continue;
      const int u = g + (dz * H + dy) * W + dx;
      const int bu = bids[u];
      if (bu == bid || bu <= 0 || ids[u] != id) continue;
      const long long rb = off + bu;
      if (rb < 1 || rb > T) continue;
      const unsigned long long lo = rb < gid ? rb : gid, hi = rb < gid ? gid : rb;
      const unsigned long long key = lo << 32 | hi;
      const long long val = min(hv, max(height[u], 0));
      if (!pt_stage_max(s_key, s_val, key, (unsigned long long)val))
        pt_global_max(keys, counts, lost, mask, bound, key, val);
    }
  }
  __syncthreads();
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR)
    if (s_key[s] != 0) pt_global_max(keys, counts, lost, mask, bound, s_key[s], (long long)s_val[s]);
}

// ---------------------------------------------------------------------------------------------
// Entry points.  ids, height, parent, roots, flags, bids int32 [N][D][H][W], each axis at most 256 and N*D*H*W
// < 2^31.
// ---------------------------------------------------------------------------------------------

static bool ws_shape_ok(int N, int D, int H, int W) {
  return ip_shape_ok(N, D, H, W) && D <= WS_MAX_S && H <= WS_MAX_S && W <= WS_MAX_S;
}

extern "C" void fn_ws_tile(int* t) { t[0] = WS_TD, t[1] = WS_TH, t[2] = WS_TW, t[3] = IP_CHUNK, t[4] = IP_SLOTS; }

// parent is written in full.  staged: 1 the tile kernel, 0 the plain one (the same parents).
extern "C" int fn_ws_ascend(const void* ids, const void* height, void* parent, int N, int D, int H, int W, int staged,
                            hipStream_t st) {
  if (!ws_shape_ok(N, D, H, W) || !ids || !height || !parent || staged < 0 || staged > 1) return -2;
  const long long V = (long long)D * H * W, total = V * N;
  if (staged) {
    const int ntz = (D + WS_TD - 1) / WS_TD, nty = (H + WS_TH - 1) / WS_TH, ntx = (W + WS_TW - 1) / WS_TW;
    const long long nblk = (long long)ntz * nty * ntx * N;
    if (nblk >= (1LL << 31)) return -2;
    hipLaunchKernelGGL(ws_ascend_kernel, dim3((unsigned)nblk), dim3(WS_NTHR), 0, st, (const int*)ids,
                       (const int*)height, (int*)parent, D, H, W, ntz, nty, ntx);
  } else {
    hipLaunchKernelGGL(ws_ascend_plain_kernel, dim3((unsigned)((total + WS_NTHR - 1) / WS_NTHR)), dim3(WS_NTHR), 0, st,
                       (const int*)ids, (const int*)height, (int*)parent, total, (int)V, D, H, W);
  }
  FN_CHECK_LAUNCH();
  return 0;
}

// roots and flags are written in full; neither may be parent's buffer.
extern "C" int fn_ws_resolve(const void* parent, void* roots, void* flags, int N, int D, int H, int W,
                             hipStream_t st) {
  if (!ws_shape_ok(N, D, H, W) || !parent || !roots || !flags || parent == roots || parent == flags) return -2;
  const long long V = (long long)D * H * W, total = V * N;
  hipLaunchKernelGGL(ws_resolve_kernel, dim3((unsigned)((total + WS_NTHR - 1) / WS_NTHR)), dim3(WS_NTHR), 0, st,
                     (const int*)parent, (int*)roots, (int*)flags, total, (int)V);
  FN_CHECK_LAUNCH();
  return 0;
}

// offsets int64 [N+1]: the basin table's; keys uint64 [cap], counts int64 [cap] and lost int64 [1] are zero on
// entry.  T rows (T <= N*V < 2^31); cap: a power of two in [2, 2^32]; probe >= 1: an update gives up (-> lost)
// after min(cap, probe) slots.
extern "C" int fn_ws_saddle(const void* ids, const void* bids, const void* offsets, const void* height, void* keys,
                            void* counts, void* lost, int N, int D, int H, int W, long long T, long long cap,
                            long long probe, hipStream_t st) {
  if (!ws_shape_ok(N, D, H, W) || !ids || !bids || !offsets || !height || !keys || !counts || !lost) return -2;
  if (!pt_shape_ok(cap, probe)) return -2;
  const long long V = (long long)D * H * W, total = V * N;
  if (T < 0 || T > total) return -2;
  hipLaunchKernelGGL(ws_saddle_kernel, dim3((unsigned)((total + IP_CHUNK - 1) / IP_CHUNK)), dim3(IP_NTHR), 0, st,
                     (const int*)ids, (const int*)bids, (const long long*)offsets, (const int*)height,
                     (unsigned long long*)keys, (long long*)counts, (long long*)lost, (int)total, (int)V, D, H, W,
                     (int)T, (unsigned long long)(cap - 1), probe < cap ? probe : cap, ip_recip((int)V), ip_recip(H),
                     ip_recip(W));
  FN_CHECK_LAUNCH();
  return 0;
}
