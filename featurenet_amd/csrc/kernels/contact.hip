// Contacts of feature instances: what each instance borders, face by face (the sixth instance pass, and the
// first that looks at a voxel's neighbours).
//
// ids int32 [N][D][H][W], indexed [n][z][y][x]: per-sample ids from 1, 0 = none; occ uint8 of the same shape: a
// voxel is material when occ != 0.  Faces in the order +z -z +x -x +y -y (k = 0..5), + the high-index end.  For
// a voxel v with ids[v] > 0 and its neighbour u toward face k in the same sample, exactly one of
//   interior  u in the grid and ids[u] == ids[v]                        counted nowhere
//   wall      u in the grid, ids[u] <= 0, occ[u] != 0                   contact[row][k]
//   open      u outside the grid, or ids[u] <= 0 and occ[u] == 0        contact[row][6 + k]
//   shared    u in the grid, ids[u] > 0, ids[u] != ids[v]               contact[row][12 + k]
// holds; contact int64 [T][19], one row per row of the instance table, column 18 the voxels.  A shared face
// whose two rows a < b (1-based, both in [1, T]) is seen from a toward face k adds 1 to the pair table of
// pair_table.h under the key a << 33 | b << 3 | k: the side with the lower row emits, so each face counts
// once.  v's own occupancy does not enter.  Every result is an integer sum that does not depend on the order
// of the atomics.
#include "pair_table.h"

constexpr int CT_NCOL = 19;                     // wall x 6, open x 6, shared x 6, voxels
constexpr int CT_NWORD = (CT_NCOL + 1) / 2;
static_assert(IP_CHUNK < (1 << 16), "a workgroup's counters fit 16 bits");
constexpr int CT_WALL = 0, CT_OPEN = 1, CT_SHARED = 2, CT_NONE = 3;

__device__ __forceinline__ int ct_class(bool in, int id, int idu, unsigned occu) {
  if (!in) return CT_OPEN;
  if (idu == id) return CT_NONE;
  if (idu > 0) return CT_SHARED;
  return occu != 0 ? CT_WALL : CT_OPEN;
}

// The pair key of a shared face seen from row gid (> 0) toward face k, or 0 where this side does not emit it:
// the neighbour's row is checked against (gid, T] before it enters a key.  gid <= T < 2^30: the key is below 2^63.
__device__ __forceinline__ unsigned long long ct_key(long long off, int gid, int idu, int T, int k) {
  const long long rb = off + idu;
  return rb > gid && rb <= T ? (unsigned long long)gid << 33 | (unsigned long long)rb << 3 | (unsigned long long)k
                             : 0ull;
}

__device__ __forceinline__ void ct_pair_add(unsigned long long* s_key, unsigned long long* s_pcnt,
                                            unsigned long long* keys, long long* counts, long long* lost,
                                            unsigned long long mask, long long bound, unsigned long long key,
                                            int cnt) {
  if (!pt_stage_add(s_key, s_pcnt, key, cnt)) pt_global_add(keys, counts, lost, mask, bound, key, cnt);
}

// The instance pass of instance_pass.h.  A run of one row number along a row of W (it breaks at x == 0) has
// one id: inside it the x neighbours are interior, so only its first lane looks toward -x and only its last
// toward +x; the y and z neighbours' classes are ballots, counted under the run's lanes by its first lane.
// Every neighbour's address is the voxel's own (clamped by ip_voxel) plus a stride that is taken only where
// the voxel's coordinate says the neighbour lies in the grid; outside it the lane reads its own voxel and
// the class is `open` whatever it read.  The pair keys of the y and z sides are run-combined on their own;
// those of the x sides come one to a run.
// The LDS table holds the 19 counters of a slot as 16-bit halves of ten words: a workgroup adds at most
// IP_CHUNK = 4096 to any of them, so no half carries into the other, and 20 KB where 38 KB stood let five
// workgroups share a CU, not three (105 -> 75 us on 32 solid 64^3 volumes: profiles/feature_contacts.md).
__global__ __launch_bounds__(IP_NTHR) void contact_stats_kernel(const int* __restrict__ ids,
                                                               const uint8_t* __restrict__ occ,
                                                               const long long* __restrict__ offsets,
                                                               long long* contact, unsigned long long* keys,
                                                               long long* counts, long long* lost, int total, int V,
                                                               int D, int H, int W, int T, unsigned long long mask,
                                                               long long bound, unsigned rV, unsigned rH,
                                                               unsigned rW) {
  __shared__ int s_gid[IP_SLOTS];
  __shared__ unsigned s_cnt[IP_SLOTS][CT_NWORD];            // counter col: half (col & 1) of word col >> 1
  __shared__ unsigned long long s_key[IP_SLOTS];
  __shared__ unsigned long long s_pcnt[IP_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) {
    s_gid[s] = 0, s_key[s] = 0, s_pcnt[s] = 0;
#pragma unroll
    for (int k = 0; k < CT_NWORD; ++k) s_cnt[s][k] = 0;
  }
  __syncthreads();
  const int HW = H * W;
  for (int it = 0; it < IP_CHUNK / IP_NTHR; ++it) {
    const auto [g, valid] = ip_voxel(it, total);
    const int n = ip_div(g, V, rV), zy = ip_div(g, W, rW), x = g - zy * W;      // zy = (n*D + z)*H + y
    const int nz = ip_div(zy, H, rH), y = zy - nz * H, z = nz - n * D;          // nz = n*D + z
    const int id = ids[g];
    const long long off = offsets[n];
    const int gid = ip_row(offsets, n, id, valid, T);
    const auto [head, len, run] = ip_run(gid, x == 0);
    const bool in[6] = {z + 1 < D, z > 0, x + 1 < W, x > 0, y + 1 < H, y > 0};
    const int step[6] = {HW, -HW, 1, -1, W, -W};
    int cls[6], idn[6];                          // (a voxel that counts nowhere has no class on any side)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const bool look = k == 2 ? len == 1 : k == 3 ? head : true;              // (+x: the run's last lane)
      int idu = id;
      unsigned occu = 0;
      if (look) {
        const int u = in[k] ? g + step[k] : g;
        idu = ids[u], occu = occ[u];
      }
      cls[k] = look && gid > 0 ? ct_class(in[k], id, idu, occu) : CT_NONE;
      idn[k] = idu;
    }
    unsigned long long b[4][3];                  // +z -z +y -y by wall, open, shared
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) b[j][c] = __ballot(cls[j < 2 ? j : j + 2] == c);
    const int cls_px = __shfl(cls[2], lane + len - 1, 64);                    // (lane + len - 1 <= 63)
    if (head && gid > 0) {
      const int slot = ip_claim(s_gid, gid);
      long long* dst = contact + (long long)(gid - 1) * CT_NCOL;
      const auto add = [&](int col, unsigned c) {                              // only non-zero counters are added
        if (c == 0) return;
        if (slot >= 0)
          atomicAdd(&s_cnt[slot][col >> 1], c << ((col & 1) * 16));
        else
          __hip_atomic_fetch_add(&dst[col], (long long)c, IP_RLX_AGENT);
      };
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c)              // (a class no lane of the wave has on that side: wave-uniform)
          if (b[j][c] != 0) add(6 * c + (j < 2 ? j : j + 2), (unsigned)__popcll(b[j][c] & run));
      if (cls_px != CT_NONE) add(6 * cls_px + 2, 1u);
      if (cls[3] != CT_NONE) add(6 * cls[3] + 3, 1u);
      add(18, (unsigned)len);
    }
    // The pairs.  Within a run of one row the key is one where the neighbour's id is one: the y and z sides
    // are run-combined over that id (32 bits), and a side on which no lane of the wave shares a face is
    // skipped whole (its ballot is wave-uniform); the 64-bit key is made by the lanes that emit only.
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      if (k == 2 || k == 3) {
        if (cls[k] == CT_SHARED) {
          const unsigned long long key = ct_key(off, gid, idn[k], T, k);
          if (key != 0) ct_pair_add(s_key, s_pcnt, keys, counts, lost, mask, bound, key, 1);
        }
      } else if (b[k < 2 ? k : k - 2][CT_SHARED] != 0) {
        const unsigned long long key = cls[k] == CT_SHARED ? ct_key(off, gid, idn[k], T, k) : 0ull;
        const IpRun same = ip_run(key != 0 ? idn[k] : 0, head);
        if (same.head && key != 0) ct_pair_add(s_key, s_pcnt, keys, counts, lost, mask, bound, key, same.len);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < IP_SLOTS * CT_NCOL; i += IP_NTHR) {
    const int s = i / CT_NCOL, k = i % CT_NCOL, gid = s_gid[s];
    const unsigned c = (s_cnt[s][k >> 1] >> ((k & 1) * 16)) & 0xffffu;
    if (gid > 0 && c)
      __hip_atomic_fetch_add(&contact[(long long)(gid - 1) * CT_NCOL + k], (long long)c, IP_RLX_AGENT);
  }
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR)
    if (s_key[s] != 0) pt_global_add(keys, counts, lost, mask, bound, s_key[s], (long long)s_pcnt[s]);
}

extern "C" void fn_contact_chunk(int* t) { t[0] = IP_CHUNK, t[1] = IP_SLOTS; }

// ids int32 [N*V], occ uint8 [N*V], offsets int64 [N+1]; contact int64 [T][19], keys uint64 [cap], counts int64
// [cap] and lost int64 [1] are zero on entry and added to.  T < 2^30 (the key holds two rows and a face); cap:
// a power of two in [2, 2^32]; probe >= 1: a pair update gives up (-> lost) after min(cap, probe) slots.
extern "C" int fn_contact_stats(const void* ids, const void* occ, const void* offsets, void* contact, void* keys,
                                void* counts, void* lost, int N, int D, int H, int W, long long T, long long cap,
                                long long probe, hipStream_t st) {
  if (!ip_shape_ok(N, D, H, W) || !ids || !occ || !offsets || !keys || !counts || !lost) return -2;
  if (!pt_shape_ok(cap, probe)) return -2;
  const long long V = (long long)D * H * W, total = V * N;
  if (T < 0 || T > total || T >= (1LL << 30) || (T > 0 && !contact)) return -2;
  hipLaunchKernelGGL(contact_stats_kernel, dim3((unsigned)((total + IP_CHUNK - 1) / IP_CHUNK)), dim3(IP_NTHR), 0, st,
                     (const int*)ids, (const uint8_t*)occ, (const long long*)offsets, (long long*)contact,
                     (unsigned long long*)keys, (long long*)counts, (long long*)lost, (int)total, (int)V, D, H, W,
                     (int)T, (unsigned long long)(cap - 1), probe < cap ? probe : cap, ip_recip((int)V), ip_recip(H),
                     ip_recip(W));
  FN_CHECK_LAUNCH();
  return 0;
}
