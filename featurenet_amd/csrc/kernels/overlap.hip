// Overlap table of two instance-id volumes (the step between the instance tables of ccl.hip and the
// feature-level score): for every pair (instance a of volume A, instance b of volume B) that shares
// a voxel, the number of shared voxels.
//
// ids_a, ids_b int32 [N*V]: per-sample ids from 1, 0 = none, as ccl_stats_kernel writes them;
// off_a, off_b int64 [N+1]: the row range of each sample in the two instance tables.  A voxel g of
// sample n with both ids > 0 lies in the 1-based global rows ra = off_a[n] + ids_a[g] and rb =
// off_b[n] + ids_b[g]; its key is ra << 32 | rb (never 0, distinct across samples).  The result is
// an open-addressing hash table keys uint64 [cap] (0 = empty) / counts int64 [cap], cap a power of
// two, which the caller has zeroed: the SET of (key, count) pairs in it is exact and does not
// depend on the order of the atomics; their slots do, so the caller sorts the occupied ones.
#include "pair_table.h"

// The instance pass of instance_pass.h with a 64-bit key for the row number: a run of equal keys
// along a row of W is one update of `len` voxels, so two solid volumes make one global update per
// workgroup, not one per voxel.  The LDS table holds (key, count) and is entered at the key's hash,
// not direct-mapped: an update goes to the global table only when the PT_LPROBE slots from its
// hash on are all held by other keys.  That costs the wave a returning global atomic inside the
// loop, which a strictly direct-mapped table (PT_LPROBE = 1) pays on most rows already at ~130
// keys per chunk (59 against 46 us on the blobs of profiles/feature_match.md).
__global__ __launch_bounds__(IP_NTHR) void overlap_pairs_kernel(const int* __restrict__ ids_a,
                                                                const int* __restrict__ ids_b,
                                                                const long long* __restrict__ off_a,
                                                                const long long* __restrict__ off_b,
                                                                unsigned long long* keys, long long* counts,
                                                                long long* lost, int total, int V, int W,
                                                                unsigned long long mask, long long bound,
                                                                unsigned rV, unsigned rW) {
  __shared__ unsigned long long s_key[IP_SLOTS];
  __shared__ unsigned long long s_cnt[IP_SLOTS];
  const int tid = threadIdx.x;
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR) s_key[s] = 0, s_cnt[s] = 0;
  __syncthreads();
  for (int it = 0; it < IP_CHUNK / IP_NTHR; ++it) {
    const auto [g, valid] = ip_voxel(it, total);
    const int n = ip_div(g, V, rV), x = g - ip_div(g, W, rW) * W;           // (V is a multiple of W)
    const int a = ids_a[g], b = ids_b[g];
    const bool on = valid && a > 0 && b > 0;
    const unsigned long long ra = (unsigned long long)(off_a[n] + a), rb = (unsigned long long)(off_b[n] + b);
    const unsigned long long key = on ? (ra << 32) | (rb & 0xffffffffull) : 0ull;
    const IpRun run = ip_run(key, x == 0);
    if (run.head && key != 0) {                  // (pt_stage_add, spelt out: see pair_table.h)
      int slot = (int)(pt_mix(key) >> 55) & (IP_SLOTS - 1);
      bool met = false;
      for (int p = 0; p < PT_LPROBE && !met; ++p) {
        const unsigned long long held = atomicCAS(&s_key[slot], 0ull, key);
        met = held == 0 || held == key;
        if (met) atomicAdd(&s_cnt[slot], (unsigned long long)run.len);
        slot = (slot + 1) & (IP_SLOTS - 1);
      }
      if (!met) pt_global_add(keys, counts, lost, mask, bound, key, run.len);
    }
  }
  __syncthreads();
  for (int s = tid; s < IP_SLOTS; s += IP_NTHR)
    if (s_key[s] != 0) pt_global_add(keys, counts, lost, mask, bound, s_key[s], (long long)s_cnt[s]);
}

extern "C" void fn_overlap_chunk(int* t) { t[0] = IP_CHUNK, t[1] = IP_SLOTS; }

// keys uint64 [cap], counts int64 [cap] and lost int64 [1] are zero on entry (a key or count left
// from an earlier call is added to).  cap: a power of two in [2, 2^32]; probe >= 1: an update gives
// up (-> lost) after min(cap, probe) slots.  W: the row length, V = D*H*W voxels per sample.
extern "C" int fn_overlap_pairs(const void* ids_a, const void* ids_b, const void* off_a, const void* off_b,
                                void* keys, void* counts, void* lost, int N, long long V, int W, long long cap,
                                long long probe, hipStream_t st) {
  if (!ids_a || !ids_b || !off_a || !off_b || !keys || !counts || !lost) return -2;
  if (N < 1 || V < 1 || W < 1 || V % W != 0) return -2;
  if (cap < 2 || cap > (1LL << 32) || (cap & (cap - 1)) != 0 || probe < 1) return -2;
  if (V >= (1LL << 31) || V * N >= (1LL << 31)) return -2;
  const long long total = V * N;
  hipLaunchKernelGGL(overlap_pairs_kernel, dim3((unsigned)((total + IP_CHUNK - 1) / IP_CHUNK)), dim3(IP_NTHR), 0, st,
                     (const int*)ids_a, (const int*)ids_b, (const long long*)off_a, (const long long*)off_b,
                     (unsigned long long*)keys, (long long*)counts, (long long*)lost, (int)total, (int)V, W,
                     (unsigned long long)(cap - 1), probe < cap ? probe : cap, ip_recip((int)V), ip_recip(W));
  FN_CHECK_LAUNCH();
  return 0;
}
