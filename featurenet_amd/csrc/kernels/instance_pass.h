// The per-voxel pass under the five instance-table kernels: ccl_stats_kernel (ccl.hip),
// overlap_pairs_kernel (overlap.hip), access_stats_kernel (access.hip), edt_stats_kernel (edt.hip),
// reach_stats_kernel (reach.hip).  What they share, and what a sixth must keep:
//   * one lane per voxel; a workgroup takes IP_CHUNK consecutive voxels of the flat [N*V] range
//     (N*V < 2^31: ip_shape_ok), IP_NTHR at a time;
//   * the spare lanes of the last workgroup are clamped onto the last voxel: they read it, take part
//     in every ballot and shuffle, and update nothing (their row number or key is 0);
//   * a run -- neighbouring lanes of one wave with one row number or key -- is ONE update, made by
//     its first lane from the run's length and the ballots under its lanes;
//   * a workgroup's updates meet in an LDS table of IP_SLOTS rows first; an update whose slot is
//     held by another row goes straight to global memory, and each occupied slot is flushed once,
//     after the barrier, with relaxed agent-scope atomics;
//   * every result is an integer sum, minimum or maximum, so it does not depend on the order of
//     the updates, and nothing waits for another wave;
//   * a row number comes from the caller's tensors: it is checked against [1, T] before anything
//     else is done with it, and no address is formed from an unchecked one.
#pragma once
#include "common.h"

constexpr int IP_NTHR = 256;
constexpr int IP_CHUNK = 16 * IP_NTHR;          // voxels per workgroup
constexpr int IP_SLOTS = 512;                   // rows of the LDS table, direct-mapped by table row
static_assert((IP_SLOTS & (IP_SLOTS - 1)) == 0 && IP_NTHR % FN_WAVE == 0, "table shape");

#define IP_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// g / d for 0 <= g < 2^31 and d >= 1 from r = ip_recip(d) = floor(2^32 / d) (d >= 2): the high word
// of g * r is the quotient or one less (g * (2^32 - d*r) / (d * 2^32) < g / 2^32 < 1), which the
// remainder tells.  The passes divide every voxel's index one to three times and are bound by their
// instructions, not by memory: as plain divisions those were most of access_stats_kernel.
static inline unsigned ip_recip(int d) { return d >= 2 ? (unsigned)((1ull << 32) / (unsigned)d) : 0u; }
__device__ __forceinline__ int ip_div(int g, int d, unsigned r) {
  const unsigned q = d == 1 ? (unsigned)g : __umulhi((unsigned)g, r);
  return (int)(q + ((unsigned)g - q * (unsigned)d >= (unsigned)d));
}

// The voxel of this lane in round `it` of its workgroup's chunk.  total < 2^31 and the grid just
// covers it, so the unsigned sum is below 2^31 + IP_CHUNK and cannot wrap; a lane past the end gets
// the last voxel and valid = false.
struct IpVoxel {
  int g;
  bool valid;
};
__device__ __forceinline__ IpVoxel ip_voxel(int it, int total) {
  const unsigned gu = blockIdx.x * (unsigned)IP_CHUNK + (unsigned)(it * IP_NTHR) + threadIdx.x;
  const bool valid = gu < (unsigned)total;
  return {valid ? (int)gu : total - 1, valid};
}

// The 1-based table row offsets[n] + id of a voxel with id > 0 in sample n, or 0 where the voxel
// counts nowhere: a spare lane, no id, or a row outside [1, T].
__device__ __forceinline__ int ip_row(const long long* __restrict__ offsets, int n, int id, bool valid, int T) {
  const long long row = offsets[n] + id;
  return valid && id > 0 && row >= 1 && row <= T ? (int)row : 0;
}

// Runs of one key within the wave.  A lane is a head at lane 0, where brk is set (x == 0: a run
// that must not cross a row of W) and where its key differs from the lane's below; len counts the
// lanes from this one to the next head, and `lanes` is their mask: on a head, its run.
struct IpRun {
  bool head;
  int len;
  unsigned long long lanes;
};
template <typename K>
__device__ __forceinline__ IpRun ip_run(K key, bool brk) {
  const int lane = threadIdx.x & 63;
  const K prev = __shfl_up(key, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || brk || key != prev);
  const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
  const int len = (above ? __builtin_ctzll(above) : 64) - lane;
  return {(bool)((heads >> lane) & 1), len, (len == 64 ? ~0ull : (1ull << len) - 1) << lane};
}

// The slot of row gid (> 0) in the workgroup's table s_gid[IP_SLOTS] (0 = free), claimed on first
// use; -1 when another row holds it, and the update goes to global memory.
__device__ __forceinline__ int ip_claim(int* s_gid, int gid) {
  const int slot = gid & (IP_SLOTS - 1), held = atomicCAS(&s_gid[slot], 0, gid);
  return held == 0 || held == gid ? slot : -1;
}

static inline bool ip_shape_ok(int N, int D, int H, int W) {
  if (N < 1 || D < 1 || H < 1 || W < 1) return false;
  const long long V = (long long)D * H * W;
  return V < (1LL << 31) && V * N < (1LL << 31);
}
