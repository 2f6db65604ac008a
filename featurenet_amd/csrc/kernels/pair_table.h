// The pair table under overlap_pairs_kernel (overlap.hip) and contact_stats_kernel (contact.hip): counts per
// 64-bit key (never 0), met in a workgroup's LDS stage first and then in an open-addressing hash table in
// global memory, keys uint64 [cap] (0 = empty) / counts int64 [cap], cap a power of two, which the caller has
// zeroed.  The SET of (key, count) pairs in the table is exact and does not depend on the order of the
// atomics; their slots do, so the caller sorts the occupied ones.
#pragma once
#include "instance_pass.h"

constexpr int PT_LPROBE = 8;                    // LDS slots an update tries before it goes to global memory

// The 64-bit finalizer of MurmurHash3: every output bit depends on every key bit.  The top 9 bits
// pick the LDS slot, the low bits (cap <= 2^32) the global one.  A single multiplication is not
// enough: the keys are pairs of small, correlated row numbers (rb = ra + d for a prediction close
// to the truth), and its middle bits put them in clusters -- 12 probes per insert at load 0.4
// where this gives 0.35, as random keys do.
__device__ __forceinline__ unsigned long long pt_mix(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// counts[slot of key] += cnt.  Linear probing from the key's home slot, at most `bound` (<= cap)
// slots: a returning compare-and-swap claims an empty slot or shows whose it is.  An update that
// finds neither its key nor an empty slot within the bound is dropped and its count added to
// lost[0] (the caller grows the table and runs again).  Nothing here waits for another thread.
__device__ __forceinline__ void pt_global_add(unsigned long long* keys, long long* counts, long long* lost,
                                              unsigned long long mask, long long bound, unsigned long long key,
                                              long long cnt) {
  unsigned long long h = pt_mix(key) & mask;
  for (long long i = 0; i < bound; ++i) {
    unsigned long long held = 0;
    __hip_atomic_compare_exchange_strong(&keys[h], &held, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    if (held == 0 || held == key) {              // (held keeps 0 when the exchange was made)
      __hip_atomic_fetch_add(&counts[h], cnt, IP_RLX_AGENT);
      return;
    }
    h = (h + 1) & mask;
  }
  __hip_atomic_fetch_add(lost, cnt, IP_RLX_AGENT);
}

// The LDS stage s_key / s_cnt [IP_SLOTS] (zeroed, 0 = free), entered at the key's hash, not direct-mapped:
// s_cnt[slot of key] += cnt within PT_LPROBE slots from the hash on, or false when other keys hold them all
// and the update must go to the global table.  (overlap_pairs_kernel spells this loop out in its body: calling
// it from there moved one instruction of that kernel's schedule, and that kernel's code is kept as it was.)
__device__ __forceinline__ bool pt_stage_add(unsigned long long* s_key, unsigned long long* s_cnt,
                                             unsigned long long key, int cnt) {
  int slot = (int)(pt_mix(key) >> 55) & (IP_SLOTS - 1);
  bool met = false;
  for (int p = 0; p < PT_LPROBE && !met; ++p) {
    const unsigned long long held = atomicCAS(&s_key[slot], 0ull, key);
    met = held == 0 || held == key;
    if (met) atomicAdd(&s_cnt[slot], (unsigned long long)cnt);
    slot = (slot + 1) & (IP_SLOTS - 1);
  }
  return met;
}

// The max forms (ws_saddle_kernel, watershed.hip): counts[slot of key] = max(counts[slot of key], val) for val >=
// 0 over the caller's zeros -- the key, not the value, says that a slot is held, so a largest value of 0 stays a
// row.  A maximum does not depend on the order of the atomics either.  A dropped update adds 1 to lost[0].
__device__ __forceinline__ void pt_global_max(unsigned long long* keys, long long* counts, long long* lost,
                                              unsigned long long mask, long long bound, unsigned long long key,
                                              long long val) {
  unsigned long long h = pt_mix(key) & mask;
  for (long long i = 0; i < bound; ++i) {
    unsigned long long held = 0;
    __hip_atomic_compare_exchange_strong(&keys[h], &held, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    if (held == 0 || held == key) {
      __hip_atomic_fetch_max(&counts[h], val, IP_RLX_AGENT);
      return;
    }
    h = (h + 1) & mask;
  }
  __hip_atomic_fetch_add(lost, 1LL, IP_RLX_AGENT);
}

__device__ __forceinline__ bool pt_stage_max(unsigned long long* s_key, unsigned long long* s_val,
                                             unsigned long long key, unsigned long long val) {
  int slot = (int)(pt_mix(key) >> 55) & (IP_SLOTS - 1);
  bool met = false;
  for (int p = 0; p < PT_LPROBE && !met; ++p) {
    const unsigned long long held = atomicCAS(&s_key[slot], 0ull, key);
    met = held == 0 || held == key;
    if (met) atomicMax(&s_val[slot], val);
    slot = (slot + 1) & (IP_SLOTS - 1);
  }
  return met;
}

// cap: a power of two in [2, 2^32]; probe >= 1
static inline bool pt_shape_ok(long long cap, long long probe) {
  return cap >= 2 && cap <= (1LL << 32) && (cap & (cap - 1)) == 0 && probe >= 1;
}
