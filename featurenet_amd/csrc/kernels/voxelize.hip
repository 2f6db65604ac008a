// Triangle meshes to voxel grids (../shared/voxelize.h has the lattice, the cover test with its
// tie rule and the crossing's voxel): the entrance of the per-voxel pipeline.
//
// tris int32 [T][9], offsets int32 [N + 1] (CSR: mesh n owns triangles offsets[n] .. offsets[n+1]).
// Outputs, each optional (null = not wanted), x fastest:
//   occ        uint8 [N][S][S][S]   1 = material: the parity of the crossings at or left of the centre
//   packed     uint8 [N][S^3/8]     occ, bit i of byte j = voxel 8j + i (the format of unpack_bits)
//   leaks_part int32 [N][slabs]     per slab, the columns whose crossings (overflow included) are odd
// Integer arithmetic only (one fp64 quotient estimate, settled exactly): the result is a pure,
// order-independent function of the table, bit for bit what the host path (the same header) and the
// torch oracle give.
//
// One workgroup owns one (mesh, slab of zs z-planes).  The slab's toggle bits (S per column, x
// fastest, so a column's bits are the bits of S/8 consecutive bytes in the layout of `packed`) and
// one overflow bit per column live in LDS.  The workgroup streams the mesh's triangles, one per
// lane: a lane whose triangle's clipped box of column centres is small rasterises it alone; the
// others are collected by ballot and taken by the whole wave, lanes over columns.  A crossing is
// one LDS atomicXor.  After a barrier a lane per column turns the toggles into their prefix
// parity in place (bytes: S % 8 == 0) and counts the odd columns; after another, lanes stream the
// slab out: one byte of `packed` and one 8-byte store of `occ` per LDS byte, contiguous over the
// wave.  No global atomics, no workgroup waits for another, every loop is bounded by T, a clipped
// box or a constant, and every address is formed from clamped indices.
#include "common.h"
#include "../shared/voxelize.h"

constexpr int VX_NTHR = 256;
constexpr int VX_LANE_COLS = 8;                  // a box of at most this many columns stays with its lane
constexpr int VX_LDS_MAX = 64 * 1024 - 256;      // per workgroup, s_leaks included: two fit a CU
constexpr int VX_SLAB_BITS = 8 * 8192;           // toggle bits of the slab that zs = 0 selects
static_assert(VX_NTHR % FN_WAVE == 0, "whole waves");

__device__ __forceinline__ void vx_toggle(unsigned* s_bits, unsigned* s_over, const VxTri& t, int S, int zlo, int iy,
                                          int iz) {
  if (!vx_covers(t, iy, iz)) return;
  const int k = vx_kmin(t, S, iy, iz);                     // 0..S
  const unsigned col = (unsigned)((iz - zlo) * S + iy);    // (iz in [zlo, zhi], iy in [0, S): vx_setup clamps)
  if (k < S) {
    const unsigned bit = col * (unsigned)S + (unsigned)k;
    atomicXor(&s_bits[bit >> 5], 1u << (bit & 31));
  } else {
    atomicXor(&s_over[col >> 5], 1u << (col & 31));
  }
}

__global__ __launch_bounds__(VX_NTHR) void voxelize_tris_kernel(const int* __restrict__ tris,
                                                                const int* __restrict__ offsets,
                                                                unsigned long long* __restrict__ occ,
                                                                unsigned char* __restrict__ packed,
                                                                int* __restrict__ leaks_part, int T, int S, int zs,
                                                                int slabs, int bit_words) {
  extern __shared__ unsigned s_mem[];            // [bit_words] toggle bits, then the overflow bits
  __shared__ int s_leaks[VX_NTHR / FN_WAVE];
  unsigned* s_bits = s_mem;
  unsigned* s_over = s_mem + bit_words;
  const int tid = threadIdx.x, lane = tid & (FN_WAVE - 1);
  const int n = blockIdx.x / slabs, slab = blockIdx.x - n * slabs;
  const int zlo = slab * zs, zhi = (zlo + zs < S ? zlo + zs : S) - 1;
  const int cols = (zhi - zlo + 1) * S;          // columns of this slab, <= zs * S
  const int over_words = (zs * S + 31) >> 5;
  for (int i = tid; i < bit_words + over_words; i += VX_NTHR) s_mem[i] = 0u;
  __syncthreads();

  int t0 = offsets[n], t1 = offsets[n + 1];
  t0 = t0 < 0 ? 0 : t0 > T ? T : t0;
  t1 = t1 < t0 ? t0 : t1 > T ? T : t1;
  for (int base = t0; base < t1; base += VX_NTHR) {        // (uniform over the workgroup)
    const int mine = base + tid;
    VxTri t;
    bool live = false;
    if (mine < t1) live = vx_setup(tris + (size_t)mine * 9, S, zlo, zhi, t);
    const int ny = live ? t.y1 - t.y0 + 1 : 0, nz = live ? t.z1 - t.z0 + 1 : 0;
    const bool wide = ny * nz > VX_LANE_COLS;
    if (live && !wide)
      for (int iz = t.z0; iz <= t.z1; ++iz)
        for (int iy = t.y0; iy <= t.y1; ++iy) vx_toggle(s_bits, s_over, t, S, zlo, iy, iz);
    unsigned long long todo = __ballot(wide);              // at most 64 turns
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int idx = __shfl(mine, src, FN_WAVE);          // < t1: the lane was live
      VxTri w;
      if (!vx_setup(tris + (size_t)idx * 9, S, zlo, zhi, w)) continue;     // (never: it was live there)
      const int wy = w.y1 - w.y0 + 1, wn = wy * (w.z1 - w.z0 + 1);          // <= S * zs
      for (int c = lane; c < wn; c += FN_WAVE) {
        const int dz = c / wy;
        vx_toggle(s_bits, s_over, w, S, zlo, w.y0 + (c - dz * wy), w.z0 + dz);
      }
    }
  }
  __syncthreads();

  // toggles -> prefix parity, in place; a column is S/8 consecutive bytes
  unsigned char* s_bytes = reinterpret_cast<unsigned char*>(s_bits);
  const int cb = S >> 3;
  int odd = 0;
  for (int col = tid; col < cols; col += VX_NTHR) {
    unsigned carry = 0;
    for (int j = 0; j < cb; ++j) {
      unsigned b = s_bytes[col * cb + j];
      b ^= b << 1;
      b ^= b << 2;
      b ^= b << 4;
      b = (b ^ (0u - carry)) & 0xffu;
      carry = b >> 7;
      s_bytes[col * cb + j] = (unsigned char)b;
    }
    odd += (int)(carry ^ ((s_over[col >> 5] >> (col & 31)) & 1u));
  }
  if (leaks_part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) odd += __shfl_xor(odd, o, FN_WAVE);
    if (lane == 0) s_leaks[tid / FN_WAVE] = odd;
  }
  __syncthreads();
  if (leaks_part && tid == 0) {
    int sum = 0;
    for (int i = 0; i < VX_NTHR / FN_WAVE; ++i) sum += s_leaks[i];
    leaks_part[blockIdx.x] = sum;                // (blockIdx.x = n * slabs + slab)
  }

  // the slab is contiguous in both outputs: bytes [first, first + nbytes) of `packed`
  const int nbytes = cols * cb;
  const size_t first = ((size_t)n * S + zlo) * S * cb;
  for (int i = tid; i < nbytes; i += VX_NTHR) {
    const unsigned b = s_bytes[i];
    if (packed) packed[first + i] = (unsigned char)b;
    if (occ) {
      // bit i of b -> byte i: a copy of b in every byte, bit i kept in byte i, non-zero bytes -> 1
      const unsigned long long own = ((unsigned long long)b * 0x0101010101010101ULL) & 0x8040201008040201ULL;
      occ[first + i] = ((own + 0x7f7f7f7f7f7f7f7fULL) >> 7) & 0x0101010101010101ULL;
    }
  }
}

// the slab height that zs = 0 selects: VX_SLAB_BITS toggle bits (8 KB), so that a batch of few
// meshes still spreads over the chip and several workgroups share a CU
extern "C" int fn_voxelize_planes(int S) {
  if (S < 8 || S > VX_MAX_S || S % 8 != 0) return -2;
  const int zs = VX_SLAB_BITS / (S * S);
  return zs < 1 ? 1 : zs > S ? S : zs;
}

// any of occ / packed / leaks_part may be null; occ must be 8-byte, tris / offsets / leaks_part
// 4-byte aligned.  S % 8 == 0, 8 <= S <= 256; zs = 0 (fn_voxelize_planes) or 1..S with the slab
// within VX_LDS_MAX; N * slabs < 2^31.  leaks_part holds N * ceil(S / zs) counts.
extern "C" int fn_voxelize_tris(const void* tris, const void* offsets, void* occ, void* packed, void* leaks_part, int N,
                                int T, int S, int zs, hipStream_t st) {
  if (N < 0 || T < 0 || S < 8 || S > VX_MAX_S || S % 8 != 0 || zs < 0 || zs > S) return -2;
  if (zs == 0) zs = fn_voxelize_planes(S);
  if ((uintptr_t)occ & 7) return -2;
  if (((uintptr_t)tris | (uintptr_t)offsets | (uintptr_t)leaks_part) & 3) return -2;
  const int bit_words = zs * S * S / 32;         // (S % 8 == 0: S * S % 32 == 0)
  const int over_words = (zs * S + 31) / 32;
  const size_t lds = (size_t)(bit_words + over_words) * 4;
  if (lds > (size_t)VX_LDS_MAX) return -2;
  if (N == 0) return 0;
  if (!offsets || (!tris && T > 0)) return -2;
  const int slabs = (S + zs - 1) / zs;
  const long long blocks = (long long)N * slabs;
  if (blocks >= (1LL << 31)) return -2;
  hipLaunchKernelGGL(voxelize_tris_kernel, dim3((unsigned)blocks), dim3(VX_NTHR), lds, st, (const int*)tris,
                     (const int*)offsets, (unsigned long long*)occ, (unsigned char*)packed, (int*)leaks_part, T, S, zs,
                     slabs, bit_words);
  FN_CHECK_LAUNCH();
  return 0;
}
