// Each selected feature instance alone in a solid stock block, at the classifier's resolution: the gather
// between the instance pipeline (ids volumes, instance tables) and the single-feature classifier.
//
// ids int32 [N][D][H][W], indexed [n][z][y][x]; sel int32 [M][14], a row being
//   n id | bz0 by0 bx0 bz1 by1 bx1 | wz0 wy0 wx0 Lz Ly Lx
// the sample and the instance's number in it, an inclusive box in the source grid, and the source window that
// becomes the stock block.  Output voxel o of an axis of part m looks, with Lmax = max(Lz, Ly, Lx) and L, w0
// those of the axis, at the window's voxel
//   s = floor((2 o + 1) Lmax - (Lmax - L) S, 2 S)
// (one scale Lmax / S, the shorter axes centred, a centre on a boundary to the higher index).  With s < 0 or
// s >= L on any axis the voxel lies outside the stock: 0.  Otherwise v = w0 + s per axis, and the voxel is 0
// iff v lies in the box and ids[n][v] == id, else 1.  A row of sel whose sample or window does not lie in the
// grid gives a part of zeros: nothing of it is stock, and no address is formed from it.
//
// fmt 0: bits, uint8 [M][S^3/8], bit i & 7 of byte i >> 3 for i = (Z S + Y) S + X; fmt 1: uint8 [M][S][S][S];
// fmt 2: bf16 [M][S][S][S] (0 / 1.0).
//
// The unit of work is an octet: 8 output voxels along X (S % 8 == 0), one byte of fmt 0.  A thread makes 4, 2
// or 1 consecutive octets of one part (fmt 0, 1, 2) and stores them as one dword or one 16-byte vector; a part
// has S^3 / 8 = 64 (S / 8)^3 octets, so no thread's octets straddle two parts and every store is aligned.
// Every output element is stored once, by one thread: no atomics, no initialising launch.  The source z and y
// of an octet, and the tests of the window and the box on them, are computed once per octet; an octet whose
// source row misses the window or the box is stored as a constant and reads nothing of ids.  ids is read
// under the predicate `in the window, in the box` only, from an address formed under that predicate: the
// window lies in the grid (checked per part, before anything else), so the address does.  A part whose window
// has S voxels on every axis maps voxel to voxel: its octets read 8 consecutive ids as two 16-byte loads and
// do no division on x.
#include "instance_pass.h"

constexpr int ISO_NTHR = 256;
constexpr int ISO_NCOL = 14;
constexpr int ISO_MAX_S = 256;

// The window's voxel of output voxel o: floor(((2 o + 1) Lmax - (Lmax - L) S) / (2 S)).  The numerator is
// at least -(Lmax - L) S > -2 S Lmax: 2 S Lmax is added before and Lmax taken off after the division, which
// then sees 0 <= num < 4 * 256 * 512.
__device__ __forceinline__ int iso_src(int o, int L, int Lmax, int S, unsigned r2S) {
  const int num = (2 * o + 1) * Lmax - (Lmax - L) * S + 2 * S * Lmax;
  return ip_div(num, 2 * S, r2S) - Lmax;
}

// Bit j of the result: voxel 8 xb + j of the octet is material.
template <bool IDENT>
__device__ __forceinline__ unsigned iso_octet(const int* __restrict__ ids, int o, int id, int n, int D, int H, int W,
                                              int S, int XB, int bz0, int by0, int bx0, int bz1, int by1, int bx1,
                                              int wz0, int wy0, int wx0, int Lz, int Ly, int Lx, int Lmax,
                                              unsigned rXB, unsigned rS, unsigned r2S) {
  const int row = ip_div(o, XB, rXB), xb = o - row * XB;
  const int Z = ip_div(row, S, rS), Y = row - Z * S;
  const int sz = IDENT ? Z : iso_src(Z, Lz, Lmax, S, r2S), sy = IDENT ? Y : iso_src(Y, Ly, Lmax, S, r2S);
  if (sz < 0 || sz >= Lz || sy < 0 || sy >= Ly) return 0u;                     // outside the stock
  const int vz = wz0 + sz, vy = wy0 + sy;                                      // in the window, so in the grid
  const bool live = vz >= bz0 && vz <= bz1 && vy >= by0 && vy <= by1;
  const int base = ((n * D + vz) * H + vy) * W;
  unsigned bits = 0;
  if (IDENT) {
    if (!live) return 0xffu;
    const int vx0 = wx0 + 8 * xb;                                              // vx0 + 7 < wx0 + S = wx0 + Lx <= W
    const int4 a = *reinterpret_cast<const int4*>(ids + base + vx0);
    const int4 b = *reinterpret_cast<const int4*>(ids + base + vx0 + 4);
    const int v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int vx = vx0 + j;
      const bool feature = vx >= bx0 && vx <= bx1 && v[j] == id;
      bits |= (feature ? 0u : 1u) << j;
    }
    return bits;
  }
  // On a longest axis every output voxel lies in the stock (0 <= floor((2 o + 1) L / (2 S)) <= L - 1 for o < S):
  // a row that misses the box is solid material there, without a look at x.
  if (!live && Lx == Lmax) return 0xffu;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int sx = iso_src(8 * xb + j, Lx, Lmax, S, r2S);
    const bool inx = sx >= 0 && sx < Lx;
    const int vx = wx0 + sx;
    bool feature = false;
    if (live && inx && vx >= bx0 && vx <= bx1) feature = ids[base + vx] == id;
    bits |= (inx && !feature ? 1u : 0u) << j;
  }
  return bits;
}

// The 4 low bits of b as 4 bytes of 0 / 1: bit k times 2^(7 i) lands on bit k + 7 i, which is a multiple of 8
// for i == k only, and no two products share a bit.
__device__ __forceinline__ unsigned iso_bytes(unsigned b) { return ((b & 0xfu) * 0x00204081u) & 0x01010101u; }
// Bits 0 and 1 of b as two bf16 of 0 / 1.0 (0x3f80).
__device__ __forceinline__ unsigned iso_bf16(unsigned b) { return (b & 1u) * 0x3f80u | ((b >> 1) & 1u) * 0x3f800000u; }

template <int FMT>
__global__ __launch_bounds__(ISO_NTHR) void isolate_kernel(const int* __restrict__ ids, const int* __restrict__ sel,
                                                          void* __restrict__ out, int N, int D, int H, int W, int S,
                                                          int groups, int bpp, int vec, unsigned rbpp, unsigned rXB,
                                                          unsigned rS, unsigned r2S) {
  constexpr int G = FMT == 0 ? 4 : FMT == 1 ? 2 : 1;                           // octets of a thread
  const int m = ip_div((int)blockIdx.x, bpp, rbpp);                            // the grid is M * bpp: m < M
  const int t = ((int)blockIdx.x - m * bpp) * ISO_NTHR + (int)threadIdx.x;     // this thread's group in the part
  if (t >= groups) return;
  const int* r = sel + (size_t)m * ISO_NCOL;
  const int n = r[0], id = r[1], bz0 = r[2], by0 = r[3], bx0 = r[4], bz1 = r[5], by1 = r[6], bx1 = r[7];
  const int wz0 = r[8], wy0 = r[9], wx0 = r[10], Lz = r[11], Ly = r[12], Lx = r[13];
  // the sample in the batch and the window in the grid, without a sum that could wrap
  const bool ok = n >= 0 && n < N && Lz >= 1 && Lz <= D && Ly >= 1 && Ly <= H && Lx >= 1 && Lx <= W && wz0 >= 0 &&
                  wz0 <= D - Lz && wy0 >= 0 && wy0 <= H - Ly && wx0 >= 0 && wx0 <= W - Lx;
  const int Lmax = max(Lz, max(Ly, Lx));
  // voxel to voxel, and every octet's 8 ids on a 16-byte boundary (vec: the ids pointer is)
  const bool ident = ok && Lz == S && Ly == S && Lx == S && vec != 0 && (W & 3) == 0 && (wx0 & 3) == 0;
  const int XB = S >> 3;
  unsigned bits[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int o = t * G + g;
    bits[g] = !ok ? 0u
              : ident ? iso_octet<true>(ids, o, id, n, D, H, W, S, XB, bz0, by0, bx0, bz1, by1, bx1, wz0, wy0, wx0,
                                        Lz, Ly, Lx, Lmax, rXB, rS, r2S)
                      : iso_octet<false>(ids, o, id, n, D, H, W, S, XB, bz0, by0, bx0, bz1, by1, bx1, wz0, wy0,
                                         wx0, Lz, Ly, Lx, Lmax, rXB, rS, r2S);
  }
  const size_t at = (size_t)m * groups + t;                                    // in stores of this format
  if (FMT == 0) {
    reinterpret_cast<unsigned*>(out)[at] = bits[0] | bits[1 % G] << 8 | bits[2 % G] << 16 | bits[3 % G] << 24;
  } else if (FMT == 1) {
    uint4 v;
    v.x = iso_bytes(bits[0]), v.y = iso_bytes(bits[0] >> 4);
    v.z = iso_bytes(bits[1 % G]), v.w = iso_bytes(bits[1 % G] >> 4);
    reinterpret_cast<uint4*>(out)[at] = v;
  } else {
    uint4 v;
    v.x = iso_bf16(bits[0]), v.y = iso_bf16(bits[0] >> 2), v.z = iso_bf16(bits[0] >> 4), v.w = iso_bf16(bits[0] >> 6);
    reinterpret_cast<uint4*>(out)[at] = v;
  }
}

// ids int32 [N*D*H*W], sel int32 [M][14], out: fmt 0 uint8 [M][S^3/8], 1 uint8 [M][S^3], 2 bf16 [M][S^3], on a
// 16-byte boundary.  D, H, W <= 256, N*D*H*W < 2^31, S % 8 == 0 in [8, 256], M * S^3 < 2^31.
extern "C" int fn_isolate_parts(const void* ids, const void* sel, void* out, int N, int D, int H, int W, long long M,
                                int S, int fmt, hipStream_t st) {
  if (!ip_shape_ok(N, D, H, W) || D > ISO_MAX_S || H > ISO_MAX_S || W > ISO_MAX_S || !ids) return -2;
  if (S < 8 || S > ISO_MAX_S || (S & 7) || fmt < 0 || fmt > 2 || M < 0) return -2;
  const long long V = (long long)S * S * S;
  if (M * V >= (1LL << 31)) return -2;
  if (M == 0) return 0;
  if (!sel || !out || ((uintptr_t)out & 15) || ((uintptr_t)sel & 3) || ((uintptr_t)ids & 3)) return -2;
  const int groups = (int)(V / 8) / (fmt == 0 ? 4 : fmt == 1 ? 2 : 1);
  const int bpp = (groups + ISO_NTHR - 1) / ISO_NTHR;
  const long long blocks = M * bpp;                                            // <= M * S^3 / 8 < 2^28
  const int vec = ((uintptr_t)ids & 15) == 0;
  const dim3 grid((unsigned)blocks), block(ISO_NTHR);
#define ISO_LAUNCH(F)                                                                                          \
  hipLaunchKernelGGL(isolate_kernel<F>, grid, block, 0, st, (const int*)ids, (const int*)sel, out, N, D, H, W, S, \
                     groups, bpp, vec, ip_recip(bpp), ip_recip(S >> 3), ip_recip(S), ip_recip(2 * S))
  if (fmt == 0)
    ISO_LAUNCH(0);
  else if (fmt == 1)
    ISO_LAUNCH(1);
  else
    ISO_LAUNCH(2);
#undef ISO_LAUNCH
  FN_CHECK_LAUNCH();
  return 0;
}
