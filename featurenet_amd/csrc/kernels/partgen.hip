// Carve multi-feature parts from their parameter tables (../shared/partgen.h has the row format
// and the 24 volumes): the data source of the per-voxel pipeline, run where the training set lives.
//
// params int32 [N][K][16].  Outputs, each optional (null = not wanted), all x fastest:
//   occ    uint8 [N][S][S][S]   1 = material, 0 = removed by some slot
//   packed uint8 [N][S^3/8]     occ, bit i of byte j = voxel 8j + i (the format of unpack_bits)
//   labels uint8 [N][S][S][S]   1 + cls of the lowest slot whose volume holds the voxel, else 0
//   slots  uint8 [N][S][S][S]   1 + that slot, else 0
// Integer arithmetic only: the result is a pure function of the table, the same on every run and
// bit for bit what the host path (the same header) and the torch oracle give.
//
// One lane owns a run of 8 voxels along x (S % 8 == 0: a run never leaves its row): it keeps the
// run's 8 labels and 8 slots in two 64-bit registers and makes one 8-byte store per byte output
// and one byte of `packed`; a wave's stores are 512 (64) contiguous bytes.  A workgroup owns
// PG_CHUNK consecutive voxels of the flat batch; the rows of the samples it touches (at most
// PG_SAMPLES: V >= 512) are read once into LDS.  A slot whose box misses the run is skipped, so
// most lanes evaluate no predicate at all; cls and orient are uniform within a sample, so the two
// switches diverge only in a workgroup that straddles samples.  No atomics, no loop that is not
// bounded by K or a constant, and no address that is not formed from a clamped run index.
#include "common.h"
#include "../shared/partgen.h"

constexpr int PG_NTHR = 256;
constexpr int PG_RUN = 8;                        // voxels per lane
constexpr int PG_CHUNK = PG_RUN * PG_NTHR;       // voxels per workgroup
constexpr int PG_SAMPLES = PG_CHUNK / 512 + 1;   // samples a workgroup can touch (S >= 8: V >= 512)
static_assert(PG_NTHR % FN_WAVE == 0, "whole waves");

__global__ __launch_bounds__(PG_NTHR) void partgen_carve_kernel(const int* __restrict__ params,
                                                                unsigned long long* __restrict__ occ,
                                                                unsigned char* __restrict__ packed,
                                                                unsigned long long* __restrict__ labels,
                                                                unsigned long long* __restrict__ slots, int N, int K,
                                                                int S, unsigned rpv, unsigned runs, unsigned magic) {
  __shared__ int s_rows[PG_SAMPLES * PG_MAX_K * PG_ROW];
  const unsigned tid = threadIdx.x;
  // the workgroup's runs [r0, r1] (runs < 2^31; r1 clamped: the last workgroup's spare lanes
  // repeat the last run, same values to the same address) and the samples they lie in; rpv =
  // S^3 / 8 runs per sample
  const unsigned r0 = blockIdx.x * PG_NTHR;
  const unsigned r1 = r0 + PG_NTHR - 1 < runs - 1 ? r0 + PG_NTHR - 1 : runs - 1;
  const unsigned n0 = r0 / rpv, n1 = r1 / rpv;
  int cnt = (int)(n1 - n0 + 1) * K * PG_ROW;
  cnt = cnt < PG_SAMPLES * PG_MAX_K * PG_ROW ? cnt : PG_SAMPLES * PG_MAX_K * PG_ROW;
  const int* src = params + (long long)n0 * K * PG_ROW;      // (n1 < N: cnt stays inside params)
  for (int i = tid; i < cnt; i += PG_NTHR) s_rows[i] = src[i];
  __syncthreads();

  const unsigned run = r0 + tid < r1 ? r0 + tid : r1;
  unsigned dn = 0, local = run - n0 * rpv;       // the run's sample, counted from n0, and its place in it
#pragma unroll
  for (int i = 0; i < PG_SAMPLES - 1; ++i)
    if (local >= rpv) local -= rpv, ++dn;
  // first voxel of the run in its sample, < 2^24: with magic = 2^32 / S + 1, __umulhi(v, magic) is
  // v / S for every v < 2^24 (the error v * (magic * S - 2^32) <= v * S stays below 2^32)
  const unsigned rem = local * PG_RUN, line = __umulhi(rem, magic), plane = __umulhi(line, magic);
  const int X0 = (int)(rem - line * S), Y = (int)(line - plane * S), Z = (int)plane;
  const int* rows = s_rows + dn * K * PG_ROW;
  unsigned long long lab = 0, slo = 0;
  unsigned open = 0xffu;                         // bit i: voxel i of the run is in no slot yet
  for (int k = 0; k < K; ++k) {
    const int* row = rows + k * PG_ROW;
    const int bx0 = row[PG_X0], bx1 = row[PG_X1];
    if (row[PG_CLS] < 0 || Z < row[PG_Z0] || Z > row[PG_Z1] || Y < row[PG_Y0] || Y > row[PG_Y1] ||
        X0 + PG_RUN - 1 < bx0 || X0 > bx1)
      continue;
    // pg_inside() for the 8 voxels: the box along x, and the canonical voxel, which moves by one
    // fixed step along the run
    int cx, cy, cz, sx, sy, sz;
    pg_canonical(row[PG_ORIENT], S, X0, Y, Z, cx, cy, cz);
    pg_canonical(row[PG_ORIENT], S, X0 + 1, Y, Z, sx, sy, sz);
    sx -= cx, sy -= cy, sz -= cz;
    const unsigned long long lv = (unsigned long long)((row[PG_CLS] + 1) & 0xff), sv = (unsigned long long)(k + 1);
#pragma unroll
    for (int i = 0; i < PG_RUN; ++i) {
      if (((open >> i) & 1u) && X0 + i >= bx0 && X0 + i <= bx1 &&
          pg_inside_canonical(row, S, cx + i * sx, cy + i * sy, cz + i * sz)) {
        lab |= lv << (8 * i);
        slo |= sv << (8 * i);
        open &= ~(1u << i);
      }
    }
  }
  if (occ) {
    unsigned long long o = 0;
#pragma unroll
    for (int i = 0; i < PG_RUN; ++i) o |= (unsigned long long)((open >> i) & 1u) << (8 * i);
    occ[run] = o;
  }
  if (packed) packed[run] = (unsigned char)open;
  if (labels) labels[run] = lab;
  if (slots) slots[run] = slo;
}

extern "C" int fn_partgen_chunk() { return PG_CHUNK; }

// any of occ / packed / labels / slots may be null; the byte volumes must be 8-byte aligned.
// S % 8 == 0, 8 <= S <= 256, 0 <= K <= 32, N >= 0, N * S^3 < 2^34 - 2^11 (the runs fit 31 bits)
extern "C" int fn_partgen_carve(const void* params, void* occ, void* packed, void* labels, void* slots, int N, int K,
                                int S, hipStream_t st) {
  if (N < 0 || K < 0 || K > PG_MAX_K || S < 8 || S > PG_MAX_S || S % 8 != 0) return -2;
  if (((uintptr_t)occ | (uintptr_t)labels | (uintptr_t)slots) & 7) return -2;
  if (N == 0) return 0;
  if (!params && K > 0) return -2;
  const unsigned rpv = (unsigned)(S * S * S / PG_RUN);       // <= 2^21
  const long long runs = (long long)N * rpv;
  if (runs >= (1LL << 31) - PG_NTHR) return -2;
  const long long blocks = (runs + PG_NTHR - 1) / PG_NTHR;
  hipLaunchKernelGGL(partgen_carve_kernel, dim3((unsigned)blocks), dim3(PG_NTHR), 0, st, (const int*)params,
                     (unsigned long long*)occ, (unsigned char*)packed, (unsigned long long*)labels,
                     (unsigned long long*)slots, N, K, S, rpv, (unsigned)runs,
                     (unsigned)((1ULL << 32) / (unsigned)S + 1));
  FN_CHECK_LAUNCH();
  return 0;
}
