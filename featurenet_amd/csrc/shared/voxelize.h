// Triangle meshes to voxel grids: the cover test of a triangle over a column of voxel centres and
// the voxel at which the column's ray crosses it, in exact integers.  One piece of code for the
// kernel (kernels/voxelize.hip) and the host path (runtime/mesh.cpp); the torch oracle
// (ops/reference.py, voxelize_tris) is written apart from it and is what the two are tested against.
//
// Lattice: VX_U = 16 units per voxel, the centre of voxel k of an axis at 16k + 8.  A triangle is
// nine int32 (ax ay az bx by bz cx cy cz), every |coordinate| <= VX_MAX_COORD = 8192; vertex
// (x, y, z) lands in volume[z][y][x].  Rays run along +x through the column centres s = (py, pz):
//
//   project to (y, z): area2 = (by-ay)(cz-az) - (bz-az)(cy-ay); 0: the triangle is skipped,
//   negative: b and c are swapped.  For each directed edge p -> q of the re-oriented triangle,
//   d = (qy-py, qz-pz) and E = d.y (s.z - p.z) - d.z (s.y - p.y); the column is covered iff every
//   edge has E > 0, or E == 0 and owns its ties (d.y > 0, or d.y == 0 and d.z < 0: exactly one of d
//   and -d, so of the two triangles that share an edge in opposite directions exactly one owns a
//   centre on it, and a closed mesh stays closed).  The owning edges of a projection are its low-z
//   and low-y ones: a box whose faces pass through voxel centres is half open, [lo, hi), on y and
//   z as it is on x.
//
//   n = (b-a) x (c-a), n.x = area2 > 0; the ray meets the plane at x_hit = ax - A / n.x with
//   A = n.y (py-ay) + n.z (pz-az), and the crossing toggles bit
//   k_min = clamp(ceil((ax n.x - A - 8 n.x) / (16 n.x)), 0, S): the first voxel whose centre is not
//   left of the crossing; k_min == S is the column's overflow bit.
//
// Edge functions stay below 2^29 (int32), the numerator below 2^45 (int64, exact in fp64).
#pragma once

#if defined(__HIPCC__)
#define VX_HD __host__ __device__ inline
#else
#define VX_HD inline
#endif

constexpr int VX_U = 16;               // lattice units per voxel
constexpr int VX_HALF = 8;             // a voxel centre within its voxel
constexpr int VX_MAX_COORD = 8192;     // largest |coordinate|
constexpr int VX_MAX_S = 256;

// A triangle ready for its columns: the three edge functions at column (0, 0) with their steps
// per column along y and z (the tie rule folded in: covered iff every e >= 0), the plane, and the
// inclusive box of column indices whose centres lie in the triangle's (y, z) box.
struct VxTri {
  int e[3], ey[3], ez[3];
  int nx, ny, nz;
  int ax, ay, az;
  int y0, y1, z0, z1;
};

VX_HD int vx_min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
VX_HD int vx_max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// False: the triangle has no area in (y, z) (no ray crosses it) or its box holds no column centre
// of planes [zlo, zhi] of an S^3 grid.
VX_HD bool vx_setup(const int* t, int S, int zlo, int zhi, VxTri& s) {
  int ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
  const int area2 = (by - ay) * (cz - az) - (bz - az) * (cy - ay);
  if (area2 == 0) return false;
  if (area2 < 0) {
    int v;
    v = bx, bx = cx, cx = v;
    v = by, by = cy, cy = v;
    v = bz, bz = cz, cz = v;
  }
  // column centres 16 i + 8 within [min, max]: ceil((min - 8) / 16) <= i <= floor((max - 8) / 16)
  int y0 = (vx_min3(ay, by, cy) - VX_HALF + VX_U - 1) >> 4, y1 = (vx_max3(ay, by, cy) - VX_HALF) >> 4;
  int z0 = (vx_min3(az, bz, cz) - VX_HALF + VX_U - 1) >> 4, z1 = (vx_max3(az, bz, cz) - VX_HALF) >> 4;
  y0 = y0 < 0 ? 0 : y0, y1 = y1 > S - 1 ? S - 1 : y1;
  z0 = z0 < zlo ? zlo : z0, z1 = z1 > zhi ? zhi : z1;
  if (y0 > y1 || z0 > z1) return false;
  s.y0 = y0, s.y1 = y1, s.z0 = z0, s.z1 = z1;
  const int py[3] = {ay, by, cy}, pz[3] = {az, bz, cz};
  for (int i = 0; i < 3; ++i) {
    const int j = i == 2 ? 0 : i + 1;
    const int dy = py[j] - py[i], dz = pz[j] - pz[i];
    const int owns = dy > 0 || (dy == 0 && dz < 0);
    // E(s) = dy (s.z - p.z) - dz (s.y - p.y) at s = (8, 8); covered iff E > 0 or (E == 0 and the
    // edge owns its ties), that is E - 1 + owns >= 0
    s.e[i] = dy * (VX_HALF - pz[i]) - dz * (VX_HALF - py[i]) - 1 + owns;
    s.ey[i] = -dz * VX_U;
    s.ez[i] = dy * VX_U;
  }
  s.nx = area2 < 0 ? -area2 : area2;
  s.ny = (bz - az) * (cx - ax) - (bx - ax) * (cz - az);
  s.nz = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
  s.ax = ax, s.ay = ay, s.az = az;
  return true;
}

// is the centre of column (iy, iz) covered?
VX_HD bool vx_covers(const VxTri& s, int iy, int iz) {
  return (s.e[0] + iy * s.ey[0] + iz * s.ez[0]) >= 0 && (s.e[1] + iy * s.ey[1] + iz * s.ez[1]) >= 0 &&
         (s.e[2] + iy * s.ey[2] + iz * s.ez[2]) >= 0;
}

// the bit of column (iy, iz) that the crossing toggles, 0..S (S: the overflow bit).  The quotient
// is estimated in fp64 (numerator and denominator are exact there) and settled by the exact test.
VX_HD int vx_kmin(const VxTri& s, int S, int iy, int iz) {
  const long long nx = s.nx;
  const long long A = (long long)s.ny * (VX_U * iy + VX_HALF - s.ay) + (long long)s.nz * (VX_U * iz + VX_HALF - s.az);
  const long long num = (long long)s.ax * nx - A - VX_HALF * nx, den = VX_U * nx;
  if (num <= 0) return 0;
  if (num > den * (S - 1)) return S;
  long long k = (long long)((double)num / (double)den);       // floor(num / den) or one more
  if (k * den < num) ++k;
  if ((k - 1) * den >= num) --k;
  return k < 0 ? 0 : k > S ? S : (int)k;
}

// The same quotient clamped to [-1, S + 1] only: ceil((x_hit - 8) / 16), the first voxel whose
// centre is not before the crossing, for a caller that looks at voxels k - 1 and k on both sides
// of the surface (-1 and S + 1: both of them lie outside the grid, on that side).
VX_HD int vx_kcross(const VxTri& s, int S, int iy, int iz) {
  const long long nx = s.nx;
  const long long A = (long long)s.ny * (VX_U * iy + VX_HALF - s.ay) + (long long)s.nz * (VX_U * iz + VX_HALF - s.az);
  const long long num = (long long)s.ax * nx - A - VX_HALF * nx, den = VX_U * nx;
  if (num <= -den) return -1;
  if (num > den * S) return S + 1;
  long long k = (long long)((double)num / (double)den);       // the quotient truncated, or one off
  if (k * den < num) ++k;
  if ((k - 1) * den >= num) --k;
  return (int)k;                                               // -den < num <= den S: 0..S
}

// ---------------------------------------------------------------------------------------------
// Mesh labels: which value of a volume lies against a triangle (kernels/meshlabel.hip and
// mesh_votes of runtime/mesh.cpp; the torch oracle is reference.mesh_votes).  The triangle is
// turned so that the dominant axis m of its normal (the first of x, y, z with the largest
// |component|) becomes the x of the rays above, u = (m + 1) % 3 its y and v = (m + 2) % 3 its z:
// the projection has area, and columns run along m.
// ---------------------------------------------------------------------------------------------

// q = the triangle with every vertex as (p[m], p[u], p[v]) -> m, or -1 when the normal is zero.
VX_HD int vx_dominant(const int* t, int* q) {
  const int e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
  int n[3];                                      // |edge| <= 2^14, a product <= 2^28, a component <= 2^29
  for (int i = 0; i < 3; ++i) {
    const int j = i == 2 ? 0 : i + 1, k = j == 2 ? 0 : j + 1;
    n[i] = e1[j] * e2[k] - e1[k] * e2[j];
    n[i] = n[i] < 0 ? -n[i] : n[i];
  }
  if ((n[0] | n[1] | n[2]) == 0) return -1;
  const int m = n[0] >= n[1] && n[0] >= n[2] ? 0 : n[1] >= n[2] ? 1 : 2;
  const int u = m == 2 ? 0 : m + 1, v = u == 2 ? 0 : u + 1;
  for (int p = 0; p < 3; ++p) q[3 * p] = t[3 * p + m], q[3 * p + 1] = t[3 * p + u], q[3 * p + 2] = t[3 * p + v];
  return m;
}

// The one vote of a triangle that covers no column centre, at its centroid: column (iu, iv) =
// floor(sum / 48) (it may lie outside the grid) and k = ceil((sum_m - 24) / 48).
VX_HD void vx_centroid(const int* q, int& k, int& iu, int& iv) {
  const int sm = q[0] + q[3] + q[6], su = q[1] + q[4] + q[7], sv = q[2] + q[5] + q[8];
  const int off = 48 * 1024;                     // |sum| <= 3 * 8192 < off: the divisions see positives
  iu = (su + off) / 48 - 1024, iv = (sv + off) / 48 - 1024;
  k = (sm - 24 + 47 + off) / 48 - 1024;
}

// the winner of two tallies (value, votes): more votes, then the lower value; votes 0 = none
VX_HD bool vx_beats(int value, int votes, int best_value, int best_votes) {
  return votes > best_votes || (votes == best_votes && votes > 0 && value < best_value);
}
