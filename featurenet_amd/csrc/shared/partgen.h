// Multi-feature parts: the parameter table's row format, the 24 feature volumes as exact integer
// predicates, and the orientation maps.  One piece of code for the carving kernel (partgen.hip),
// the host path and the sampler (runtime/voxel.cpp); the torch oracle (ops/reference.py,
// carve_parts) has its own predicates and is what the two are tested against.
//
// A part is a solid S^3 block from which up to K features are removed.  Row k of a part's table:
//
//   cls orient cu cv r r2 a b depth w x0 x1 y0 y1 z0 z1          (16 x int32)
//
// cls 0..23: the classes of voxel.cpp, -1: the slot is unused.  orient = o + 6*fx + 12*fy: o in
// 0..5 is the access face (orient() of voxel.cpp), fx / fy mirror the canonical x / y before it.
// The geometry fields are in quarter voxels: the centre of canonical voxel (x, y, z) is X = 4x,
// Y = 4y, Z = 4z, the access face is at top = 4(S-1) and dz = top - Z is the depth below it.  With
// u = X - cu and v = Y - cv the volumes are (every one also needs dz <= depth unless noted):
//
//    0 O-ring            u2+v2 <= r2  and not  u2+v2 <= r2_2
//    1 / 2 hole          u2+v2 <= r2                      (through: depth >= 4S, as for all pairs)
//    3 / 9 triangle      2v >= -r, v <= r, 3u2 <= (r-v)2
//    4 / 10 rectangle    |u| <= a, |v| <= b
//    5 / 11 round slot   (|u| <= a, |v| <= r) or a disc of radius r round (cu -+ a, cv)
//    6 V groove          5|u| <= 3(depth - dz)
//    7 / 8 slot          |u| <= a               / and v <= b (open towards y = 0 only)
//   12 corner triangle   X + Y <= r             13 corner disc  X2 + Y2 <= r2
//   14 corner block      X <= a, Y <= b         15 edge step    X <= a
//   16 two edge steps    X <= a or X >= top-a   17 slanted step 2 X depth <= 4a(depth-dz) + a depth
//   18 chamfer           X + dz < w             (no depth)
//   19 round             X < w, dz < w, (w-X)2 + (w-dz)2 > w2           (no depth)
//   20 vertical slot     (|u| <= r, v <= 0) or u2+v2 <= r2
//   21 horizontal slot   v <= b and ((dz <= depth-r, |u| <= r) or u2 + (dz-(depth-r))2 <= r2)
//   22 / 23 hexagon      4v2 <= 3r2, |u| <= r, v2 <= 3(r-|u|)2
//
// x0..z1: the feature's inclusive bounding box in OUTPUT voxel coordinates.  A voxel belongs to a
// slot's volume when it lies in the box and the predicate holds, so a box that is too small clips
// its feature (here; the oracle ignores the box -- the table's author keeps it large enough).
// With S <= 256 and every geometry field within +-PG_FIELD_MAX(S) no product leaves int32.
#pragma once

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ inline
#else
#define PG_HD inline
#endif

constexpr int PG_ROW = 16;             // int32 per row
constexpr int PG_Q = 4;                // sub-voxel units per voxel
constexpr int PG_CLASSES = 24;
constexpr int PG_MAX_S = 256;
constexpr int PG_MAX_K = 32;
enum PgField : int { PG_CLS = 0, PG_ORIENT, PG_CU, PG_CV, PG_R, PG_R2, PG_A, PG_B, PG_DEPTH, PG_W,
                     PG_X0, PG_X1, PG_Y0, PG_Y1, PG_Z0, PG_Z1 };

// the largest magnitude a geometry field may have: the largest square formed is (3 * 8S)^2 * 3
PG_HD int pg_field_max(int S) { return 2 * PG_Q * S; }

// canonical voxel (x, y, z) of output voxel (X, Y, Z): the inverse of orient() in voxel.cpp, then
// the mirrors
PG_HD void pg_canonical(int orient, int S, int X, int Y, int Z, int& x, int& y, int& z) {
  const int o = orient % 6, m = orient / 6, e = S - 1;
  switch (o) {
    case 0: x = X, y = Y, z = Z; break;
    case 1: x = X, y = e - Y, z = e - Z; break;
    case 2: x = e - Z, y = Y, z = X; break;
    case 3: x = Z, y = Y, z = e - X; break;
    case 4: x = X, y = e - Z, z = Y; break;
    default: x = X, y = Z, z = e - Y; break;
  }
  if (m & 1) x = e - x;
  if (m & 2) y = e - y;
}

// output voxel of canonical voxel (x, y, z): the mirrors, then orient()
PG_HD void pg_output(int orient, int S, int x, int y, int z, int& X, int& Y, int& Z) {
  const int o = orient % 6, m = orient / 6, e = S - 1;
  if (m & 1) x = e - x;
  if (m & 2) y = e - y;
  X = x, Y = y, Z = z;
  switch (o) {
    case 0: break;
    case 1: Z = e - z, Y = e - y; break;
    case 2: X = z, Z = e - x; break;
    case 3: X = e - z, Z = x; break;
    case 4: Y = z, Z = e - y; break;
    default: Y = e - z, Z = y; break;
  }
}

PG_HD int pg_abs(int v) { return v < 0 ? -v : v; }
PG_HD bool pg_circle(int u, int v, int r) { return u * u + v * v <= r * r; }
PG_HD bool pg_rect(int u, int v, int a, int b) { return pg_abs(u) <= a && pg_abs(v) <= b; }
PG_HD bool pg_tri(int u, int v, int r) { return 2 * v >= -r && v <= r && 3 * u * u <= (r - v) * (r - v); }
PG_HD bool pg_hex(int u, int v, int r) {
  const int au = pg_abs(u);
  return 4 * v * v <= 3 * r * r && au <= r && v * v <= 3 * (r - au) * (r - au);
}

// the predicate of `row` at canonical voxel (x, y, z); a class outside 0..23 has no volume
PG_HD bool pg_inside_canonical(const int* row, int S, int x, int y, int z) {
  const int X = PG_Q * x, Y = PG_Q * y, top = PG_Q * (S - 1), dz = top - PG_Q * z;
  const int u = X - row[PG_CU], v = Y - row[PG_CV];
  const int r = row[PG_R], a = row[PG_A], b = row[PG_B], depth = row[PG_DEPTH], w = row[PG_W];
  const bool in_depth = dz <= depth;
  switch (row[PG_CLS]) {
    case 0: return in_depth && pg_circle(u, v, r) && !pg_circle(u, v, row[PG_R2]);
    case 1:
    case 2: return in_depth && pg_circle(u, v, r);
    case 3:
    case 9: return in_depth && pg_tri(u, v, r);
    case 4:
    case 10: return in_depth && pg_rect(u, v, a, b);
    case 5:
    case 11: return in_depth && (pg_rect(u, v, a, r) || pg_circle(u - a, v, r) || pg_circle(u + a, v, r));
    case 6: return in_depth && 5 * pg_abs(u) <= 3 * (depth - dz);
    case 7: return in_depth && pg_abs(u) <= a;
    case 8: return in_depth && pg_abs(u) <= a && v <= b;
    case 12: return in_depth && X + Y <= r;
    case 13: return in_depth && pg_circle(X, Y, r);
    case 14: return in_depth && X <= a && Y <= b;
    case 15: return in_depth && X <= a;
    case 16: return in_depth && (X <= a || X >= top - a);
    case 17: return in_depth && 2 * X * depth <= 4 * a * (depth - dz) + a * depth;
    case 18: return X + dz < w;
    case 19: return X < w && dz < w && (w - X) * (w - X) + (w - dz) * (w - dz) > w * w;
    case 20: return in_depth && ((pg_abs(u) <= r && v <= 0) || pg_circle(u, v, r));
    case 21: return v <= b && ((dz <= depth - r && pg_abs(u) <= r) || pg_circle(u, dz - (depth - r), r));
    case 22:
    case 23: return in_depth && pg_hex(u, v, r);
    default: return false;
  }
}

PG_HD bool pg_in_box(const int* row, int X, int Y, int Z) {
  return X >= row[PG_X0] && X <= row[PG_X1] && Y >= row[PG_Y0] && Y <= row[PG_Y1] && Z >= row[PG_Z0] &&
         Z <= row[PG_Z1];
}

// does the volume of `row` hold output voxel (X, Y, Z) of an S^3 part?
PG_HD bool pg_inside(const int* row, int S, int X, int Y, int Z) {
  if (row[PG_CLS] < 0 || !pg_in_box(row, X, Y, Z)) return false;
  int x, y, z;
  pg_canonical(row[PG_ORIENT], S, X, Y, Z, x, y, z);
  return pg_inside_canonical(row, S, x, y, z);
}

// the lowest slot of rows[K][16] whose volume holds the voxel, or -1
PG_HD int pg_first_slot(const int* rows, int K, int S, int X, int Y, int Z) {
  for (int k = 0; k < K; ++k)
    if (pg_inside(rows + k * PG_ROW, S, X, Y, Z)) return k;
  return -1;
}
