// Native voxel data pipeline (host C++17): synthetic machining-feature parts,
// binvox I/O and bit-packing.
//
// FeatureNet-3D (the north-star workload) classifies 24 machining features
// in 64^3 occupancy grids of a stock block.  No dataset can be downloaded
// here, so the framework ships a procedural generator of the same task:
// a solid stock with ONE subtractive feature of random size / position /
// depth, in one of 6 orientations (the access face).  Classes follow the
// FeatureNet taxonomy:
//
//   0 O-ring               8 rect. blind slot      16 2-sides through step
//   1 through hole         9 triangular pocket     17 slanted through step
//   2 blind hole          10 rectangular pocket    18 chamfer
//   3 triangular passage  11 circular end pocket   19 round
//   4 rect. passage       12 triangular blind step 20 vertical circ.-end blind slot
//   5 circ. through slot  13 circular blind step   21 horizontal circ.-end blind slot
//   6 tri. through slot   14 rect. blind step      22 6-sides passage
//   7 rect. through slot  15 rect. through step    23 6-sides pocket
//
// Output is bit-packed (1 bit per voxel, x fastest) so a 64^3 sample is
// 32 KiB on the host / over PCIe; the GPU unpacks to bf16 (misc.hip,
// unpack_bits).  Generation is multi-threaded and deterministic per
// (seed, sample index).  binvox (RLE) read/write keeps the classic voxelised
// CAD file format usable.  sample_parts / carve_parts (at the end) make parts with several
// features and per-voxel labels from integer parameter tables.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../shared/partgen.h"
#include "parallel_for.h"

namespace py = pybind11;

namespace {

constexpr int kNumClasses = 24;

struct Grid {
  int S;
  std::vector<uint8_t> v;  // S^3, index (z*S + y)*S + x
  explicit Grid(int s) : S(s), v((size_t)s * s * s, 1) {}
  uint8_t& at(int x, int y, int z) { return v[((size_t)z * S + y) * S + x]; }
};

// 2-D cross-section predicates in (u, v) plane coordinates relative to a centre
bool in_circle(double u, double v, double r) { return u * u + v * v <= r * r; }
bool in_rect(double u, double v, double a, double b) { return std::fabs(u) <= a && std::fabs(v) <= b; }
bool in_tri(double u, double v, double r) {  // equilateral, pointing +v
  const double h = r * 1.5;
  if (v < -r * 0.5 || v > r) return false;
  const double half = (r - v) / h * (r * std::sqrt(3.0));
  return std::fabs(u) <= half * 0.5 + 1e-9;
}
bool in_hex(double u, double v, double r) {
  u = std::fabs(u);
  v = std::fabs(v);
  return v <= r * std::sqrt(3.0) / 2 && u * std::sqrt(3.0) / 2 + v * 0.5 <= r * std::sqrt(3.0) / 2;
}

// Carve the feature with the access face at z = S-1 (top); depth measured down.
void carve(Grid& g, int cls, std::mt19937_64& rng) {
  const int S = g.S;
  auto U = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
  const double c = (S - 1) / 2.0;
  const double cu = c + U(-0.12, 0.12) * S, cv = c + U(-0.12, 0.12) * S;
  const double r = U(0.12, 0.25) * S;
  const double a = U(0.10, 0.22) * S, b = U(0.10, 0.30) * S;
  const double depth = U(0.25, 0.6) * S;          // blind features
  const double top = S - 1;
  auto sweep = [&](auto&& inside, double d) {       // extrude a section from the top face
    for (int z = 0; z < S; ++z) {
      if (top - z > d) continue;
      for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x)
          if (inside(x - cu, y - cv)) g.at(x, y, z) = 0;
    }
  };
  const double thru = S + 1.0;
  switch (cls) {
    case 0: {  // O-ring groove on the top face
      const double r2 = r * U(0.55, 0.8);
      sweep([&](double u, double v) { return in_circle(u, v, r) && !in_circle(u, v, r2); }, depth * 0.5);
      break;
    }
    case 1: sweep([&](double u, double v) { return in_circle(u, v, r * 0.8); }, thru); break;
    case 2: sweep([&](double u, double v) { return in_circle(u, v, r * 0.8); }, depth); break;
    case 3: sweep([&](double u, double v) { return in_tri(u, v, r); }, thru); break;
    case 4: sweep([&](double u, double v) { return in_rect(u, v, a, b); }, thru); break;
    case 5: {  // circular-ended through slot: rectangle + two half discs, through
      sweep([&](double u, double v) {
        return in_rect(u, v, a, r * 0.5) || in_circle(u - a, v, r * 0.5) || in_circle(u + a, v, r * 0.5);
      }, thru);
      break;
    }
    case 6:  // triangular through slot: V groove across the whole top face
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x) {
            const double dz = top - z;
            if (dz <= depth && std::fabs(x - cu) <= (depth - dz) * 0.6) g.at(x, y, z) = 0;
          }
      break;
    case 7:  // rectangular through slot across the top face
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (top - z <= depth && std::fabs(x - cu) <= a * 0.6) g.at(x, y, z) = 0;
      break;
    case 8:  // rectangular blind slot: open on one side face only
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (top - z <= depth && std::fabs(x - cu) <= a * 0.6 && y <= cv + b) g.at(x, y, z) = 0;
      break;
    case 9: sweep([&](double u, double v) { return in_tri(u, v, r); }, depth); break;
    case 10: sweep([&](double u, double v) { return in_rect(u, v, a, b); }, depth); break;
    case 11:
      sweep([&](double u, double v) {
        return in_rect(u, v, a, r * 0.5) || in_circle(u - a, v, r * 0.5) || in_circle(u + a, v, r * 0.5);
      }, depth);
      break;
    case 12:  // triangular blind step (corner)
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (top - z <= depth && x + y <= 2.2 * r) g.at(x, y, z) = 0;
      break;
    case 13:  // circular blind step at a corner
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (top - z <= depth && in_circle(x, y, 2.0 * r)) g.at(x, y, z) = 0;
      break;
    case 14:  // rectangular blind step at a corner
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (top - z <= depth && x <= 2 * a && y <= 2 * b) g.at(x, y, z) = 0;
      break;
    case 15:  // rectangular through step along one edge
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (top - z <= depth && x <= 2 * a) g.at(x, y, z) = 0;
      break;
    case 16:  // 2-sides through step (two opposite edges)
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (top - z <= depth && (x <= a || x >= S - 1 - a)) g.at(x, y, z) = 0;
      break;
    case 17:  // slanted through step
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if ((top - z) <= depth && x <= 2 * a * (1.0 - (top - z) / depth) + a * 0.5) g.at(x, y, z) = 0;
      break;
    case 18: {  // chamfer on a top edge (45 degree)
      const double w = U(0.15, 0.35) * S;
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (x + (top - z) < w) g.at(x, y, z) = 0;
      break;
    }
    case 19: {  // round (convex fillet) on a top edge
      const double w = U(0.15, 0.35) * S;
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x) {
            const double dx = w - x, dz = w - (top - z);
            if (x < w && (top - z) < w && dx * dx + dz * dz > w * w) g.at(x, y, z) = 0;
          }
      break;
    }
    case 20:  // vertical circular end blind slot: slot from a side face ending in a half disc
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x)
            if (top - z <= depth && ((std::fabs(x - cu) <= r * 0.5 && y <= cv) || in_circle(x - cu, y - cv, r * 0.5)))
              g.at(x, y, z) = 0;
      break;
    case 21:  // horizontal circular end blind slot (semicircular floor)
      for (int z = 0; z < S; ++z)
        for (int y = 0; y < S; ++y)
          for (int x = 0; x < S; ++x) {
            const double dz = top - z;
            if (y <= cv + b && ((dz <= depth - r * 0.5 && std::fabs(x - cu) <= r * 0.5) ||
                                in_circle(x - cu, dz - (depth - r * 0.5), r * 0.5)))
              g.at(x, y, z) = 0;
          }
      break;
    case 22: sweep([&](double u, double v) { return in_hex(u, v, r); }, thru); break;
    case 23: sweep([&](double u, double v) { return in_hex(u, v, r); }, depth); break;
    default: throw std::runtime_error("bad class");
  }
}

// rotate so the access face becomes one of the 6 faces (axis permutation + flip)
void orient(const Grid& src, Grid& dst, int o) {
  const int S = src.S;
  for (int z = 0; z < S; ++z)
    for (int y = 0; y < S; ++y)
      for (int x = 0; x < S; ++x) {
        int X = x, Y = y, Z = z;
        switch (o) {
          case 0: break;                                  // +z
          case 1: Z = S - 1 - z; Y = S - 1 - y; break;    // -z
          case 2: X = z; Z = S - 1 - x; break;            // +x
          case 3: X = S - 1 - z; Z = x; break;            // -x
          case 4: Y = z; Z = S - 1 - y; break;            // +y
          default: Y = S - 1 - z; Z = y; break;           // -y
        }
        dst.v[((size_t)Z * S + Y) * S + X] = src.v[((size_t)z * S + y) * S + x];
      }
}

void gen_one(int S, int cls, uint64_t seed, uint8_t* packed, bool random_orient) {
  std::mt19937_64 rng(seed);
  Grid g(S), o(S);
  carve(g, cls, rng);
  const int ori = random_orient ? (int)(rng() % 6) : 0;
  orient(g, o, ori);
  const size_t n = (size_t)S * S * S;
  std::memset(packed, 0, (n + 7) / 8);
  for (size_t i = 0; i < n; ++i)
    if (o.v[i]) packed[i >> 3] |= (uint8_t)(1u << (i & 7));
}

py::tuple generate(int n, int size, uint64_t seed, int num_classes, bool random_orient, int threads,
                   py::object labels_in) {
  if (size < 8) throw std::runtime_error("voxel grid too small");
  if (num_classes < 1 || num_classes > kNumClasses) throw std::runtime_error("num_classes must be in [1, 24]");
  const size_t per = ((size_t)size * size * size + 7) / 8;
  py::array_t<uint8_t> bits({(py::ssize_t)n, (py::ssize_t)per});
  py::array_t<int64_t> labels(n);
  auto L = labels.mutable_unchecked<1>();
  if (!labels_in.is_none()) {
    auto li = labels_in.cast<py::array_t<int64_t>>();
    auto r = li.unchecked<1>();
    if (r.shape(0) != n) throw std::runtime_error("labels length mismatch");
    for (int i = 0; i < n; ++i) L(i) = r(i);
  } else {
    std::mt19937_64 lr(seed * 7919 + 17);
    for (int i = 0; i < n; ++i) L(i) = (int64_t)(lr() % (uint64_t)num_classes);
  }
  uint8_t* out = bits.mutable_data();
  std::vector<int64_t> lab(n);
  for (int i = 0; i < n; ++i) lab[i] = L(i);
  if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
  threads = std::min(threads, std::max(1, n));
  {
    py::gil_scoped_release nogil;
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
      pool.emplace_back([&, t]() {
        for (int i = t; i < n; i += threads)
          gen_one(size, (int)lab[i], seed * 1000003ULL + (uint64_t)i * 2654435761ULL + 1, out + (size_t)i * per,
                  random_orient);
      });
    for (auto& th : pool) th.join();
  }
  return py::make_tuple(bits, labels);
}

py::array_t<uint8_t> pack_bits(py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dense) {
  const size_t n = (size_t)dense.size();
  py::array_t<uint8_t> out((py::ssize_t)((n + 7) / 8));
  const uint8_t* d = dense.data();
  uint8_t* o = out.mutable_data();
  std::memset(o, 0, (n + 7) / 8);
  for (size_t i = 0; i < n; ++i)
    if (d[i]) o[i >> 3] |= (uint8_t)(1u << (i & 7));
  return out;
}

py::array_t<uint8_t> unpack_bits(py::array_t<uint8_t, py::array::c_style | py::array::forcecast> packed, size_t n) {
  py::array_t<uint8_t> out((py::ssize_t)n);
  const uint8_t* p = packed.data();
  uint8_t* o = out.mutable_data();
  for (size_t i = 0; i < n; ++i) o[i] = (p[i >> 3] >> (i & 7)) & 1u;
  return out;
}

// binvox: "#binvox 1\ndim D D D\ntranslate tx ty tz\nscale s\ndata\n" + RLE (value, count) bytes,
// voxel order x-major in the file (index = x*W*H + z*W + y); we convert to our (z, y, x) layout.
py::tuple read_binvox(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot open " + path);
  std::string line;
  std::getline(f, line);
  if (line.rfind("#binvox", 0) != 0) throw std::runtime_error("not a binvox file");
  int d = 0, h = 0, w = 0;
  double tx = 0, ty = 0, tz = 0, sc = 1;
  while (std::getline(f, line)) {
    std::istringstream is(line);
    std::string key;
    is >> key;
    if (key == "dim") is >> d >> h >> w;
    else if (key == "translate") is >> tx >> ty >> tz;
    else if (key == "scale") is >> sc;
    else if (key == "data") break;
  }
  if (d <= 0 || d != h || h != w) throw std::runtime_error("binvox: only cubic grids supported");
  const size_t n = (size_t)d * h * w;
  std::vector<uint8_t> raw;
  raw.reserve(n);
  uint8_t pair[2];
  while (raw.size() < n && f.read(reinterpret_cast<char*>(pair), 2)) raw.insert(raw.end(), pair[1], pair[0] ? 1 : 0);
  if (raw.size() < n) throw std::runtime_error("binvox: truncated data");
  const int S = d;
  py::array_t<uint8_t> out({S, S, S});
  auto o = out.mutable_unchecked<3>();
  for (int x = 0; x < S; ++x)
    for (int z = 0; z < S; ++z)
      for (int y = 0; y < S; ++y) o(z, y, x) = raw[((size_t)x * S + z) * S + y];
  return py::make_tuple(out, py::make_tuple(tx, ty, tz), sc);
}

void write_binvox(const std::string& path, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> grid,
                  std::vector<double> translate, double scale) {
  if (grid.ndim() != 3 || grid.shape(0) != grid.shape(1) || grid.shape(1) != grid.shape(2))
    throw std::runtime_error("write_binvox: need a cubic [S,S,S] grid");
  const int S = (int)grid.shape(0);
  auto g = grid.unchecked<3>();
  std::ofstream f(path, std::ios::binary);
  f << "#binvox 1\ndim " << S << " " << S << " " << S << "\n";
  if (translate.size() != 3) translate = {0, 0, 0};
  f << "translate " << translate[0] << " " << translate[1] << " " << translate[2] << "\nscale " << scale
    << "\ndata\n";
  uint8_t cur = 2;
  int run = 0;
  auto flush = [&]() {
    if (run > 0) {
      const uint8_t b[2] = {cur, (uint8_t)run};
      f.write(reinterpret_cast<const char*>(b), 2);
    }
  };
  for (int x = 0; x < S; ++x)
    for (int z = 0; z < S; ++z)
      for (int y = 0; y < S; ++y) {
        const uint8_t v = g(z, y, x) ? 1 : 0;
        if (v == cur && run < 255) ++run;
        else { flush(); cur = v; run = 1; }
      }
  flush();
}

// ---------------------------------------------------------------------------------------------
// Multi-feature parts with per-voxel truth: a sampler of parameter tables and the host carving
// path (../shared/partgen.h has the table format; the GPU path is kernels/partgen.hip).
//
// The sampler draws integers only (lo + rng() % span on mt19937_64), so a table is the same on
// every build.  Ranges, in thousandths of s = 4S (the part's edge in quarter voxels) -- smaller
// sizes and wider centres than generate_voxels uses, so that several features fit one part:
constexpr int kPmR[2] = {80, 180};        // r   (holes use 0.8 r, slot ends r / 2, corner steps 2 r / 2.2 r)
constexpr int kPmA[2] = {60, 160};        // a   (slots use 0.6 a, corner and edge steps 2 a)
constexpr int kPmB[2] = {60, 200};        // b   (corner blocks use 2 b)
constexpr int kPmDepth[2] = {150, 500};   // blind depth (the O-ring groove uses half of it)
constexpr int kPmW[2] = {100, 250};       // chamfer / round width
constexpr int kPmCentre = 300;            // |centre offset| from the middle of the face
constexpr int kRingInner[2] = {55, 80};   // O-ring: r2 in percent of r, wall r - r2 >= 2 voxels
constexpr int kRedraws = 64;              // candidates per slot before the slot is given up
constexpr int kRestarts = 16;             // attempts per part before it keeps fewer than min_features

int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
int ceil_div(int a, int b) { return -floor_div(-a, b); }

// One candidate feature of class cls into row[16] (box included).  False: its box misses the part.
bool draw_feature(int S, int cls, std::mt19937_64& rng, int* row) {
  const int s = PG_Q * S, top = PG_Q * (S - 1), thru = s + PG_Q;
  auto pm = [&](const int* range) {
    const int lo = s * range[0] / 1000, hi = s * range[1] / 1000;
    return lo + (int)(rng() % (uint64_t)(hi - lo + 1));
  };
  auto centre = [&]() {
    const int off = s * kPmCentre / 1000;
    return top / 2 - off + (int)(rng() % (uint64_t)(2 * off + 1));
  };
  // every draw is made for every class: the stream does not depend on the class
  const int orient = (int)(rng() % 24);
  const int cu = centre(), cv = centre();
  int r = pm(kPmR), a = pm(kPmA), b = pm(kPmB), depth = pm(kPmDepth);
  const int w = pm(kPmW);
  const int ring = kRingInner[0] + (int)(rng() % (uint64_t)(kRingInner[1] - kRingInner[0] + 1));
  for (int i = 0; i < PG_ROW; ++i) row[i] = 0;
  row[PG_CLS] = cls, row[PG_ORIENT] = orient;
  // the class's fields and its extent [xl, xh] x [yl, yh] x (dz <= dzmax) in quarter voxels, canonical frame
  int xl = 0, xh = top, yl = 0, yh = top, dzmax = 0;
  auto section = [&](int ru, int rv_lo, int rv_hi, int d) {
    row[PG_CU] = cu, row[PG_CV] = cv, row[PG_DEPTH] = d;
    xl = cu - ru, xh = cu + ru, yl = cv + rv_lo, yh = cv + rv_hi, dzmax = d;
  };
  switch (cls) {
    case 0: {
      int r2 = r * ring / 100;
      if (r - r2 < 2 * PG_Q) r2 = std::max(0, r - 2 * PG_Q);
      row[PG_R] = r, row[PG_R2] = r2;
      section(r, -r, r, depth / 2);
      break;
    }
    case 1: case 2: r = r * 8 / 10; row[PG_R] = r; section(r, -r, r, cls == 1 ? thru : depth); break;
    case 3: case 9: row[PG_R] = r; section(r, -(r / 2), r, cls == 3 ? thru : depth); break;
    case 4: case 10: row[PG_A] = a, row[PG_B] = b; section(a, -b, b, cls == 4 ? thru : depth); break;
    case 5: case 11:
      r /= 2;
      row[PG_R] = r, row[PG_A] = a;
      section(a + r, -r, r, cls == 5 ? thru : depth);
      break;
    case 22: case 23: row[PG_R] = r; section(r, -r, r, cls == 22 ? thru : depth); break;
    case 6: section(3 * depth / 5, 0, 0, depth); yl = 0, yh = top; break;
    case 7: a = a * 6 / 10; row[PG_A] = a; section(a, 0, 0, depth); yl = 0, yh = top; break;
    case 8: a = a * 6 / 10; row[PG_A] = a, row[PG_B] = b; section(a, 0, b, depth); yl = 0; break;
    case 12: r = 22 * r / 10; row[PG_R] = r, row[PG_DEPTH] = depth; xh = r, yh = r, dzmax = depth; break;
    case 13: r = 2 * r; row[PG_R] = r, row[PG_DEPTH] = depth; xh = r, yh = r, dzmax = depth; break;
    case 14:
      a *= 2, b *= 2;
      row[PG_A] = a, row[PG_B] = b, row[PG_DEPTH] = depth;
      xh = a, yh = b, dzmax = depth;
      break;
    case 15: a *= 2; row[PG_A] = a, row[PG_DEPTH] = depth; xh = a, dzmax = depth; break;
    case 16: row[PG_A] = a, row[PG_DEPTH] = depth; dzmax = depth; break;
    case 17: row[PG_A] = a, row[PG_DEPTH] = depth; xh = 5 * a / 2, dzmax = depth; break;
    case 18: case 19: row[PG_W] = w; xh = w - 1, dzmax = w - 1; break;
    case 20: r /= 2; row[PG_R] = r; section(r, 0, r, depth); yl = 0; break;
    case 21:
      r /= 2;
      depth = std::max(depth, r + PG_Q);
      row[PG_R] = r, row[PG_B] = b;
      section(r, 0, b, depth);
      yl = 0;
      break;
    default: throw std::runtime_error("bad class");
  }
  // the voxels whose centres lie in the extent, clipped to the part
  int lo[3] = {std::max(0, ceil_div(xl, PG_Q)), std::max(0, ceil_div(yl, PG_Q)),
               std::max(0, S - 1 - floor_div(dzmax, PG_Q))};
  int hi[3] = {std::min(S - 1, floor_div(xh, PG_Q)), std::min(S - 1, floor_div(yh, PG_Q)), S - 1};
  if (dzmax < 0 || lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) return false;
  int p[3], q[3];
  pg_output(orient, S, lo[0], lo[1], lo[2], p[0], p[1], p[2]);
  pg_output(orient, S, hi[0], hi[1], hi[2], q[0], q[1], q[2]);
  for (int d = 0; d < 3; ++d) {
    row[PG_X0 + 2 * d] = std::min(p[d], q[d]);
    row[PG_X0 + 2 * d + 1] = std::max(p[d], q[d]);
  }
  return true;
}

bool boxes_meet(const int* ra, const int* rb, int gap) {   // box of ra grown by gap against box of rb
  for (int d = 0; d < 3; ++d)
    if (ra[PG_X0 + 2 * d] - gap > rb[PG_X0 + 2 * d + 1] || ra[PG_X0 + 2 * d + 1] + gap < rb[PG_X0 + 2 * d])
      return false;
  return true;
}

// One part's table rows[K][16]: the used slots first, the others cls = -1.  Returns the used count.
int sample_one(int S, uint64_t seed, int lo_n, int hi_n, int num_classes, bool separate, int gap, int* rows) {
  const int K = hi_n;
  std::vector<int> best((size_t)K * PG_ROW, 0), cur((size_t)K * PG_ROW), cand(PG_ROW);
  int best_n = -1;
  for (int attempt = 0; attempt < kRestarts && best_n < lo_n; ++attempt) {
    std::mt19937_64 rng(seed + (uint64_t)attempt * 0xD1B54A32D192ED03ULL);
    const int want = lo_n + (int)(rng() % (uint64_t)(hi_n - lo_n + 1));
    int kept = 0;
    for (int slot = 0; slot < want; ++slot)
      for (int t = 0; t < kRedraws; ++t) {
        const int cls = (int)(rng() % (uint64_t)num_classes);
        if (!draw_feature(S, cls, rng, cand.data())) continue;
        bool clash = false;
        for (int j = 0; separate && j < kept && !clash; ++j)
          clash = boxes_meet(cand.data(), &cur[(size_t)j * PG_ROW], gap) ||
                  boxes_meet(&cur[(size_t)j * PG_ROW], cand.data(), gap);
        if (clash) continue;
        std::copy(cand.begin(), cand.end(), cur.begin() + (size_t)kept * PG_ROW);
        ++kept;
        break;
      }
    if (kept > best_n) {
      best_n = kept;
      std::copy(cur.begin(), cur.begin() + (size_t)kept * PG_ROW, best.begin());
    }
  }
  for (int k = 0; k < K; ++k)
    for (int f = 0; f < PG_ROW; ++f)
      rows[k * PG_ROW + f] = k < best_n ? best[(size_t)k * PG_ROW + f] : (f == PG_CLS ? -1 : 0);
  return std::max(best_n, 0);
}

py::array_t<int32_t> sample_parts(int n, int size, uint64_t seed, int min_features, int max_features,
                                  int num_classes, bool separate, int gap, int threads) {
  if (n < 0) throw std::runtime_error("sample_parts: n must not be negative");
  if (size < 8 || size > PG_MAX_S || size % 8 != 0)
    throw std::runtime_error("sample_parts: size must be a multiple of 8 in [8, 256]");
  if (min_features < 0 || max_features < min_features || max_features > PG_MAX_K)
    throw std::runtime_error("sample_parts: need 0 <= min_features <= max_features <= 32");
  if (num_classes < 1 || num_classes > kNumClasses) throw std::runtime_error("num_classes must be in [1, 24]");
  if (gap < 0) throw std::runtime_error("sample_parts: gap must not be negative");
  py::array_t<int32_t> out({(py::ssize_t)n, (py::ssize_t)max_features, (py::ssize_t)PG_ROW});
  int32_t* o = out.mutable_data();
  const size_t per = (size_t)max_features * PG_ROW;
  {
    py::gil_scoped_release nogil;
    if (per)
      parallel_for(n, threads, [&](int i) {
        sample_one(size, seed * 1000003ULL + (uint64_t)i * 2654435761ULL + 0x9E3779B97F4A7C15ULL, min_features,
                   max_features, num_classes, separate, gap, o + (size_t)i * per);
      });
  }
  return out;
}

py::tuple carve_parts(py::array_t<int32_t, py::array::c_style | py::array::forcecast> params, int size, int threads) {
  if (params.ndim() != 3 || params.shape(2) != PG_ROW)
    throw std::runtime_error("carve_parts: params must be int32 [N, K, 16]");
  if (size < 8 || size > PG_MAX_S || size % 8 != 0)
    throw std::runtime_error("carve_parts: size must be a multiple of 8 in [8, 256]");
  if (params.shape(1) > PG_MAX_K) throw std::runtime_error("carve_parts: at most 32 feature slots per part");
  const int N = (int)params.shape(0), K = (int)params.shape(1), S = size;
  const std::vector<py::ssize_t> shape{N, S, S, S};
  py::array_t<uint8_t> occ(shape), labels(shape), slots(shape);
  const int32_t* p = params.data();
  uint8_t *po = occ.mutable_data(), *pl = labels.mutable_data(), *ps = slots.mutable_data();
  {
    py::gil_scoped_release nogil;
    parallel_for(N * S, threads, [&](int item) {     // one z plane of one part
      const int n = item / S, Z = item % S;
      const int* rows = p + (size_t)n * K * PG_ROW;
      size_t g = ((size_t)n * S + Z) * S * S;
      for (int Y = 0; Y < S; ++Y)
        for (int X = 0; X < S; ++X, ++g) {
          const int k = pg_first_slot(rows, K, S, X, Y, Z);
          po[g] = k < 0;
          pl[g] = k < 0 ? 0 : (uint8_t)(rows[k * PG_ROW + PG_CLS] + 1);
          ps[g] = (uint8_t)(k + 1);
        }
    });
  }
  return py::make_tuple(occ, labels, slots);
}

}  // namespace

void register_voxel(py::module_& m) {
  m.def("sample_parts", &sample_parts, py::arg("n"), py::arg("size") = 64, py::arg("seed") = 0,
        py::arg("min_features") = 1, py::arg("max_features") = 4, py::arg("num_classes") = 24,
        py::arg("separate") = true, py::arg("gap") = 1, py::arg("threads") = 0,
        "n parameter tables of multi-feature parts -> int32 [n, max_features, 16]");
  m.def("carve_parts", &carve_parts, py::arg("params"), py::arg("size"), py::arg("threads") = 0,
        "parts of the tables int32 [N, K, 16] -> (occupancy, labels, slots), each uint8 [N, S, S, S]");
  m.attr("NUM_FEATURE_CLASSES") = kNumClasses;
  m.def("generate_voxels", &generate, py::arg("n"), py::arg("size") = 64, py::arg("seed") = 0,
        py::arg("num_classes") = 24, py::arg("random_orient") = true, py::arg("threads") = 0,
        py::arg("labels") = py::none(),
        "n synthetic machining-feature parts -> (bit-packed uint8 [n, S^3/8], int64 labels [n])");
  m.def("pack_bits", &pack_bits);
  m.def("unpack_bits", &unpack_bits, py::arg("packed"), py::arg("n"));
  m.def("read_binvox", &read_binvox);
  m.def("write_binvox", &write_binvox, py::arg("path"), py::arg("grid"),
        py::arg("translate") = std::vector<double>{0, 0, 0}, py::arg("scale") = 1.0);
}
