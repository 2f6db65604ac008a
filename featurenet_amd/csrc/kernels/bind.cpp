// pybind11 surface of the featurenet_amd HIP kernel library (module `_C`).
//
// Every entry point takes raw device addresses (Python ints from
// tensor.data_ptr()) and the HIP stream handle of the caller's current torch
// stream, so the Python op layer owns allocation and the kernels can be
// captured into hipGraphs.  Errors raise RuntimeError with the HIP message.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace py = pybind11;

extern "C" {
int fn_igemm_fwd(const void*, const void*, const float*, void*, float*, const int*, const int*, long long, int, int,
                 int, int, int, hipStream_t, float*, int);
int fn_igemm_fwd_splits(long long, int, int);
int fn_igemm_fwd_mblocks(long long);
int fn_conv_halo(const void*, const void*, const float*, void*, float*, const int*, const int*, int, int, int*,
                 hipStream_t);
long long fn_conv_halo_lds(const int*, int);
int fn_conv_halo_workers(const int*, int);
int fn_pw_fwd(const void*, const void*, const float*, void*, long long, int, int, int, hipStream_t, const float*,
              const float*, int, const void*, const float*, const float*, float*, int);
int fn_seghead_part_len();
int fn_part_reduce(const float*, float*, long long, int, int, hipStream_t);
int fn_seghead_blocks(long long);
int fn_seghead_loss(const void*, const float*, const float*, const void*, const float*, const void*, void*, float*,
                    long long, int, int, int, float, float, hipStream_t, int, int);
int fn_pw_xent_blocks(long long);
int fn_pw_fwd_xent(const void*, const void*, const float*, void*, long long, int, int, const float*, const float*, int,
                   const long long*, float*, float, float, hipStream_t);
int fn_pw_fwd_blocks(long long, int, int);
int fn_pw_argmax_blocks(long long, int, int);
int fn_pw_argmax(const void*, const void*, const float*, void*, void*, long long, int, int, const float*,
                 const float*, int, hipStream_t);
int fn_pw_argmax_cm_blocks(long long, int, int);
int fn_pw_argmax_cm(const void*, const void*, const float*, const void*, void*, void*, void*, long long, int, int, int,
                    const float*, const float*, int, hipStream_t);
void fn_ccl_tile(int*);
int fn_ccl_local(const void*, void*, int, int, int, int, int, int, hipStream_t);
int fn_ccl_merge(const void*, void*, int, int, int, int, int, int, hipStream_t);
int fn_ccl_flatten(void*, void*, int, int, int, int, hipStream_t);
int fn_ccl_stats(const void*, const void*, const void*, void*, void*, int, int, int, int, long long, hipStream_t);
int fn_partgen_chunk();
int fn_partgen_carve(const void*, void*, void*, void*, void*, int, int, int, hipStream_t);
int fn_voxelize_planes(int);
int fn_voxelize_tris(const void*, const void*, void*, void*, void*, int, int, int, int, hipStream_t);
int fn_mesh_votes_thread_cols();
int fn_mesh_votes(const void*, const void*, const void*, void*, void*, int, int, int, int, int, hipStream_t);
void fn_overlap_chunk(int*);
int fn_overlap_pairs(const void*, const void*, const void*, const void*, void*, void*, void*, int, long long, int,
                     long long, long long, hipStream_t);
void fn_access_chunk(int*);
int fn_access_extents(const void*, void*, void*, void*, int, int, int, int, hipStream_t);
int fn_access_stats(const void*, const void*, const void*, const void*, const void*, void*, void*, int, int, int, int,
                    long long, hipStream_t);
void fn_edt_chunk(int*);
int fn_edt_transform(const void*, void*, void*, int, int, int, int, int, int, hipStream_t);
int fn_edt_stats(const void*, const void*, const void*, void*, int, int, int, int, long long, hipStream_t);
void fn_nn_chunk(int*);
int fn_nn_transform(const void*, void*, void*, int, int, int, int, int, hipStream_t);
int fn_wall_stats(const void*, const void*, const void*, void*, int, int, int, int, long long, int, hipStream_t);
void fn_reach_chunk(int*);
int fn_reach_scan(const void*, void*, int, int, int, int, hipStream_t);
int fn_reach_stats(const void*, const void*, const void*, const void*, void*, int, int, int, int, long long, int, int,
                   hipStream_t);
int fn_isolate_parts(const void*, const void*, void*, int, int, int, int, long long, int, int, hipStream_t);
void fn_contact_chunk(int*);
int fn_contact_stats(const void*, const void*, const void*, void*, void*, void*, void*, int, int, int, int, long long,
                     long long, long long, hipStream_t);
void fn_ws_tile(int*);
int fn_ws_ascend(const void*, const void*, void*, int, int, int, int, int, hipStream_t);
int fn_ws_resolve(const void*, void*, void*, int, int, int, int, hipStream_t);
int fn_ws_saddle(const void*, const void*, const void*, const void*, void*, void*, void*, int, int, int, int, long long,
                 long long, long long, hipStream_t);
int fn_pw_wgrad(const void*, const void*, float*, long long, int, int, hipStream_t, const float*, const float*, int,
                float*);
int fn_pw_wgrad_blocks(long long, int, int);
int fn_conv_halo_wgrad_yblocks(const int*, int);
int fn_conv_halo_f8(const void*, const void*, const float*, const float*, void*, float, const int*, const int*, int,
                    int, int, hipStream_t);
int fn_quant_fp8(const void*, void*, long long, float, hipStream_t);
int fn_quant_fp8_block(const void*, void*, void*, long long, int, hipStream_t);
int fn_mfma_scale_probe(const void*, const void*, const int*, const int*, float*, hipStream_t);
int fn_s2d_tap_f8(const void*, void*, int, int, int, int, int, int, int, int, float, int, hipStream_t);
int fn_dw_fwd(const void*, const float*, const float*, void*, const int*, int, hipStream_t);
int fn_dw_dgrad(const void*, const float*, void*, const int*, hipStream_t);
int fn_dw_wgrad(const void*, const void*, float*, const int*, int, hipStream_t, float*);
int fn_conv_halo_wgrad(const void*, const void*, float*, float*, const int*, int, int, hipStream_t);
int fn_conv_halo_wgrad_gx(const int*, int);
int fn_s2d_pack(const void*, void*, const int*, int, hipStream_t, int);
int fn_dense_splits(int, int, int);
int fn_ew_binary(const void*, const void*, void*, long long, int, hipStream_t);
int fn_ew_mul_bwd(const void*, const void*, const void*, void*, void*, long long, hipStream_t);
int fn_concat2(void*, void*, void*, long long, int, int, int, hipStream_t);
int fn_pad3(void*, void*, const int*, int, hipStream_t);
int fn_pad_channels(void*, void*, long long, int, int, int, hipStream_t);
int fn_dense_fwd(const void*, const void*, const float*, void*, float*, int, int, int, int, int, int, int, hipStream_t);
int fn_dense_dgrad(const void*, const float*, void*, int, int, int, hipStream_t, const void*, int);
int fn_dense_wgrad(const void*, const void*, float*, float*, int, int, int, float*, int, hipStream_t, const void*, int);
int fn_dense_wgrad_slices(int, int, int);
int fn_s2d_weight_map(const float*, float*, const int*, int, hipStream_t);
int fn_subpixel_wmap(const float*, float*, int, int, int, hipStream_t);
int fn_halo_pack_w(const float*, void*, int, int, int, int, int, int, int, hipStream_t);
int fn_igemm_pack_w(const float*, void*, int, int, int, int, int, int, int, int, int, hipStream_t);
int fn_pack_w_multi(const long long*, int, hipStream_t);
int fn_igemm_wgrad(const void*, const void*, float*, const int*, const int*, long long, int, int, int, int,
                   hipStream_t, int, int, const void*, int, float*, int, float*);
long long fn_igemm_wgrad_part(int, int, int, int, int, int, int);
int fn_colstats(const void*, const void*, const float*, const float*, const float*, const float*, float*, long long,
                int, int, int, int, hipStream_t);
int fn_bn_finalize(const float*, int, int, double, const float*, const float*, float*, float*, float, float, float*,
                   float*, float*, float*, int, hipStream_t);
int fn_bn_apply(const void*, const float*, const float*, void*, long long, int, int, hipStream_t, void*);
int fn_bn_wdot(const float*, const float*, float*, int, int, int, hipStream_t);
int fn_bn_bwd_prep(const float*, int, const float*, int, int, double, const float*, const float*, const float*,
                   const float*, const float*, const float*, float*, float*, const void*, const void*, long long,
                   hipStream_t);
int fn_bn_bwd_apply_k_blocks(long long, int);
int fn_bn_bwd_apply_k(const void*, const void*, const float*, const float*, const float*, const float*, void*,
                      long long, int, float*, int, hipStream_t);
int fn_bn_bwd_apply(const void*, const void*, const float*, const float*, const float*, const float*, const float*,
                    const float*, void*, long long, int, float, int, hipStream_t);
int fn_bn_bwd_apply_s2d(const void*, const void*, const float*, const float*, const float*, const float*,
                        const float*, const float*, void*, int, int, int, int, int, float, int, hipStream_t);
int fn_pool_fwd(const void*, void*, const float*, const float*, const int*, int, int, int, hipStream_t);
int fn_pool_bwd(const void*, const void*, void*, const float*, const float*, const int*, int, int, int, hipStream_t);
int fn_pool_bwd_stats_blocks(const int*);
int fn_colstats_blocks(long long, int, int, int);
int fn_pool_bn_bwd_apply(const void*, const void*, const float*, const float*, const float*, const float*,
                         const float*, const float*, void*, const int*, int, float, hipStream_t);
int fn_pool_bwd_stats(const void*, const void*, void*, const float*, const float*, const int*, int, float*,
                      hipStream_t);
int fn_softmax_xent_blocks(long long, int);
int fn_upsample2x(const void*, void*, int, int, int, int, int, int, hipStream_t);
int fn_softmax_xent_rows(const void*, int, const long long*, float*, void*, int*, long long, int, float, float,
                         hipStream_t);
int fn_adam_flat_dev(float*, const float*, float*, float*, void*, long long, const float*, int*, int, hipStream_t);
int fn_adam_flat(float*, const float*, float*, float*, void*, long long, float, float, float, float, float, float,
                 float, float, int, hipStream_t);
int fn_sgd_flat(float*, const float*, float*, void*, long long, float, float, float, int, float, hipStream_t);
int fn_bias_act(const void*, const float*, void*, long long, int, int, hipStream_t);
int fn_act_bwd(const void*, const void*, void*, long long, int, hipStream_t);
int fn_dropout(const void*, void*, long long, float, unsigned, unsigned, hipStream_t);
int fn_cast_f32_bf16(const float*, void*, long long, hipStream_t);
int fn_scale_unless_one(void*, int, const float*, long long, hipStream_t);
int fn_copy2(void*, const void*, long long, void*, const void*, long long, hipStream_t);
int fn_cu_occupy(int, int, int, void*, hipStream_t);
int fn_softmax_rows(const float*, float*, long long, int, int, const float*, hipStream_t);
int fn_unpack_bits(const void*, void*, long long, hipStream_t);
int fn_conv_tile(const void*, const void*, const void*, const void*, const void*, const float*, void*, float*,
                 const int*, int, int, int, int, int*, hipStream_t, const void*, const float*, float, void*);
int fn_conv_tile_workers(const int*, int, int);
int fn_conv_tile_slab_rows(const int*, int, int);
void fn_conv_tile_grid_cap(int);
void fn_conv_tile_set_schedule(int);
int fn_conv_tile_schedule();
int fn_conv_tile_f8(const void*, const void*, const void*, const void*, const void*, const float*, const float*, void*,
                    float, const int*, int, int, int, int, int*, hipStream_t, const void*, void*);
int fn_conv_tile_f8_supported(int, int, int);
int fn_conv_wtile(const void*, const void*, float*, float*, const void*, const void*, const void*, const int*, int, int,
                  int*, hipStream_t, const float*, float*, const float*, int);
int fn_conv_wtile_supported(int, int);
int fn_conv_wtile_prologue_built();
int fn_tile_pack_w(const float*, void*, int, int, int, int, int, int, int, int, int, hipStream_t);
int fn_tile_pack_w2(const float*, void*, void*, int, int, int, const int*, const int*, hipStream_t);
}

template <typename T>
static T P(uintptr_t a) {
  return reinterpret_cast<T>(a);
}
static hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

static void chk(int rc, const char* what) {
  if (rc == 0) return;
  if (rc < 0) throw std::runtime_error(std::string(what) + ": unsupported configuration (code " + std::to_string(rc) + ")");
  throw std::runtime_error(std::string(what) + ": " + hipGetErrorString((hipError_t)rc));
}

static void need(const std::vector<int>& v, size_t n, const char* what) {
  if (v.size() != n) throw std::runtime_error(std::string(what) + ": bad geometry length");
}

// Extent checks: the geometry implies how many elements every kernel operand
// spans; the caller passes the numel of the tensors it hands over (``ext``),
// and a geometry/tensor mismatch raises here instead of reading or writing
// out of bounds on the GPU.  ``ext`` may be empty (no check) for internal
// callers that size their own scratch.
static void fits(const std::vector<long long>& ext, size_t i, long long need_elems, const char* what,
                 const char* operand) {
  if (ext.empty()) return;
  if (i >= ext.size()) throw std::runtime_error(std::string(what) + ": missing extent for " + operand);
  if (need_elems < 0 || ext[i] < need_elems)
    throw std::runtime_error(std::string(what) + ": " + operand + " has " + std::to_string(ext[i]) +
                             " elements, geometry needs " + std::to_string(need_elems));
}
static long long prod(std::initializer_list<long long> v) {
  long long r = 1;
  for (long long x : v) {
    if (x < 0) return -1;
    r *= x;
  }
  return r;
}
// halo geometry: N ID IH IW C | OD OH OW | KD KH KW | pd ph pw | TD TH TW
static void check_halo(const std::vector<int>& g, const std::vector<long long>& ext, int ncol, bool wgrad,
                       const char* what) {
  const long long src = prod({g[0], g[1], g[2], g[3], g[4]});
  const long long out = prod({g[0], g[5], g[6], g[7], ncol});
  const int T = g[8] * g[9] * g[10];
  if (g[4] <= 0 || ncol <= 0 || T <= 0) throw std::runtime_error(std::string(what) + ": empty geometry");
  if (g[5] > g[1] + 2 * g[11] || g[6] > g[2] + 2 * g[12] || g[7] > g[3] + 2 * g[13])
    throw std::runtime_error(std::string(what) + ": output larger than the padded input");
  if (wgrad) {                       // ext = {dy, src, dw}
    fits(ext, 0, out, what, "dy");
    fits(ext, 1, src, what, "src");
    fits(ext, 2, prod({ncol, T, g[4]}), what, "dw");
  } else {                           // ext = {src, wt, out, toffs}
    const int cs = g[4] % 16 == 0 ? 16 : 8, tps = 128 / cs;
    const long long Tp = (T + tps - 1) / tps * tps;
    fits(ext, 0, src, what, "src");
    fits(ext, 1, prod({ncol, g[4], Tp}), what, "wt");
    fits(ext, 2, out, what, "out");
    fits(ext, 3, Tp, what, "toffs");
  }
}

// tile geometry: halo geometry (17) | CS HPpad nks nct mHW mHHW BUF mTW mTH; ext = {src, wpk, out, rowtab rows}
// elements an output view (geometry entries 26-30: osn, ob, osd, osh, osw) spans
static long long view_extent(const std::vector<int>& g, int ncol) {
  if (g[26] < 0 || g[27] < 0 || g[28] < 0 || g[29] < 0 || g[30] < 0) throw std::runtime_error("conv_tile: bad output view");
  return ((long long)(g[0] - 1) * g[26] + g[27] + (long long)(g[5] - 1) * g[28] + (long long)(g[6] - 1) * g[29] +
          (long long)(g[7] - 1) * g[30] + 1) * ncol;
}

static void check_tile(const std::vector<int>& g, const std::vector<long long>& ext, int ncol, int MT,
                       const char* what, int NT = 2) {
  if (g[4] <= 0 || ncol <= 0 || g[17] <= 0 || g[4] % g[17]) throw std::runtime_error(std::string(what) + ": bad slice");
  if (g[5] > g[1] + 2 * g[11] + g[8] || g[6] > g[2] + 2 * g[12] + g[9] || g[7] > g[3] + 2 * g[13] + g[10])
    throw std::runtime_error(std::string(what) + ": output larger than the padded input");
  fits(ext, 0, prod({g[0], g[1], g[2], g[3], g[4]}), what, "src");
  // the stream's rows (+ 4 zero ring k-steps) x nct fragments, of which the last row is read up to the
  // ncol columns' fragments (a view may start inside a wider stream: the sub-pixel class weights)
  const long long ncb = (ncol + NT * 16 - 1) / (NT * 16);
  fits(ext, 1, ((long long)(g[4] / g[17] * g[19] + 3) * g[20] + ncb * NT) * 64 * 8, what, "wpk");
  fits(ext, 2, view_extent(g, ncol), what, "out");
  fits(ext, 3, 4LL * MT * 16, what, "rowtab");
  fits(ext, 4, g[19] + 6LL, what, "ktab");
}

PYBIND11_MODULE(_C, m) {
  m.doc() = "featurenet_amd gfx950 HIP kernels";
  m.attr("ARCH") = "gfx950";

  // part / splits (optional): the split-K form (fn_igemm_fwd_splits), part = splits x M x N floats
  m.def("igemm_fwd", [](uintptr_t src, uintptr_t wt, uintptr_t bias, uintptr_t out, uintptr_t stats, uintptr_t tab,
                        std::vector<int> geom, long long M, int N, int K, int ldw, int vec, int act, uintptr_t st,
                        uintptr_t part, int splits, long long part_elems) {
    need(geom, 14, "igemm_fwd");
    if (splits > 1 && part_elems < (long long)splits * M * N)
      throw std::runtime_error("igemm_fwd: part has " + std::to_string(part_elems) + " elements, split-K needs " +
                               std::to_string((long long)splits * M * N));
    chk(fn_igemm_fwd(P<const void*>(src), P<const void*>(wt), P<const float*>(bias), P<void*>(out), P<float*>(stats),
                     P<const int*>(tab), geom.data(), M, N, K, ldw, vec, act, S(st), P<float*>(part), splits),
        "igemm_fwd");
  }, py::arg("src"), py::arg("wt"), py::arg("bias"), py::arg("out"), py::arg("stats"), py::arg("tab"), py::arg("geom"),
     py::arg("M"), py::arg("N"), py::arg("K"), py::arg("ldw"), py::arg("vec"), py::arg("act"), py::arg("st"),
     py::arg("part") = 0, py::arg("splits") = 1, py::arg("part_elems") = 0);
  m.def("igemm_fwd_splits", &fn_igemm_fwd_splits);
  m.def("igemm_fwd_mblocks", &fn_igemm_fwd_mblocks);
  m.def("conv_halo", [](uintptr_t src, uintptr_t wt, uintptr_t bias, uintptr_t out, uintptr_t stats,
                        uintptr_t toffs, std::vector<int> geom, int ncol, int act, uintptr_t sched, uintptr_t st,
                        std::vector<long long> ext) {
    need(geom, 17, "conv_halo");
    check_halo(geom, ext, ncol, false, "conv_halo");
    chk(fn_conv_halo(P<const void*>(src), P<const void*>(wt), P<const float*>(bias), P<void*>(out), P<float*>(stats),
                     P<const int*>(toffs), geom.data(), ncol, act, P<int*>(sched), S(st)),
        "conv_halo");
  }, py::arg("src"), py::arg("wt"), py::arg("bias"), py::arg("out"), py::arg("stats"), py::arg("toffs"),
     py::arg("geom"), py::arg("ncol"), py::arg("act"), py::arg("sched"), py::arg("st"),
     py::arg("ext") = std::vector<long long>());
  // part: fp32 scratch of conv_halo_wgrad_gx(geom, grid_x) x cout x taps x C (the per-workgroup
  // partial weight gradients, added into dw in a fixed order); ext = {dy, src, dw, part}
  m.def("conv_halo_wgrad", [](uintptr_t dy, uintptr_t src, uintptr_t dw, uintptr_t part, std::vector<int> geom,
                              int cout, int grid_x, uintptr_t st, std::vector<long long> ext) {
    need(geom, 17, "conv_halo_wgrad");
    check_halo(geom, ext, cout, true, "conv_halo_wgrad");
    const int gx = fn_conv_halo_wgrad_gx(geom.data(), grid_x);
    fits(ext, 3, prod({gx, cout, geom[8] * geom[9] * geom[10], geom[4]}), "conv_halo_wgrad", "part");
    chk(fn_conv_halo_wgrad(P<const void*>(dy), P<const void*>(src), P<float*>(dw), P<float*>(part), geom.data(), cout,
                           grid_x, S(st)),
        "conv_halo_wgrad");
  }, py::arg("dy"), py::arg("src"), py::arg("dw"), py::arg("part"), py::arg("geom"), py::arg("cout"),
     py::arg("grid_x"), py::arg("st"), py::arg("ext") = std::vector<long long>());
  m.def("conv_halo_wgrad_gx", [](std::vector<int> geom, int grid_x) {
    need(geom, 17, "conv_halo_wgrad_gx");
    return fn_conv_halo_wgrad_gx(geom.data(), grid_x);
  });
  m.def("conv_tile", [](uintptr_t src, uintptr_t wpk, uintptr_t rowtab, uintptr_t ktab, uintptr_t zp, uintptr_t bias,
                        uintptr_t out, uintptr_t stats, std::vector<int> geom, int ncol, int act, int MT, int NT,
                        uintptr_t sched, uintptr_t st, std::vector<long long> ext, uintptr_t bny, uintptr_t bnp,
                        float oscale, uintptr_t osc, long long osc_n) {
    need(geom, 31, "conv_tile");
    check_tile(geom, ext, ncol, MT, "conv_tile", NT);
    // osc: block scales of an e4m3 output, one dword per output position
    if (osc && osc_n < view_extent(geom, 1)) throw std::runtime_error("conv_tile: osc smaller than the output");
    if (bny && bnp) {   // ext[5] = numel of the BN input (the output's shape), ext[6] = numel of bnp
      fits(ext, 5, view_extent(geom, ncol), "conv_tile", "bny");
      fits(ext, 6, 4LL * ncol, "conv_tile", "bnp");
    } else if (bny) {   // the relu-mask bytes: ext[5] = their count (one per 8 output columns)
      fits(ext, 5, view_extent(geom, ncol) / 8, "conv_tile", "mask");
    }
    chk(fn_conv_tile(P<const void*>(src), P<const void*>(wpk), P<const void*>(rowtab), P<const void*>(ktab),
                     P<const void*>(zp), P<const float*>(bias), P<void*>(out), P<float*>(stats), geom.data(), ncol,
                     act, MT, NT, P<int*>(sched), S(st), P<const void*>(bny), P<const float*>(bnp), oscale,
                     P<void*>(osc)),
        "conv_tile");
  }, py::arg("src"), py::arg("wpk"), py::arg("rowtab"), py::arg("ktab"), py::arg("zp"), py::arg("bias"), py::arg("out"),
     py::arg("stats"), py::arg("geom"), py::arg("ncol"), py::arg("act"), py::arg("MT"), py::arg("NT"),
     py::arg("sched"), py::arg("st"), py::arg("ext") = std::vector<long long>(), py::arg("bny") = 0,
     py::arg("bnp") = 0, py::arg("oscale") = 0.f, py::arg("osc") = 0, py::arg("osc_n") = 0);
  m.def("conv_tile_f8", [](uintptr_t src, uintptr_t wpk, uintptr_t rowtab, uintptr_t ktab, uintptr_t zp,
                           uintptr_t scale, uintptr_t bias, uintptr_t out, float oscale, std::vector<int> geom, int ncol,
                           int relu, int MT, int NT, uintptr_t st, uintptr_t sched, std::vector<long long> ext,
                           uintptr_t xsc, uintptr_t osc) {
    need(geom, 31, "conv_tile_f8");
    // xsc / osc: block scales (a dword per input / output position): ext[5] / ext[6] their counts
    if (xsc) fits(ext, 5, prod({geom[0], geom[1], geom[2], geom[3]}), "conv_tile_f8", "xsc");
    if (osc) fits(ext, 6, view_extent(geom, 1), "conv_tile_f8", "osc");
    if (geom[4] <= 0 || ncol <= 0 || geom[17] <= 0 || geom[4] % geom[17])
      throw std::runtime_error("conv_tile_f8: bad slice");
    fits(ext, 0, prod({geom[0], geom[1], geom[2], geom[3], geom[4]}), "conv_tile_f8", "src");
    fits(ext, 1, prod({geom[4] / geom[17] * geom[19] + 4, geom[20], 64, 32}), "conv_tile_f8", "wpk");
    fits(ext, 2, (relu & 2) ? prod({geom[0], geom[5] / 2, geom[6] / 2, geom[7] / 2, ncol}) : view_extent(geom, ncol),
         "conv_tile_f8", "out");
    fits(ext, 3, 4LL * MT * 16, "conv_tile_f8", "rowtab");
    fits(ext, 4, geom[19] + 6LL, "conv_tile_f8", "ktab");
    chk(fn_conv_tile_f8(P<const void*>(src), P<const void*>(wpk), P<const void*>(rowtab), P<const void*>(ktab),
                        P<const void*>(zp), P<const float*>(scale), P<const float*>(bias), P<void*>(out), oscale,
                        geom.data(), ncol, relu, MT, NT, P<int*>(sched), S(st), P<const void*>(xsc), P<void*>(osc)),
        "conv_tile_f8");
  }, py::arg("src"), py::arg("wpk"), py::arg("rowtab"), py::arg("ktab"), py::arg("zp"), py::arg("scale"),
     py::arg("bias"), py::arg("out"), py::arg("oscale"), py::arg("geom"), py::arg("ncol"), py::arg("relu"),
     py::arg("MT"), py::arg("NT"), py::arg("st"), py::arg("sched"), py::arg("ext") = std::vector<long long>(),
     py::arg("xsc") = 0, py::arg("osc") = 0);
  m.def("conv_tile_f8_supported", &fn_conv_tile_f8_supported);
  m.def("conv_wtile", [](uintptr_t x, uintptr_t dy, uintptr_t dw, uintptr_t part, uintptr_t rowtab, uintptr_t postab,
                         uintptr_t zp, std::vector<int> geom, int nacc, int workers, uintptr_t sched, uintptr_t st,
                         std::vector<long long> ext, uintptr_t wsrc, uintptr_t wdp, uintptr_t pst, int pact) {
    need(geom, 24, "conv_wtile");
    // the BN prologue: pst = [scale C][shift C] of x's channels (ext[8] = its element count)
    if (pst) fits(ext, 8, 2LL * geom[4], "conv_wtile", "pst");
    const long long T = (long long)geom[9] * geom[10] * geom[11];
    fits(ext, 0, prod({geom[0], geom[1], geom[2], geom[3], geom[4]}), "conv_wtile", "x");
    const bool sp = (nacc >> 14) & 1;             // sub-pixel form: dy = [N, OD+1, OH+1, OW+1, 8 K]
    if (sp)
      fits(ext, 1, prod({geom[0], geom[5] + 1, geom[6] + 1, geom[7] + 1, 8 * geom[8]}), "conv_wtile", "dy");
    else
      fits(ext, 1, prod({geom[0], geom[5], geom[6], geom[7], geom[8]}), "conv_wtile", "dy");
    const long long tw = sp ? 64 : T;             // (sub-pixel form: 8 classes x 8 folded taps)
    fits(ext, 2, prod({geom[8], tw, geom[4]}), "conv_wtile", "dw");
    fits(ext, 3, 32LL * geom[19], "conv_wtile", "rowtab");
    fits(ext, 4, geom[18], "conv_wtile", "postab");
    fits(ext, 5, 8LL * workers * ((nacc >> 13) & 1 ? 2 : 1) * geom[8] * tw * geom[4], "conv_wtile", "part");
    if (wsrc) {                                   // S = sum W . dW partials: [ceil(dW / 256)][C], W like dW
      fits(ext, 6, prod({geom[8], tw, geom[4]}), "conv_wtile", "wsrc");
      fits(ext, 7, (prod({geom[8], tw, geom[4]}) + 255) / 256 * geom[4], "conv_wtile", "wdp");
    }
    if (geom[5] > geom[1] + 2 * geom[12] || geom[6] > geom[2] + 2 * geom[13] || geom[7] > geom[3] + 2 * geom[14])
      throw std::runtime_error("conv_wtile: output larger than the padded input");
    chk(fn_conv_wtile(P<const void*>(x), P<const void*>(dy), P<float*>(dw), P<float*>(part), P<const void*>(rowtab),
                      P<const void*>(postab), P<const void*>(zp), geom.data(), nacc, workers, P<int*>(sched), S(st),
                      P<const float*>(wsrc), P<float*>(wdp), P<const float*>(pst), pact),
        "conv_wtile");
  }, py::arg("x"), py::arg("dy"), py::arg("dw"), py::arg("part"), py::arg("rowtab"), py::arg("postab"), py::arg("zp"),
     py::arg("geom"), py::arg("nacc"), py::arg("workers"), py::arg("sched"), py::arg("st"),
     py::arg("ext") = std::vector<long long>(), py::arg("wsrc") = 0, py::arg("wdp") = 0, py::arg("pst") = 0,
     py::arg("pact") = 0);
  m.def("conv_wtile_supported", &fn_conv_wtile_supported);
  m.def("conv_wtile_prologue_built", &fn_conv_wtile_prologue_built);
  m.def("conv_tile_workers", [](std::vector<int> geom, int ncol, int NT) {
    need(geom, 31, "conv_tile_workers");
    return fn_conv_tile_workers(geom.data(), ncol, NT);
  });
  m.def("conv_tile_grid_cap", [](int cap) { fn_conv_tile_grid_cap(cap); });   // (tests: grid independence)
  // the BN-statistics tile schedule: -1 = FN_TILE_SCHED (default static), 0 static, 1 chunked
  m.def("conv_tile_set_schedule", [](int mode) { fn_conv_tile_set_schedule(mode); });
  m.def("conv_tile_schedule", [] { return fn_conv_tile_schedule(); });
  m.def("conv_tile_slab_rows", [](std::vector<int> geom, int ncol, int NT) {
    // rows of the BN-statistics slab a conv_tile launch with statistics writes (one per tile chunk)
    need(geom, 31, "conv_tile_slab_rows");
    return fn_conv_tile_slab_rows(geom.data(), ncol, NT);
  });
  m.def("tile_pack_w", [](uintptr_t w, uintptr_t out, int K, int T, int C, int CS, int nks, int nct, int nslice,
                          int dgrad, uintptr_t st, int nt) {
    chk(fn_tile_pack_w(P<const float*>(w), P<void*>(out), K, T, C, CS, nks, nct, nslice, dgrad, nt, S(st)),
        "tile_pack_w");
  });
  m.def("tile_pack_w2", [](uintptr_t w, uintptr_t out0, uintptr_t out1, int K, int T, int C, std::vector<int> p0,
                           std::vector<int> p1, uintptr_t st, std::vector<long long> ext) {
    // p = {CS, nks, nct, nslice, dgrad, nt}; ext = {numel(w), numel(out0) and numel(out1) in uint4 x 2 bf16x4}
    need(p0, 6, "tile_pack_w2");
    need(p1, 6, "tile_pack_w2");
    fits(ext, 0, (long long)K * T * C, "tile_pack_w2", "w");
    fits(ext, 1, ((long long)p0[3] * p0[1] + 4) * p0[2] * 64 * 8, "tile_pack_w2", "out0");
    fits(ext, 2, ((long long)p1[3] * p1[1] + 4) * p1[2] * 64 * 8, "tile_pack_w2", "out1");
    chk(fn_tile_pack_w2(P<const float*>(w), P<void*>(out0), P<void*>(out1), K, T, C, p0.data(), p1.data(), S(st)),
        "tile_pack_w2");
  });
  m.def("igemm_pack_w", [](uintptr_t w, uintptr_t out, int K0, int C0, int K, int T, int C, int mode, int ld, int KW,
                           int R, uintptr_t st, std::vector<long long> ext) {
    // ext = {numel(w), numel(out)}
    fits(ext, 0, (long long)K0 * T * C0, "igemm_pack_w", "w");
    fits(ext, 1, (long long)(mode == 1 ? C : K) * ld, "igemm_pack_w", "out");
    chk(fn_igemm_pack_w(P<const float*>(w), P<void*>(out), K0, C0, K, T, C, mode, ld, KW, R, S(st)), "igemm_pack_w");
  });
  m.def("pack_w_multi", [](std::vector<long long> jobs, uintptr_t st, std::vector<long long> ext) {
    // jobs: n rows of (w, out, kind, a0..a8) (pack_w.h PackJob); ext: n rows of (numel(w), numel(out))
    if (jobs.size() % 12 || ext.size() != jobs.size() / 6)
      throw std::invalid_argument("pack_w_multi: 12 values per job and 2 extents per job");
    const int n = (int)(jobs.size() / 12);
    for (int k = 0; k < n; ++k) {
      const long long* r = jobs.data() + 12 * k;
      const long long kind = r[2];
      long long wn, on;
      if (kind >= 0 && kind <= 2) {                // K0, C0, K, T, C, ld
        wn = r[3] * r[6] * r[4];
        on = (kind == 1 ? r[7] : r[5]) * r[8];
      } else if (kind <= 4) {                      // K0, C0, K, T, C, CS, Tp
        wn = r[3] * r[6] * r[4];
        on = r[5] * r[7] * r[9];
      } else {                                     // K, T, C, CS, nks, nct, nslice, dgrad, nt: bf16 x 8 per index
        wn = r[3] * r[4] * r[5];
        on = (r[9] * r[7] + 4) * r[8] * 64 * 8;
      }
      std::vector<long long> e = {ext[2 * k], ext[2 * k + 1]};
      fits(e, 0, wn, "pack_w_multi", "w");
      fits(e, 1, on, "pack_w_multi", "out");
    }
    chk(fn_pack_w_multi(jobs.data(), n, S(st)), "pack_w_multi");
  });
  m.def("halo_pack_w", [](uintptr_t w, uintptr_t out, int K0, int C0, int K, int T, int C, int mode, int stage_k,
                          uintptr_t st, std::vector<long long> ext) {
    // ext = {numel(w), numel(out)}; out holds K * C * (taps padded to the stage) elements
    fits(ext, 0, (long long)K0 * T * C0, "halo_pack_w", "w");
    // (the kernel writes K * C * Tp elements: the tap count padded to whole stages, as
    // fn_halo_pack_w derives it -- checking K * C * T would let an output sized by T overrun)
    {
      const int Csrc = mode == 0 ? C : K;
      const int CS = Csrc % 16 == 0 ? 16 : (Csrc % 8 == 0 ? 8 : 0);
      const int tps = CS > 0 && stage_k > 0 ? stage_k / CS : 0;
      const long long Tp = tps > 0 ? (long long)(T + tps - 1) / tps * tps : T;
      fits(ext, 1, (long long)K * C * Tp, "halo_pack_w", "out");
    }
    chk(fn_halo_pack_w(P<const float*>(w), P<void*>(out), K0, C0, K, T, C, mode, stage_k, S(st)), "halo_pack_w");
  });
  m.def("ew_binary", [](uintptr_t a, uintptr_t b, uintptr_t out, long long n, int op, uintptr_t st) {
    chk(fn_ew_binary(P<const void*>(a), P<const void*>(b), P<void*>(out), n, op, S(st)), "ew_binary");
  });
  m.def("ew_mul_bwd", [](uintptr_t g, uintptr_t a, uintptr_t b, uintptr_t da, uintptr_t db, long long n,
                         uintptr_t st) {
    chk(fn_ew_mul_bwd(P<const void*>(g), P<const void*>(a), P<const void*>(b), P<void*>(da), P<void*>(db), n, S(st)),
        "ew_mul_bwd");
  });
  m.def("concat2", [](uintptr_t a, uintptr_t b, uintptr_t out, long long outer, int ia, int ib, int dir,
                      uintptr_t st) {
    chk(fn_concat2(P<void*>(a), P<void*>(b), P<void*>(out), outer, ia, ib, dir, S(st)), "concat2");
  });
  m.def("pad3", [](uintptr_t x, uintptr_t out, std::vector<int> geom, int dir, uintptr_t st) {
    need(geom, 8, "pad3");
    chk(fn_pad3(P<void*>(x), P<void*>(out), geom.data(), dir, S(st)), "pad3");
  });
  m.def("pad_channels", [](uintptr_t x, uintptr_t out, long long rows, int C, int CP, int dir, uintptr_t st,
                           std::vector<long long> ext) {
    // dir 0: x [rows, C] -> out [rows, CP]; dir 1: x [rows, CP] -> out [rows, C]
    fits(ext, 0, rows * (dir == 0 ? C : CP), "pad_channels", "x");
    fits(ext, 1, rows * (dir == 0 ? CP : C), "pad_channels", "out");
    chk(fn_pad_channels(P<void*>(x), P<void*>(out), rows, C, CP, dir, S(st)), "pad_channels");
  }, py::arg("x"), py::arg("out"), py::arg("rows"), py::arg("C"), py::arg("CP"), py::arg("dir"), py::arg("st"),
     py::arg("ext"));
  m.def("dense_splits", &fn_dense_splits);
  m.def("dense_fwd", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t out, uintptr_t part, int M, int N, int K,
                        int nsplit, int act, int out_fp32, uintptr_t st, std::vector<long long> ext, int wbf16) {
    fits(ext, 0, (long long)M * K, "dense_fwd", "x");
    fits(ext, 1, (long long)N * K, "dense_fwd", "w");
    fits(ext, 2, (long long)M * N, "dense_fwd", "out");
    fits(ext, 3, (long long)nsplit * M * N, "dense_fwd", "part");
    chk(fn_dense_fwd(P<const void*>(x), P<const void*>(w), P<const float*>(bias), P<void*>(out), P<float*>(part), M,
                     N, K, nsplit, act, out_fp32, wbf16, S(st)),
        "dense_fwd");
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("out"), py::arg("part"), py::arg("M"), py::arg("N"),
     py::arg("K"), py::arg("S"), py::arg("act"), py::arg("out_fp32"), py::arg("st"),
     py::arg("ext") = std::vector<long long>(), py::arg("wbf16") = 0);
  // ya / act: g is dy and the layer's activation backward is applied as it is loaded (ya =
  // the activation output [M][N], the same extent as g)
  m.def("dense_dgrad", [](uintptr_t g, uintptr_t w, uintptr_t dx, int M, int N, int K, uintptr_t st,
                          std::vector<long long> ext, uintptr_t ya, int act) {
    fits(ext, 0, (long long)M * N, "dense_dgrad", "g");
    fits(ext, 1, (long long)N * K, "dense_dgrad", "w");
    fits(ext, 2, (long long)M * K, "dense_dgrad", "dx");
    if (ya) fits(ext, 3, (long long)M * N, "dense_dgrad", "ya");
    chk(fn_dense_dgrad(P<const void*>(g), P<const float*>(w), P<void*>(dx), M, N, K, S(st), P<const void*>(ya), act),
        "dense_dgrad");
  }, py::arg("g"), py::arg("w"), py::arg("dx"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("st"),
     py::arg("ext") = std::vector<long long>(), py::arg("ya") = 0, py::arg("act") = 0);
  m.def("dense_wgrad_slices", &fn_dense_wgrad_slices);
  // part: fp32 workspace of S * (N*K + N) elements when S > 1 (dense_wgrad_slices)
  m.def("dense_wgrad", [](uintptr_t g, uintptr_t x, uintptr_t dw, uintptr_t db, int M, int N, int K, uintptr_t st,
                          std::vector<long long> ext, uintptr_t part, int slices, uintptr_t ya, int act) {
    fits(ext, 0, (long long)M * N, "dense_wgrad", "g");
    fits(ext, 1, (long long)M * K, "dense_wgrad", "x");
    fits(ext, 2, (long long)N * K, "dense_wgrad", "dw");
    if (slices > 1) fits(ext, 3, (long long)slices * ((long long)N * K + N), "dense_wgrad", "part");
    if (ya) fits(ext, 4, (long long)M * N, "dense_wgrad", "ya");   // (the activation output dy is taken through)
    chk(fn_dense_wgrad(P<const void*>(g), P<const void*>(x), P<float*>(dw), P<float*>(db), M, N, K, P<float*>(part),
                       slices, S(st), P<const void*>(ya), act),
        "dense_wgrad");
  }, py::arg("g"), py::arg("x"), py::arg("dw"), py::arg("db"), py::arg("M"), py::arg("N"), py::arg("K"),
     py::arg("st"), py::arg("ext") = std::vector<long long>(), py::arg("part") = 0, py::arg("slices") = 1,
     py::arg("ya") = 0, py::arg("act") = 0);
  // sub-pixel decoder weight maps (conv_halo.hip): mode 0 class weights [8][K][8][C] from w
  // [K][27][C], 1 dgrad weights [C][8][8][K], 2 the folded weight gradient [K][27][C] from [8][K][8][C]
  m.def("subpixel_wmap", [](uintptr_t src, uintptr_t dst, int K, int C, int mode, uintptr_t st,
                            std::vector<long long> ext) {
    const long long small = 27LL * K * C, big = 64LL * K * C;
    fits(ext, 0, mode == 2 ? big : small, "subpixel_wmap", "src");
    fits(ext, 1, mode == 2 ? small : big, "subpixel_wmap", "dst");
    chk(fn_subpixel_wmap(P<const float*>(src), P<float*>(dst), K, C, mode, S(st)), "subpixel_wmap");
  });
  m.def("s2d_weight_map", [](uintptr_t src, uintptr_t dst, std::vector<int> geom, int dir, uintptr_t st,
                             std::vector<long long> ext) {
    need(geom, 12, "s2d_weight_map");
    const long long big = prod({geom[0], geom[8], geom[9], geom[10], geom[11]});
    const long long small = prod({geom[0], geom[1], geom[2], geom[3], geom[4]});
    fits(ext, 0, dir == 0 ? small : big, "s2d_weight_map", "src");
    fits(ext, 1, dir == 0 ? big : small, "s2d_weight_map", "dst");
    chk(fn_s2d_weight_map(P<const float*>(src), P<float*>(dst), geom.data(), dir, S(st)), "s2d_weight_map");
  }, py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("dir"), py::arg("st"),
     py::arg("ext") = std::vector<long long>());
  m.def("s2d_pack", [](uintptr_t x, uintptr_t out, std::vector<int> geom, uintptr_t st, int u8) {
    // u8: x holds uint8 voxels (binary occupancy), else bf16
    if (geom.size() != 12 && geom.size() != 15) throw std::runtime_error("s2d_pack: geometry of 12 or 15 ints");
    chk(fn_s2d_pack(P<const void*>(x), P<void*>(out), geom.data(), (int)geom.size(), S(st), u8), "s2d_pack");
  });
  m.def("conv_halo_f8", [](uintptr_t src, uintptr_t wt, uintptr_t scale, uintptr_t bias, uintptr_t out,
                           float inv_out_scale, uintptr_t toffs, std::vector<int> geom, int ncol, int out_f8, int relu,
                           uintptr_t st) {
    need(geom, 16, "conv_halo_f8");
    chk(fn_conv_halo_f8(P<const void*>(src), P<const void*>(wt), P<const float*>(scale), P<const float*>(bias),
                        P<void*>(out), inv_out_scale, P<const int*>(toffs), geom.data(), ncol, out_f8, relu, S(st)),
        "conv_halo_f8");
  });
  m.def("s2d_tap_f8", [](uintptr_t x, uintptr_t y, std::vector<int> g, float inv_scale, uintptr_t st,
                         std::vector<long long> ext, int i8) {
    // g = {N, D, H, W, D2, H2, W2o, J}; ext = {numel(x), numel(y)}
    need(g, 8, "s2d_tap_f8");
    fits(ext, 0, prod({g[0], g[1], g[2], g[3]}), "s2d_tap_f8", "x");
    fits(ext, 1, prod({g[0], g[4], g[5], g[6], 8LL * g[7]}), "s2d_tap_f8", "y");
    chk(fn_s2d_tap_f8(P<const void*>(x), P<void*>(y), g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], inv_scale, i8, S(st)),
        "s2d_tap_f8");
  });
  // block-scaled e4m3 of a bf16 [M][C] tensor: y [M][C] bytes, sc a scale dword per row (ext = {x, y, sc})
  m.def("quant_fp8_block", [](uintptr_t x, uintptr_t y, uintptr_t sc, long long M, int C, uintptr_t st,
                              std::vector<long long> ext) {
    fits(ext, 0, M * C, "quant_fp8_block", "x");
    fits(ext, 1, M * C, "quant_fp8_block", "y");
    fits(ext, 2, M, "quant_fp8_block", "sc");
    chk(fn_quant_fp8_block(P<const void*>(x), P<void*>(y), P<void*>(sc), M, C, S(st)), "quant_fp8_block");
  }, py::arg("x"), py::arg("y"), py::arg("sc"), py::arg("M"), py::arg("C"), py::arg("st"),
     py::arg("ext") = std::vector<long long>());
  // one v_mfma_scale_f32_16x16x128_f8f6f4 on one wave (a, b: 64 x 32 bytes; sa, sb: 64 int32; d: 64 x 4 fp32)
  m.def("mfma_scale_probe", [](uintptr_t a, uintptr_t b, uintptr_t sa, uintptr_t sb, uintptr_t d, uintptr_t st) {
    chk(fn_mfma_scale_probe(P<const void*>(a), P<const void*>(b), P<const int*>(sa), P<const int*>(sb), P<float*>(d),
                            S(st)),
        "mfma_scale_probe");
  });
  m.def("quant_fp8", [](uintptr_t x, uintptr_t y, long long n, float inv_scale, uintptr_t st) {
    chk(fn_quant_fp8(P<const void*>(x), P<void*>(y), n, inv_scale, S(st)), "quant_fp8");
  });
  m.def("dw_fwd", [](uintptr_t x, uintptr_t w, uintptr_t b, uintptr_t y, std::vector<int> geom, int act,
                     uintptr_t st) {
    need(geom, 20, "dw_fwd");
    chk(fn_dw_fwd(P<const void*>(x), P<const float*>(w), P<const float*>(b), P<void*>(y), geom.data(), act, S(st)),
        "dw_fwd");
  });
  m.def("dw_dgrad", [](uintptr_t dy, uintptr_t w, uintptr_t dx, std::vector<int> geom, uintptr_t st) {
    need(geom, 20, "dw_dgrad");
    chk(fn_dw_dgrad(P<const void*>(dy), P<const float*>(w), P<void*>(dx), geom.data(), S(st)), "dw_dgrad");
  });
  // part: fp32 scratch [splits][C][taps] (the per-split partials, added into dw in a fixed order)
  m.def("dw_wgrad", [](uintptr_t dy, uintptr_t x, uintptr_t dw, std::vector<int> geom, int splits, uintptr_t st,
                       uintptr_t part, long long part_n) {
    need(geom, 20, "dw_wgrad");
    if (part_n < prod({splits, geom[4], geom[8] * geom[9] * geom[10]}))
      throw std::runtime_error("dw_wgrad: part scratch too small");
    chk(fn_dw_wgrad(P<const void*>(dy), P<const void*>(x), P<float*>(dw), geom.data(), splits, S(st), P<float*>(part)),
        "dw_wgrad");
  });
  m.def("conv_halo_wgrad_yblocks", [](std::vector<int> geom, int cout) {
    need(geom, 17, "conv_halo_wgrad_yblocks");
    return fn_conv_halo_wgrad_yblocks(geom.data(), cout);
  });
  // psc / psh / pact: optional input prologue x <- pact(x * psc[k] + psh[k]) (BN + act of the
  // producing layer, never materialised)
  // sy / ssc / ssh / spart / sact: BN-backward moments of the layer whose dz this call computes
  // (spart fp32 [pw_fwd_blocks][2][N])
  m.def("pw_fwd", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t y, long long M, int K, int N, int act,
                     uintptr_t st, uintptr_t psc, uintptr_t psh, int pact, uintptr_t sy, uintptr_t ssc,
                     uintptr_t ssh, uintptr_t spart, int sact) {
    chk(fn_pw_fwd(P<const void*>(x), P<const void*>(w), P<const float*>(bias), P<void*>(y), M, K, N, act, S(st),
                  P<const float*>(psc), P<const float*>(psh), pact, P<const void*>(sy), P<const float*>(ssc),
                  P<const float*>(ssh), P<float*>(spart), sact),
        "pw_fwd");
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("M"), py::arg("K"), py::arg("N"),
     py::arg("act"), py::arg("st"), py::arg("psc") = 0, py::arg("psh") = 0, py::arg("pact") = 0, py::arg("sy") = 0,
     py::arg("ssc") = 0, py::arg("ssh") = 0, py::arg("spart") = 0, py::arg("sact") = 0);
  m.def("pw_fwd_blocks", &fn_pw_fwd_blocks);
  m.def("pw_xent_blocks", &fn_pw_xent_blocks);
  m.def("part_reduce", [](uintptr_t part, uintptr_t dst, long long n, int W, int accumulate, uintptr_t st,
                          std::vector<long long> ext) {
    // dst[i] (+)= sum over the W partial rows part[w][i], added in row order; ext = {numel(part), numel(dst)}
    fits(ext, 0, n * W, "part_reduce", "part");
    fits(ext, 1, n, "part_reduce", "dst");
    chk(fn_part_reduce(P<const float*>(part), P<float*>(dst), n, W, accumulate, S(st)), "part_reduce");
  });
  m.def("seghead_part_len", &fn_seghead_part_len);
  m.def("seghead_blocks", &fn_seghead_blocks);
  m.def("seghead_loss", [](uintptr_t y, uintptr_t sc, uintptr_t sh, uintptr_t w, uintptr_t bias, uintptr_t labels,
                           uintptr_t dz, uintptr_t part, long long M, int K, int NC, int act, float xscale,
                           float smoothing, uintptr_t st, std::vector<long long> ext, int lab8, int hits) {
    fits(ext, 0, M * K, "seghead_loss", "y");
    fits(ext, 1, (long long)NC * K, "seghead_loss", "w");
    fits(ext, 2, M, "seghead_loss", "labels");
    fits(ext, 3, M * K, "seghead_loss", "dz");
    fits(ext, 4, (long long)fn_seghead_blocks(M) * fn_seghead_part_len(), "seghead_loss", "part");
    chk(fn_seghead_loss(P<const void*>(y), P<const float*>(sc), P<const float*>(sh), P<const void*>(w),
                        P<const float*>(bias), P<const void*>(labels), P<void*>(dz), P<float*>(part), M, K, NC,
                        act, xscale, smoothing, S(st), lab8, hits),
        "seghead_loss");
  }, py::arg("y"), py::arg("sc"), py::arg("sh"), py::arg("w"), py::arg("bias"), py::arg("labels"), py::arg("dz"),
     py::arg("part"), py::arg("M"), py::arg("K"), py::arg("NC"), py::arg("act"), py::arg("xscale"),
     py::arg("smoothing"), py::arg("st"), py::arg("ext"), py::arg("lab8") = 0, py::arg("hits") = 1);
  m.def("pw_fwd_xent", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t dlog, long long M, int K, int N,
                          uintptr_t psc, uintptr_t psh, int pact, uintptr_t labels, uintptr_t xpart, float xscale,
                          float smoothing, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, M * K, "pw_fwd_xent", "x");
    fits(ext, 1, M * N, "pw_fwd_xent", "dlog");
    fits(ext, 2, M, "pw_fwd_xent", "labels");
    fits(ext, 3, 2LL * fn_pw_xent_blocks(M), "pw_fwd_xent", "xpart");
    chk(fn_pw_fwd_xent(P<const void*>(x), P<const void*>(w), P<const float*>(bias), P<void*>(dlog), M, K, N,
                       P<const float*>(psc), P<const float*>(psh), pact, P<const long long*>(labels), P<float*>(xpart),
                       xscale, smoothing, S(st)),
        "pw_fwd_xent");
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("dlog"), py::arg("M"), py::arg("K"), py::arg("N"),
     py::arg("psc"), py::arg("psh"), py::arg("pact"), py::arg("labels"), py::arg("xpart"), py::arg("xscale"),
     py::arg("smoothing"), py::arg("st"), py::arg("ext"));
  // classifier head -> labels uint8 [M] (+ conf bf16 [M], 0 = not wanted); ext = {numel(x), numel(labels),
  // numel(conf)}
  m.def("pw_argmax_blocks", &fn_pw_argmax_blocks);
  m.def("pw_argmax", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t labels, uintptr_t conf, long long M,
                        int K, int N, uintptr_t psc, uintptr_t psh, int pact, uintptr_t st,
                        std::vector<long long> ext) {
    fits(ext, 0, M * K, "pw_argmax", "x");
    fits(ext, 1, M, "pw_argmax", "labels");
    if (conf) fits(ext, 2, M, "pw_argmax", "conf");
    chk(fn_pw_argmax(P<const void*>(x), P<const void*>(w), P<const float*>(bias), P<void*>(labels), P<void*>(conf),
                     M, K, N, P<const float*>(psc), P<const float*>(psh), pact, S(st)),
        "pw_argmax");
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("labels"), py::arg("conf"), py::arg("M"), py::arg("K"),
     py::arg("N"), py::arg("psc"), py::arg("psh"), py::arg("pact"), py::arg("st"), py::arg("ext"));
  // classifier head -> confusion matrix: acc int64 [N*N + 1] += counts of (truth, arg-max) over the M rows
  // (slot N*N: truth >= N; truth == ignore is skipped, -1 = none); labels uint8 [M] or 0 = not wanted; part:
  // uint32 scratch [pw_argmax_cm_blocks(M, K, N)][N*N + 1]; ext = {numel(x), numel(truth), numel(labels),
  // numel(part), numel(acc)}
  m.def("pw_argmax_cm_blocks", &fn_pw_argmax_cm_blocks);
  m.def("pw_argmax_cm", [](uintptr_t x, uintptr_t w, uintptr_t bias, uintptr_t truth, uintptr_t labels, uintptr_t part,
                           uintptr_t acc, long long M, int K, int N, int ignore, uintptr_t psc, uintptr_t psh, int pact,
                           uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, M * K, "pw_argmax_cm", "x");
    fits(ext, 1, M, "pw_argmax_cm", "truth");
    if (labels) fits(ext, 2, M, "pw_argmax_cm", "labels");
    fits(ext, 4, (long long)N * N + 1, "pw_argmax_cm", "acc");
    fits(ext, 3, (long long)fn_pw_argmax_cm_blocks(M, K, N) * ((long long)N * N + 1), "pw_argmax_cm", "part");
    chk(fn_pw_argmax_cm(P<const void*>(x), P<const void*>(w), P<const float*>(bias), P<const void*>(truth),
                        P<void*>(labels), P<void*>(part), P<void*>(acc), M, K, N, ignore, P<const float*>(psc),
                        P<const float*>(psh), pact, S(st)),
        "pw_argmax_cm");
  }, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("truth"), py::arg("labels"), py::arg("part"), py::arg("acc"),
     py::arg("M"), py::arg("K"), py::arg("N"), py::arg("ignore"), py::arg("psc"), py::arg("psh"), py::arg("pact"),
     py::arg("st"), py::arg("ext"));
  // connected components of a label volume (ccl.hip): labels uint8 [N][D][H][W]; roots / flags / rank / ids
  // int32 of that shape; background -1 = none; connectivity 6 or 26.  ccl_local + ccl_merge + ccl_flatten,
  // in this order, leave roots[v] = 1 + the smallest linear index of v's component (0: background) and
  // flags[v] = (roots[v] == v + 1); ext = {numel(labels), numel(roots)} / {numel(roots), numel(flags)}
  m.def("ccl_tile", []() {
    int t[3];
    fn_ccl_tile(t);
    return py::make_tuple(t[0], t[1], t[2]);
  });
  m.def("ccl_local", [](uintptr_t labels, uintptr_t roots, int N, int D, int H, int W, int background,
                        int connectivity, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "ccl_local", "labels");
    fits(ext, 1, prod({N, D, H, W}), "ccl_local", "roots");
    chk(fn_ccl_local(P<const void*>(labels), P<void*>(roots), N, D, H, W, background, connectivity, S(st)),
        "ccl_local");
  }, py::arg("labels"), py::arg("roots"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"),
     py::arg("background"), py::arg("connectivity"), py::arg("st"), py::arg("ext"));
  m.def("ccl_merge", [](uintptr_t labels, uintptr_t roots, int N, int D, int H, int W, int background,
                        int connectivity, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "ccl_merge", "labels");
    fits(ext, 1, prod({N, D, H, W}), "ccl_merge", "roots");
    chk(fn_ccl_merge(P<const void*>(labels), P<void*>(roots), N, D, H, W, background, connectivity, S(st)),
        "ccl_merge");
  }, py::arg("labels"), py::arg("roots"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"),
     py::arg("background"), py::arg("connectivity"), py::arg("st"), py::arg("ext"));
  m.def("ccl_flatten", [](uintptr_t roots, uintptr_t flags, int N, int D, int H, int W, uintptr_t st,
                          std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "ccl_flatten", "roots");
    fits(ext, 1, prod({N, D, H, W}), "ccl_flatten", "flags");
    chk(fn_ccl_flatten(P<void*>(roots), P<void*>(flags), N, D, H, W, S(st)), "ccl_flatten");
  }, py::arg("roots"), py::arg("flags"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"), py::arg("st"),
     py::arg("ext"));
  // rank: inclusive prefix sum of flags over the flat batch (N*D*H*W < 2^31), T = its last element; table int64
  // [T][13] (fully rewritten), ids 0 = not wanted; ext = {numel(labels), numel(roots), numel(rank), numel(ids),
  // numel(table)}
  m.def("ccl_stats", [](uintptr_t labels, uintptr_t roots, uintptr_t rank, uintptr_t ids, uintptr_t table, int N,
                        int D, int H, int W, long long T, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "ccl_stats", "labels");
    fits(ext, 1, prod({N, D, H, W}), "ccl_stats", "roots");
    fits(ext, 2, prod({N, D, H, W}), "ccl_stats", "rank");
    if (ids) fits(ext, 3, prod({N, D, H, W}), "ccl_stats", "ids");
    fits(ext, 4, prod({T, 13}), "ccl_stats", "table");
    chk(fn_ccl_stats(P<const void*>(labels), P<const void*>(roots), P<const void*>(rank), P<void*>(ids),
                     P<void*>(table), N, D, H, W, T, S(st)),
        "ccl_stats");
  }, py::arg("labels"), py::arg("roots"), py::arg("rank"), py::arg("ids"), py::arg("table"), py::arg("N"),
     py::arg("D"), py::arg("H"), py::arg("W"), py::arg("T"), py::arg("st"), py::arg("ext"));
  // overlap table of two id volumes (overlap.hip): ids_a / ids_b int32 [N*V] (per-sample ids from 1, 0 = none),
  // off_a / off_b int64 [N+1] (the instance tables' offsets), keys uint64 [cap] / counts int64 [cap] / lost int64
  // [1], all three zero on entry; cap a power of two, an update probes min(cap, probe) slots and is counted in
  // lost when none is free; ext = {numel(ids_a), numel(ids_b), numel(off_a), numel(off_b), numel(keys),
  // numel(counts), numel(lost)}
  m.def("overlap_chunk", []() {
    int t[2];
    fn_overlap_chunk(t);
    return py::make_tuple(t[0], t[1]);
  });
  m.def("overlap_pairs", [](uintptr_t ids_a, uintptr_t ids_b, uintptr_t off_a, uintptr_t off_b, uintptr_t keys,
                            uintptr_t counts, uintptr_t lost, int N, long long V, int W, long long cap,
                            long long probe, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, V}), "overlap_pairs", "ids_a");
    fits(ext, 1, prod({N, V}), "overlap_pairs", "ids_b");
    fits(ext, 2, N + 1LL, "overlap_pairs", "off_a");
    fits(ext, 3, N + 1LL, "overlap_pairs", "off_b");
    fits(ext, 4, cap, "overlap_pairs", "keys");
    fits(ext, 5, cap, "overlap_pairs", "counts");
    fits(ext, 6, 1, "overlap_pairs", "lost");
    chk(fn_overlap_pairs(P<const void*>(ids_a), P<const void*>(ids_b), P<const void*>(off_a), P<const void*>(off_b),
                         P<void*>(keys), P<void*>(counts), P<void*>(lost), N, V, W, cap, probe, S(st)),
        "overlap_pairs");
  }, py::arg("ids_a"), py::arg("ids_b"), py::arg("off_a"), py::arg("off_b"), py::arg("keys"), py::arg("counts"),
     py::arg("lost"), py::arg("N"), py::arg("V"), py::arg("W"), py::arg("cap"), py::arg("probe"), py::arg("st"),
     py::arg("ext"));
  // access directions of feature instances (access.hip): occ uint8 [N][D][H][W] (material: != 0); column extents
  // ex int32 [N][D][H][2], ey [N][D][W][2], ez [N][H][W][2] = (lo, hi) of the material along x / y / z, (axis length,
  // -1) for an empty column, written in full; ext = {numel(occ), numel(ex), numel(ey), numel(ez)}
  m.def("access_chunk", []() {
    int t[2];
    fn_access_chunk(t);
    return py::make_tuple(t[0], t[1]);
  });
  m.def("access_extents", [](uintptr_t occ, uintptr_t ex, uintptr_t ey, uintptr_t ez, int N, int D, int H, int W,
                             uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "access_extents", "occ");
    fits(ext, 1, prod({N, D, H, 2}), "access_extents", "ex");
    fits(ext, 2, prod({N, D, W, 2}), "access_extents", "ey");
    fits(ext, 3, prod({N, H, W, 2}), "access_extents", "ez");
    chk(fn_access_extents(P<const void*>(occ), P<void*>(ex), P<void*>(ey), P<void*>(ez), N, D, H, W, S(st)),
        "access_extents");
  }, py::arg("occ"), py::arg("ex"), py::arg("ey"), py::arg("ez"), py::arg("N"), py::arg("D"), py::arg("H"),
     py::arg("W"), py::arg("st"), py::arg("ext"));
  // ids int32 [N*V] (per-sample ids from 1, 0 = none), offsets int64 [N+1] (the instance table's), ex / ey / ez as
  // access_extents writes them; mask uint8 [N*V], 0 = not wanted: bit k = open toward face k (+z -z +x -x +y -y), 0
  // where ids is 0; acc int64 [T][8] (fully rewritten): voxels open toward each face, toward none, voxels; ext =
  // {numel(ids), numel(offsets), numel(ex), numel(ey), numel(ez), numel(mask), numel(acc)}
  m.def("access_stats", [](uintptr_t ids, uintptr_t offsets, uintptr_t ex, uintptr_t ey, uintptr_t ez, uintptr_t mask,
                           uintptr_t acc, int N, int D, int H, int W, long long T, uintptr_t st,
                           std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "access_stats", "ids");
    fits(ext, 1, N < 0 ? -1 : N + 1LL, "access_stats", "offsets");
    fits(ext, 2, prod({N, D, H, 2}), "access_stats", "ex");
    fits(ext, 3, prod({N, D, W, 2}), "access_stats", "ey");
    fits(ext, 4, prod({N, H, W, 2}), "access_stats", "ez");
    if (mask) fits(ext, 5, prod({N, D, H, W}), "access_stats", "mask");
    fits(ext, 6, prod({T, 8}), "access_stats", "acc");
    chk(fn_access_stats(P<const void*>(ids), P<const void*>(offsets), P<const void*>(ex), P<const void*>(ey),
                        P<const void*>(ez), P<void*>(mask), P<void*>(acc), N, D, H, W, T, S(st)),
        "access_stats");
  }, py::arg("ids"), py::arg("offsets"), py::arg("ex"), py::arg("ey"), py::arg("ez"), py::arg("mask"), py::arg("acc"),
     py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"), py::arg("T"), py::arg("st"), py::arg("ext"));
  // dimensions of feature instances (edt.hip): seeds uint8 [N][D][H][W] (a seed: != 0; border: every position just
  // outside the grid is one too), D, H, W <= 256; t and d2 int32 [N][D][H][W], which may be one buffer: passes bit 0
  // writes t (the squared distance within the voxel's plane), bit 1 d2 from t (the squared distance, 1 << 30 where
  // the sample has no seed); ext = {numel(seeds), numel(t), numel(d2)}
  m.def("edt_chunk", []() {
    int t[2];
    fn_edt_chunk(t);
    return py::make_tuple(t[0], t[1]);
  });
  m.def("edt_transform", [](uintptr_t seeds, uintptr_t t, uintptr_t d2, int N, int D, int H, int W, bool border,
                            int passes, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "edt_transform", "seeds");
    fits(ext, 1, prod({N, D, H, W}), "edt_transform", "t");
    fits(ext, 2, prod({N, D, H, W}), "edt_transform", "d2");
    chk(fn_edt_transform(P<const void*>(seeds), P<void*>(t), P<void*>(d2), N, D, H, W, border, passes, S(st)),
        "edt_transform");
  }, py::arg("seeds"), py::arg("t"), py::arg("d2"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"),
     py::arg("border"), py::arg("passes"), py::arg("st"), py::arg("ext"));
  // ids int32 [N*V] and offsets int64 [N+1] as for access_stats, d2 int32 [N*V]; raw int64 [T][3] (fully rewritten):
  // the largest d2 << 32 | (0xFFFFFFFF - index in the sample) over the row's voxels, its voxels with d2 == 1, its
  // voxels (all 0: no voxel carries the row); ext = {numel(ids), numel(offsets), numel(d2), numel(raw)}
  m.def("edt_stats", [](uintptr_t ids, uintptr_t offsets, uintptr_t d2, uintptr_t raw, int N, int D, int H, int W,
                        long long T, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "edt_stats", "ids");
    fits(ext, 1, N < 0 ? -1 : N + 1LL, "edt_stats", "offsets");
    fits(ext, 2, prod({N, D, H, W}), "edt_stats", "d2");
    fits(ext, 3, prod({T, 3}), "edt_stats", "raw");
    chk(fn_edt_stats(P<const void*>(ids), P<const void*>(offsets), P<const void*>(d2), P<void*>(raw), N, D, H, W, T,
                     S(st)),
        "edt_stats");
  }, py::arg("ids"), py::arg("offsets"), py::arg("d2"), py::arg("raw"), py::arg("N"), py::arg("D"), py::arg("H"),
     py::arg("W"), py::arg("T"), py::arg("st"), py::arg("ext"));
  // walls between feature instances (nearest.hip): ids int32 [N][D][H][W] (a seed of label ids: ids > 0), D, H, W <=
  // 128; t and nn int64 [N][2][D][H][W], which may be one buffer: per voxel the keys d2 << 32 | label of the nearest
  // label and of the nearest other label ((1 << 30) << 32: none); passes bit 0 writes t (over the seeds of the
  // voxel's plane), bit 1 nn from t; ext = {numel(ids), numel(t), numel(nn)}
  m.def("nn_chunk", []() {
    int t[2];
    fn_nn_chunk(t);
    return py::make_tuple(t[0], t[1]);
  });
  m.def("nn_transform", [](uintptr_t ids, uintptr_t t, uintptr_t nn, int N, int D, int H, int W, int passes,
                           uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "nn_transform", "ids");
    fits(ext, 1, prod({N, 2, D, H, W}), "nn_transform", "t");
    fits(ext, 2, prod({N, 2, D, H, W}), "nn_transform", "nn");
    chk(fn_nn_transform(P<const void*>(ids), P<void*>(t), P<void*>(nn), N, D, H, W, passes, S(st)), "nn_transform");
  }, py::arg("ids"), py::arg("t"), py::arg("nn"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"),
     py::arg("passes"), py::arg("st"), py::arg("ext"));
  // ids int32 [N*V] and offsets int64 [N+1] as for access_stats, nn int64 [N][2][V] as nn_transform writes it; raw
  // int64 [T][3] (fully rewritten): the smallest rank-1 d2 << 32 | index in the sample over the row's voxels (all
  // ones: no voxel carries the row), its voxels with rank-1 d2 <= limit2, its voxels; 0 <= limit2 < 1 << 30; ext =
  // {numel(ids), numel(offsets), numel(nn), numel(raw)}
  m.def("wall_stats", [](uintptr_t ids, uintptr_t offsets, uintptr_t nn, uintptr_t raw, int N, int D, int H, int W,
                         long long T, int limit2, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "wall_stats", "ids");
    fits(ext, 1, N < 0 ? -1 : N + 1LL, "wall_stats", "offsets");
    fits(ext, 2, prod({N, 2, D, H, W}), "wall_stats", "nn");
    fits(ext, 3, prod({T, 3}), "wall_stats", "raw");
    chk(fn_wall_stats(P<const void*>(ids), P<const void*>(offsets), P<const void*>(nn), P<void*>(raw), N, D, H, W, T,
                      limit2, S(st)),
        "wall_stats");
  }, py::arg("ids"), py::arg("offsets"), py::arg("nn"), py::arg("raw"), py::arg("N"), py::arg("D"), py::arg("H"),
     py::arg("W"), py::arg("T"), py::arg("limit2"), py::arg("st"), py::arg("ext"));
  // tool reach of feature instances (reach.hip): vol int32 [N][D][H][W], D, H, W <= 256; r6 int32 [N][6][D][H][W]
  // (written in full): the minimum of vol from each voxel to face k (+z -z +x -x +y -y) of the grid along that face's
  // axis, the voxel included; ext = {numel(vol), numel(r6)}
  m.def("reach_chunk", []() {
    int t[2];
    fn_reach_chunk(t);
    return py::make_tuple(t[0], t[1]);
  });
  m.def("reach_scan", [](uintptr_t vol, uintptr_t r6, int N, int D, int H, int W, uintptr_t st,
                         std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "reach_scan", "vol");
    fits(ext, 1, prod({N, 6, D, H, W}), "reach_scan", "r6");
    chk(fn_reach_scan(P<const void*>(vol), P<void*>(r6), N, D, H, W, S(st)), "reach_scan");
  }, py::arg("vol"), py::arg("r6"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"), py::arg("st"),
     py::arg("ext"));
  // ids int32 [N*V] and offsets int64 [N+1] as for access_stats, r6 int32 [N][6][V] (>= 0) as reach_scan writes it,
  // dc2 int32 [N*V]; raw int64 [T][15] (fully rewritten): the largest r6[k] over the row's voxels (0..5; -1: no voxel
  // carries the row), its voxels with r6[k] >= need2 (6..11), with no such k (12), with dc2 <= cut2 (13), its voxels
  // (14); need2 >= 1, cut2 >= 0; ext = {numel(ids), numel(offsets), numel(r6), numel(dc2), numel(raw)}
  m.def("reach_stats", [](uintptr_t ids, uintptr_t offsets, uintptr_t r6, uintptr_t dc2, uintptr_t raw, int N, int D,
                          int H, int W, long long T, int need2, int cut2, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "reach_stats", "ids");
    fits(ext, 1, N < 0 ? -1 : N + 1LL, "reach_stats", "offsets");
    fits(ext, 2, prod({N, 6, D, H, W}), "reach_stats", "r6");
    fits(ext, 3, prod({N, D, H, W}), "reach_stats", "dc2");
    fits(ext, 4, prod({T, 15}), "reach_stats", "raw");
    chk(fn_reach_stats(P<const void*>(ids), P<const void*>(offsets), P<const void*>(r6), P<const void*>(dc2),
                       P<void*>(raw), N, D, H, W, T, need2, cut2, S(st)),
        "reach_stats");
  }, py::arg("ids"), py::arg("offsets"), py::arg("r6"), py::arg("dc2"), py::arg("raw"), py::arg("N"), py::arg("D"),
     py::arg("H"), py::arg("W"), py::arg("T"), py::arg("need2"), py::arg("cut2"), py::arg("st"), py::arg("ext"));
  // contacts of feature instances (contact.hip): ids int32 [N*V] and offsets int64 [N+1] as for access_stats, occ
  // uint8 [N*V] (material: != 0); contact int64 [T][19]: the faces of the row's voxels toward +z -z +x -x +y -y that
  // meet material (0..5), free space or the outside of the grid (6..11), another instance (12..17), its voxels (18);
  // keys uint64 [cap] / counts int64 [cap] / lost int64 [1]: the pair table of overlap_pairs under the key row_a <<
  // 33 | row_b << 3 | face (1-based rows, row_a < row_b; T < 2^30), counts in faces; contact, keys, counts and lost
  // are zero on entry; ext = {numel(ids), numel(occ), numel(offsets), numel(contact), numel(keys), numel(counts),
  // numel(lost)}
  m.def("contact_chunk", []() {
    int t[2];
    fn_contact_chunk(t);
    return py::make_tuple(t[0], t[1]);
  });
  m.def("contact_stats", [](uintptr_t ids, uintptr_t occ, uintptr_t offsets, uintptr_t contact, uintptr_t keys,
                            uintptr_t counts, uintptr_t lost, int N, int D, int H, int W, long long T, long long cap,
                            long long probe, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "contact_stats", "ids");
    fits(ext, 1, prod({N, D, H, W}), "contact_stats", "occ");
    fits(ext, 2, N < 0 ? -1 : N + 1LL, "contact_stats", "offsets");
    fits(ext, 3, prod({T, 19}), "contact_stats", "contact");
    fits(ext, 4, cap, "contact_stats", "keys");
    fits(ext, 5, cap, "contact_stats", "counts");
    fits(ext, 6, 1, "contact_stats", "lost");
    chk(fn_contact_stats(P<const void*>(ids), P<const void*>(occ), P<const void*>(offsets), P<void*>(contact),
                         P<void*>(keys), P<void*>(counts), P<void*>(lost), N, D, H, W, T, cap, probe, S(st)),
        "contact_stats");
  }, py::arg("ids"), py::arg("occ"), py::arg("offsets"), py::arg("contact"), py::arg("keys"), py::arg("counts"),
     py::arg("lost"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"), py::arg("T"), py::arg("cap"),
     py::arg("probe"), py::arg("st"), py::arg("ext"));
  // watershed split of touching instances (watershed.hip): ids and height int32 [N][D][H][W], D, H, W <= 256 and
  // N*D*H*W < 2^31; parent int32 of that shape: 1 + the index in the sample of the 26-neighbour of the same id with
  // the largest (max(height, 0), lowest index) when that beats the voxel's own, else of the voxel, 0 where ids <= 0;
  // staged 1: the LDS tile kernel, 0: the plain one; ext = {numel(ids), numel(height), numel(parent)}
  m.def("ws_tile", []() {
    int t[5];
    fn_ws_tile(t);
    return py::make_tuple(t[0], t[1], t[2], t[3], t[4]);
  });
  m.def("ws_ascend", [](uintptr_t ids, uintptr_t height, uintptr_t parent, int N, int D, int H, int W, int staged,
                        uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "ws_ascend", "ids");
    fits(ext, 1, prod({N, D, H, W}), "ws_ascend", "height");
    fits(ext, 2, prod({N, D, H, W}), "ws_ascend", "parent");
    chk(fn_ws_ascend(P<const void*>(ids), P<const void*>(height), P<void*>(parent), N, D, H, W, staged, S(st)),
        "ws_ascend");
  }, py::arg("ids"), py::arg("height"), py::arg("parent"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"),
     py::arg("staged"), py::arg("st"), py::arg("ext"));
  // roots int32: 1 + the end of each voxel's chain of parents (0: no id, or a word that is no parent pointer on
  // the way), flags int32: roots[v] == v + 1; both written in full; ext = {numel(parent), numel(roots), numel(flags)}
  m.def("ws_resolve", [](uintptr_t parent, uintptr_t roots, uintptr_t flags, int N, int D, int H, int W, uintptr_t st,
                         std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "ws_resolve", "parent");
    fits(ext, 1, prod({N, D, H, W}), "ws_resolve", "roots");
    fits(ext, 2, prod({N, D, H, W}), "ws_resolve", "flags");
    chk(fn_ws_resolve(P<const void*>(parent), P<void*>(roots), P<void*>(flags), N, D, H, W, S(st)), "ws_resolve");
  }, py::arg("parent"), py::arg("roots"), py::arg("flags"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"),
     py::arg("st"), py::arg("ext"));
  // bids int32 [N*V] and offsets int64 [N+1]: the basin ids and the basin table's offsets (T rows); keys uint64
  // [cap] / counts int64 [cap] / lost int64 [1]: the pair table of overlap_pairs under the key row_lo << 32 | row_hi
  // (1-based rows), counts the largest min(height, height) over the adjacent voxel pairs of the two basins inside
  // one component, lost the updates that found no slot; keys, counts and lost are zero on entry; ext = {numel(ids),
  // numel(bids), numel(offsets), numel(height), numel(keys), numel(counts), numel(lost)}
  m.def("ws_saddle", [](uintptr_t ids, uintptr_t bids, uintptr_t offsets, uintptr_t height, uintptr_t keys,
                        uintptr_t counts, uintptr_t lost, int N, int D, int H, int W, long long T, long long cap,
                        long long probe, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "ws_saddle", "ids");
    fits(ext, 1, prod({N, D, H, W}), "ws_saddle", "bids");
    fits(ext, 2, N < 0 ? -1 : N + 1LL, "ws_saddle", "offsets");
    fits(ext, 3, prod({N, D, H, W}), "ws_saddle", "height");
    fits(ext, 4, cap, "ws_saddle", "keys");
    fits(ext, 5, cap, "ws_saddle", "counts");
    fits(ext, 6, 1, "ws_saddle", "lost");
    chk(fn_ws_saddle(P<const void*>(ids), P<const void*>(bids), P<const void*>(offsets), P<const void*>(height),
                     P<void*>(keys), P<void*>(counts), P<void*>(lost), N, D, H, W, T, cap, probe, S(st)),
        "ws_saddle");
  }, py::arg("ids"), py::arg("bids"), py::arg("offsets"), py::arg("height"), py::arg("keys"), py::arg("counts"),
     py::arg("lost"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"), py::arg("T"), py::arg("cap"),
     py::arg("probe"), py::arg("st"), py::arg("ext"));
  // each selected instance alone in a solid stock block (isolate.hip): ids int32 [N][D][H][W], D, H, W <= 256 and
  // N*D*H*W < 2^31; sel int32 [M][14] = n id | box z0 y0 x0 z1 y1 x1 | window z0 y0 x0 Lz Ly Lx (a row whose sample
  // or window lies outside the grid gives a part of zeros); out on a 16-byte boundary: fmt 0 the bits, uint8
  // [M][S^3/8], fmt 1 uint8 [M][S^3], fmt 2 bf16 [M][S^3]; S % 8 == 0, 8 <= S <= 256, M * S^3 < 2^31; ext =
  // {numel(ids), numel(sel), numel(out)}
  m.def("isolate_parts", [](uintptr_t ids, uintptr_t sel, uintptr_t out, int N, int D, int H, int W, long long M,
                            int size, int fmt, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({N, D, H, W}), "isolate_parts", "ids");
    fits(ext, 1, prod({M, 14}), "isolate_parts", "sel");
    fits(ext, 2, size < 8 || size % 8 ? -1 : prod({M, size, size, size}) / (fmt == 0 ? 8 : 1), "isolate_parts",
         "out");
    chk(fn_isolate_parts(P<const void*>(ids), P<const void*>(sel), P<void*>(out), N, D, H, W, M, size, fmt, S(st)),
        "isolate_parts");
  }, py::arg("ids"), py::arg("sel"), py::arg("out"), py::arg("N"), py::arg("D"), py::arg("H"), py::arg("W"),
     py::arg("M"), py::arg("size"), py::arg("fmt"), py::arg("st"), py::arg("ext"));
  // multi-feature parts from their parameter tables (partgen.hip): params int32 [N][K][16]; occ / labels / slots
  // uint8 [N][S][S][S] (8-byte aligned) and packed uint8 [N][S^3/8], each 0 = not wanted; S % 8 == 0, 8 <= S <=
  // 256, K <= 32; ext = {numel(params), numel(occ), numel(packed), numel(labels), numel(slots)}
  m.def("partgen_chunk", []() { return fn_partgen_chunk(); });
  m.def("partgen_carve", [](uintptr_t params, uintptr_t occ, uintptr_t packed, uintptr_t labels, uintptr_t slots,
                            int N, int K, int size, uintptr_t st, std::vector<long long> ext) {
    const long long vox = prod({N, size, size, size});
    fits(ext, 0, prod({N, K, 16}), "partgen_carve", "params");
    if (occ) fits(ext, 1, vox, "partgen_carve", "occ");
    if (packed) fits(ext, 2, vox < 0 ? -1 : vox / 8, "partgen_carve", "packed");
    if (labels) fits(ext, 3, vox, "partgen_carve", "labels");
    if (slots) fits(ext, 4, vox, "partgen_carve", "slots");
    chk(fn_partgen_carve(P<const void*>(params), P<void*>(occ), P<void*>(packed), P<void*>(labels), P<void*>(slots),
                         N, K, size, S(st)),
        "partgen_carve");
  }, py::arg("params"), py::arg("occ"), py::arg("packed"), py::arg("labels"), py::arg("slots"), py::arg("N"),
     py::arg("K"), py::arg("S"), py::arg("st"), py::arg("ext"));
  // triangle meshes to voxel grids (voxelize.hip): tris int32 [T][9] on the 16-units-per-voxel lattice, offsets
  // int32 [N + 1]; occ uint8 [N][S][S][S] (8-byte aligned), packed uint8 [N][S^3/8] and leaks_part int32
  // [N][ceil(S / zs)], each 0 = not wanted; zs z-planes per workgroup, 0 = voxelize_planes(S); ext = {numel(tris),
  // numel(offsets), numel(occ), numel(packed), numel(leaks_part)}
  m.def("voxelize_planes", [](int size) {
    const int zs = fn_voxelize_planes(size);
    chk(zs < 0 ? zs : 0, "voxelize_planes");
    return zs;
  }, py::arg("S"));
  m.def("voxelize_tris", [](uintptr_t tris, uintptr_t offsets, uintptr_t occ, uintptr_t packed, uintptr_t leaks_part,
                            int N, int T, int size, int zs, uintptr_t st, std::vector<long long> ext) {
    const long long vox = prod({N, size, size, size});
    fits(ext, 0, prod({T, 9}), "voxelize_tris", "tris");
    fits(ext, 1, N < 0 ? -1 : N + 1LL, "voxelize_tris", "offsets");
    if (occ) fits(ext, 2, vox, "voxelize_tris", "occ");
    if (packed) fits(ext, 3, vox < 0 ? -1 : vox / 8, "voxelize_tris", "packed");
    if (leaks_part) {
      const int planes = zs > 0 ? zs : fn_voxelize_planes(size);
      fits(ext, 4, planes <= 0 || size <= 0 ? -1 : prod({N, (size + planes - 1) / planes}), "voxelize_tris",
           "leaks_part");
    }
    chk(fn_voxelize_tris(P<const void*>(tris), P<const void*>(offsets), P<void*>(occ), P<void*>(packed),
                         P<void*>(leaks_part), N, T, size, zs, S(st)),
        "voxelize_tris");
  }, py::arg("tris"), py::arg("offsets"), py::arg("occ"), py::arg("packed"), py::arg("leaks_part"), py::arg("N"),
     py::arg("T"), py::arg("S"), py::arg("zs"), py::arg("st"), py::arg("ext"));
  // mesh labels (meshlabel.hip): tris / offsets as voxelize_tris, vol int32 (elem = 4) or uint8 (elem = 1)
  // [N][S][S][S] -> votes int32 [T][3] = winner, votes, covered; thr: a triangle whose box holds more than thr
  // columns takes the wave form (-1: every triangle; at most mesh_votes_thread_cols()); wide: int32 scratch [T + 1];
  // ext = {numel(tris), numel(offsets), numel(vol), numel(votes), numel(wide)}
  m.def("mesh_votes_thread_cols", []() { return fn_mesh_votes_thread_cols(); });
  m.def("mesh_votes", [](uintptr_t tris, uintptr_t offsets, uintptr_t vol, uintptr_t votes, uintptr_t wide, int N, int T,
                         int size, int elem, int thr, uintptr_t st, std::vector<long long> ext) {
    fits(ext, 0, prod({T, 9}), "mesh_votes", "tris");
    fits(ext, 1, N < 0 ? -1 : N + 1LL, "mesh_votes", "offsets");
    fits(ext, 2, prod({N, size, size, size}), "mesh_votes", "vol");
    fits(ext, 3, prod({T, 3}), "mesh_votes", "votes");
    fits(ext, 4, T < 0 ? -1 : T + 1LL, "mesh_votes", "wide");
    chk(fn_mesh_votes(P<const void*>(tris), P<const void*>(offsets), P<const void*>(vol), P<void*>(votes),
                      P<void*>(wide), N, T, size, elem, thr, S(st)),
        "mesh_votes");
  }, py::arg("tris"), py::arg("offsets"), py::arg("vol"), py::arg("votes"), py::arg("wide"), py::arg("N"),
     py::arg("T"), py::arg("S"), py::arg("elem"), py::arg("thr"), py::arg("st"), py::arg("ext"));
  // part: fp32 scratch of pw_wgrad_blocks(M, K, N) x N x K floats (per-workgroup partials)
  m.def("pw_wgrad", [](uintptr_t dy, uintptr_t x, uintptr_t dw, long long M, int K, int N, uintptr_t st,
                       uintptr_t psc, uintptr_t psh, int pact, uintptr_t part, long long part_n) {
    if (part_n < (long long)fn_pw_wgrad_blocks(M, K, N) * N * K) throw std::runtime_error("pw_wgrad: part scratch too small");
    chk(fn_pw_wgrad(P<const void*>(dy), P<const void*>(x), P<float*>(dw), M, K, N, S(st), P<const float*>(psc),
                    P<const float*>(psh), pact, P<float*>(part)),
        "pw_wgrad");
  }, py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("M"), py::arg("K"), py::arg("N"), py::arg("st"),
     py::arg("psc") = 0, py::arg("psh") = 0, py::arg("pact") = 0, py::arg("part") = 0, py::arg("part_n") = 0);
  m.def("pw_wgrad_blocks", &fn_pw_wgrad_blocks);
  m.def("conv_halo_workers", [](std::vector<int> geom, int ncol) {
    need(geom, 17, "conv_halo_workers");
    return fn_conv_halo_workers(geom.data(), ncol);
  });
  m.def("conv_halo_lds", [](std::vector<int> geom, int ncol) {
    need(geom, 17, "conv_halo_lds");
    return fn_conv_halo_lds(geom.data(), ncol);
  });
  // dw (and db) are accumulated into from the split partials in `scratch` (igemm_wgrad_part floats)
  m.def("igemm_wgrad", [](uintptr_t dy, uintptr_t src, uintptr_t dw, uintptr_t tab, std::vector<int> geom,
                          long long M, int Cout, int K, int splits, int vec, uintptr_t st, int ccrop, int cpad,
                          uintptr_t ya, int act, uintptr_t db, int kout, uintptr_t scratch, long long scratch_n) {
    need(geom, 14, "igemm_wgrad");
    if (scratch_n < fn_igemm_wgrad_part(Cout, K, splits, ccrop, cpad, kout, db ? 1 : 0))
      throw std::runtime_error("igemm_wgrad: partial scratch too small");
    chk(fn_igemm_wgrad(P<const void*>(dy), P<const void*>(src), P<float*>(dw), P<const int*>(tab), geom.data(), M,
                       Cout, K, splits, vec, S(st), ccrop, cpad, P<const void*>(ya), act, P<float*>(db), kout,
                       P<float*>(scratch)),
        "igemm_wgrad");
  }, py::arg("dy"), py::arg("src"), py::arg("dw"), py::arg("tab"), py::arg("geom"), py::arg("M"), py::arg("Cout"),
     py::arg("K"), py::arg("splits"), py::arg("vec"), py::arg("st"), py::arg("ccrop") = 0, py::arg("cpad") = 0,
     py::arg("ya") = 0, py::arg("act") = 0, py::arg("db") = 0, py::arg("kout") = 0, py::arg("scratch") = 0,
     py::arg("scratch_n") = 0);
  m.def("igemm_wgrad_part", &fn_igemm_wgrad_part);
  m.def("colstats", [](uintptr_t x, uintptr_t dz, uintptr_t scale, uintptr_t shift, uintptr_t mean, uintptr_t invstd,
                       uintptr_t part, long long M, int C, int act, int mode, int nb, uintptr_t st) {
    chk(fn_colstats(P<const void*>(x), P<const void*>(dz), P<const float*>(scale), P<const float*>(shift),
                    P<const float*>(mean), P<const float*>(invstd), P<float*>(part), M, C, act, mode, nb, S(st)),
        "colstats");
  });
  m.def("experiments_built", [] {
    // FN_BUILD_EXPERIMENTS=1 builds: the int8 fp8-stem instance, timing variants
#ifdef FN_EXPERIMENTS
    return true;
#else
    return false;
#endif
  });
  m.def("colstats_blocks", &fn_colstats_blocks, py::arg("M"), py::arg("C"), py::arg("mode"), py::arg("act"));
  m.def("bn_finalize", [](uintptr_t part, int nb, int C, double count, uintptr_t gamma, uintptr_t beta,
                          uintptr_t rmean, uintptr_t rvar, float momentum, float eps, uintptr_t o0, uintptr_t o1,
                          uintptr_t o2, uintptr_t o3, int mode, uintptr_t st) {
    chk(fn_bn_finalize(P<const float*>(part), nb, C, count, P<const float*>(gamma), P<const float*>(beta),
                       P<float*>(rmean), P<float*>(rvar), momentum, eps, P<float*>(o0), P<float*>(o1), P<float*>(o2),
                       P<float*>(o3), mode, S(st)),
        "bn_finalize");
  });
  m.def("bn_apply", [](uintptr_t y, uintptr_t scale, uintptr_t shift, uintptr_t z, long long total, int C, int act,
                       uintptr_t st, uintptr_t mask, long long mask_numel) {
    // mask: optional uint8 [total / 8] relu-mask bytes (one per 8-channel chunk)
    if (mask && mask_numel * 8 != total) throw std::runtime_error("bn_apply: mask needs total / 8 bytes");
    chk(fn_bn_apply(P<const void*>(y), P<const float*>(scale), P<const float*>(shift), P<void*>(z), total, C, act,
                    S(st), P<void*>(mask)),
        "bn_apply");
  }, py::arg("y"), py::arg("scale"), py::arg("shift"), py::arg("z"), py::arg("total"), py::arg("C"), py::arg("act"),
     py::arg("st"), py::arg("mask") = 0, py::arg("mask_numel") = 0);
  m.def("bn_wdot", [](uintptr_t w, uintptr_t dw, uintptr_t part, int R, int C, int nb, uintptr_t st,
                      std::vector<long long> ext) {
    fits(ext, 0, (long long)R * C, "bn_wdot", "w");
    fits(ext, 1, (long long)R * C, "bn_wdot", "dw");
    fits(ext, 2, (long long)nb * C, "bn_wdot", "part");
    chk(fn_bn_wdot(P<const float*>(w), P<const float*>(dw), P<float*>(part), R, C, nb, S(st)), "bn_wdot");
  });
  m.def("bn_bwd_prep", [](uintptr_t gslab, int nbg, uintptr_t wpart, int nbw, int C, double count, uintptr_t gamma,
                          uintptr_t beta, uintptr_t mean, uintptr_t invstd, uintptr_t scale, uintptr_t shift,
                          uintptr_t dbeta, uintptr_t kc, uintptr_t g, uintptr_t y, long long M, uintptr_t st,
                          std::vector<long long> ext) {
    fits(ext, 0, 2LL * nbg * C, "bn_bwd_prep", "gslab");
    fits(ext, 1, (long long)nbw * C, "bn_bwd_prep", "wpart");
    fits(ext, 2, 3LL * C, "bn_bwd_prep", "kc");
    fits(ext, 3, M * C, "bn_bwd_prep", "g");
    fits(ext, 4, M * C, "bn_bwd_prep", "y");
    chk(fn_bn_bwd_prep(P<const float*>(gslab), nbg, P<const float*>(wpart), nbw, C, count, P<const float*>(gamma),
                       P<const float*>(beta), P<const float*>(mean), P<const float*>(invstd), P<const float*>(scale),
                       P<const float*>(shift), P<float*>(dbeta), P<float*>(kc), P<const void*>(g), P<const void*>(y),
                       M, S(st)),
        "bn_bwd_prep");
  });
  m.def("bn_bwd_apply_k_blocks", &fn_bn_bwd_apply_k_blocks);
  m.def("bn_bwd_apply_k", [](uintptr_t g, uintptr_t y, uintptr_t kc, uintptr_t mean, uintptr_t invstd,
                             uintptr_t shift, uintptr_t dy, long long M, int C, uintptr_t part, int nb, uintptr_t st,
                             std::vector<long long> ext) {
    fits(ext, 0, M * C, "bn_bwd_apply_k", "g");
    fits(ext, 1, M * C, "bn_bwd_apply_k", "y");
    fits(ext, 2, M * C, "bn_bwd_apply_k", "dy");
    fits(ext, 3, 2LL * nb * C, "bn_bwd_apply_k", "part");
    chk(fn_bn_bwd_apply_k(P<const void*>(g), P<const void*>(y), P<const float*>(kc), P<const float*>(mean),
                          P<const float*>(invstd), P<const float*>(shift), P<void*>(dy), M, C, P<float*>(part), nb,
                          S(st)),
        "bn_bwd_apply_k");
  });
  m.def("bn_bwd_apply", [](uintptr_t dz, uintptr_t y, uintptr_t scale, uintptr_t shift, uintptr_t mean,
                           uintptr_t invstd, uintptr_t dbeta, uintptr_t dgamma, uintptr_t dy, long long total, int C,
                           float inv_count, int act, uintptr_t st) {
    chk(fn_bn_bwd_apply(P<const void*>(dz), P<const void*>(y), P<const float*>(scale), P<const float*>(shift),
                        P<const float*>(mean), P<const float*>(invstd), P<const float*>(dbeta),
                        P<const float*>(dgamma), P<void*>(dy), total, C, inv_count, act, S(st)),
        "bn_bwd_apply");
  });
  // ext = {dz / y numel, dsh numel}
  m.def("bn_bwd_apply_s2d", [](uintptr_t dz, uintptr_t y, uintptr_t scale, uintptr_t shift, uintptr_t mean,
                               uintptr_t invstd, uintptr_t dbeta, uintptr_t dgamma, uintptr_t dsh, int N, int FD,
                               int FH, int FW, int C, float inv_count, int act, uintptr_t st,
                               std::vector<long long> ext) {
    fits(ext, 0, prod({N, FD, FH, FW, C}), "bn_bwd_apply_s2d", "dz/y");
    fits(ext, 1, prod({N, FD / 2 + 1, FH / 2 + 1, FW / 2 + 1, 8LL * C}), "bn_bwd_apply_s2d", "dsh");
    chk(fn_bn_bwd_apply_s2d(P<const void*>(dz), P<const void*>(y), P<const float*>(scale), P<const float*>(shift),
                            P<const float*>(mean), P<const float*>(invstd), P<const float*>(dbeta),
                            P<const float*>(dgamma), P<void*>(dsh), N, FD, FH, FW, C, inv_count, act, S(st)),
        "bn_bwd_apply_s2d");
  }, py::arg("dz"), py::arg("y"), py::arg("scale"), py::arg("shift"), py::arg("mean"), py::arg("invstd"),
     py::arg("dbeta"), py::arg("dgamma"), py::arg("dsh"), py::arg("N"), py::arg("FD"), py::arg("FH"), py::arg("FW"),
     py::arg("C"), py::arg("inv_count"), py::arg("act"), py::arg("st"), py::arg("ext"));
  // pool geometry: N D H W C | OD OH OW | KD KH KW | sd sh sw | pd ph pw; ext = {x, out}
  auto check_pool = [](const std::vector<int>& g, const std::vector<long long>& ext, const char* what) {
    fits(ext, 0, prod({g[0], g[1], g[2], g[3], g[4]}), what, "x");
    fits(ext, 1, prod({g[0], g[5], g[6], g[7], g[4]}), what, "out");
  };
  m.def("pool_fwd", [check_pool](uintptr_t x, uintptr_t out, uintptr_t scale, uintptr_t shift, std::vector<int> geom,
                       int is_max, int count_pad, int act, uintptr_t st, std::vector<long long> ext) {
    need(geom, 17, "pool_fwd");
    check_pool(geom, ext, "pool_fwd");
    chk(fn_pool_fwd(P<const void*>(x), P<void*>(out), P<const float*>(scale), P<const float*>(shift), geom.data(),
                    is_max, count_pad, act, S(st)),
        "pool_fwd");
  }, py::arg("x"), py::arg("out"), py::arg("scale"), py::arg("shift"), py::arg("geom"), py::arg("is_max"),
     py::arg("count_pad"), py::arg("act"), py::arg("st"), py::arg("ext") = std::vector<long long>());
  m.def("pool_bwd", [check_pool](uintptr_t dout, uintptr_t x, uintptr_t dx, uintptr_t scale, uintptr_t shift,
                       std::vector<int> geom, int is_max, int count_pad, int act, uintptr_t st,
                       std::vector<long long> ext) {
    need(geom, 17, "pool_bwd");
    check_pool(geom, ext, "pool_bwd");   // ext = {x (and dx), dout}
    chk(fn_pool_bwd(P<const void*>(dout), P<const void*>(x), P<void*>(dx), P<const float*>(scale),
                    P<const float*>(shift), geom.data(), is_max, count_pad, act, S(st)),
        "pool_bwd");
  }, py::arg("dout"), py::arg("x"), py::arg("dx"), py::arg("scale"), py::arg("shift"), py::arg("geom"),
     py::arg("is_max"), py::arg("count_pad"), py::arg("act"), py::arg("st"), py::arg("ext") = std::vector<long long>());
  m.def("pool_bwd_stats_blocks", [](std::vector<int> geom) {
    need(geom, 17, "pool_bwd_stats_blocks");
    return fn_pool_bwd_stats_blocks(geom.data());
  });
  m.def("pool_bwd_stats", [check_pool](uintptr_t dout, uintptr_t x, uintptr_t dx, uintptr_t scale, uintptr_t shift,
                             std::vector<int> geom, int act, uintptr_t part, uintptr_t st, std::vector<long long> ext) {
    need(geom, 17, "pool_bwd_stats");
    check_pool(geom, ext, "pool_bwd_stats");   // ext = {x (and dx), dout, part}
    fits(ext, 2, 2LL * fn_pool_bwd_stats_blocks(geom.data()) * geom[4], "pool_bwd_stats", "part");
    chk(fn_pool_bwd_stats(P<const void*>(dout), P<const void*>(x), P<void*>(dx), P<const float*>(scale),
                          P<const float*>(shift), geom.data(), act, P<float*>(part), S(st)),
        "pool_bwd_stats");
  }, py::arg("dout"), py::arg("x"), py::arg("dx"), py::arg("scale"), py::arg("shift"), py::arg("geom"),
     py::arg("act"), py::arg("part"), py::arg("st"), py::arg("ext") = std::vector<long long>());
  m.def("pool_bn_bwd_apply", [check_pool](uintptr_t dout, uintptr_t y, uintptr_t scale, uintptr_t shift,
                                uintptr_t mean, uintptr_t invstd, uintptr_t dbeta, uintptr_t dgamma, uintptr_t dy,
                                std::vector<int> geom, int act, float inv_count, uintptr_t st,
                                std::vector<long long> ext) {
    need(geom, 17, "pool_bn_bwd_apply");
    check_pool(geom, ext, "pool_bn_bwd_apply");   // ext = {y (and dy), dout}
    chk(fn_pool_bn_bwd_apply(P<const void*>(dout), P<const void*>(y), P<const float*>(scale), P<const float*>(shift),
                             P<const float*>(mean), P<const float*>(invstd), P<const float*>(dbeta),
                             P<const float*>(dgamma), P<void*>(dy), geom.data(), act, inv_count, S(st)),
        "pool_bn_bwd_apply");
  }, py::arg("dout"), py::arg("y"), py::arg("scale"), py::arg("shift"), py::arg("mean"), py::arg("invstd"),
     py::arg("dbeta"), py::arg("dgamma"), py::arg("dy"), py::arg("geom"), py::arg("act"), py::arg("inv_count"),
     py::arg("st"), py::arg("ext") = std::vector<long long>());
  m.def("upsample2x", [](uintptr_t x, uintptr_t y, int N, int D, int H, int W, int C, int backward, uintptr_t st) {
    chk(fn_upsample2x(P<const void*>(x), P<void*>(y), N, D, H, W, C, backward, S(st)), "upsample2x");
  });
  m.def("softmax_xent_blocks", [](long long B, int NC) { return fn_softmax_xent_blocks(B, NC); });
  m.def("softmax_xent_rows", [](uintptr_t logits, int in_bf16, uintptr_t labels, uintptr_t block_loss,
                                uintptr_t dlogits, uintptr_t correct, long long B, int NC, float gscale,
                                float smoothing, uintptr_t st) {
    chk(fn_softmax_xent_rows(P<const void*>(logits), in_bf16, P<const long long*>(labels), P<float*>(block_loss),
                             P<void*>(dlogits), P<int*>(correct), B, NC, gscale, smoothing, S(st)),
        "softmax_xent_rows");
  });
  m.def("softmax_rows", [](uintptr_t x, uintptr_t y, long long M, int N, int backward, uintptr_t g, uintptr_t st,
                           std::vector<long long> ext) {
    // forward: y = softmax(x) over rows of N fp32; backward (x = y, y = dx): dx = y * (g - sum g y)
    fits(ext, 0, M * N, "softmax_rows", "x");
    fits(ext, 1, M * N, "softmax_rows", "y");
    if (backward) fits(ext, 2, M * N, "softmax_rows", "g");
    chk(fn_softmax_rows(P<const float*>(x), P<float*>(y), M, N, backward, P<const float*>(g), S(st)), "softmax_rows");
  });
  m.def("cu_occupy", [](int nwg, int usec, int lds, uintptr_t sink, uintptr_t st) {
    // (measurement only: pins nwg CUs on the given stream for usec microseconds; sink >= 1 KB)
    chk(fn_cu_occupy(nwg, usec, lds, P<void*>(sink), S(st)), "cu_occupy");
  });
  m.def("adam_flat_dev", [](uintptr_t p, uintptr_t g, uintptr_t mm, uintptr_t v, uintptr_t pb, long long n,
                            uintptr_t hp, uintptr_t t, int keras_eps, uintptr_t st) {
    chk(fn_adam_flat_dev(P<float*>(p), P<const float*>(g), P<float*>(mm), P<float*>(v), P<void*>(pb), n,
                         P<const float*>(hp), P<int*>(t), keras_eps, S(st)),
        "adam_flat_dev");
  });
  m.def("adam_flat", [](uintptr_t p, uintptr_t g, uintptr_t mm, uintptr_t v, uintptr_t pb, long long n, float lr,
                        float b1, float b2, float eps, float wd, float bc1, float bc2, float gscale, int keras_eps,
                        uintptr_t st) {
    chk(fn_adam_flat(P<float*>(p), P<const float*>(g), P<float*>(mm), P<float*>(v), P<void*>(pb), n, lr, b1, b2, eps,
                     wd, bc1, bc2, gscale, keras_eps, S(st)),
        "adam_flat");
  });
  m.def("sgd_flat", [](uintptr_t p, uintptr_t g, uintptr_t buf, uintptr_t pb, long long n, float lr, float momentum,
                       float wd, int nesterov, float gscale, uintptr_t st) {
    chk(fn_sgd_flat(P<float*>(p), P<const float*>(g), P<float*>(buf), P<void*>(pb), n, lr, momentum, wd, nesterov,
                    gscale, S(st)),
        "sgd_flat");
  });
  m.def("bias_act", [](uintptr_t x, uintptr_t bias, uintptr_t y, long long total, int C, int act, uintptr_t st) {
    chk(fn_bias_act(P<const void*>(x), P<const float*>(bias), P<void*>(y), total, C, act, S(st)), "bias_act");
  });
  m.def("act_bwd", [](uintptr_t dy, uintptr_t y, uintptr_t dx, long long total, int act, uintptr_t st) {
    chk(fn_act_bwd(P<const void*>(dy), P<const void*>(y), P<void*>(dx), total, act, S(st)), "act_bwd");
  });
  m.def("dropout", [](uintptr_t x, uintptr_t y, long long total, float p, unsigned seed, unsigned offset,
                      uintptr_t st) {
    chk(fn_dropout(P<const void*>(x), P<void*>(y), total, p, seed, offset, S(st)), "dropout");
  });
  m.def("unpack_bits", [](uintptr_t bits, uintptr_t out, long long nbytes, uintptr_t st) {
    chk(fn_unpack_bits(P<const void*>(bits), P<void*>(out), nbytes, S(st)), "unpack_bits");
  });
  m.def("copy2", [](uintptr_t d0, uintptr_t s0, long long n0, uintptr_t d1, uintptr_t s1, long long n1, uintptr_t st) {
    chk(fn_copy2(P<void*>(d0), P<const void*>(s0), n0, P<void*>(d1), P<const void*>(s1), n1, S(st)), "copy2");
  });
  m.def("scale_unless_one", [](uintptr_t x, int is_bf16, uintptr_t s, long long n, uintptr_t st) {
    chk(fn_scale_unless_one(P<void*>(x), is_bf16, P<const float*>(s), n, S(st)), "scale_unless_one");
  });
  m.def("cast_f32_bf16", [](uintptr_t x, uintptr_t y, long long n, uintptr_t st) {
    chk(fn_cast_f32_bf16(P<const float*>(x), P<void*>(y), n, S(st)), "cast_f32_bf16");
  });
}
