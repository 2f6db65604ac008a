"""A plain float64 oracle of the conv kernels (``csrc/kernels/conv_tile.hip``, ``conv_wtile.hip``,
``conv_halo.hip``, ``conv_igemm.hip``), the inputs that make them exact, and the case table.

The oracle is the definition: one slice of the zero-padded input and one ``matmul`` per tap,
in float64.  No library convolution, no autograd, nothing from ``ops/reference.py`` -- it shares
no code with the kernels it judges nor with the reference the other tests use.

Activations are channels-last ``[N, D, H, W, C]``, weights ``[K, KD, KH, KW, C]``, the geometry a
``ConvSpec`` (strides, dilations, leading pads ``pd / ph / pw``; taps past the end read zero).

Why the comparisons need no tolerance
-------------------------------------
Every input lies on a dyadic grid (``make_inputs``):

* ``x``    integers in [-4, 4]            (step 1)
* ``xs``   integers in [-1, 1], half of them zeroed: the input of the statistics runs, small
  so that the sum of squares stays exact too
* ``dy``   integers in [-4, 4]            (step 1)
* ``w``    from {+-1/4, +-1/2, +-1}       (step 1/4; never zero: a zero weight hides a
  mis-addressed tap)
* ``bias`` multiples of 1/4 in [-1, 1]

All are bf16 values, so the MFMA products are exact in fp32, and every partial sum of a
result -- whatever the MFMA, slice, slab, split or atomic order -- is a multiple of the
result's ``step``.  An fp32 partial sum of multiples of ``step`` is exact while its magnitude
stays below ``2^24 step``; the magnitude of any partial sum is at most ``sum |terms|``.  So
the condition

    sum |terms| / step < 2^24                                   (``exact_margin``)

makes the kernel's fp32 sum *the* sum, in any order.  The oracle returns ``sum |terms|`` of
every sum as ``*_abs`` and ``tests/test_conv_oracle_cpu.py`` asserts the condition for every
case and quantity.  At the largest case (4,000 terms of magnitude <= 4, step 1/4) it is
6.4e4 of 1.7e7.

Exact quantities (``check_exact``, bit for bit) -- ``STEPS`` holds each one's step:

* ``y``, ``dx``   = ``bf16_round`` of the oracle: the exact fp32 sum, then one rounding to
  nearest even (outputs beyond 64 = 2^8 steps are common, so the rounding and its ties are
  real: the CPU test counts them);
* ``dW``, ``db``  = the oracle as fp32 (sums of integers);
* ``sum_v``, ``sum_v2`` the BN statistics.  All three forward kernels take them from the
  *stored* bf16 values (conv_tile.hip's epilogue unpacks the stored words; conv_halo.hip and
  conv_igemm.hip re-read the staged bf16 tile), so the oracle sums ``bf16_round(y)`` and its
  square.  A rounded ``y`` is still a multiple of 1/4, its square of 1/16.  The test adds the
  slab rows in float64; the condition is asserted on the whole tensor's sum, which covers
  every way of dealing the tiles to slab rows.  (At the large batches of ``STAT_BATCH``, where
  a slab row adds several tiles, it is asserted per row instead: rows x the largest tile sum.)

Bounded quantities are named in ``BOUNDED`` as ``(case, quantity)``:

* ``y_tanh``, the tanh epilogue (``TANH_CASES``): the argument is the exact fp32 sum, so what
  remains is ``tanhf`` (a few fp32 ulps) and the bf16 rounding of its result -- judged by
  ``check_one_rounding`` with the magnitude |tanh|: 2^-8 |r| + 2^-18 |r|;
* a sum that misses the condition.  With these magnitudes there is none.  The CPU test
  recomputes the set of sums that miss it and requires it to equal what ``BOUNDED`` lists, so a
  later case that leaves the exact regime fails there; the GPU test then judges such a sum by
  ``check_reduction`` with ``sum |terms|`` from here and n = the number of terms (any order of
  m additions errs by at most (m - 1) 2^-24 sum |terms|).

Guard bands (``Guard`` is in the GPU file): inputs are built by ``banded`` -- a contiguous
view of the middle of a flat buffer whose two ends hold ``SENTINEL``, a large finite bf16
value.  A read outside the tensor that reaches a result breaks the exact comparison; one that
is multiplied by a zero weight or masked stays harmless, as it should.
"""
from __future__ import annotations

import dataclasses
import zlib

import torch

from _bn_pool_oracle import ACT_NONE, ACT_RELU, bf16_round, grid  # noqa: F401  (re-exported)
from featurenet_amd.ops.spec import ConvSpec

SENTINEL = 2.0 ** 60                             # a bf16 value; one product with it swamps any result
BAND = 512                                       # guard elements on each side (a multiple of 16 B in every dtype)

# the step of each checked quantity (see the module docstring)
STEPS = {"y": 0.25, "dx": 0.25, "dW": 1.0, "db": 1.0, "sum_v": 0.25, "sum_v2": 0.0625}
# (case name, quantity) pairs that are not compared bit for bit (filled in below the case table)
BOUNDED: list = []

W_VALUES = (-1.0, -0.5, -0.25, 0.25, 0.5, 1.0)


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def _padded(x: torch.Tensor, s: ConvSpec) -> torch.Tensor:
    hd, hh, hw = s.pads_hi
    N, D, H, W, C = x.shape
    xp = torch.zeros(N, D + s.pd + hd, H + s.ph + hh, W + s.pw + hw, C, dtype=x.dtype)
    xp[:, s.pd: s.pd + D, s.ph: s.ph + H, s.pw: s.pw + W] = x
    return xp


def _taps(s: ConvSpec):
    """(tap index, slices of the padded input that the tap multiplies) in (kd, kh, kw) scan order."""
    t = 0
    for kd in range(s.KD):
        for kh in range(s.KH):
            for kw in range(s.KW):
                z = (kd * s.dd, kh * s.dh, kw * s.dw)
                yield t, (slice(None), slice(z[0], z[0] + s.sd * (s.OD - 1) + 1, s.sd),
                          slice(z[1], z[1] + s.sh * (s.OH - 1) + 1, s.sh),
                          slice(z[2], z[2] + s.sw * (s.OW - 1) + 1, s.sw))
                t += 1


def act_fwd(u: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return torch.where(u > 0, u, torch.zeros_like(u))
    assert act == ACT_NONE, "the exact oracle has the identity and relu"
    return u


def forward(x: torch.Tensor, w: torch.Tensor, b, s: ConvSpec, act: int = ACT_NONE) -> dict:
    """y = act(conv(x, w) + b) [N, OD, OH, OW, K] and ``y_abs`` (sum |terms| in front of the
    activation); the BN statistics of the stored values, ``sum_v`` / ``sum_v2`` [K], with their
    ``*_abs``."""
    assert x.dtype == w.dtype == torch.float64
    xp = _padded(x, s)
    w3 = w.reshape(s.K, s.taps, s.C)
    pre = torch.zeros(s.out_shape5, dtype=torch.float64)
    mag = torch.zeros_like(pre)
    for t, sl in _taps(s):
        xs = xp[sl]
        pre += xs @ w3[:, t].T
        mag += xs.abs() @ w3[:, t].abs().T
    if b is not None:
        pre, mag = pre + b, mag + b.abs()
    y = act_fwd(pre, act)
    v = bf16_round(y).reshape(-1, s.K)
    return {"y": y, "y_abs": mag, "sum_v": v.sum(0), "sum_v_abs": v.abs().sum(0), "sum_v2": (v * v).sum(0),
            "sum_v2_abs": (v * v).sum(0)}


def backward(x: torch.Tensor, w: torch.Tensor, g: torch.Tensor, s: ConvSpec, want=("dx", "dW")) -> dict:
    """Gradients of sum(g * conv(x, w)): ``dx`` like x, ``dW`` [K, taps, C] (the kernels' order),
    ``db`` [K], each with its ``*_abs``.  ``g`` is the gradient at the conv's output, in front of
    any activation.  ``want``: which of dx / dW to work out (the large-batch cases need dW only)."""
    assert x.dtype == w.dtype == g.dtype == torch.float64
    xp = _padded(x, s)
    w3 = w.reshape(s.K, s.taps, s.C)
    dxp, dxp_abs = torch.zeros_like(xp), torch.zeros_like(xp)
    dW = torch.zeros(s.K, s.taps, s.C, dtype=torch.float64)
    dW_abs = torch.zeros_like(dW)
    g2 = g.reshape(-1, s.K)
    g2a = g2.abs()
    for t, sl in _taps(s):
        if "dx" in want:
            dxp[sl] += g @ w3[:, t]
            dxp_abs[sl] += g.abs() @ w3[:, t].abs()
        if "dW" in want:
            xs2 = xp[sl].reshape(-1, s.C)
            dW[:, t] = g2.T @ xs2
            dW_abs[:, t] = g2a.T @ xs2.abs()
    crop = (slice(None), slice(s.pd, s.pd + s.D), slice(s.ph, s.ph + s.H), slice(s.pw, s.pw + s.W))
    return {"dx": dxp[crop].contiguous(), "dx_abs": dxp_abs[crop].contiguous(), "dW": dW, "dW_abs": dW_abs,
            "db": g2.sum(0), "db_abs": g2.abs().sum(0)}


def exact_margin(sum_abs: torch.Tensor, step: float) -> float:
    """Largest sum |terms| / (2^24 step): below 1, an fp32 sum of multiples of ``step`` is exact
    in any order."""
    return float(sum_abs.max()) / (2.0 ** 24 * step)


def on_grid(t: torch.Tensor, step: float) -> bool:
    return bool(((t / step).round() * step == t).all())


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def make_inputs(case: dict, N: int | None = None) -> dict:
    """float64 x, xs, w, b, dy of a case (at batch ``N`` when given) on the grids of the module
    docstring (CPU)."""
    s = make_spec(case, N)
    g = gen(case["name"])
    x = grid((s.N, s.D, s.H, s.W, s.C), 1.0, 4.0, g)
    wi = torch.randint(0, len(W_VALUES), (s.K, s.KD, s.KH, s.KW, s.C), generator=g)
    w = torch.tensor(W_VALUES, dtype=torch.float64)[wi]
    b = grid((s.K,), 0.25, 1.0, g)
    dy = grid(s.out_shape5, 1.0, 4.0, g)
    xs = grid(x.shape, 1.0, 1.0, g) * torch.randint(0, 2, x.shape, generator=g).to(torch.float64)
    return {"x": x, "xs": xs, "w": w, "b": b, "dy": dy, "spec": s}


def banded(t64: torch.Tensor, dtype: torch.dtype, device) -> torch.Tensor:
    """``t64`` as a contiguous ``dtype`` view of the middle of a flat device buffer whose ends
    hold SENTINEL; the values must survive the cast."""
    n = t64.numel()
    flat = torch.full((n + 2 * BAND,), SENTINEL, dtype=dtype)
    flat[BAND: BAND + n] = t64.reshape(-1).to(dtype)
    assert torch.equal(flat[BAND: BAND + n].double(), t64.reshape(-1)), "input is not representable"
    flat = flat.to(device)
    return flat[BAND: BAND + n].view(t64.shape)


# ---------------------------------------------------------------------------
# the case table: the smallest shapes at which each path can still go wrong
#   (N, D, H, W, C, K, kernel, padding[, stride, dilation]); ``reach``: what the row reaches at the
#   plans of ops/conv_tile.py, ops/conv_wtile.py and ops/conv.py (asserted property by property
#   in tests/test_conv_oracle_cpu.py)
# ---------------------------------------------------------------------------
def _case(name, shape, K, kernel, padding="valid", stride=1, dilation=1, reach=""):
    return {"name": name, "shape": shape, "K": K, "kernel": kernel, "padding": padding, "stride": stride,
            "dilation": dilation, "reach": reach}


TILE_CASES = [
    _case("conv2_c32_k5", (2, 11, 12, 13, 32), 32, 5,
          reach="fwd tile partial in D; dgrad partial in D and H; wtile 8 waves, nacc 16, 2 column groups, unsplit"),
    _case("conv4_c64_k3", (2, 9, 10, 11, 64), 64, 3,
          reach="fwd CS 16 x 4 slices, 2 column blocks; dgrad NT 4 / MT 4 / CS 32; wtile k-step split, dead taps"),
    _case("conv4_c64_k3_same", (1, 9, 10, 11, 64), 64, 3, "same", reach="the same with padding on every face"),
    _case("c16_k48_same", (3, 7, 9, 11, 16), 48, 3, "same", reach="48 columns: a partial column block; no wtile plan"),
    _case("c32_k96_same", (1, 9, 10, 11, 32), 96, 3, "same", reach="3 column blocks"),
    _case("flat_c32_k5", (2, 1, 23, 27, 32), 32, (1, 5, 5), "same", reach="2-D, tile partial in H"),
    _case("stem_c8_k4", (2, 10, 11, 12, 8), 32, 4, reach="the s2d stem's class: CS 8, no dgrad plan, wtile c8"),
    _case("c16_k16_same", (1, 8, 9, 10, 16), 16, 3, "same", reach="Cout 16: the 4-wave wtile form"),
    _case("wsplit_c32", (1, 5, 6, 61, 32), 32, 3, "same", reach="W split: last tile narrower, fwd / dgrad / wtile"),
    _case("c24_k40_same", (1, 8, 9, 10, 24), 40, 3, "same", reach="C % 16 != 0: three 8-channel slices; 40 columns"),
]
# no tile forward plan: 336 output positions, under the 384 a tile needs (the halo kernel's)
NO_TILE_CASE = _case("conv3_small_k4", (2, 9, 10, 11, 32), 64, 4, reach="no conv_tile forward plan; halo")
# the gathered kernel (conv_igemm.hip): strided, dilated, few or odd channels
IGEMM_CASES = [
    _case("ig_s2_k7_c1", (2, 16, 16, 16, 1), 32, 7, "valid", 2, reach="packed-W gather, stride 2"),
    _case("ig_flat_c3", (2, 1, 14, 15, 3), 16, (1, 3, 3), "same", reach="packed-W gather, 2-D, rows of 9 -> 16"),
    _case("ig_flat_c3_dil2", (2, 1, 14, 15, 3), 16, (1, 3, 3), "same", 1, (1, 2, 2),
          reach="scalar gather (3 channels; dilated, so the packed-W rows do not apply)"),
    _case("ig_s2_same_c8", (2, 9, 10, 11, 8), 24, 3, "same", 2, reach="vector gather, dgrad by zero insertion"),
    _case("ig_dil2_c16", (1, 9, 10, 11, 16), 32, 3, "same", 1, 2, reach="vector gather, dilation 2"),
    _case("ig_lenet_c12_k120", (4, 1, 5, 5, 12), 120, (1, 5, 5), reach="scalar gather; split-K forward and dgrad"),
]
# the halo kernel's own W split: a 57-wide output whose full-width tile would leave the 256 rows empty
HALO_WSPLIT_CASE = _case("halo_wsplit_c32", (1, 6, 6, 61, 32), 32, 5, reach="conv_halo tiles narrower than the output")
CASES = TILE_CASES + [NO_TILE_CASE, HALO_WSPLIT_CASE] + IGEMM_CASES
STRIDE1_CASES = TILE_CASES + [NO_TILE_CASE, HALO_WSPLIT_CASE]
# forward plans with 32-channel slices exist only when forced (FN_TILE_CS=32), as in the CS tests
CS32_CASES = ("conv4_c64_k3", "conv4_c64_k3_same", "c32_k96_same", "flat_c32_k5", "wsplit_c32")
# conv_wtile.hip deals the tiles of each of the 8 XCDs round-robin to the plan's ``workers``; the
# batch at which every form of the plan (FN_WTILE_KS2 0 / 1, FN_WTILE_NW 4 / 8) gives a worker at
# least three jobs, so that the 3-slot job ring wraps (``wtile_jobs``; only dW is taken at this
# batch, which costs the oracle about a second)
WTILE_N = {"conv2_c32_k5": 86, "conv4_c64_k3": 43, "conv4_c64_k3_same": 33, "flat_c32_k5": 129, "stem_c8_k4": 257,
           "c16_k16_same": 171, "wsplit_c32": 65, "conv3_small_k4": 86}
WTILE_FORMS = ({}, {"FN_WTILE_KS2": "0"}, {"FN_WTILE_KS2": "1"}, {"FN_WTILE_NW": "4"}, {"FN_WTILE_NW": "8"})


def wtile_jobs(p, s: ConvSpec) -> int:
    """Jobs of the busiest worker of a conv_wtile plan: ceil(tiles of one XCD / workers)."""
    tiles = s.N * -(-s.OD // p.TD) * -(-s.OH // p.TH) * -(-s.OW // p.TW)
    return -(-(-(-tiles // 8)) // p.workers)


BY_NAME = {c["name"]: c for c in CASES}
# BN statistics where one slab row adds up several tiles.  At the table's own batches every
# statistics launch has a workgroup (static schedule) or a chunk (chunked schedule) per tile.
# The static schedule -- the one-GPU production path -- deals ntiles tiles to at most
# 256 / column blocks workgroups (conv_tile.hip) or 512 / column blocks (conv_halo.hip, two
# workgroups per CU): at these batches each gets three or more.  ``xs`` keeps every slab row
# exact (``max_tile_sums``); only the statistics run is taken at this batch.  Chunks of more
# than one tile need over 8192 tiles and stay uncovered.
STAT_BATCH = {"c16_k16_same": 512, "c16_k48_same": 192}
STAT_HALO = ("c16_k16_same",)                    # (48 columns at batch 192: only two halo tiles a row)


def tile_count(s: ConvSpec, dims) -> int:
    return s.N * -(-s.OD // dims[0]) * -(-s.OH // dims[1]) * -(-s.OW // dims[2])


def max_tile_sums(v: torch.Tensor, s: ConvSpec, dims) -> tuple:
    """(max sum |v|, max sum v^2) over the output tiles of extent ``dims`` and the columns of the
    stored values ``v`` [N, OD, OH, OW, K].  A slab row that adds r tiles sums at most r times
    these, whichever tiles they are -- the exactness condition of a row, free of the kernel's
    tile-to-workgroup map."""
    TD, TH, TW = dims
    nd, nh, nw = -(-s.OD // TD), -(-s.OH // TH), -(-s.OW // TW)
    vp = torch.zeros(s.N, nd * TD, nh * TH, nw * TW, s.K, dtype=v.dtype)
    vp[:, : s.OD, : s.OH, : s.OW] = v
    t = vp.reshape(s.N, nd, TD, nh, TH, nw, TW, s.K)
    return float(t.abs().sum((2, 4, 6)).max()), float((t * t).sum((2, 4, 6)).max())
# the tanh epilogue of conv_halo.hip and conv_igemm.hip (conv_tile.hip has the identity and relu
# only), on ``xs`` + bias so that a good share of the outputs is not saturated
TANH_CASES = ("c16_k16_same", "stem_c8_k4", "c24_k40_same", "ig_flat_c3", "ig_flat_c3_dil2", "ig_s2_same_c8")
BOUNDED += [(n, "y_tanh") for n in TANH_CASES]


def make_spec(case: dict, N: int | None = None) -> ConvSpec:
    shape = tuple(case["shape"]) if N is None else (N,) + tuple(case["shape"][1:])
    return ConvSpec.make(shape, case["K"], case["kernel"], case["stride"], case["padding"], case["dilation"])


def padded_channels(s: ConvSpec, cp: int) -> ConvSpec:
    return dataclasses.replace(s, C=cp)
