"""The BN and pooling kernels (csrc/kernels/bn_pool.hip) against the fp64 oracle of
tests/_bn_pool_oracle.py, host-dispatch path by path.

Kernel level: the bindings are called directly with inputs on dyadic grids -- y and dout
multiples of 1/8 in [-4, 4], scale and shift multiples of 1/16 in [-2, 2] (both signs of scale and
scale = 0 in every case) -- so y * scale + shift is exact in fp32 and arg-max, ties, relu masks
and sums are decidable without a tolerance: max pooling, its backward, bn_apply and the moment
slabs are compared bit for bit; average pooling, the dy kernels and tanh / sigmoid get the
one-rounding bound, inexact sums the reduction bound (both in the oracle module).  Every output
buffer starts as NaN, so an element a kernel does not write fails.

Module level: ops.pool / global_avg_pool / batchnorm_act / batchnorm_act_pool with real
bn_finalize parameters.  Those parameters are judged against the oracle's own first; what
follows them is judged against the oracle evaluated at them, under the same one-rounding and
(n + 8) 2^-24 bounds as at kernel level.  Relu inputs with z ~ 0 are undecidable (the fp32
roundings of y * scale + shift decide them) and are left out (elements, or their windows), sums
are widened by the oracle's own difference with those elements' mask on and off; the bf16 store
of the pool's input gradient is modelled, its rare undecidable roundings handled the same way.

Out of scope: the 64-bit instances (I = long long) of the pooled kernels need more than 2^31
elements.
"""
import json
import math
import os
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import _bn_pool_oracle as O  # noqa: E402
from featurenet_amd import _native, ops  # noqa: E402
from featurenet_amd.ops.spec import PoolSpec  # noqa: E402

NONE, RELU, TANH, SIGMOID = O.ACT_NONE, O.ACT_RELU, O.ACT_TANH, O.ACT_SIGMOID
_REC = []            # (case, kernels reached, check, worst error / bound)


def _rec(case, kernels, check, frac):
    _REC.append({"case": case, "kernels": kernels, "check": check, "frac": float(frac)})


@pytest.fixture(scope="module", autouse=True)
def _report():
    """FN_BN_POOL_ORACLE_REPORT=<file>: the observed error / bound of every check as JSON lines
    (the source of profiles/bn_pool_oracle.md)."""
    yield
    path = os.environ.get("FN_BN_POOL_ORACLE_REPORT")
    if path:
        with open(path, "w") as f:
            for r in _REC:
                f.write(json.dumps(r) + "\n")


def _dev():
    return torch.device("cuda", 0)


def _gen(name, device="cpu"):
    return torch.Generator(device=device).manual_seed(zlib.crc32(name.encode()))


def _bf(t64):
    b = t64.to(torch.float32).to(torch.bfloat16).to(_dev()).contiguous()
    assert torch.equal(b.double(), t64.to(_dev())), "input is not a bf16 value"
    return b


def _f32(t64):
    f = t64.to(torch.float32).to(_dev()).contiguous()
    assert torch.equal(f.double(), t64.to(_dev())), "input is not an fp32 value"
    return f


def _invstd_grid(C, gen):
    """Multiples of 1/16 in (0, 2]."""
    return torch.randint(1, 33, (C,), generator=gen, device=gen.device).double() / 16


def _nan(shape, dtype=torch.bfloat16):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=_dev())


def _params(C, gen, act):
    """scale / shift on the 1/16 grid; channel 0 has scale 0, channel 1 a negative, channel 2 a
    positive scale.  tanh / sigmoid: |scale| <= 3/4, |shift| <= 1, so |u| <= 4."""
    soft = act in (TANH, SIGMOID)
    scale = O.grid((C,), 1 / 16, 0.75 if soft else 2.0, gen)
    shift = O.grid((C,), 1 / 16, 1.0 if soft else 2.0, gen)
    scale[0], shift[0] = 0.0, 0.5
    scale[1] = -scale[1].abs().clamp_min(1 / 16)
    scale[2] = scale[2].abs().clamp_min(1 / 16)
    return scale, shift


def _f32_of(t64):
    """The fp32 rounding of a float64 tensor, as float64 (what a kernel reads)."""
    return t64.to(torch.float32).to(torch.float64)


# ---------------------------------------------------------------------------
# pooled kernels
# ---------------------------------------------------------------------------
def _pool_case(case, kind, count_pad, act, pro, N=None, odev="cpu"):
    """One geometry through pool_fwd, pool_bwd and -- max pooling with the prologue -- the
    pool_bwd_stats / pool_bn_bwd_apply pair.  The oracle runs on ``odev``."""
    Kn = _native.kernels()
    s = O.make_spec(case, N)
    geom, C, is_max = s.geom17(), s.C, kind == "max"
    tag = f"{case['name']}-{kind}-cp{int(count_pad)}-{'pro-' + O.ACT_NAMES[act] if pro else 'plain'}"
    gen = _gen(tag, odev)
    y64 = O.grid((s.N, s.D, s.H, s.W, C), 1 / 8, 4.0, gen)
    dout64 = O.grid(s.out_shape5, 1 / 8, 4.0, gen)
    sc64, sh64 = _params(C, gen, act) if pro else (None, None)
    y, dout = _bf(y64), _bf(dout64)
    scale, shift = (_f32(sc64), _f32(sh64)) if pro else (None, None)
    sp, hp = _native.ptr(scale), _native.ptr(shift)
    st = _native.stream(y)
    exact = not pro or act in (NONE, RELU)

    z, dact = O.prologue(y64, sc64, sh64, act)
    f = O.pool_fwd(z, s, kind, count_pad)
    b = O.pool_bwd(dout64, s, f["sel"])
    if is_max and not exact:
        # input precondition of the near-tie cases: the two largest distinct candidates of every
        # window are further apart than any error of tanhf / __expf at |u| <= 4
        assert float((y64 * sc64 + sh64).abs().max()) <= 4.0
        assert O.window_gap(f["win"]) > 1e-6

    out = _nan(s.out_shape5)
    Kn.pool_fwd(y.data_ptr(), out.data_ptr(), sp, hp, geom, int(is_max), int(count_pad), act, st,
                [y.numel(), out.numel()])
    dx = _nan(y.shape)
    Kn.pool_bwd(dout.data_ptr(), y.data_ptr(), dx.data_ptr(), sp, hp, geom, int(is_max), int(count_pad), act, st,
                [y.numel(), dout.numel()])
    kn = case["kernels"]
    if is_max:
        if exact:
            _rec(tag, kn, "fwd exact", O.check_exact(out, O.bf16_round(f["out"]), "pool_fwd"))
        else:
            _rec(tag, kn, "fwd one rounding", O.check_one_rounding(out, f["out"], f["mag"], "pool_fwd"))
        # the backward only routes dout (a bf16 value) or adds a few of them: exact for every act
        _rec(tag, kn, "bwd exact", O.check_exact(dx, O.bf16_round(b["dx"]), "pool_bwd"))
    else:
        _rec(tag, kn, "fwd one rounding", O.check_one_rounding(out, f["out"], f["mag"], "pool_fwd avg"))
        _rec(tag, kn, "bwd one rounding", O.check_one_rounding(dx, b["dx"], b["mag"], "pool_bwd avg"))

    nb = Kn.pool_bwd_stats_blocks(geom)
    assert (nb > 0) == case["stats"], f"pool_bwd_stats_blocks = {nb}"
    if not (is_max and pro):
        return s, nb
    # --- BN backward of act(bn(y)) under the max pool: g = dz * act'(z), dz = the pool's dx
    M = y64.numel() // C
    g = b["dx"] * dact
    g_abs = b["dx"].abs() * O.act_bwd_mag(z, act)
    y2, g2, ga2 = y64.reshape(-1, C), g.reshape(-1, C), g_abs.reshape(-1, C)
    zero, one = torch.zeros(C, dtype=torch.float64, device=odev), torch.ones(C, dtype=torch.float64, device=odev)
    raw = O.bn_bwd_sums(g2, y2, zero, one, ga2)
    want = torch.stack([raw["sg"], raw["sgy"]])
    if nb > 0:
        cpr = C // 8
        total = s.N * s.OD * s.OH * s.OW * cpr
        win = s.KD * s.KH * s.KW
        # longest chain of additions: a thread's windows, then the 256 / cpr threads of a channel
        # chunk, then the nb slab rows
        n = -(-total // (nb * 256)) + 256 // cpr + nb
        if exact:
            # precondition of the exact slab checks: per window and channel one term |g| (1/8 grid)
            # and |g * y| (1/64 grid); window chunk i = window * cpr + chunk is added by workgroup
            # (i mod nb * 256) / 256, in pool_bn_moments8 and pool_bwd_tiled<8, true> alike
            gw = (dout64 * O.act_bwd_from_out(f["out"], act)).reshape(-1, cpr, 8)
            yarg = (f["sel"] * O.windows(y64, s, 0.0)).sum(-1).reshape(-1, cpr, 8)
            i = torch.arange(gw.shape[0] * cpr, device=odev)
            row = (i % (nb * 256)) // 256
            O.slab_rows_exact(gw.abs().reshape(-1, 8), row, nb, 1 / 8)
            O.slab_rows_exact((gw * yarg).abs().reshape(-1, 8), row, nb, 1 / 64)
        for with_dx in (True, False):
            # with dx: pool_bwd_tiled<8, true>; dx = 0: pool_bn_moments8<int> (<= 8 positions) or
            # pool_bwd_tiled<8, true> writing nothing
            part = _nan((nb, 2, C), torch.float32)
            dxs = _nan(y.shape) if with_dx else None
            Kn.pool_bwd_stats(dout.data_ptr(), y.data_ptr(), _native.ptr(dxs), sp, hp, geom, act, part.data_ptr(), st,
                              [y.numel(), dout.numel(), part.numel()])
            what = f"stats {'dx' if with_dx else 'moments only'}"
            if with_dx:
                _rec(tag, kn, what + " dx exact", O.check_exact(dxs, O.bf16_round(b["dx"]), "pool_bwd_stats dx"))
            got = part.double().sum(0)
            if exact:
                _rec(tag, kn, what + " slabs exact", O.check_exact(got, want, "moment slabs"))
            else:
                _rec(tag, kn, what + f" reduction n={n}",
                     O.check_reduction(got, want, torch.stack([raw["sg_abs"], raw["sgy_abs"]]), n, "moments"))
        assert win <= 8 or not case["fused"]
    # --- the fused apply: dy straight from (dout, y)
    mean64 = O.grid((C,), 1 / 8, 1.0, gen)
    invstd64 = _invstd_grid(C, gen)
    sums = O.bn_bwd_sums(g2, y2, mean64, invstd64, ga2)
    dbeta64, dgamma64 = _f32_of(sums["dbeta"]), _f32_of(sums["dgamma"])
    inv = float(torch.tensor(1.0 / M, dtype=torch.float32))
    want_dy = O.bn_dy(g, y64, sc64, mean64, invstd64, dbeta64, dgamma64, inv, g_abs)
    mean, invstd, dbeta, dgamma = _f32(mean64), _f32(invstd64), _f32(dbeta64), _f32(dgamma64)
    dy = _nan(y.shape)
    args = (dout.data_ptr(), y.data_ptr(), sp, hp, mean.data_ptr(), invstd.data_ptr(), dbeta.data_ptr(),
            dgamma.data_ptr(), dy.data_ptr(), geom, act, inv, st, [y.numel(), dout.numel()])
    if case["fused"]:
        Kn.pool_bn_bwd_apply(*args)              # pool_bn_bwd_apply<int, act>
        _rec(tag, kn, "fused apply one rounding",
             O.check_one_rounding(dy, want_dy["dy"], want_dy["mag"], "pool_bn_bwd_apply"))
    else:
        with pytest.raises(RuntimeError):        # the host refuses (-2): no kernel for this geometry
            Kn.pool_bn_bwd_apply(*args)
    # the unfused pair on the same numbers: bn_bwd_apply over the pool's dz
    dy2 = _nan(y.shape)
    Kn.bn_bwd_apply(dx.data_ptr(), y.data_ptr(), sp, hp, mean.data_ptr(), invstd.data_ptr(), dbeta.data_ptr(),
                    dgamma.data_ptr(), dy2.data_ptr(), y.numel(), C, inv, act, st)
    _rec(tag, kn, "bn_bwd_apply one rounding",
         O.check_one_rounding(dy2, want_dy["dy"], want_dy["mag"], "bn_bwd_apply after pool_bwd"))
    return s, nb


def _pool_params():
    out = []
    for c in O.POOL_CASES:
        for kind in c["kinds"]:
            for cp in c["count_pad"]:
                modes = [(False, NONE), (True, NONE), (True, RELU)]
                if c["dagger"]:                  # (avg: the runtime-activation pool2_fwd<2, -1>)
                    modes += [(True, TANH), (True, SIGMOID)]
                for pro, act in modes:
                    name = f"{c['name']}-{kind}-cp{int(cp)}-{'pro-' + O.ACT_NAMES[act] if pro else 'plain'}"
                    out.append(pytest.param(c, kind, cp, act, pro, id=name))
    return out


@pytest.mark.parametrize("case,kind,count_pad,act,pro", _pool_params())
def test_pool_kernels(case, kind, count_pad, act, pro):
    _pool_case(case, kind, count_pad, act, pro)


def test_pool_kernels_second_round():
    """33 x 80^3 x 8, 2^3 windows, relu: 2,112,000 window chunks > 8192 * 256, the smallest
    geometry whose resident-grid kernels (pool2_fwd, moments8, pool_bn_bwd_apply) and
    ew_blocks-capped kernels (pool_bwd_tiled) take a second grid-stride round -- the
    software-pipelined prefetch and its re-load of the current window past the end."""
    case = O.LARGE_CASE
    s, nb = _pool_case(case, "max", False, RELU, True, odev=_dev())
    total = s.N * s.OD * s.OH * s.OW * (s.C // 8)
    assert 8192 * 256 < total                   # every grid cap of the file is <= 8192
    assert 0 < nb and nb * 256 < total
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# bn_apply / bn_bwd_apply
# ---------------------------------------------------------------------------
def _bn_apply_case(M, C, act, odev="cpu"):
    Kn = _native.kernels()
    tag = f"bn-M{M}-C{C}-{O.ACT_NAMES[act]}"
    vw = 8 if C % 8 == 0 else 1
    fixed = 256 % (C // vw) == 0
    kn = f"bn_apply / bn_bwd_apply <VW {vw}>, {'fixed-chunk' if fixed else 'per-element'} parameters"
    gen = _gen(tag, odev)
    y64, dz64 = O.grid((M, C), 1 / 8, 4.0, gen), O.grid((M, C), 1 / 8, 4.0, gen)
    sc64, sh64 = _params(C, gen, act)
    mean64 = O.grid((C,), 1 / 8, 1.0, gen)
    invstd64 = _invstd_grid(C, gen)
    y, dz, scale, shift = _bf(y64), _bf(dz64), _f32(sc64), _f32(sh64)
    st = _native.stream(y)
    z64, dact = O.prologue(y64, sc64, sh64, act)
    exact = act in (NONE, RELU)

    z = _nan((M, C))
    with_mask = vw == 8 and fixed
    mask = torch.full((M * C // 8,), 0xAA, dtype=torch.uint8, device=_dev()) if vw == 8 else None
    call = lambda m: Kn.bn_apply(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), z.data_ptr(), M * C, C, act, st,  # noqa: E731
                                 _native.ptr(m), 0 if m is None else m.numel())
    if mask is not None and not with_mask:
        with pytest.raises(RuntimeError):        # only the fixed-chunk path writes the mask: -2
            call(mask)
        mask = None
    call(mask)
    if exact:
        _rec(tag, kn, "bn_apply exact", O.check_exact(z, O.bf16_round(z64), "bn_apply"))
    else:
        _rec(tag, kn, "bn_apply one rounding", O.check_one_rounding(z, z64, z64.abs(), "bn_apply"))
    if mask is not None:
        bits = ((z64 > 0).reshape(-1, 8).to(torch.int64) << torch.arange(8, device=odev)).sum(1)
        O.check_exact(mask, bits, "bn_apply mask bytes")

    g, g_abs = dz64 * dact, dz64.abs() * O.act_bwd_mag(z64, act)
    sums = O.bn_bwd_sums(g, y64, mean64, invstd64, g_abs)
    dbeta64, dgamma64 = _f32_of(sums["dbeta"]), _f32_of(sums["dgamma"])
    inv = float(torch.tensor(1.0 / M, dtype=torch.float32))
    want = O.bn_dy(g, y64, sc64, mean64, invstd64, dbeta64, dgamma64, inv, g_abs)
    mean, invstd, dbeta, dgamma = _f32(mean64), _f32(invstd64), _f32(dbeta64), _f32(dgamma64)
    dy = _nan((M, C))
    Kn.bn_bwd_apply(dz.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                    invstd.data_ptr(), dbeta.data_ptr(), dgamma.data_ptr(), dy.data_ptr(), M * C, C, inv, act, st)
    _rec(tag, kn, "bn_bwd_apply one rounding", O.check_one_rounding(dy, want["dy"], want["mag"], "bn_bwd_apply"))


@pytest.mark.parametrize("act", [NONE, RELU, TANH, SIGMOID], ids=lambda a: O.ACT_NAMES[a])
@pytest.mark.parametrize("C", [64, 24, 4, 5, 300])
def test_bn_apply_kernels(C, act):
    # C = 64: VW 8 fixed chunk (+ mask); 24: VW 8 per element (mask refused); 4: VW 1 fixed;
    # 5, 300: VW 1 per element.  257 rows: a tail past the last full workgroup
    _bn_apply_case(257, C, act)


def test_bn_apply_kernels_second_round():
    """16.8M elements at C = 64: 2,099,200 chunks > 8192 * 256, the second grid-stride round of
    bn_apply<8> / bn_bwd_apply<8>."""
    M = 262400
    assert 8192 * 256 < M * 64 // 8
    _bn_apply_case(M, 64, RELU, odev=_dev())
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# colstats / native_colsum
# ---------------------------------------------------------------------------
def _colstats_n(M, C, nb):
    vw = 8 if C % 8 == 0 else 1
    cpr = C // vw
    rpp = 256 // cpr                             # rows per pass = threads that share a channel chunk
    rpb = -(-M // nb)
    return -(-rpb // rpp) + rpp + nb             # a thread's rows + the LDS column + the slab rows


@pytest.mark.parametrize("M", [1, 255, 1000])
@pytest.mark.parametrize("C", [64, 24, 5, 2048])
def test_colstats_mode0_exact(M, C):
    # C = 64, 24, 2048: colstats<8, 0>; C = 5: colstats_sr (M = 1000, whole super rows) or
    # colstats<1, 0> (M = 1, 255)
    Kn = _native.kernels()
    tag = f"colstats0-M{M}-C{C}"
    x64 = O.grid((M, C), 1 / 8, 4.0, _gen(tag))
    x = _bf(x64)
    nb = Kn.colstats_blocks(M, C, 0, 0)
    part = _nan((nb, 2, C), torch.float32)
    Kn.colstats(x.data_ptr(), 0, 0, 0, 0, 0, part.data_ptr(), M, C, 0, 0, nb, _native.stream(x))
    # exact partial sums: even a whole column's sum |terms| / step stays below 2^24
    one_row = torch.zeros(M, dtype=torch.int64)
    O.slab_rows_exact(x64.abs(), one_row, 1, 1 / 8)
    O.slab_rows_exact(x64 * x64, one_row, 1, 1 / 64)
    want = torch.stack([x64.sum(0), (x64 * x64).sum(0)])
    _rec(tag, "colstats mode 0", "slabs exact", O.check_exact(part.double().sum(0), want, "colstats mode 0"))


@pytest.mark.parametrize("act", [NONE, RELU, TANH, SIGMOID], ids=lambda a: O.ACT_NAMES[a])
@pytest.mark.parametrize("M", [1, 255, 1000])
@pytest.mark.parametrize("C", [64, 24, 5, 2048])
def test_colstats_mode1(M, C, act):
    # colstats<8, 1, act> (C = 64, 24, 2048) / colstats<1, 1, act> (C = 5)
    Kn = _native.kernels()
    tag = f"colstats1-M{M}-C{C}-{O.ACT_NAMES[act]}"
    gen = _gen(tag)
    y64, dz64 = O.grid((M, C), 1 / 8, 4.0, gen), O.grid((M, C), 1 / 8, 4.0, gen)
    sc64, sh64 = _params(C, gen, act)
    mean64 = O.grid((C,), 1 / 8, 1.0, gen)
    invstd64 = _invstd_grid(C, gen)
    y, dz = _bf(y64), _bf(dz64)
    scale, shift, mean, invstd = _f32(sc64), _f32(sh64), _f32(mean64), _f32(invstd64)
    nb = Kn.colstats_blocks(M, C, 1, act)
    part = _nan((nb, 2, C), torch.float32)
    Kn.colstats(y.data_ptr(), dz.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                part.data_ptr(), M, C, act, 1, nb, _native.stream(y))
    z64, dact = O.prologue(y64, sc64, sh64, act)
    sums = O.bn_bwd_sums(dz64 * dact, y64, mean64, invstd64, dz64.abs() * O.act_bwd_mag(z64, act))
    n = _colstats_n(M, C, nb)
    frac = O.check_reduction(part.double().sum(0), torch.stack([sums["dbeta"], sums["dgamma"]]),
                             torch.stack([sums["dbeta_abs"], sums["dgamma_abs"]]), n, "colstats mode 1")
    _rec(tag, "colstats mode 1", f"reduction n={n}", frac)


def test_colstats_refuses_2056_channels():
    # C / 8 = 257 chunks > 256 threads and C > 256 for the scalar kernel: -2
    Kn = _native.kernels()
    x = torch.zeros(4, 2056, dtype=torch.bfloat16, device=_dev())
    part = torch.zeros(1, 2, 2056, dtype=torch.float32, device=_dev())
    with pytest.raises(RuntimeError):
        Kn.colstats(x.data_ptr(), 0, 0, 0, 0, 0, part.data_ptr(), 4, 2056, 0, 0, 1, _native.stream(x))


@pytest.mark.parametrize("M", [1000, 1001])
def test_native_colsum_c25(M):
    # M = 1000: colstats_sr (super rows of 8 rows = 25 chunks); M = 1001: its scalar fallback
    # colstats<1, 0>.  Sums of multiples of 1/8 below 2^24 / 8: exact in fp32 and in the fp64 finalize
    from featurenet_amd.ops.conv import native_colsum

    x64 = O.grid((M, 25), 1 / 8, 4.0, _gen(f"colsum{M}"))
    got = native_colsum(_bf(x64))
    O.slab_rows_exact(x64.abs(), torch.zeros(M, dtype=torch.int64), 1, 1 / 8)
    _rec(f"native_colsum-M{M}-C25", "colstats_sr" if M % 8 == 0 else "colstats<1,0>", "exact",
         O.check_exact(got, x64.sum(0), "native_colsum"))


# ---------------------------------------------------------------------------
# bn_finalize
# ---------------------------------------------------------------------------
def _finalize(part, count, gamma, beta, rm, rv, momentum, eps, mode):
    Kn = _native.kernels()
    nb, _, C = part.shape
    out = _nan((4, C), torch.float32)
    Kn.bn_finalize(part.data_ptr(), nb, C, float(count), _native.ptr(gamma), _native.ptr(beta), _native.ptr(rm),
                   _native.ptr(rv), float(momentum), float(eps), out[0].data_ptr(), out[1].data_ptr(),
                   out[2].data_ptr(), out[3].data_ptr(), mode, _native.stream(part))
    return out


def _finalize_data(nb, rows, C, gen):
    """x [nb, rows, C] float64: channel 1 constant (var 0), channel 2 mean 8 with values
    8 +- k/8 (exact slabs), the rest randn * 2 + 0.5."""
    x = torch.randn(nb, rows, C, generator=gen, dtype=torch.float64) * 2 + 0.5
    x[..., 1] = 3.0
    x[..., 2] = 8.0 + O.grid((nb, rows), 1 / 8, 1.0, gen)
    return x


@pytest.mark.parametrize("affine,running", [(True, True), (False, False)])
def test_bn_finalize_mode0(affine, running):
    nb, rows, C = 700, 16, 6                     # nb > 256: the strided slab loop takes three trips
    gen = _gen(f"fin0{affine}{running}")
    x = _finalize_data(nb, rows, C, gen)
    part = torch.stack([x.sum(1), (x * x).sum(1)], 1).to(torch.float32).to(_dev()).contiguous()
    count, mom = nb * rows, 0.1
    eps = float(torch.tensor(1e-5, dtype=torch.float32))   # the kernel takes eps as a float
    gamma64 = _f32_of(torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
    gamma64[0], gamma64[3] = -gamma64[0], 0.0
    beta64 = _f32_of(torch.randn(C, generator=gen, dtype=torch.float64) * 0.1)
    rm64 = _f32_of(torch.randn(C, generator=gen, dtype=torch.float64))
    rv64 = _f32_of(torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
    gamma, beta = (_f32(gamma64), _f32(beta64)) if affine else (None, None)
    rm, rv = (_f32(rm64), _f32(rv64)) if running else (None, None)
    out = _finalize(part, count, gamma, beta, rm, rv, mom, eps, 0).cpu()
    # the oracle: the same slabs in float64 (exact for channels 1 and 2, where it is also checked
    # against the two-pass statistics of x itself)
    p64 = part.double().cpu()
    A, B = p64[:, 0].sum(0), p64[:, 1].sum(0)
    mean, var = A / count, (B / count - (A / count) ** 2).clamp_min(0.0)
    two = O.bn_stats(x.reshape(-1, C))
    for c in (1, 2):
        assert abs(float(mean[c] - two["mean"][c])) <= 1e-13 * 8 and abs(float(var[c] - two["var"][c])) <= 1e-11
        mean[c], var[c] = two["mean"][c], two["var"][c]
    assert float(var[1]) == 0.0
    prm = O.bn_params(mean, var, gamma64 if affine else None, beta64 if affine else None, eps)
    # float64 cancellation of E[x^2] - mean^2, carried into invstd = (var + eps)^-1/2
    cancel = prm["invstd"] * 0.5 * 2.0 ** -50 * (B / count) / (var + eps)
    tag = f"bn_finalize0-affine{int(affine)}-running{int(running)}"
    _rec(tag, "bn_finalize<0>", "mean 1 ulp", O.check_fp32(out[0], prm["mean"], 1, "mean"))
    _rec(tag, "bn_finalize<0>", "invstd 1 ulp", O.check_fp32(out[1], prm["invstd"], 1, "invstd", extra=cancel))
    assert float(out[1][1]) == float(torch.tensor(1.0 / math.sqrt(eps), dtype=torch.float64).to(torch.float32))
    g = gamma64 if affine else torch.ones(C, dtype=torch.float64)
    _rec(tag, "bn_finalize<0>", "scale 2 ulp", O.check_fp32(out[2], prm["scale"], 2, "scale", extra=g.abs() * cancel))
    # shift = beta - float(mean) * gamma * invstd in fp32: three roundings of its terms
    _rec(tag, "bn_finalize<0>", "shift 4 ulp", O.check_fp32(out[3], prm["shift"], 4, "shift", mag=prm["shift_mag"],
                                                           extra=(mean * g).abs() * cancel))
    if running:
        _rec(tag, "bn_finalize<0>", "running mean 3 ulp",
             O.check_fp32(rm.cpu(), O.bn_running(rm64, mean, mom), 3, "running mean", mag=rm64.abs() + mean.abs()))
        unb = var * count / (count - 1)
        _rec(tag, "bn_finalize<0>", "running var 3 ulp",
             O.check_fp32(rv.cpu(), O.bn_running(rv64, unb, mom), 3, "running var", mag=rv64.abs() + unb.abs(),
                          extra=mom * 2.0 ** -50 * (B / count)))


def test_bn_finalize_count_one():
    """One value per channel: mean = x, var 0, invstd = 1 / sqrt(eps), and the unbiased running
    variance is the biased one (no division by count - 1 = 0)."""
    C, mom = 5, 0.25
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    x = O.grid((1, C), 1 / 8, 4.0, _gen("count1"))
    part = torch.stack([x, x * x], 1).to(torch.float32).to(_dev()).contiguous()
    rm, rv = torch.zeros(C, device=_dev()), torch.ones(C, device=_dev())
    out = _finalize(part, 1, None, None, rm, rv, mom, eps, 0).cpu()
    O.check_exact(out[0], x[0], "mean")
    O.check_fp32(out[1], torch.full((C,), 1.0 / math.sqrt(eps), dtype=torch.float64), 1, "invstd")
    O.check_fp32(rm.cpu(), mom * x[0], 2, "running mean")
    O.check_fp32(rv.cpu(), torch.full((C,), 1.0 - mom, dtype=torch.float64), 2, "running var")


def test_bn_finalize_modes_1_2():
    """Mode 1: the slab sums.  Mode 2: raw moments (sum g, sum g*y) centred in fp64,
    dgamma = invstd * (sum g*y - mean * sum g), on a channel whose mean (8) is far above its
    spread: the slabs are exact there, so the centring is judged against the two-pass sum."""
    nb, rows, C = 700, 16, 6
    gen = _gen("fin12")
    y = _finalize_data(nb, rows, C, gen)
    y[..., 0] = O.grid((nb, rows), 1 / 8, 4.0, gen)
    g = O.grid((nb, rows, C), 1 / 8, 4.0, gen)
    part = torch.stack([g.sum(1), (g * y).sum(1)], 1).to(torch.float32).to(_dev()).contiguous()
    p64 = part.double().cpu()
    A, B = p64[:, 0].sum(0), p64[:, 1].sum(0)
    Aabs, Babs = p64[:, 0].abs().sum(0), p64[:, 1].abs().sum(0)
    out = _finalize(part, nb * rows, None, None, None, None, 0.0, 0.0, 1).cpu()
    _rec("bn_finalize1", "bn_finalize<1>", "sums 1 ulp", O.check_fp32(out[0], A, 1, "sum 0", extra=2.0 ** -50 * Aabs))
    O.check_fp32(out[1], B, 1, "sum 1", extra=2.0 ** -50 * Babs)
    st = O.bn_stats(y.reshape(-1, C))
    mean64, invstd64 = _f32_of(st["mean"]), _f32_of(1.0 / torch.sqrt(st["var"] + 1e-5))
    mean, invstd = _f32(mean64), _f32(invstd64)
    out = _finalize(part, nb * rows, None, None, mean, invstd, 0.0, 0.0, 2).cpu()
    want = invstd64 * (B - mean64 * A)
    extra = invstd64 * 2.0 ** -50 * (Babs + mean64.abs() * Aabs)
    O.check_fp32(out[0], A, 1, "mode 2 dbeta", extra=2.0 ** -50 * Aabs)
    _rec("bn_finalize2", "bn_finalize<2>", "dgamma 1 ulp", O.check_fp32(out[1], want, 1, "mode 2 dgamma", extra=extra))
    # channels 0 and 2 (grid values: exact slabs): against sum g * (y - mean) * invstd itself
    for c in (0, 2):
        two = (g[..., c] * (y[..., c] - mean64[c])).sum() * invstd64[c]
        O.check_fp32(out[1][c], two, 1, f"mode 2 centring, channel {c}", extra=extra[c])
    with pytest.raises(RuntimeError):            # mode 2 without mean / invstd: -2
        _finalize(part, nb * rows, None, None, None, None, 0.0, 0.0, 2)


# ---------------------------------------------------------------------------
# module level: ops.* with real bn_finalize parameters
# ---------------------------------------------------------------------------
def _count(monkeypatch, names):
    Kn = _native.kernels()
    calls = {n: 0 for n in names}
    for n in names:
        orig = getattr(Kn, n)

        def counted(*a, _o=orig, _n=n, **k):
            calls[_n] += 1
            return _o(*a, **k)

        monkeypatch.setattr(Kn, n, counted)
    return calls


def _covered(flag_win, s):
    """Input elements that lie in a flagged window."""
    K = s.KD * s.KH * s.KW
    return O._fold(flag_win.unsqueeze(-1).expand(*flag_win.shape, K).to(torch.float64) * O.valid_mask(s), s) > 0


def _module_oracle(y64, dout64, gamma64, beta64, rm64, rv64, s, kind, count_pad, act, training, eps, und_as=None,
                   native=None):
    """The whole block in float64.  ``native``: None = the oracle's own BN parameters (to judge the
    native ones); else the native (mean, invstd, scale, shift, dbeta, dgamma) as float64, already
    judged, so that what follows them -- z, the pool, the sums, dy -- is compared at the same
    parameters.  ``und_as``: None, or 1.0 / 0.0 = the undecided relu elements forced active /
    inactive (returns the same dict)."""
    C = y64.shape[-1]
    y2 = y64.reshape(-1, C)
    M = y2.shape[0]
    stt = O.bn_stats(y2) if training else None
    if native is not None:
        prm = {"mean": native[0], "invstd": native[1], "scale": native[2], "shift": native[3],
               "shift_mag": native[3].abs()}
    elif training:
        prm = O.bn_params(stt["mean"], stt["var"], gamma64, beta64, eps)
    else:
        prm = O.bn_params(rm64, rv64, gamma64, beta64, eps)
    u = y64 * prm["scale"] + prm["shift"]
    und = torch.zeros_like(u, dtype=torch.bool)
    if act == RELU:
        und = u.abs() < 1e-4 * ((y64 * prm["scale"]).abs() + prm["shift"].abs())
        if und_as is not None:
            u = torch.where(und, torch.full_like(u, 1e-30 if und_as else 0.0), u)
    z = O.act_fwd(u, act)
    dact = O.act_bwd_from_out(z, act)
    zmag = (y64 * prm["scale"]).abs() + prm["shift_mag"]
    if s is not None:
        f = O.pool_fwd(z, s, kind, count_pad)
        b = O.pool_bwd(dout64, s, f["sel"])
        # BN's backward reads the pool's input gradient as a stored bf16 tensor dz (the fused apply
        # never stores it, but there dz is dout itself, a bf16 value): the oracle rounds it too.
        # The kernel rounds an fp32 sum of <= 4 terms -- exact for max pooling (bf16 terms), a few
        # fp32 roundings off for average pooling (dout * (1 / count)) -- so the rounding is decided
        # unless the exact value lies within that error of a rounding boundary: ``near``
        out, dz = f["out"], O.bf16_round(b["dx"])
        dz_ulp = O.bf16_ulp(b["dx"])
        fr = b["dx"].abs() / dz_ulp
        dist = (fr - torch.floor(fr) - 0.5).abs() * dz_ulp
        tol = (8 if kind == "avg" else 4) * 2.0 ** -24 * b["mag"]
        # (terms that cancel to |dz| below ~2^8 tol: the bf16 step there is finer than the fp32
        # error itself, nothing is left to decide -- the two sides differ by that error, ``small``)
        small = (0.5 * dz_ulp <= tol) & (b["mag"] > 0)
        # (dist = 0, an exact tie, takes a value of 9 significant bits: a sum of bf16 terms, each times
        # 1 or a power of two (windows of 4 positions at the border) -- products and sums the kernel
        # makes exactly, so both sides round it to even; dout / 6 or / 9 never lands there)
        near = (dist <= tol) & (dist > 0) & (b["mag"] > 0) & ~small
        # what the two sides' stored dz can differ by
        dz_slack = torch.where(small | near, dz_ulp + 2 * tol, torch.zeros_like(tol))
        out_mag = (f["sel"] * O.windows(zmag, s, 0.0)).sum(-1)
        und_win = O.windows(und.to(torch.float64), s, 0.0).sum(-1) > 0
        und_el = _covered(und_win, s) | und
    else:
        out, out_mag, dz = z, zmag, dout64
        und_win = und_el = und
        near, dz_slack = torch.zeros_like(und), torch.zeros_like(u)
    g, g_abs = dz * dact, dz.abs() * O.act_bwd_mag(z, act)
    sums = O.bn_bwd_sums(g.reshape(-1, C), y2, prm["mean"], prm["invstd"], g_abs.reshape(-1, C))
    if training:
        db, dg = (sums["dbeta"], sums["dgamma"]) if native is None else (native[4], native[5])
        dy = O.bn_dy(g, y64, prm["scale"], prm["mean"], prm["invstd"], db, dg, 1.0 / M, g_abs)
    else:
        zero = torch.zeros(C, dtype=torch.float64)
        dy = O.bn_dy(g, y64, prm["scale"], prm["mean"], prm["invstd"], zero, zero, 0.0, g_abs)
    return {"out": out, "out_mag": out_mag, "dy": dy, "sums": sums, "prm": prm, "stats": stt, "und": und,
            "und_win": und_win, "und_el": und_el, "M": M, "near": near, "dz_slack": dz_slack, "dact": dact}


def _module_case(monkeypatch, tag, shape, pool, kind, act, training, env=("1", "1"), want_calls=None,
                 shifted=False, input_only=False, count_pad=False, dout_step=None):
    """ops.batchnorm_act(_pool) forward + backward against the oracle.  ``pool``: None or
    (kernel, stride, padding).  ``want_calls``: expected (pool_bn_bwd_apply, pool_bwd_stats,
    pool_bwd) launch counts.  ``dout_step``: the output gradient as multiples of it (|k| <= 4), not
    randn.

    Two stages.  The native BN parameters (mean, invstd, scale, shift; running statistics) are
    judged against the oracle's: fp32 ulps plus the reduction bound of the colstats sums they
    come from.  Everything after them -- the forward output, dbeta, dgamma, dy -- is judged
    against the oracle evaluated at those native parameters (and, for dy, at the native dbeta /
    dgamma, judged just before), so each check carries its own bound only."""
    monkeypatch.setenv("FN_POOL_BN_STATS", env[0])
    monkeypatch.setenv("FN_POOL_BN_APPLY", env[1])
    calls = _count(monkeypatch, ("pool_bn_bwd_apply", "pool_bwd_stats", "pool_bwd"))
    C, eps, mom = shape[-1], 1e-5, 0.1
    gen = _gen(tag)
    y64 = (torch.randn(shape, generator=gen) * (0.125 if shifted else 2.0) + (8.0 if shifted else 0.5)
           ).to(torch.bfloat16).double()
    gamma64 = _f32_of(torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
    gamma64[1], gamma64[2] = -gamma64[1], 0.0
    beta64 = _f32_of(torch.randn(C, generator=gen, dtype=torch.float64) * 0.1)
    rm64 = _f32_of(torch.randn(C, generator=gen, dtype=torch.float64) * 0.1 + (8.0 if shifted else 0.5))
    rv64 = _f32_of(torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
    s = PoolSpec.make(shape, pool[0], pool[1], pool[2]) if pool else None
    oshape = s.out_shape5 if s else shape
    dout64 = torch.randn(oshape, generator=gen).to(torch.bfloat16).double()
    if dout_step is not None:
        dout64 = torch.randint(-4, 5, oshape, generator=gen).double() * dout_step

    y = _bf(y64).requires_grad_(True)
    gamma = _f32(gamma64).requires_grad_(not input_only)
    beta = _f32(beta64).requires_grad_(not input_only)
    rm, rv = _f32(rm64), _f32(rv64)
    name = O.ACT_NAMES[act] if act else None
    if s is not None:
        out = ops.batchnorm_act_pool(y, gamma, beta, rm, rv, training, s, kind, mom, eps, name, count_pad=count_pad)
    else:
        out = ops.batchnorm_act(y, gamma, beta, rm, rv, training, mom, eps, name)
    nat = out.grad_fn.saved_tensors[1].detach().cpu().double()   # (mean, invstd, scale, shift) [4, C]
    assert nat.shape == (4, C)
    out.backward(_bf(dout64))
    if want_calls is not None:
        assert (calls["pool_bn_bwd_apply"], calls["pool_bwd_stats"], calls["pool_bwd"]) == want_calls, calls
    kn = "ops.batchnorm_act" + ("_pool" if s else "")
    Kn = _native.kernels()

    # --- stage 1: the BN parameters
    args = (y64, dout64, gamma64, beta64, rm64, rv64, s, kind, count_pad, act, training, eps)
    own = _module_oracle(*args)
    M, prm = own["M"], own["prm"]
    ga = gamma64.abs()
    if training:
        # colstats mode 0 slabs (sum x, sum x^2), chain n0, finalised in fp64: mean = A / M,
        # var = B / M - mean^2, invstd = (var + eps)^-1/2
        st = own["stats"]
        y2 = y64.reshape(-1, C)
        n0 = _colstats_n(M, C, Kn.colstats_blocks(M, C, 0, 0))
        e_mean = (n0 + 8) * 2.0 ** -24 * y2.abs().sum(0) / M
        e_var = (n0 + 8) * 2.0 ** -24 * ((y2 * y2).sum(0) / M + 2 * st["mean"].abs() * y2.abs().sum(0) / M)
        e_is = prm["invstd"] * 0.5 * prm["invstd"] ** 2 * e_var
        ulps = (1, 1, 2, 4)
        _rec(tag, kn, "running mean (reduction)",
             O.check_fp32(rm.cpu(), O.bn_running(rm64, st["mean"], mom), 3, "running mean",
                          mag=rm64.abs() + st["mean"].abs(), extra=mom * e_mean))
        _rec(tag, kn, "running var (reduction)",
             O.check_fp32(rv.cpu(), O.bn_running(rv64, st["unbiased"], mom), 3, "running var",
                          mag=rv64.abs() + st["unbiased"], extra=mom * e_var * M / (M - 1)))
    else:
        # eval: torch fp32 on the running statistics (rsqrt, two products, a difference)
        e_mean = e_is = torch.zeros(C, dtype=torch.float64)
        ulps = (0, 3, 4, 6)
        O.check_exact(rm, rm64, "running mean in eval")
        O.check_exact(rv, rv64, "running var in eval")
    _rec(tag, kn, "native mean (reduction)", O.check_fp32(nat[0], prm["mean"], ulps[0], "mean", extra=e_mean))
    _rec(tag, kn, "native invstd (reduction)", O.check_fp32(nat[1], prm["invstd"], ulps[1], "invstd", extra=e_is))
    _rec(tag, kn, "native scale (reduction)", O.check_fp32(nat[2], prm["scale"], ulps[2], "scale", extra=ga * e_is))
    _rec(tag, kn, "native shift (reduction)",
         O.check_fp32(nat[3], prm["shift"], ulps[3], "shift", mag=prm["shift_mag"],
                      extra=ga * (prm["invstd"] * e_mean + prm["mean"].abs() * e_is)))

    # --- stage 2: at the native parameters
    db = dg = torch.zeros(C, dtype=torch.float64)
    if not input_only:
        db, dg = beta.grad.cpu().double(), gamma.grad.cpu().double()
    native = (nat[0], nat[1], nat[2], nat[3], db, dg)
    r = _module_oracle(*args, native=native)
    r_on, r_off = ((_module_oracle(*args, und_as=1.0, native=native), _module_oracle(*args, und_as=0.0, native=native))
                   if act == RELU else (r, r))
    # the cap: at most 1e-3 of the elements and 1e-2 of the windows may be left out as undecided
    share_el = float(r["und"].double().mean())
    share_win = float(r["und_win"].double().mean())
    assert share_el <= 1e-3, f"undecided elements: {share_el:.2e}"
    assert share_win <= (1e-2 if s is not None else 1e-3), f"undecided windows: {share_win:.2e}"
    _rec(tag, "undecided share", f"elements {share_el:.2e} windows {share_win:.2e}", 0.0)
    # stored dz elements whose bf16 rounding the kernel's fp32 roundings decide (``near``): handled
    # like the undecided relu elements -- a cap, left out elementwise, and the sums widened by
    # what their two roundings differ by (one bf16 ulp of dz and the fp32 error, times |act'| and
    # |act' * xhat|)
    near = r["near"]
    share_near = float(near.double().mean())
    assert share_near <= 1e-3, f"dz elements next to a bf16 rounding boundary: {share_near:.2e}"
    _rec(tag, "undecided dz rounding", f"elements {share_near:.2e}", 0.0)
    _rec(tag, kn, "forward one rounding",
         O.check_one_rounding(out.detach().cpu(), r["out"], r["out_mag"], "forward", keep=~r["und_win"]))
    if not input_only:
        sums = r["sums"]
        xhat = (y64 - nat[0]) * nat[1]
        near_g = r["dz_slack"] * r["dact"].abs()
        x_b = near_g.reshape(-1, C).sum(0) + (r_on["sums"]["dbeta"] - r_off["sums"]["dbeta"]).abs()
        x_g = (near_g * xhat.abs()).reshape(-1, C).sum(0) + (r_on["sums"]["dgamma"] - r_off["sums"]["dgamma"]).abs()
        if calls["pool_bwd_stats"] > 0:
            # raw moments (sum g, sum g*y) from pool_bn_moments8 / pool_bwd_tiled<8, true>: a thread's
            # windows + the 256 / cpr threads of a channel chunk + the slab rows; centred in fp64 by
            # bn_finalize mode 2, dgamma = invstd * (sum g*y - mean * sum g)
            nb = Kn.pool_bwd_stats_blocks(s.geom17())
            cpr = C // 8
            n = -(-(M // (s.KD * s.KH * s.KW)) * cpr // (nb * 256)) + 256 // cpr + nb
            abs_b = sums["sg_abs"]
            abs_g = nat[1] * (sums["sgy_abs"] + nat[0].abs() * sums["sg_abs"])
        else:
            n = _colstats_n(M, C, Kn.colstats_blocks(M, C, 1, act))   # colstats mode 1
            abs_b, abs_g = sums["dbeta_abs"], sums["dgamma_abs"]
        _rec(tag, kn, f"dbeta reduction n={n}", O.check_reduction(db, sums["dbeta"], abs_b, n, "dbeta", extra=x_b))
        _rec(tag, kn, f"dgamma reduction n={n}", O.check_reduction(dg, sums["dgamma"], abs_g, n, "dgamma", extra=x_g))
    else:
        assert gamma.grad is None and beta.grad is None
    # --- input gradient: one rounding
    dy = r["dy"]
    _rec(tag, kn, "dy one rounding",
         O.check_one_rounding(y.grad.cpu(), dy["dy"], dy["mag"], "dy", keep=~r["und_el"] & ~near,
                              extra=(r_on["dy"]["dy"] - r_off["dy"]["dy"]).abs()
                              + nat[2].abs() * r["dz_slack"] * r["dact"].abs()))


_FUSED = {("1", "1"): (1, 1, 0), ("1", "0"): (0, 1, 0), ("0", "1"): (0, 0, 1)}


@pytest.mark.parametrize("env", list(_FUSED), ids=lambda e: f"stats{e[0]}-apply{e[1]}")
@pytest.mark.parametrize("shape", [(2, 8, 8, 8, 32), (3, 6, 6, 6, 8)], ids=["2x8^3x32", "3x6^3x8"])
def test_module_bn_relu_maxpool_training(monkeypatch, shape, env):
    # 1/1: pool_bwd_stats (moments only) + pool_bn_bwd_apply; 1/0: pool_bwd_stats with dz +
    # bn_bwd_apply; 0/-: pool_bwd + colstats mode 1 + bn_bwd_apply
    _module_case(monkeypatch, f"mod-max-train-{shape}-{env}", shape, (2, None, "valid"), "max", RELU, True, env,
                 _FUSED[env])


@pytest.mark.parametrize("kind,act", [("max", RELU), ("avg", RELU), ("max", NONE)])
def test_module_overlapping_pool_training(monkeypatch, kind, act):
    # pool_bwd (gather) + colstats mode 1 + bn_bwd_apply; an input collects from up to four windows
    # (average: dout / 4, / 6 or / 9 at the border and inside) and the sum is stored as bf16 dz.
    # Average pooling with randn dout: sums such as (a + b) / 6 with a + b a multiple of 3 are exact
    # bf16 ties which the kernel's a * (1/6) + b * (1/6) in fp32 breaks either way; they and their
    # near misses were 0.31 % of this case's elements (0.04 - 0.42 % over five other seeds), above
    # the 1e-3 cap on undecided elements.  dout in multiples of 4.5 makes every term a multiple of 1/8 and every
    # sum (<= 18) a bf16 value, so the stored dz is decided; the rounding of such sums itself is
    # judged at kernel level (over3_s2_same_c16, avg).
    _module_case(monkeypatch, f"mod-over-{kind}-{act}", (2, 1, 9, 9, 16), ((1, 3, 3), (1, 2, 2), "same"), kind, act,
                 True, want_calls=(0, 0, 1), dout_step=4.5 if kind == "avg" else None)


def test_module_avgpool_c6_training(monkeypatch):
    _module_case(monkeypatch, "mod-avg-c6", (3, 6, 6, 6, 6), (2, None, "valid"), "avg", RELU, True,
                 want_calls=(0, 0, 1))


@pytest.mark.parametrize("kind", ["max", "avg"])
def test_module_pool_eval(monkeypatch, kind):
    _module_case(monkeypatch, f"mod-eval-{kind}", (2, 8, 8, 8, 32), (2, None, "valid"), kind, RELU, False,
                 want_calls=(0, 0, 1))


def test_module_pool_eval_input_gradient_only(monkeypatch):
    """Eval mode, frozen parameters, requires_grad only on the input (the robustness attacks):
    dy = scale * g, no statistics pass."""
    cs = _count(monkeypatch, ("colstats",))
    _module_case(monkeypatch, "mod-eval-input-only", (3, 6, 6, 6, 8), (2, None, "valid"), "max", RELU, False,
                 want_calls=(0, 0, 1), input_only=True)
    assert cs["colstats"] == 0


@pytest.mark.parametrize("env", [("1", "1"), ("0", "1")], ids=["raw-moments", "colstats"])
def test_module_shifted_mean_training(monkeypatch, env):
    """randn * 0.125 + 8: the mean is 64 standard deviations out, the fp32 raw moments
    (sum g, sum g*y) cancel in bn_finalize mode 2.  Without an activation: bf16 has 1/16 steps at 8,
    so a channel whose mean falls next to a step has that whole step's elements at z ~ 0 -- under
    relu the undecided rule (relative to |y * scale| + |shift| ~ 128 gamma here) leaves out 0.4 - 2.7 %
    of the elements, above its cap.  The centring under test does not depend on the activation."""
    _module_case(monkeypatch, f"mod-shifted-{env}", (2, 8, 8, 8, 32), (2, None, "valid"), "max", NONE, True, env,
                 _FUSED[env], shifted=True)


@pytest.mark.parametrize("act", [RELU, NONE, TANH])
@pytest.mark.parametrize("training", [True, False])
def test_module_batchnorm_act(monkeypatch, training, act):
    _module_case(monkeypatch, f"mod-bn-{training}-{act}", (3, 5, 6, 7, 8), None, None, act, training,
                 want_calls=(0, 0, 0))


@pytest.mark.parametrize("case,kind", [(c, k) for c in O.POOL_CASES for k in c["kinds"]
                                       if c["name"] in ("cube2_c64", "odd2_c16", "over3_s2_same_c16", "over2_s1_c3",
                                                        "avg2_same_c6")],
                         ids=lambda v: v["name"] if isinstance(v, dict) else v)
def test_module_pool(case, kind):
    """ops.pool on randn inputs.  Max pooling: the forward is exact, the backward exact where the
    windows do not overlap (dx is dout or 0) and one rounding of a sum of bf16 values where they
    do.  Average pooling: one rounding."""
    s = O.make_spec(case)
    tag = f"ops.pool-{case['name']}-{kind}"
    gen = _gen(tag)
    x64 = (torch.randn((s.N, s.D, s.H, s.W, s.C), generator=gen) * 2 + 0.5).to(torch.bfloat16).double()
    dout64 = torch.randn(s.out_shape5, generator=gen).to(torch.bfloat16).double()
    x = _bf(x64).requires_grad_(True)
    out = ops.pool(x, s, kind)
    out.backward(_bf(dout64))
    f = O.pool_fwd(x64, s, kind)
    b = O.pool_bwd(dout64, s, f["sel"])
    kn = case["kernels"]
    if kind == "max":
        _rec(tag, kn, "fwd exact", O.check_exact(out.detach(), f["out"], "ops.pool max"))
        if (s.sd, s.sh, s.sw) == (s.KD, s.KH, s.KW):
            _rec(tag, kn, "bwd exact", O.check_exact(x.grad, b["dx"], "ops.pool max backward"))
        else:
            _rec(tag, kn, "bwd one rounding",
                 O.check_one_rounding(x.grad, b["dx"], b["mag"], "ops.pool max backward"))
    else:
        _rec(tag, kn, "fwd one rounding", O.check_one_rounding(out.detach(), f["out"], f["mag"], "ops.pool avg"))
        _rec(tag, kn, "bwd one rounding", O.check_one_rounding(x.grad, b["dx"], b["mag"], "ops.pool avg backward"))


@pytest.mark.parametrize("C", [40, 5])
def test_module_global_avg_pool(C):
    gen = _gen(f"gap{C}")
    x64 = (torch.randn((3, 4, 5, 6, C), generator=gen) * 2 + 0.5).to(torch.bfloat16).double()
    dout64 = torch.randn((3, C), generator=gen).to(torch.bfloat16).double()
    x = _bf(x64).requires_grad_(True)
    out = ops.global_avg_pool(x)
    out.backward(_bf(dout64))
    s = PoolSpec.make(x64.shape, (4, 5, 6), (4, 5, 6), "valid")
    f = O.pool_fwd(x64, s, "avg")
    b = O.pool_bwd(dout64.reshape(s.out_shape5), s, f["sel"])
    kn = "pool_fwd<8>, pool_bwd_tiled<8>" if C % 8 == 0 else "pool_fwd<1>, pool_bwd_tiled<1>"
    _rec(f"ops.global_avg_pool-C{C}", kn, "fwd one rounding",
         O.check_one_rounding(out.detach(), f["out"].reshape(3, C), f["mag"].reshape(3, C), "global_avg_pool"))
    _rec(f"ops.global_avg_pool-C{C}", kn, "bwd one rounding",
         O.check_one_rounding(x.grad, b["dx"], b["mag"], "global_avg_pool backward"))
