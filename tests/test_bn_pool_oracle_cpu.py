"""The fp64 oracle of the BN / pooling kernels (tests/_bn_pool_oracle.py) judged itself: against
torch autograd through the library ops, in float64, on every geometry the GPU file uses -- and
the comparison helpers of the GPU file must reject an oracle output that is wrong in each of
the ways a kernel is likely to be wrong."""
import pytest
import torch
import torch.nn.functional as F

import _bn_pool_oracle as O
from featurenet_amd.ops.spec import PoolSpec


def _rel(a, r, mag, what):
    """1e-12 relative, elementwise (relative to the terms the value was added up from)."""
    err = (a - r).abs()
    bound = 1e-12 * torch.maximum(r.abs(), mag)
    assert bool((err <= bound).all()), f"{what}: max err {float(err.max()):.3e}"


def _torch_pool(x5, s, kind, count_pad):
    """ops/reference.py's pooling (-inf / zero padded input through the library op), float64."""
    xin = x5.permute(0, 4, 1, 2, 3)
    k, st = (s.KD, s.KH, s.KW), (s.sd, s.sh, s.sw)
    hd, hh, hw = O._hi_pads(s)
    pads = (s.pw, hw, s.ph, hh, s.pd, hd)
    if kind == "max":
        y = F.max_pool3d(F.pad(xin, pads, value=float("-inf")) if any(pads) else xin, k, st)
    elif any(pads):
        num = F.avg_pool3d(F.pad(xin, pads), k, st, divisor_override=1)
        den = (torch.full_like(num[:, :1], float(s.KD * s.KH * s.KW)) if count_pad else
               F.avg_pool3d(F.pad(torch.ones_like(xin[:, :1]), pads), k, st, divisor_override=1))
        y = num / den
    else:
        y = F.avg_pool3d(xin, k, st)
    return y[:, :, : s.OD, : s.OH, : s.OW].permute(0, 2, 3, 4, 1)


_POOL = [(c, kind, cp) for c in O.POOL_CASES + [O.LARGE_CASE] for kind in c["kinds"] for cp in c["count_pad"]]


@pytest.mark.parametrize("case,kind,count_pad", _POOL, ids=[f"{c['name']}-{k}-cp{int(p)}" for c, k, p in _POOL])
def test_pool_oracle_matches_autograd(case, kind, count_pad):
    # (the large case: its geometry with one sample instead of 33 -- the windows are the same)
    s = O.make_spec(case, N=1 if case is O.LARGE_CASE else None)
    gen = torch.Generator().manual_seed(11)
    shape = (s.N, s.D, s.H, s.W, s.C)
    x = O.grid(shape, 0.125, 4.0, gen)           # 65 values: tied windows are common
    dout = O.grid(s.out_shape5, 0.125, 4.0, gen)
    f = O.pool_fwd(x, s, kind, count_pad)
    b = O.pool_bwd(dout, s, f["sel"])
    xr = x.clone().requires_grad_(True)
    out = _torch_pool(xr, s, kind, count_pad)
    (dx,) = torch.autograd.grad(out, xr, dout)
    if kind == "max":
        win = f["win"]
        assert int(((win == f["out"].unsqueeze(-1)).sum(-1) > 1).sum()) > 0 or win.shape[-1] == 1, "no tied window"
    _rel(f["out"], out.detach(), f["mag"], "forward")
    _rel(b["dx"], dx, b["mag"], "backward")


def test_last_wins_differs_from_first_wins():
    s = PoolSpec.make((1, 2, 2, 2, 1), 2)
    x = torch.zeros(1, 2, 2, 2, 1, dtype=torch.float64)
    d = torch.ones(s.out_shape5, dtype=torch.float64)
    first = O.pool_bwd(d, s, O.pool_fwd(x, s, "max")["sel"])["dx"].flatten()
    last = O.pool_bwd(d, s, O.pool_fwd(x, s, "max", tie="last")["sel"])["dx"].flatten()
    assert first.tolist() == [1.0] + [0.0] * 7 and last.tolist() == [0.0] * 7 + [1.0]


@pytest.mark.parametrize("act", [O.ACT_NONE, O.ACT_RELU, O.ACT_TANH, O.ACT_SIGMOID])
@pytest.mark.parametrize("M,C", [(257, 5), (1, 3), (40, 8)])
def test_bn_oracle_matches_autograd(act, M, C):
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(M, C, generator=gen, dtype=torch.float64) * 2 + 0.5
    if M > 1:
        y[:, 1] = 3.0                            # a constant channel: var 0
    dz = torch.randn(M, C, generator=gen, dtype=torch.float64)
    gamma = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    gamma[0], gamma[2] = -gamma[0], 0.0
    beta = torch.randn(C, generator=gen, dtype=torch.float64) * 0.1
    rm, rv = torch.randn(C, generator=gen, dtype=torch.float64), torch.rand(C, generator=gen, dtype=torch.float64)
    eps, mom = 1e-5, 0.1

    st = O.bn_stats(y)
    prm = O.bn_params(st["mean"], st["var"], gamma, beta, eps)
    z, dact = O.prologue(y, prm["scale"], prm["shift"], act)
    g = dz * dact
    sums = O.bn_bwd_sums(g, y, prm["mean"], prm["invstd"])
    dy = O.bn_dy(g, y, prm["scale"], prm["mean"], prm["invstd"], sums["dbeta"], sums["dgamma"], 1.0 / M)

    if M == 1:                                   # (the library refuses one value per channel in training)
        assert torch.equal(st["var"], torch.zeros(C, dtype=torch.float64))
        assert torch.equal(st["unbiased"], st["var"])
        return
    yr, gr, br = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm2, rv2 = rm.clone(), rv.clone()
    u = F.batch_norm(yr, rm2, rv2, gr, br, True, mom, eps)
    zt = {O.ACT_NONE: lambda t: t, O.ACT_RELU: torch.relu, O.ACT_TANH: torch.tanh, O.ACT_SIGMOID: torch.sigmoid}[act](u)
    dyt, dgt, dbt = torch.autograd.grad(zt, (yr, gr, br), dz)
    one = torch.ones(())
    _rel(z, zt.detach(), (y * prm["scale"]).abs() + prm["shift_mag"], "z")
    _rel(O.bn_running(rm, st["mean"], mom), rm2, rm.abs() + st["mean"].abs(), "running mean")
    _rel(O.bn_running(rv, st["unbiased"], mom), rv2, one, "running var")
    _rel(sums["dbeta"], dbt, sums["dbeta_abs"], "dbeta")
    _rel(sums["dgamma"], dgt, sums["dgamma_abs"], "dgamma")
    # raw moments: dgamma = invstd * (sum g*y - mean * sum g)
    _rel(prm["invstd"] * (sums["sgy"] - prm["mean"] * sums["sg"]), dgt,
         prm["invstd"] * (sums["sgy_abs"] + prm["mean"].abs() * sums["sg_abs"]), "dgamma from raw moments")
    # (act' = 1 - z^2 or z (1 - z) is itself a difference of terms up to 1: |scale * dz| joins the magnitude)
    _rel(dy["dy"], dyt, dy["mag"] + (prm["scale"] * dz).abs(), "dy")
    assert torch.equal(dy["dy"], dy["t1"] + dy["t2"] + dy["t3"])
    # eval mode with frozen statistics: dy = scale * g
    pe = O.bn_params(rm, rv, gamma, beta, eps)
    ze, de = O.prologue(y, pe["scale"], pe["shift"], act)
    ye = y.clone().requires_grad_(True)
    ue = F.batch_norm(ye, rm.clone(), rv.clone(), gamma, beta, False, mom, eps)
    zte = {O.ACT_NONE: lambda t: t, O.ACT_RELU: torch.relu, O.ACT_TANH: torch.tanh, O.ACT_SIGMOID: torch.sigmoid}[act](ue)
    (dye,) = torch.autograd.grad(zte, ye, dz)
    zero = torch.zeros(C, dtype=torch.float64)
    got = O.bn_dy(dz * de, y, pe["scale"], pe["mean"], pe["invstd"], zero, zero, 0.0)
    _rel(got["dy"], dye, got["mag"] + (pe["scale"] * dz).abs(), "eval dy")


# ---------------------------------------------------------------------------
# the comparison helpers must have teeth
# ---------------------------------------------------------------------------
def _scenario(tie="first", move=False, bump_dout=False, drop_term=False, drop_tail=False):
    """BN + ReLU + 2x2x2 max pool backward on the dyadic grids of the GPU file: dx (what
    check_exact judges), dy of the fused apply (check_one_rounding) and the raw moments
    (check_reduction, and check_exact as the slab check)."""
    s = PoolSpec.make((2, 8, 8, 8, 8), 2)
    gen = torch.Generator().manual_seed(3)
    y = O.grid((2, 8, 8, 8, 8), 0.125, 4.0, gen)
    dout = O.grid(s.out_shape5, 0.125, 4.0, gen)
    dout = torch.where(dout == 0, torch.full_like(dout, 0.5), dout)
    scale = O.grid((8,), 0.0625, 2.0, gen)
    shift = O.grid((8,), 0.0625, 2.0, gen)
    scale[0], shift[0] = 0.0, 1.0                # z constant: every window tied, y differs
    scale[1], scale[2] = -1.25, 0.75
    C = 8
    z, _ = O.prologue(y, scale, shift, O.ACT_RELU)
    f = O.pool_fwd(z, s, "max", tie=tie)
    d2 = dout.reshape(-1, C).clone()
    nwin = d2.shape[0]
    # the window whose gradient the mutations touch: an active one (z max > 0) in channel 2
    act_w = (f["out"].reshape(-1, C)[:, 2] > 0).nonzero().flatten()
    w0 = int(act_w[len(act_w) // 2])
    if bump_dout:                                # one element off by 2 bf16 ulps
        d2[w0, 2] += 2 * O.bf16_ulp(d2[w0, 2])
    sel = f["sel"].reshape(nwin, C, -1).clone()
    if move:                                     # window w0's gradient lands in its neighbour
        d2[w0 + 1] += d2[w0]
        d2[w0] = 0.0
    if drop_term:                                # channel 2 loses window w0's term
        d2[w0, 2] = 0.0
    if drop_tail:
        d2[nwin - 1] = 0.0
    sel = sel.reshape(f["sel"].shape)
    b = O.pool_bwd(d2.reshape(dout.shape), s, sel)
    dz = b["dx"]                                 # gradient of z
    g = dz * O.act_bwd_from_out(z, O.ACT_RELU)
    mean, invstd = shift * 0 + 0.25, shift * 0 + 0.5
    sums = O.bn_bwd_sums(g.reshape(-1, C), y.reshape(-1, C), mean, invstd)
    M = y.numel() // C
    dy = O.bn_dy(g, y, scale, mean, invstd, sums["dbeta"], sums["dgamma"], 1.0 / M)
    return {"dx": b["dx"], "dy": dy["dy"], "dy_mag": dy["mag"],
            "mom": torch.stack([sums["sg"], sums["sgy"]]), "mom_abs": torch.stack([sums["sg_abs"], sums["sgy_abs"]])}


def test_slab_precondition_rejects_inexact_rows():
    terms = torch.full((4, 1), 2.0 ** 22, dtype=torch.float64)      # 2^22 steps of 1 each
    assert O.slab_rows_exact(terms, torch.arange(4), 4, 1.0) == 0.25  # one term per slab row
    with pytest.raises(AssertionError):                              # all four in one row: 2^24
        O.slab_rows_exact(terms, torch.zeros(4, dtype=torch.int64), 1, 1.0)


def _bump_output(t, mag=None):
    """One element of an elementwise result off by 2 bf16 ulps (the one largest against its
    magnitude)."""
    t = t.clone()
    score = t.abs() / (mag if mag is not None else torch.ones_like(t)).clamp_min(1e-30)
    i = int(score.flatten().argmax())
    t.view(-1)[i] += 2 * O.bf16_ulp(t.view(-1)[i])
    return t


def _drop_tail_rows(t):
    """The last row never written: it keeps the NaN the test filled the output with."""
    t = t.clone()
    t.reshape(-1, t.shape[-1])[-1] = float("nan")
    return t


def test_comparators_have_teeth():
    ref = _scenario()
    # what a correct kernel stores: one bf16 rounding of the oracle's value (fp32 for the sums)
    a_dx, a_dy = O.bf16_round(ref["dx"]), O.bf16_round(ref["dy"])
    a_mom = ref["mom"].to(torch.float32)
    n = 40
    checks = {
        "exact": lambda r: O.check_exact(a_dx, O.bf16_round(r["dx"]), "dx"),
        "one_rounding": lambda r: O.check_one_rounding(a_dy, r["dy"], r["dy_mag"], "dy"),
        "reduction": lambda r: O.check_reduction(a_mom, r["mom"], r["mom_abs"], n, "moments"),
        "exact_slab": lambda r: O.check_exact(a_mom, r["mom"], "moment slabs"),
        "fp32": lambda r: O.check_fp32(a_mom, r["mom"], 1, "finalised sums"),
    }
    for name, chk in checks.items():             # the unchanged oracle passes
        assert chk(ref) <= 1.0, name
    wrong = {
        "last-wins ties": _scenario(tie="last"),
        "gradient moved to the neighbour window": _scenario(move=True),
        "reduction off by one term": _scenario(drop_term=True),
    }
    # one element off by 2 bf16 ulps: of the result itself (elementwise), of one input term (sums)
    two_ulp_out = dict(ref, dx=_bump_output(ref["dx"]), dy=_bump_output(ref["dy"], ref["dy_mag"]))
    two_ulp_in = _scenario(bump_dout=True)
    tail_out = dict(ref, dx=_drop_tail_rows(ref["dx"]), dy=_drop_tail_rows(ref["dy"]))
    tail_in = _scenario(drop_tail=True)
    for name, chk in checks.items():
        elementwise = name in ("exact", "one_rounding")
        cases = dict(wrong)
        cases["one element off by 2 bf16 ulps"] = two_ulp_out if elementwise else two_ulp_in
        cases["tail row dropped"] = tail_out if elementwise else tail_in
        for change, r in cases.items():
            try:
                chk(r)
            except AssertionError:
                continue
            pytest.fail(f"{name} accepted: {change}", pytrace=False)
