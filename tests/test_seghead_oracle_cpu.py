"""The fp64 oracle of the fused head + loss kernels (tests/_seghead_oracle.py) judged itself:
against torch autograd through ``cross_entropy`` in float64, its input builders against what
they promise for every case the GPU file runs, and the judges of the GPU file against the
oracle's own outputs carrying each defect a kernel is likely to have."""
import zlib

import pytest
import torch
import torch.nn.functional as F

import _seghead_oracle as S

NB = 512                                         # the grid of a large launch on 256 CUs (2 per CU)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _rel(a, r, mag, what):
    err = (a - r).abs()
    bound = 1e-12 * torch.maximum(r.abs(), mag)
    assert bool((err <= bound).all()), f"{what}: max err {float(err.max()):.3e}"


def _fwd(inp, lab, xscale, smoothing):
    return S.forward(inp["y"], inp["sc"], inp["sh"], inp["act"], inp["w"], inp["bias"], lab, xscale, smoothing)


@pytest.mark.parametrize("smoothing", [0.0, 0.125])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("act", [S.ACT_NONE, S.ACT_RELU])
@pytest.mark.parametrize("NC", [2, 3, 16, 17, 24, 25, 31, 32])
def test_oracle_matches_autograd(NC, act, bias, smoothing):
    M, xscale = 264, 1.0 / 264
    gen = _gen(f"autograd-{NC}-{act}-{bias}-{smoothing}")
    inp = S.build_readout(M, NC, act, gen, bias)
    lab = S.make_labels(inp, gen)
    f = _fwd(inp, lab, xscale, smoothing)
    b = S.backward(f["z"], inp["w"], f["d"])
    m = S.moments(b["dz"], inp["y"], f["u"], act)

    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    sc, sh, w = leaf(inp["sc"]), leaf(inp["sh"]), leaf(inp["w"])
    bb = leaf(inp["bias"]) if bias else None
    u = inp["y"] * sc + sh
    z = F.relu(u) if act == S.ACT_RELU else u * 1.0
    l = F.linear(z, w, bb)
    z.retain_grad()
    l.retain_grad()
    rows = F.cross_entropy(l, lab, label_smoothing=smoothing, reduction="none")
    total = F.cross_entropy(l, lab, label_smoothing=smoothing, reduction="sum")
    (total * xscale).backward()

    _rel(f["loss"], rows.detach(), f["l"].abs().amax(1), "row loss")
    _rel(f["loss"].sum(), total.detach(), f["loss"].abs().sum(), "loss")
    _rel(f["d"], l.grad, torch.full_like(f["d"], xscale), "d")
    # (d = (p - tgt) * xscale is a difference of terms of size xscale: what is added up from d is
    # judged relative to the same sums with |d| replaced by xscale)
    wcol = xscale * inp["w"].abs().sum(0)
    _rel(b["dWt"], w.grad.t(), xscale * f["z"].abs().sum(0)[:, None].expand(-1, NC), "dWt")
    _rel(b["dz"], z.grad, wcol.expand(M, -1), "dz")
    _rel(m["sg"], sh.grad, M * wcol, "sum g")
    _rel(m["sgy"], sc.grad, 2 * M * wcol, "sum g y")
    if bias:
        _rel(b["db"], bb.grad, torch.full_like(b["db"], xscale * M), "db")
    assert f["hits"] == int(((l.detach() == l.detach().amax(1, keepdim=True)).int().argmax(1) == lab).sum())


def test_out_of_range_rule():
    """tgt = off for every class: the row's loss is smoothing * lse - off * sum l, d = (softmax - off) * xscale,
    no hit -- whatever the label's value."""
    gen = _gen("oor")
    inp = S.build_readout(264, 17, S.ACT_RELU, gen)
    lab = S.make_labels(inp, gen, out_of_range=[-1, 17, 255, -2])
    for s in (0.0, 0.125):
        f = _fwd(inp, lab, 0.5, s)
        out = ~f["yin"]
        assert int(out.sum()) == 33 and not bool(f["hit"][out].any())
        want = s * f["lse"] - s / 17 * f["l"].sum(1)
        _rel(f["loss"][out], want[out], f["lse"][out].abs(), "row loss")
        _rel(f["d"][out], ((torch.softmax(f["l"], 1) - s / 17) * 0.5)[out], torch.ones_like(f["d"][out]), "d")
        if s == 0.0:
            assert float(f["loss"][out].abs().max()) < 1e-14


# every (builder, NC, act) the GPU file uses
_SEG = sorted({(c["NC"], c["act"], c["bias"]) for c in S.SEGHEAD_CASES})


@pytest.mark.parametrize("NC,act,bias", _SEG)
def test_readout_builder_promises(NC, act, bias):
    gen = _gen(f"readout-{NC}-{act}-{bias}")
    for M in S.m_values(NB)[2:]:
        inp = S.build_readout(M, NC, act, gen, bias)
        lab = S.make_labels(inp, gen)
        f = _fwd(inp, lab, 1.0 / M, 0.125)
        S.check_promises(inp, f)
        # the readout: dz[:, perm[c]] is d[:, c] itself
        d = S.bf16_round(f["d"])
        assert torch.equal((d @ inp["w"])[:, inp["perm"]], d)
        tied = (f["l"] == f["l"].amax(1, keepdim=True)).sum(1) > 1
        if M > 1000 and NC >= 16:                # (a sample large enough to count them; 2 or 3 classes
            #                                      may never tie under one draw of the parameters)
            assert 0.002 < float(tied.double().mean()) < 0.5, "tied top logits are neither absent nor the rule"
        assert 0 < f["hits"] < M


@pytest.mark.parametrize("case", S.XENT_CASES, ids=[c["name"] for c in S.XENT_CASES])
def test_general_builder_promises(case):
    gen = _gen(case["name"])
    M = 264
    inp = S.build_general(M, case["K"], case["NC"], case["pro"] or 0, gen, case["pro"] is not None, case["bias"])
    f = _fwd(inp, S.make_labels(inp, gen), 1.0 / M, case["smoothing"])
    S.check_promises(inp, f)


@pytest.mark.parametrize("NC", [2, 25])
@pytest.mark.parametrize("act", [S.ACT_NONE, S.ACT_RELU])
def test_tied_builder_promises(act, NC):
    gen = _gen(f"tied-{act}-{NC}")
    inp = S.build_tied(264, NC, act, gen)
    lab = S.make_labels(inp, gen)
    f = _fwd(inp, lab, 1.0 / 264, 0.0)
    S.check_promises(inp, f)
    assert bool((f["l"] == f["l"][:, :1]).all()) and bool((f["am"] == 0).all())
    assert f["hits"] == int((lab == 0).sum()) > 0


@pytest.mark.parametrize("NC,act,smoothing", S.EXACT_CASES)
def test_uniform_builder_promises(NC, act, smoothing):
    gen = _gen(f"uniform-{NC}-{act}-{smoothing}")
    for M, xscale in ((264, 2.0 ** -8), (S.m_values(NB)[3], 2.0 ** -17)):
        nb = min(NB, (M + 255) // 256)
        inp = S.build_uniform(M, NC, act, gen)
        lab = S.make_labels(inp, gen, mix=False)   # (uniform labels: no column collects half the targets)
        f = _fwd(inp, lab, xscale, smoothing)
        S.check_promises(inp, f)
        assert bool((f["l"] == f["l"][:, :1]).all()) and bool((f["am"] == 0).all())
        d = S.uniform_d(NC, f["tgt"], xscale)
        assert torch.equal(S.bf16_round(d), d), "the uniform d is not a bf16 value"
        _rel(f["d"], d, torch.full_like(d, xscale), "d")
        worst = S.exact_tier_preconditions(inp, f, d, xscale, nb)
        print(f"uniform NC {NC} M {M}: {worst:.3f} of 2^24 steps")
        assert worst < 1.0
        # and the oracle's own outputs pass the exact comparison
        out = S.simulate(inp, dict(f, d=d), nb)
        S.judge_exact(inp, f, d, out, nb, "uniform")


# ---------------------------------------------------------------------------
# planted defects: each applied to the oracle's own outputs, each must be rejected
# ---------------------------------------------------------------------------
def _planted_case(M=264, NC=17, smoothing=0.125, oor=None, name="planted"):
    gen = _gen(name)
    inp = S.build_readout(M, NC, S.ACT_RELU, gen)
    lab = S.make_labels(inp, gen, out_of_range=oor)
    nb = min(NB, (M + 255) // 256)
    xscale = 1.0 / M
    f = _fwd(inp, lab, xscale, smoothing)
    return inp, lab, f, S.simulate(inp, f, nb), xscale, nb


def test_judges_accept_the_oracle():
    for M in (8, 264, S.m_values(NB)[3]):
        inp, lab, f, out, xscale, nb = _planted_case(M)
        res = S.judge_all(inp, f, out, xscale, nb, "clean")
        assert max(res.values()) <= 1.0


def _rejects(inp, f, out, xscale, nb):
    with pytest.raises(AssertionError):
        S.judge_all(inp, f, out, xscale, nb, "planted")


@pytest.mark.parametrize("M", [264, 256 * 513 + 8])
def test_rejects_a_row_dropped_from_dwt_and_db(M):
    inp, lab, f, out, xscale, nb = _planted_case(M)
    r = 256 + 5 if M > 264 + 256 else 5          # a row of workgroup 1's first tile / of tile 0
    wg = (r // 256) % nb
    part = out["part"].double()
    part[wg, S.P_DB:S.P_DB + 17] -= out["d"][r]
    part[wg, S.P_DW:S.P_DW + 1024].view(32, 32)[:, :17] -= f["z"][r][:, None] * out["d"][r][None, :]
    _rejects(inp, f, dict(out, part=part.float()), xscale, nb)


def test_rejects_rotated_class_columns():
    inp, lab, f, out, xscale, nb = _planted_case()
    with pytest.raises(AssertionError):
        S.judge_d(out["d"].roll(1, 1), f, xscale, "rotated")


def test_rejects_a_skipped_target_fixup():
    inp, lab, f, out, xscale, nb = _planted_case()
    d = out["d"].clone()
    r = 100
    d[r, lab[r]] = S.bf16_round((torch.softmax(f["l"][r], 0)[lab[r]] - 0.125 / 17) * xscale)   # `off`, not `on`
    with pytest.raises(AssertionError):
        S.judge_d(d, f, xscale, "fix-up")


def test_rejects_on_without_off_under_smoothing():
    inp, lab, f, out, xscale, nb = _planted_case()
    tgt = torch.where(f["tgt"] > 0.5, f["tgt"], torch.zeros_like(f["tgt"]))   # off forgotten
    with pytest.raises(AssertionError):
        S.judge_d(S.bf16_round((torch.softmax(f["l"], 1) - tgt) * xscale), f, xscale, "no off")
    part = out["part"].clone()
    part[:, 0] = S.wg_sum(-(tgt * (f["l"] - f["lse"][:, None])).sum(1), nb).float()
    with pytest.raises(AssertionError):
        S.judge_loss(part[:, 0], f, inp["M"], nb, "no off")


def test_rejects_last_wins_argmax():
    inp, lab, f, out, xscale, nb = _planted_case()
    last = S.last_argmax(f["l"])
    tied = (last != f["am"]) & ((lab == last) | (lab == f["am"]))
    assert int(tied.sum()) > 0, "no tied row decides a hit"
    part = out["part"].clone()
    part[:, 1] = S.wg_sum((last == lab).double(), nb).float()
    with pytest.raises(AssertionError):
        S.judge_hits(part[:, 1], f, nb, "last wins")


def test_rejects_two_bf16_ulps_on_one_d():
    inp, lab, f, out, xscale, nb = _planted_case()
    d = out["d"].clone()
    d[77, 3] += 2 * S.O.bf16_ulp(d[77, 3])
    with pytest.raises(AssertionError):
        S.judge_d(d, f, xscale, "2 ulps")


@pytest.mark.parametrize("smoothing", [0.0, 0.125])
def test_rejects_an_out_of_range_row_charged_a_whole_lse(smoothing):
    inp, lab, f, out, xscale, nb = _planted_case(smoothing=smoothing, oor=[17, 255, -1], name="oor-planted")
    bad = torch.where(f["yin"], f["loss"], f["lse"] - smoothing / 17 * f["l"].sum(1))   # lse, not smoothing * lse
    part = out["part"].clone()
    part[:, 0] = S.wg_sum(bad, nb).float()
    with pytest.raises(AssertionError):
        S.judge_loss(part[:, 0], f, inp["M"], nb, "whole lse")
    # ... and the truncated int64 label 2^32 + arg-max counted as a hit
    inp, lab, f, out, xscale, nb = _planted_case(smoothing=smoothing, oor=[-2], name="oor-planted")
    part = out["part"].clone()
    part[:, 1] = S.wg_sum(((lab & 0xFFFFFFFF) == f["am"]).double(), nb).float()
    with pytest.raises(AssertionError):
        S.judge_hits(part[:, 1], f, nb, "truncated label")
