"""The fused head + loss kernels -- seghead_loss_kernel (csrc/kernels/seghead.hip) and the XENT
instance of pw_fwd_kernel (csrc/kernels/pointwise.hip) -- against the fp64 oracle of
tests/_seghead_oracle.py, host-dispatch instance by instance.

The bindings are called directly with inputs on dyadic grids, so z and the logits are bf16
values, the kernels' logits are exact and what remains is the softmax, the roundings of the
stores and the order of the sums.  seghead_loss emits dz = d w, not d: its head is a readout
head (w = [P | R], P a permutation), so dz[:, perm[c]] is the kernel's own bf16 d[:, c].

Stage 1 judges d, the loss and the hits against the oracle; stage 2 judges db, dWt, dz and the
BN moments against the oracle evaluated at the kernel's own d (then its own dz), so that only
the sums are in question there.  Three bounds (tests/_bn_pool_oracle.py): one bf16 rounding
(d, dz), the fp32 reduction bound (n + 8) 2^-24 sum|terms| with n counted from the code (loss,
db, dWt, moments; per workgroup and in total), and bit-for-bit equality (hits, padded slots,
the uniform-logit tier, the relations between calls).  Every output starts as NaN or a
sentinel and carries guard rows, so a slot that is not written, or one written out of bounds,
fails.

Labels outside [0, NC) follow one rule on all three loss paths (seghead_loss, pw_fwd_xent,
ops.loss.softmax_xent): no target class, no hit.
"""
import json
import os
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import _seghead_oracle as S  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.ops import loss as loss_ops  # noqa: E402

NONE, RELU = S.ACT_NONE, S.ACT_RELU
SENT = -7.0                                      # guard rows of the bf16 outputs
GUARD = 8
_REC = []


def _rec(case, inst, res):
    for check, frac in res.items():
        _REC.append({"case": case, "instance": inst, "check": check, "frac": float(frac)})
    print(f"{case} [{inst}]: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))


@pytest.fixture(scope="module", autouse=True)
def _report():
    """FN_SEGHEAD_ORACLE_REPORT=<file>: the observed error / bound of every check as JSON lines
    (the source of profiles/seghead_oracle.md)."""
    yield
    path = os.environ.get("FN_SEGHEAD_ORACLE_REPORT")
    if path:
        with open(path, "w") as f:
            for r in _REC:
                f.write(json.dumps(r) + "\n")


def _dev():
    return torch.device("cuda", 0)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _bf(t64):
    b = t64.to(torch.float32).to(torch.bfloat16).to(_dev()).contiguous()
    assert torch.equal(b.double().cpu(), t64), "input is not a bf16 value"
    return b


def _f32(t64):
    if t64 is None:
        return None
    f = t64.to(torch.float32).to(_dev()).contiguous()
    assert torch.equal(f.double().cpu(), t64), "input is not an fp32 value"
    return f


def _m_values(xent=False):
    Kn = _native.kernels()
    return S.m_values(Kn.pw_xent_blocks(1 << 30) if xent else Kn.seghead_blocks(1 << 30))


def _on_device(inp):
    return {"y": _bf(inp["y"]), "sc": _f32(inp["sc"]), "sh": _f32(inp["sh"]), "w": _bf(inp["w"]),
            "bias": _f32(inp["bias"])}


def _fwd(inp, lab, xscale, smoothing):
    return S.forward(inp["y"], inp["sc"], inp["sh"], inp["act"], inp["w"], inp["bias"], lab, xscale, smoothing)


def _lab_dev(lab, lab8):
    if lab8:
        assert int(lab.min()) >= 0 and int(lab.max()) <= 255
        return lab.to(torch.uint8).to(_dev())
    return lab.to(_dev())


def _seghead(dv, lab, M, NC, act, xscale, smoothing, hits, K=S.K_HEAD, expect_refusal=False):
    """One seghead_loss call into NaN / sentinel buffers with guard rows -> (dz, part, part_reduce's
    total) on the CPU.  Every slot of every partial row must have been written, no guard touched."""
    Kn = _native.kernels()
    nb = Kn.seghead_blocks(M)
    dz = torch.full((M + GUARD, K), SENT, dtype=torch.bfloat16, device=_dev())
    part = torch.full((nb + 1, S.PART_LEN), float("nan"), dtype=torch.float32, device=_dev())
    st = _native.stream(dz)
    call = lambda: Kn.seghead_loss(  # noqa: E731
        dv["y"].data_ptr(), dv["sc"].data_ptr(), dv["sh"].data_ptr(), dv["w"].data_ptr(), _native.ptr(dv["bias"]),
        lab.data_ptr(), dz.data_ptr(), part.data_ptr(), M, K, NC, act, xscale, smoothing, st,
        [dv["y"].numel(), dv["w"].numel(), lab.numel(), M * K, nb * S.PART_LEN], int(lab.dtype == torch.uint8), hits)
    if expect_refusal:
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            call()
        torch.cuda.synchronize()
        assert bool((dz == SENT).all()) and bool(torch.isnan(part).all()), "a refused call wrote something"
        return None
    call()
    tot = torch.full((S.PART_LEN,), float("nan"), dtype=torch.float32, device=_dev())
    Kn.part_reduce(part.data_ptr(), tot.data_ptr(), S.PART_LEN, nb, 0, st, [nb * S.PART_LEN, S.PART_LEN])
    torch.cuda.synchronize()
    assert bool((dz[M:] == SENT).all()), "dz guard rows were written"
    assert bool(torch.isnan(part[nb]).all()), "the partial slab's guard row was written"
    assert not bool(torch.isnan(part[:nb]).any()), "a partial slot was not written"
    assert not bool(torch.isnan(dz[:M].float()).any()) and not bool((dz[:M] == SENT).all(1).any()), "a dz row is missing"
    return {"dz": dz[:M].cpu().double(), "part": part[:nb].cpu(), "tot": tot.cpu(), "nb": nb}


def _readout_d(out, inp):
    """The kernel's own bf16 d, read through the readout columns of dz."""
    return dict(out, d=out["dz"][:, inp["perm"]])


def _seghead_inputs(name, mi):
    case = next(c for c in S.SEGHEAD_CASES if c["name"] == name)
    M = _m_values()[mi]
    gen = _gen(f"{name}-{mi}")
    inp = S.build_readout(M, case["NC"], case["act"], gen, case["bias"])
    lab = S.make_labels(inp, gen)
    xscale = 1.0 if case["xone"] else 1.0 / M
    f = _fwd(inp, lab, xscale, case["smoothing"])
    S.check_promises(inp, f)
    return inp, lab, xscale, f


# which case reaches which instance of SH_LAUNCH: the ``inst`` column of S.SEGHEAD_CASES
#   <A, T, 25, false>  NC 25, smoothing 0, hits 0   (relu-nc25-lean, none-nc25-lean-nobias)
#   <A, T, 25>         NC 25 otherwise              (relu-nc25-smooth, relu-nc25-smooth-nohits, none-nc25-hits)
#   <A, T>             every other NC               (the rest), each with T = long long and unsigned char
@pytest.mark.parametrize("mi", range(4), ids=["m8", "m256", "m264", "mbig"])
@pytest.mark.parametrize("case", S.SEGHEAD_CASES, ids=[c["name"] for c in S.SEGHEAD_CASES])
def test_seghead_loss(case, mi):
    inp, lab, xscale, f = _seghead_inputs(case["name"], mi)
    M, NC = inp["M"], inp["NC"]
    dv = _on_device(inp)
    lean = NC == 25 and not case["hits"] and case["smoothing"] == 0.0
    outs = []
    for lab8 in (0, 1):
        out = _seghead(dv, _lab_dev(lab, lab8), M, NC, case["act"], xscale, case["smoothing"], case["hits"])
        outs.append(out)
        if lab8:                                 # uint8 labels: the int64 call's results, bit for bit
            for k in ("dz", "part", "tot"):
                assert torch.equal(out[k], outs[0][k]), f"uint8 labels change {k}"
            continue
        res = S.judge_all(inp, f, _readout_d(out, inp), xscale, out["nb"], case["name"], hits=not lean,
                          reduced=out["tot"])
        if lean:
            assert bool((out["part"][:, 1] == 0).all()), "the lean instance's hits column is not 0"
        _rec(f"seghead {case['name']} M {M}", case["inst"], res)


@pytest.mark.parametrize("NC", [2, 25])
@pytest.mark.parametrize("act", [NONE, RELU], ids=["none", "relu"])
def test_seghead_all_logits_tied(act, NC):
    """Every class row of w the same, a constant bias: every row's first arg-max is class 0."""
    M = 264
    gen = _gen(f"tied-{act}-{NC}")
    inp = S.build_tied(M, NC, act, gen)
    lab = S.make_labels(inp, gen)
    f = _fwd(inp, lab, 1.0 / M, 0.0)
    S.check_promises(inp, f)
    assert bool((f["am"] == 0).all()) and f["hits"] == int((lab == 0).sum()) > 0
    for lab8 in (0, 1):
        out = _seghead(_on_device(inp), _lab_dev(lab, lab8), M, NC, act, 1.0 / M, 0.0, 1)
        res = {"loss": S.judge_loss(out["part"][:, 0], f, M, out["nb"], "tied"),
               "hits": S.judge_hits(out["part"][:, 1], f, out["nb"], "tied")}
    _rec(f"seghead tied NC {NC} act {S.ACT_NAMES[act]}", "<A, T, 25> / <A, T>", res)


@pytest.mark.parametrize("big", [False, True], ids=["m264", "mbig"])
@pytest.mark.parametrize("NC,act,smoothing", S.EXACT_CASES,
                         ids=[f"nc{n}-{S.ACT_NAMES[a]}-s{s}" for n, a, s in S.EXACT_CASES])
def test_seghead_exact_tier(NC, act, smoothing, big):
    """Uniform logits: d = (1/NC - tgt) * xscale is a bf16 value and every sum is exact in fp32, so
    dz, db, dWt and the moments compare bit for bit."""
    M, xscale = (_m_values()[3], 2.0 ** -17) if big else (264, 2.0 ** -8)
    gen = _gen(f"uniform-{NC}-{act}-{smoothing}-{big}")
    inp = S.build_uniform(M, NC, act, gen)
    lab = S.make_labels(inp, gen, mix=False)
    f = _fwd(inp, lab, xscale, smoothing)
    S.check_promises(inp, f)
    d = S.uniform_d(NC, f["tgt"], xscale)
    out = _seghead(_on_device(inp), _lab_dev(lab, 0), M, NC, act, xscale, smoothing, 1)
    room = S.exact_tier_preconditions(inp, f, d, xscale, out["nb"])     # (slab_rows_exact inside)
    frac = S.judge_exact(inp, f, d, _readout_d(out, inp), out["nb"], "uniform", reduced=out["tot"])
    _rec(f"seghead uniform NC {NC} act {S.ACT_NAMES[act]} s {smoothing} M {M}", "<A, long long>",
         {"exact": 0.0, "loss": frac, "2^24 steps used": room})


@pytest.mark.parametrize("NC", [25, 17])
def test_seghead_bitwise_relations(NC):
    """uint8 against int64 labels, the lean call against the full one (everything but the hits
    column), and two runs of one call, at the largest M."""
    M = _m_values()[3]
    gen = _gen(f"relations-{NC}")
    inp = S.build_readout(M, NC, RELU, gen)
    lab = S.make_labels(inp, gen)
    dv = _on_device(inp)
    run = lambda lab8, hits: _seghead(dv, _lab_dev(lab, lab8), M, NC, RELU, 1.0 / M, 0.0, hits)  # noqa: E731
    full, again, full8, lean, lean8 = run(0, 1), run(0, 1), run(1, 1), run(0, 0), run(1, 0)
    for name, other in (("second run", again), ("uint8 labels", full8)):
        for k in ("dz", "part", "tot"):
            assert torch.equal(full[k], other[k]), f"{name}: {k} differs"
    for name, other in (("lean", lean), ("lean, uint8 labels", lean8)):
        assert torch.equal(full["dz"], other["dz"]), f"{name}: dz differs"
        assert torch.equal(full["part"][:, 0], other["part"][:, 0]), f"{name}: the loss differs"
        assert torch.equal(full["part"][:, 2:], other["part"][:, 2:]), f"{name}: the gradients differ"
        assert torch.equal(full["tot"][2:], other["tot"][2:]) and torch.equal(full["tot"][0], other["tot"][0])
    assert int(full["part"][:, 1].double().sum()) > 0


def test_seghead_refusals():
    """Host-side -2 returns before any launch: nothing is written."""
    gen = _gen("refusals")
    inp = S.build_general(264, 33, 33, RELU, gen)           # buffers large enough for every variant below
    dv = _on_device(inp)
    lab = torch.zeros(264, dtype=torch.int64, device=_dev())
    ok = dict(M=264, NC=25, act=RELU, K=32)
    for change in (dict(K=16), dict(NC=1), dict(NC=33), dict(M=4), dict(M=12), dict(act=2)):
        a = dict(ok, **change)
        _seghead(dv, lab, a["M"], a["NC"], a["act"], 1.0, 0.0, 1, K=a["K"], expect_refusal=True)


# ---------------------------------------------------------------------------
# pw_fwd_xent
# ---------------------------------------------------------------------------
def _xent(dv, lab, M, K, NC, pro, xscale, smoothing):
    Kn = _native.kernels()
    nb = Kn.pw_xent_blocks(M)
    dlog = torch.full((M + GUARD, NC), SENT, dtype=torch.bfloat16, device=_dev())
    xpart = torch.full((nb + 1, 2), float("nan"), dtype=torch.float32, device=_dev())
    Kn.pw_fwd_xent(dv["y"].data_ptr(), dv["w"].data_ptr(), _native.ptr(dv["bias"]), dlog.data_ptr(), M, K, NC,
                   _native.ptr(dv["sc"]), _native.ptr(dv["sh"]), pro or 0, lab.data_ptr(), xpart.data_ptr(), xscale,
                   smoothing, _native.stream(dlog), [M * K, M * NC, M, 2 * nb])
    torch.cuda.synchronize()
    assert bool((dlog[M:] == SENT).all()), "dlog guard rows were written"
    assert bool(torch.isnan(xpart[nb]).all()) and not bool(torch.isnan(xpart[:nb]).any()), "xpart slots"
    return {"d": dlog[:M].cpu().double(), "xpart": xpart[:nb].cpu(), "nb": nb}


def _judge_xent(out, f, M, xscale, what):
    return {"d": S.judge_d(out["d"], f, xscale, what), "loss": S.judge_loss(out["xpart"][:, 0], f, M, out["nb"], what),
            "hits": S.judge_hits(out["xpart"][:, 1], f, out["nb"], what)}


@pytest.mark.parametrize("mi", range(4), ids=["m8", "m256", "m264", "mbig"])
@pytest.mark.parametrize("case", S.XENT_CASES, ids=[c["name"] for c in S.XENT_CASES])
def test_pw_fwd_xent(case, mi):
    M = _m_values(xent=True)[mi]
    K, NC, pro = case["K"], case["NC"], case["pro"]
    gen = _gen(f"{case['name']}-{mi}")
    inp = S.build_general(M, K, NC, pro or 0, gen, pro is not None, case["bias"])
    lab = S.make_labels(inp, gen)
    xscale = 1.0 / M
    f = _fwd(inp, lab, xscale, case["smoothing"])
    S.check_promises(inp, f)
    dv = _on_device(inp)
    out = _xent(dv, lab.to(_dev()), M, K, NC, pro, xscale, case["smoothing"])
    res = _judge_xent(out, f, M, xscale, case["name"])
    if K == 32:
        # the logits pw_fwd stores under the same prologue are the oracle's, exactly: what the XENT
        # epilogue reads from its staged tile carries no error of its own
        lg = torch.full((M, NC), float("nan"), dtype=torch.bfloat16, device=_dev())
        _native.kernels().pw_fwd(dv["y"].data_ptr(), dv["w"].data_ptr(), _native.ptr(dv["bias"]), lg.data_ptr(), M, K,
                                 NC, 0, _native.stream(lg), _native.ptr(dv["sc"]), _native.ptr(dv["sh"]), pro or 0)
        res["pw_fwd logits"] = S.check_exact(lg.cpu(), f["l"], "pw_fwd logits")
    _rec(f"pw_fwd_xent {case['name']} M {M}", case["inst"], res)


# ---------------------------------------------------------------------------
# labels outside [0, NC): one rule on the three loss paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("NC,act,smoothing,hits", [(25, RELU, 0.0, 0), (25, NONE, 0.0, 1), (25, RELU, 0.125, 1),
                                                   (17, NONE, 0.125, 1), (17, RELU, 0.0, 0)],
                         ids=["nc25-lean", "nc25-hits", "nc25-smooth", "nc17-smooth", "nc17-nohits"])
def test_out_of_range_labels(NC, act, smoothing, hits):
    """1 row in 8 out of range.  Such a row has no target class (tgt = off everywhere: its loss is
    smoothing * lse - off * sum l, 0 without smoothing) and is never a hit, on every path."""
    M, xscale = 264, 1.0 / 264
    gen = _gen(f"oor-{NC}-{act}-{smoothing}")
    inp = S.build_readout(M, NC, act, gen)
    dv = _on_device(inp)
    lean = NC == 25 and not hits and smoothing == 0.0
    counts = {}
    for kind, oor in (("int64", [-1, NC, -2]), ("uint8", [NC, 255])):
        lab = S.make_labels(inp, _gen(f"oor-lab-{NC}"), out_of_range=oor)
        f = _fwd(inp, lab, xscale, smoothing)
        assert int((~f["yin"]).sum()) == 33
        out = _seghead(dv, _lab_dev(lab, kind == "uint8"), M, NC, act, xscale, smoothing, hits)
        res = S.judge_all(inp, f, _readout_d(out, inp), xscale, out["nb"], f"seghead {kind}", hits=not lean,
                          reduced=out["tot"])
        _rec(f"out of range NC {NC} s {smoothing} seghead_loss {kind}", "seghead_loss", res)
        if not lean:
            counts[f"seghead {kind}"] = (int(out["part"][:, 1].double().sum()), f["hits"])
        if kind == "uint8" and (NC == 25 or hits == 0):
            continue                             # (the other paths take int64 labels; one pass each)
        # pw_fwd_xent: the same head, the prologue in front
        xo = _xent(dv, lab.to(_dev()), M, S.K_HEAD, NC, act, xscale, smoothing)
        _rec(f"out of range NC {NC} s {smoothing} pw_fwd_xent {kind}", "pw_fwd_xent", _judge_xent(xo, f, M, xscale, "xent"))
        counts[f"xent {kind}"] = (int(xo["xpart"][:, 1].double().sum()), f["hits"])
        # ops.loss.softmax_xent on pw_fwd's logits
        lg = torch.empty(M, NC, dtype=torch.bfloat16, device=_dev())
        _native.kernels().pw_fwd(dv["y"].data_ptr(), dv["w"].data_ptr(), _native.ptr(dv["bias"]), lg.data_ptr(), M,
                                 S.K_HEAD, NC, 0, _native.stream(lg), dv["sc"].data_ptr(), dv["sh"].data_ptr(), act)
        S.check_exact(lg.cpu(), f["l"], "pw_fwd logits")
        lg.requires_grad_(True)
        mean, correct = loss_ops.softmax_xent(lg, lab.to(_dev()), smoothing, with_correct=True)
        loss_ops.backward(mean)
        res = {"d": S.judge_d(lg.grad.cpu().double(), f, xscale, "softmax_xent"),
               # one block for <= 2048 rows: the kernel's sum times 1 / M
               "loss": S.check_reduction(mean.detach().cpu().double() * M, f["loss"].sum(), f["loss"].abs().sum(),
                                         S.loss_chain(2, 1) + 1, "softmax_xent loss", extra=f["loss_bound"].sum())}
        assert torch.equal(correct.cpu().bool(), f["hit"]), "softmax_xent: per-row hits"
        counts[f"softmax_xent {kind}"] = (int(correct.sum()), f["hits"])
        _rec(f"out of range NC {NC} s {smoothing} softmax_xent {kind}", "softmax_xent_tile_kernel<32>", res)
    for path, (got, want) in counts.items():
        assert got == want, f"{path}: {got} hits, the oracle counts {want}"
