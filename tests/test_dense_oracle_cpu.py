"""The Dense oracle of tests/_dense_oracle.py judged on the CPU: it agrees with float64
``torch.nn.functional.linear`` + autograd; every case keeps every checked sum inside the regime
where fp32 is exact (``BOUNDED`` lists exactly the rest); the case table reaches every path of
dense.hip it claims (from a mirror of the launchers' arithmetic, which needs no GPU); and the
inputs are what they claim: weights that the bf16 conversion has to round, ties among them, no
zero weight, and outputs that need the final rounding."""
import pytest
import torch
import torch.nn.functional as F

import _dense_oracle as O
from _bn_pool_oracle import bf16_round, check_exact

BWD_CASES = O.DGRAD_CASES + O.WGRAD_CASES


def _ids(cases):
    return [c["name"] for c in cases]


def _bwd_oracle(c):
    dgrad = c["name"].startswith("dgrad")
    inp = O.make_inputs(c, need=("w", "dy", "ya") if dgrad else ("x", "dy", "ya"))
    gp = O.g_prime(inp["dy"], inp.get("ya"), c["ya"])
    return inp, gp, O.backward(inp.get("x"), inp.get("w"), gp, want=("dx",) if dgrad else ("dW",))


# ---------------------------------------------------------------------------
# the oracle against a second formulation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in O.FWD_CASES + O.DISPATCH_CASES], ids=_ids(O.FWD_CASES + O.DISPATCH_CASES))
def test_oracle_matches_linear_and_autograd(c):
    """float64 on grids is exact on both sides, so equality is bit for bit.  The second
    formulation: F.linear on bf16_round(w) and autograd, with g' fed in."""
    inp = O.make_inputs(c)
    x = inp["x"].clone().requires_grad_(True)
    w = bf16_round(inp["w"]).requires_grad_(True)
    b = inp["b"].clone().requires_grad_(True) if c["bias"] else None
    pre = F.linear(x, w, b)
    f = O.forward(inp["x"], inp["w"], inp["b"] if c["bias"] else None, c["act"])
    assert torch.equal(pre, f["pre"])
    assert torch.equal(O.act_fwd(pre.detach(), c["act"]), f["y"])
    # the activation against the library's own form (the sigmoid is written 1 / (1 + exp(-u)): an ulp)
    lib = {O.NONE: pre, O.RELU: torch.relu(pre), O.TANH: torch.tanh(pre), O.SIGMOID: torch.sigmoid(pre)}[c["act"]]
    if c["act"] == O.SIGMOID:
        assert torch.allclose(lib, f["y"], rtol=1e-15, atol=0)
    else:
        assert torch.equal(lib, f["y"])
    for act in (O.NONE, O.RELU, O.TANH, O.SIGMOID):
        ya = O.make_ya(c["M"], c["N"], act, O.gen(c["name"] + ":ya")) if act else None
        gp = O.g_prime(inp["dy"], ya, act)
        bw = O.backward(inp["x"], inp["w"], gp)
        grads = torch.autograd.grad(pre, (x, w) + ((b,) if b is not None else ()), gp, retain_graph=True)
        assert torch.equal(grads[0], bw["dx"]) and torch.equal(grads[1], bw["dW"])
        if b is not None:
            assert torch.equal(grads[2], bw["db"])
        if act:                                  # g' is dy * act'(ya), exactly: the rounding changes nothing
            assert torch.equal(gp, inp["dy"] * O.act_bwd_from_out(ya, act))
            assert O.on_grid(gp, 1 / 64) and float(gp.abs().max()) <= 4.0


@pytest.mark.parametrize("c", BWD_CASES, ids=_ids(BWD_CASES))
def test_backward_oracle_matches_autograd(c):
    """The dgrad and wgrad cases with their own ``ya``: autograd of F.linear on bf16_round(w), g' fed in."""
    inp = O.make_inputs(c)
    gp = O.g_prime(inp["dy"], inp.get("ya"), c["ya"])
    x = inp["x"].clone().requires_grad_(True)
    w = bf16_round(inp["w"]).requires_grad_(True)
    b = torch.zeros(c["N"], dtype=torch.float64, requires_grad=True)
    dx, dW, db = torch.autograd.grad(F.linear(x, w, b), (x, w, b), gp)
    bw = _bwd_oracle(c)[2]
    if "dx" in bw:
        assert torch.equal(dx, bw["dx"])
    else:
        assert torch.equal(dW, bw["dW"])
    assert torch.equal(db, bw["db"])


# ---------------------------------------------------------------------------
# exactness: sum |terms| / step < 2^24 for every case and quantity
# ---------------------------------------------------------------------------
def test_bounded_is_exactly_what_misses_the_exact_regime():
    """Every sum is exact in fp32; what is not compared bit for bit is the tanh and the sigmoid
    forward output, whose inexactness is the activation's, not the sum's.  ``BOUNDED`` must equal
    the recomputed set: every sum that misses the condition, and every forward output that is
    not on its grid (recomputed from the values, not from the case's activation code)."""
    missed, margins = [], {}
    for c in O.FWD_CASES + O.DISPATCH_CASES:
        inp = O.make_inputs(c, need=("x", "w", "b"))
        f = O.forward(inp["x"], inp["w"], inp["b"] if c["bias"] else None, c["act"])
        m = O.exact_margin(f["y_abs"], O.step_of("y"))
        margins[c["name"], "y"] = m
        assert m < 1.0 and O.on_grid(f["pre"], O.step_of("y")), (c["name"], m)
        if not O.on_grid(f["y"], O.step_of("y")):                    # act(pre) is no dyadic value
            missed.append((c["name"], "y"))
            assert float(f["pre"].abs().max()) < O.SOFT_ARG_LIMIT, c["name"]
    for c in BWD_CASES:
        _, gp, bw = _bwd_oracle(c)
        for q in ("dx", "dW", "db"):
            if q not in bw:
                continue
            step = O.step_of(q, bool(c["ya"]))
            m = O.exact_margin(bw[q + "_abs"], step)
            margins[c["name"], q] = m
            if not (m < 1.0 and O.on_grid(bw[q], step)):
                missed.append((c["name"], q))
            if q != "dx":                        # handed to check_exact as fp32
                assert torch.equal(bw[q].float().double(), bw[q])
    assert sorted(missed) == sorted(O.BOUNDED), (missed, O.BOUNDED)
    assert {O.FWD_CASES[i]["act"] for i in range(len(O.FWD_CASES)) if (O.FWD_CASES[i]["name"], "y") in O.BOUNDED} == {
        O.TANH, O.SIGMOID}
    worst = max(margins.items(), key=lambda kv: kv[1])
    print(f"worst exactness margin {worst[1]:.4f} at {worst[0]}")


def test_every_forward_instance_has_an_exact_case():
    """The tanh / sigmoid cases saturate and are judged by a bound: each of the eight
    (load form, column waves, one slice or slabs) instances also has a none or relu case."""
    inst = {}
    for c in O.FWD_CASES:
        S = O.dense_splits(c["M"], c["N"], c["K"]) if c["S"] is None else c["S"]
        p = O.fwd_plan(c["M"], c["N"], c["K"], S)
        inst.setdefault((p["vec"], p["ncw"], p["Sr"] == 1), set()).add((c["name"], "y") not in O.BOUNDED)
    assert len(inst) == 8 and all(True in v for v in inst.values()), inst


def test_dispatch_backward_stays_exact():
    """The LinearFn cases: the backward runs on g' = dy * relu'(y) of the kernel's own y."""
    for c in O.DISPATCH_CASES:
        inp = O.make_inputs(c)
        f = O.forward(inp["x"], inp["w"], inp["b"] if c["bias"] else None, c["act"])
        assert c["act"] in (O.NONE, O.RELU)      # (with tanh the backward would leave the grid)
        gp = O.g_prime(inp["dy"], bf16_round(f["y"]) if c["act"] else None, c["act"])
        bw = O.backward(inp["x"], inp["w"], gp)
        for q in ("dx", "dW", "db"):
            assert O.exact_margin(bw[q + "_abs"], O.step_of(q)) < 1.0 and O.on_grid(bw[q], O.step_of(q)), (c["name"], q)


# ---------------------------------------------------------------------------
# path coverage
# ---------------------------------------------------------------------------
def test_case_table_reaches_every_path():
    have = O.all_tags()
    assert not (O.REQUIRED_TAGS - have), sorted(O.REQUIRED_TAGS - have)


def test_case_table_is_what_the_comments_say():
    """The launcher arithmetic of the cases named in the table's comments."""
    p = O.fwd_plan(33, 65, 544, 17)
    assert (p["kc"], p["Sr"], p["ncw"], p["vec"]) == (32, 17, 1, True)
    p = O.fwd_plan(33, 65, 544, 16)
    assert (p["kc"], p["Sr"]) == (64, 9)
    assert O.fwd_plan(20, 24, 800, 5)["kc"] == 160
    p = O.fwd_plan(20, 10, 1095, 4)
    assert not p["vec"] and p["Sr"] == 4 and p["slices"][-1][1] - p["slices"][-1][0] < p["kc"]
    assert O.fwd_plan(130, 130, 512, 2)["ncw"] == 2 and O.fwd_plan(130, 65, 516, 1)["ncw"] == 2
    assert O.fwd_plan(129, 65, 64, 1)["ncw"] == 1            # K < 512 and few tiles
    assert O.fwd_plan(20, 24, 800, O.dense_splits(20, 24, 800))["Sr"] == 3
    assert O.dgrad_plan(130, 8, 32768)["mrep"] == 3 and O.dgrad_plan(300, 8, 32768)["mrep"] == 4
    assert O.dgrad_plan(300, 8, 32768)["grid_y"] == 2
    assert O.dgrad_plan(16, 512, 64)["lds"] == 66560 and O.dgrad_plan(64, 24, 64)["NP"] == 32
    assert O.dgrad_plan(*O.DGRAD_REFUSED)["refused"] and not O.dgrad_plan(4, 1248, 8)["refused"]
    p = O.wgrad_plan(545, 24, 40, 1)
    assert p["chunks"] == [[512, 33]] and p["MCH"] == 512 and p["lds"] == 133120
    assert [b - a for a, b in O.wgrad_plan(300, 24, 40, 2)["slices"]] == [160, 140]
    assert [b - a for a, b in O.wgrad_plan(300, 24, 40, 4)["slices"]] == [96, 96, 96, 12]
    assert O.wgrad_plan(400, 24, 40, 3)["Sr"] == 3 and O.wgrad_plan(130, 24, 40, 4)["Sr"] == 3
    # the dispatcher's cases: the ya path, and the separate act_bwd pass above K = 4096
    assert O.DISPATCH_CASES[0]["K"] <= 4096 < O.DISPATCH_CASES[1]["K"]
    S = O.dense_splits(16, 24, 4104)
    assert S == 16 and O.fwd_plan(16, 24, 4104, S)["Sr"] == 15
    assert [O.dn_ncw(*s) for s in O.INFER_SHAPES] == [2, 1]
    assert O.dense_splits(*O.SPLITS_FC1) == 128 and O.dense_wgrad_slices(*O.SPLITS_FC1) == 1


# ---------------------------------------------------------------------------
# the inputs are what they claim
# ---------------------------------------------------------------------------
def _is_tie(v):
    """v lies exactly half way between two neighbouring bf16 values."""
    r = bf16_round(v).to(torch.bfloat16)
    up = torch.nextafter(r, torch.full_like(r, float("inf"))).double()
    dn = torch.nextafter(r, torch.full_like(r, float("-inf"))).double()
    r = r.double()
    return (r != v) & (((v - r).abs() == (up - v).abs()) | ((v - r).abs() == (v - dn).abs()))


def test_weights_need_rounding_and_hold_ties():
    changed = ties = total = up = 0
    for c in O.FWD_CASES + O.DGRAD_CASES:
        w = O.make_inputs(c, need=("w",))["w"]
        r = bf16_round(w)
        assert not bool((w == 0).any()) and not bool((r == 0).any()), "a zero weight hides a wrong product"
        assert float(w.abs().max()) <= 1.0 and float(r.abs().max()) <= 1.0
        assert O.on_grid(w, O.W_STEP) and O.on_grid(r, O.W_STEP)
        assert torch.equal(w.float().double(), w)
        ne, tie = r != w, _is_tie(w)
        assert bool((tie[ne]).all())             # on this grid every rounding is a tie
        # at least one tie that truncation would get wrong (nearest even lies away from zero)
        assert bool((ne & (r.abs() > w.abs())).any()) and bool((ne & (r.abs() < w.abs())).any()), c["name"]
        changed, ties, total = changed + int(ne.sum()), ties + int(tie.sum()), total + w.numel()
        up += int((ne & (r.abs() > w.abs())).sum())
    print(f"weights: {changed} of {total} change under bf16_round ({changed / total:.3f}), {ties} ties, "
          f"{up} rounded away from zero")
    assert 0.2 < changed / total < 0.3 and ties == changed and up > 0


def test_output_rounding_is_exercised():
    """y and dx are compared as bf16_round(oracle): a counted share of them must need the rounding."""
    for cases, q in ((O.FWD_CASES, "y"), (O.DGRAD_CASES, "dx")):
        changed = total = 0
        for c in cases:
            if q == "y":
                if c["act"] in (O.TANH, O.SIGMOID) or c["out_fp32"]:
                    continue
                inp = O.make_inputs(c, need=("x", "w", "b"))
                v = O.forward(inp["x"], inp["w"], inp["b"] if c["bias"] else None, c["act"])["y"]
            else:
                v = _bwd_oracle(c)[2]["dx"]
            n = int((bf16_round(v) != v).sum())
            assert n > 0, c["name"]
            changed, total = changed + n, total + v.numel()
        print(f"{q}: {changed} of {total} need the final rounding ({changed / total:.3f})")
        assert changed / total > 0.3, (q, changed, total)


def test_one_wrong_term_is_visible():
    """The comparison the GPU file uses reports the smallest possible mistakes: one weight rounded
    by truncation, one product lost, one row of g' with the activation backward skipped."""
    c = O.FWD_CASES[0]
    inp = O.make_inputs(c)
    y = bf16_round(O.forward(inp["x"], inp["w"], inp["b"], O.NONE)["y"])
    r = bf16_round(inp["w"])
    n, k = [int(i) for i in ((r.abs() > inp["w"].abs()) & (inp["x"][0] != 0)).nonzero()[0]]
    w2 = r.clone()
    w2[n, k] -= torch.sign(w2[n, k]) * 2 * O.W_STEP          # the truncated neighbour (a bf16 value)
    with pytest.raises(AssertionError, match="differ"):
        check_exact(bf16_round(O.forward(inp["x"], w2, inp["b"], O.NONE)["pre"])[:, n], y[:, n], "y, one truncated weight")
    d = [c for c in O.DGRAD_CASES if c["ya"] == O.TANH][0]
    inp, gp, bw = _bwd_oracle(d)
    gp2 = gp.clone()
    gp2[:, 7] = inp["dy"][:, 7]
    assert not torch.equal(gp2, gp)
    with pytest.raises(AssertionError, match="differ"):
        check_exact(bf16_round(O.backward(None, inp["w"], gp2, want=("dx",))["dx"]), bf16_round(bw["dx"]), "dx, lane 7")
