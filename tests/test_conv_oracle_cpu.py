"""The conv oracle of tests/_conv_oracle.py judged on the CPU: it agrees with ops.reference.conv +
autograd in float64; every case keeps every checked sum inside the regime where fp32 is exact;
the case table reaches every kernel path it claims (asserted from the plans, which need no GPU);
and one wrong product is visible to the comparison the GPU file uses."""
import importlib

import pytest
import torch

import _conv_oracle as O
from _bn_pool_oracle import bf16_round, check_exact
from featurenet_amd.ops import conv_tile as ct
from featurenet_amd.ops import conv_wtile as cw
from featurenet_amd.ops import reference as ref

C = importlib.import_module("featurenet_amd.ops.conv")
IDS = [c["name"] for c in O.CASES]


@pytest.fixture(scope="module")
def data():
    """Inputs and oracle results of every case, worked out once."""
    out = {}
    for c in O.CASES:
        inp = O.make_inputs(c)
        s = inp["spec"]
        out[c["name"]] = {"inp": inp, "fwd": O.forward(inp["x"], inp["w"], inp["b"], s),
                          "stat": O.forward(inp["xs"], inp["w"], None, s),
                          "bwd": O.backward(inp["x"], inp["w"], inp["dy"], s)}
    return out


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_reference(name, data):
    """float64 on grids is exact on both sides, so equality is bit for bit (strided and dilated
    cases included)."""
    d = data[name]
    inp, s = d["inp"], d["inp"]["spec"]
    x = inp["x"].clone().requires_grad_(True)
    w = inp["w"].clone().requires_grad_(True)
    b = inp["b"].clone().requires_grad_(True)
    y = ref.conv(x, w, b, s)
    assert torch.equal(y, d["fwd"]["y"])
    assert torch.equal(torch.relu(y), O.forward(inp["x"], inp["w"], inp["b"], s, O.ACT_RELU)["y"])
    assert torch.equal(ref.conv(inp["xs"], inp["w"], None, s), d["stat"]["y"])
    y.backward(inp["dy"])
    assert torch.equal(x.grad, d["bwd"]["dx"])
    assert torch.equal(w.grad.reshape(s.K, s.taps, s.C), d["bwd"]["dW"])
    assert torch.equal(b.grad, d["bwd"]["db"])


def _margins(d):
    """{quantity: (sum |terms| / (2^24 step), value on its grid)} of one case; y over both of
    its inputs (x + bias, and xs of the statistics runs)."""
    f, st, bw = d["fwd"], d["stat"], d["bwd"]
    m = {"y": (max(O.exact_margin(f["y_abs"], O.STEPS["y"]), O.exact_margin(st["y_abs"], O.STEPS["y"])),
               O.on_grid(f["y"], O.STEPS["y"]) and O.on_grid(st["y"], O.STEPS["y"]))}
    for q in ("sum_v", "sum_v2"):
        m[q] = (O.exact_margin(st[q + "_abs"], O.STEPS[q]), O.on_grid(st[q], O.STEPS[q]))
    for q in ("dx", "dW", "db"):
        m[q] = (O.exact_margin(bw[q + "_abs"], O.STEPS[q]), O.on_grid(bw[q], O.STEPS[q]))
    return m


@pytest.mark.parametrize("name", IDS)
def test_every_checked_sum_is_exact_in_fp32(name, data):
    d = data[name]
    m = _margins(d)
    # y, dx, dW and db are always compared bit for bit; only a statistics sum may be listed as bounded
    for q in ("y", "dx", "dW", "db"):
        assert m[q][0] < 1.0 and m[q][1], (q, m[q])
    missed = sorted((name, q) for q in ("sum_v", "sum_v2") if not (m[q][0] < 1.0 and m[q][1]))
    assert missed == sorted(b for b in O.BOUNDED if b[0] == name and b[1] != "y_tanh"), m
    # what the GPU file hands to check_exact is representable: bf16 inputs, fp32 dW / db / sums
    inp = d["inp"]
    for k in ("x", "xs", "w", "b", "dy"):
        assert torch.equal(bf16_round(inp[k]), inp[k]), k
    for t in (d["bwd"]["dW"], d["bwd"]["db"], d["stat"]["sum_v"], d["stat"]["sum_v2"]):
        assert torch.equal(t.float().double(), t)
    assert not bool((inp["w"] == 0).any()), "a zero weight hides a mis-addressed tap"


@pytest.mark.parametrize("name", sorted(O.WTILE_N))
def test_wtile_batch_keeps_dw_exact_and_wraps_the_job_ring(name, monkeypatch):
    """At the large batch of the weight-gradient test dW (and three launches' 3 dW) stays exact, and
    every form of the plan gives its busiest worker three jobs or more."""
    inp = O.make_inputs(O.BY_NAME[name], O.WTILE_N[name])
    s = inp["spec"]
    bw = O.backward(inp["x"], inp["w"], inp["dy"], s, want=("dW",))
    assert 3 * O.exact_margin(bw["dW_abs"], O.STEPS["dW"]) < 1.0
    assert torch.equal((3 * bw["dW"]).float().double(), 3 * bw["dW"])
    planned = 0
    try:
        for form in O.WTILE_FORMS:
            for k in ("FN_WTILE_KS2", "FN_WTILE_NW"):
                monkeypatch.delenv(k, raising=False)
            for k, v in form.items():
                monkeypatch.setenv(k, v)
            cw._PLANS.clear()
            p = cw.plan(s)
            if p is not None:
                planned += 1
                assert O.wtile_jobs(p, s) >= 3, (form, p)
    finally:
        cw._PLANS.clear()
    assert planned >= 3


def test_rounding_to_bf16_is_exercised(data):
    """y and dx are compared as bf16_round(oracle): the table must hold outputs that the rounding
    changes, and exact ties among them (where nearest-even differs from every other mode)."""
    for q, part in (("y", "fwd"), ("dx", "bwd")):
        changed = ties = 0
        for c in O.TILE_CASES:
            v = data[c["name"]][part][q]
            r = bf16_round(v)
            ne = r != v
            changed += int(ne.sum())
            up = torch.nextafter(r.to(torch.bfloat16), torch.full_like(r, float("inf"), dtype=torch.bfloat16)).double()
            dn = torch.nextafter(r.to(torch.bfloat16), torch.full_like(r, float("-inf"), dtype=torch.bfloat16)).double()
            ties += int((ne & (((v - r).abs() == (up - v).abs()) | ((v - r).abs() == (v - dn).abs()))).sum())
        assert changed > 1000 and ties > 100, (q, changed, ties)


def test_tanh_cases_are_not_all_saturated(data):
    """The bounded tanh check says something only where tanh is not +-1: at least a tenth of each
    case's arguments lie within +-2, and none is so large that fp32 could not hold the sum."""
    assert sorted(b for b in O.BOUNDED if b[1] == "y_tanh") == sorted((n, "y_tanh") for n in O.TANH_CASES)
    for n in O.TANH_CASES:
        inp = data[n]["inp"]
        f = O.forward(inp["xs"], inp["w"], inp["b"], inp["spec"])
        assert float((f["y"].abs() < 2).double().mean()) > 0.1, n
        assert O.exact_margin(f["y_abs"], O.STEPS["y"]) < 1.0


@pytest.mark.parametrize("name", sorted(O.STAT_BATCH))
def test_statistics_batch_gives_every_workgroup_three_tiles(name):
    """At O.STAT_BATCH the static statistics launch of conv_tile (at most 256 / column blocks
    workgroups) and of conv_halo (512 / column blocks) adds three tiles or more into every slab
    row, and every row stays exact: rows x the largest tile sum, in steps, is below 2^24."""
    inp = O.make_inputs(O.BY_NAME[name], O.STAT_BATCH[name])
    s = inp["spec"]
    st = O.forward(inp["xs"], inp["w"], None, s)
    assert O.exact_margin(st["y_abs"], O.STEPS["y"]) < 1.0
    v = bf16_round(st["y"])
    ct._PLANS.clear()
    p = ct.fwd_plan(s)
    plans = [((p.TD, p.TH, p.TW), -(-256 // (p.nct // p.NT)))]
    if name in O.STAT_HALO:
        plans.append((C.halo_fwd_plan(s), -(-512 // (1 if s.K <= 64 else -(-s.K // 64)))))
    for dims, workers in plans:
        nt = O.tile_count(s, dims)
        assert nt >= 3 * workers, (dims, nt, workers)
        per_row = -(-nt // workers)
        sa, sq = O.max_tile_sums(v, s, dims)
        assert per_row * sa / O.STEPS["sum_v"] < 2 ** 24 and per_row * sq / O.STEPS["sum_v2"] < 2 ** 24, (sa, sq)


def test_halo_statistics_refuse_a_bias():
    """conv_halo.hip's statistics instance has no bias operand: asking for both is an error, not a
    bias silently dropped (every caller takes statistics without a bias)."""
    s = O.make_spec(O.BY_NAME["c16_k16_same"])
    with pytest.raises(ValueError, match="bias"):
        C.halo_conv_fwd(None, None, torch.zeros(s.K), s, 0, True, C.halo_fwd_plan(s))


def _partial(p, dims):
    return tuple(o % t != 0 for o, t in zip(dims, (p.TD, p.TH, p.TW)))


def test_case_table_reaches_every_path(monkeypatch):
    specs = {c["name"]: O.make_spec(c) for c in O.CASES}
    monkeypatch.delenv("FN_TILE_CS", raising=False)
    for k in ("FN_WTILE_KS2", "FN_WTILE_NW", "FN_WTILE", "FN_CONV_TILE", "FN_TILE_PLAN_RANK", "FEATURENET_CONV_HALO"):
        monkeypatch.delenv(k, raising=False)
    ct._PLANS.clear()
    cw._PLANS.clear()
    fwd = {n: ct.fwd_plan(s) for n, s in specs.items()}
    dgr = {n: ct.dgrad_plan(s) for n, s in specs.items()}
    wt = {n: cw.plan(s) for n, s in specs.items()}
    tile = [c["name"] for c in O.TILE_CASES]
    assert all(fwd[n] is not None for n in tile)
    # channel slices: 8 and 16 as planned, 32 forced (the cost model never picks it at these sizes)
    assert {fwd[n].CS for n in tile} >= {8, 16}
    try:
        monkeypatch.setenv("FN_TILE_CS", "32")
        ct._PLANS.clear()
        for n in O.CS32_CASES:
            p = ct.fwd_plan(specs[n])
            assert p is not None and p.CS == 32, (n, p)
    finally:
        monkeypatch.delenv("FN_TILE_CS")
        ct._PLANS.clear()
    assert {dgr[n].NT for n in tile if dgr[n] is not None} == {2, 4}
    # a partial last tile along each of D, H and W (forward or dgrad)
    part = [_partial(fwd[n], (specs[n].OD, specs[n].OH, specs[n].OW)) for n in tile]
    part += [_partial(dgr[n], (specs[n].D, specs[n].H, specs[n].W)) for n in tile if dgr[n] is not None]
    assert all(any(p[i] for p in part) for i in range(3)), part
    # slices, column blocks, a partial column block
    assert any(specs[n].C // fwd[n].CS > 1 for n in tile)
    assert any(fwd[n].nct // fwd[n].NT > 1 for n in tile)
    assert any(fwd[n].nct // fwd[n].NT == 3 for n in tile)
    assert any(specs[n].K % (fwd[n].NT * 16) for n in tile)
    # three tiles or more: under conv_tile_grid_cap(1) one workgroup walks them all (the cap binds
    # launches without statistics and chunked statistics launches; static ones: O.STAT_BATCH)
    for n in tile:
        s, p = specs[n], fwd[n]
        assert s.N * -(-s.OD // p.TD) * -(-s.OH // p.TH) * -(-s.OW // p.TW) >= 3, n
    # the weight-gradient forms
    wts = [p for p in wt.values() if p is not None]
    assert {p.nw for p in wts} == {4, 8} and {p.ks2 for p in wts} == {True, False}
    assert any(p.c8 for p in wts) and any(p.G > 1 for p in wts)
    assert set(O.WTILE_N) == {n for n in tile + [O.NO_TILE_CASE["name"]] if wt[n] is not None}
    # no tile plan / no weight-gradient tile plan; the halo kernel takes both
    assert fwd[O.NO_TILE_CASE["name"]] is None and C.halo_fwd_plan(specs[O.NO_TILE_CASE["name"]]) is not None
    assert dgr["stem_c8_k4"] is None
    assert wt["c16_k48_same"] is None and C.halo_wgrad_plan(specs["c16_k48_same"]) is not None
    # the halo kernel: every stride-1 case plans a forward, one splits W
    for n in [c["name"] for c in O.STRIDE1_CASES]:
        assert C.halo_fwd_plan(specs[n]) is not None, n
    hw = O.HALO_WSPLIT_CASE["name"]
    assert all(p[2] < o for p, o in ((C.halo_fwd_plan(specs[hw]), specs[hw].OW), (C.halo_dgrad_plan(specs[hw]), specs[hw].W),
                                     (C.halo_wgrad_plan(specs[hw]), specs[hw].OW)))
    # the weights-resident form (conv_halo.hip halo_resident): 32 columns, 8-channel slices and at
    # most 4 weight stages (slices x ceil(taps / 16))
    st = specs["stem_c8_k4"]
    assert C.halo_cs(st.C) == 8 and st.K <= 32 and (st.C // 8) * -(-st.taps // 16) <= 4
    # the gathered kernel: no other kernel plans its cases, and the three gather modes occur
    ig = [c["name"] for c in O.IGEMM_CASES]
    for n in ig:
        s = specs[n]
        assert fwd[n] is None and dgr[n] is None and wt[n] is None, n
        assert C.halo_fwd_plan(s) is None and C.halo_dgrad_plan(s) is None and C.igemm_wgrad_takes(s), n
    assert {C.gather_mode(specs[n]) for n in ig} == {C.GM_SCALAR, C.GM_VEC, C.GM_PACKW}
    assert any(max(specs[n].sd, specs[n].sh, specs[n].sw) > 1 for n in ig)
    assert any(max(specs[n].dd, specs[n].dh, specs[n].dw) > 1 for n in ig)


def test_one_wrong_product_is_visible(data):
    """The mutation check, at the largest case (4,000 terms per output): one x value off by one,
    or one weight of one tap changed, and the comparison the GPU file uses reports it -- for y,
    the statistics, dx and dW."""
    name = "conv2_c32_k5"
    d = data[name]
    inp, s = d["inp"], d["inp"]["spec"]

    def differs(a, r, what):
        with pytest.raises(AssertionError, match="differ"):
            check_exact(a, r, what)

    x2 = inp["x"].clone()
    x2[1, 5, 6, 7, 3] += 1.0                                          # one input value
    differs(bf16_round(O.forward(x2, inp["w"], inp["b"], s)["y"]), bf16_round(d["fwd"]["y"]), "y, one x")
    differs(O.backward(x2, inp["w"], inp["dy"], s, want=("dW",))["dW"], d["bwd"]["dW"], "dW, one x")
    xs2 = inp["xs"].clone()
    xs2[1, 5, 6, 7, 3] += 1.0
    st2 = O.forward(xs2, inp["w"], None, s)
    differs(st2["sum_v"], d["stat"]["sum_v"], "sum v, one x")
    differs(st2["sum_v2"], d["stat"]["sum_v2"], "sum v^2, one x")
    w2 = inp["w"].clone()
    w2[17, 2, 3, 1, 9] = -w2[17, 2, 3, 1, 9]                          # one weight of one tap
    differs(bf16_round(O.forward(inp["x"], w2, inp["b"], s)["y"]), bf16_round(d["fwd"]["y"]), "y, one weight")
    differs(bf16_round(O.backward(inp["x"], w2, inp["dy"], s, want=("dx",))["dx"]), bf16_round(d["bwd"]["dx"]),
            "dx, one weight")
    # the smallest possible error of a single product, a quarter, at a single output
    y3 = bf16_round(d["stat"]["y"]).clone()
    i = int(y3.abs().flatten().argmin())
    y3.view(-1)[i] += 0.25
    differs(y3, bf16_round(d["stat"]["y"]), "y, one quarter")
