"""The conv kernels -- conv_tile.hip, conv_wtile.hip, conv_halo.hip, conv_igemm.hip -- against the
float64 oracle of tests/_conv_oracle.py, kernel family by kernel family, bit for bit.

Each family's own entry point is called, so the dispatcher cannot route around it; the
dispatcher (``ConvFn``) has a test of its own.  Inputs lie on the dyadic grids of the oracle's
docstring, which make every fp32 sum of the kernels exact in any order: y and dx are
``bf16_round(oracle)``, dW, db and the BN statistics are the oracle itself, and ``check_exact``
allows nothing else.  The one bounded quantity is the tanh epilogue (``check_one_rounding``);
a sum listed in ``O.BOUNDED`` would get ``check_reduction``, but there is none, and
tests/test_conv_oracle_cpu.py keeps that list honest.

Guard bands: inputs sit in the middle of flat buffers whose ends hold a large finite sentinel
(``O.banded``).  Every launch runs inside ``Guard`` (tests/_guard.py), which makes each device tensor the entry
point allocates -- outputs, statistics slabs, partial-sum scratch, packed weights -- the
middle of a flat buffer too, its ends holding a known pattern and its middle NaN (``empty``)
or zero (``zeros``); after the launch the bands of every such buffer still alive must be
unchanged, and an output slot nobody wrote is a NaN that fails the comparison.  ``launch`` also
asserts that what the entry point returned lives in such a buffer.

BN statistics: at the table's batches every slab row is one tile's sums, in both schedules of
conv_tile.hip and in conv_halo.hip.  ``test_statistics_rows_of_several_tiles`` runs the static
schedules at batches where every workgroup adds three tiles or more into its row; chunks of
more than one tile (over 8192 tiles) are not covered.
"""
import functools
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import _conv_oracle as O  # noqa: E402
from _bn_pool_oracle import ACT_TANH, bf16_round, check_exact, check_one_rounding, check_reduction  # noqa: E402
from _guard import Guard, assert_guarded, launch  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.ops import conv_tile as ct  # noqa: E402
from featurenet_amd.ops import conv_wtile as cw  # noqa: E402

C = importlib.import_module("featurenet_amd.ops.conv")
NONE, RELU = O.ACT_NONE, O.ACT_RELU
DEV = "cuda"


# ---------------------------------------------------------------------------
# inputs and oracle results, worked out once per case
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data(name):
    inp = O.make_inputs(O.BY_NAME[name])
    s = inp["spec"]
    dv = {k: O.banded(inp[k], torch.bfloat16, DEV) for k in ("x", "xs", "dy")}
    dv["w"], dv["b"] = O.banded(inp["w"], torch.float32, DEV), O.banded(inp["b"], torch.float32, DEV)
    fwd = O.forward(inp["x"], inp["w"], inp["b"], s)
    return {"inp": inp, "spec": s, "dev": dv, "fwd": fwd, "stat": O.forward(inp["xs"], inp["w"], None, s),
            "bwd": O.backward(inp["x"], inp["w"], inp["dy"], s)}


def want_y(d, act):
    return bf16_round(O.act_fwd(d["fwd"]["y"], act))


def check_stats(slab, d, what):
    """The slab's rows, added in float64, are the column sums of the stored values and their squares."""
    st, K = d["stat"], d["spec"].K
    assert slab.shape[1:] == (2, K) and slab.dtype == torch.float32
    tot = slab.double().sum(0).cpu()
    for i, q in enumerate(("sum_v", "sum_v2")):
        if (what.split(":")[0], q) in O.BOUNDED:
            check_reduction(tot[i], st[q], st[q + "_abs"], d["spec"].M, f"{what} {q}")
        else:
            check_exact(tot[i], st[q], f"{what} {q}")


def fwd_checks(run, d, what):
    """bias + none / relu on x, statistics on xs: ``run(x, bias, act, stats) -> (y, slab)``."""
    dv = d["dev"]
    for act in (NONE, RELU):
        y, _ = launch(lambda: run(dv["x"], dv["b"], act, False))
        check_exact(y, want_y(d, act), f"{what} y act {act}")
    y, slab = launch(lambda: run(dv["xs"], None, NONE, True))
    check_exact(y, bf16_round(d["stat"]["y"]), f"{what} y (statistics run)")
    check_stats(slab, d, what)


def names(cases):
    return [c["name"] for c in cases]


# ---------------------------------------------------------------------------
# conv_tile.hip
# ---------------------------------------------------------------------------
def _tile_forward(d, p, what):
    s, dv = d["spec"], d["dev"]
    Kn = _native.kernels()
    fwd_checks(lambda x, b, act, st: ct.conv_fwd(x, dv["w"], b, s, act, st, p), d, what)
    ys = []
    try:
        # static: a workgroup per tile at these sizes, and the launcher does not cap its grid
        # (several tiles per workgroup: test_statistics_rows_of_several_tiles); chunked: a chunk
        # per tile, grabbed by every workgroup or, under cap 1, all walked by one per column block
        # (the two halo buffers, the job ring, the chunk walk)
        for sched, cap in ((0, 0), (1, 0), (1, 1)):
            Kn.conv_tile_set_schedule(sched)
            Kn.conv_tile_grid_cap(cap)
            y, slab = launch(lambda: ct.conv_fwd(dv["xs"], dv["w"], None, s, NONE, True, p))
            check_exact(y, bf16_round(d["stat"]["y"]), f"{what} y sched {sched} cap {cap}")
            check_stats(slab, d, f"{what} sched {sched} cap {cap}")
            ys.append(y)
            assert int(ct.sched(y.device, _native.stream(y)).abs().sum()) == 0, "schedule counters left set"
        Kn.conv_tile_set_schedule(-1)
        Kn.conv_tile_grid_cap(1)                 # without statistics: single tiles from the XCD queues
        y, _ = launch(lambda: ct.conv_fwd(dv["x"], dv["w"], dv["b"], s, RELU, False, p))
        check_exact(y, want_y(d, RELU), f"{what} y relu cap 1")
        assert int(ct.sched(y.device, _native.stream(y)).abs().sum()) == 0, "schedule counters left set"
    finally:
        Kn.conv_tile_grid_cap(0)
        Kn.conv_tile_set_schedule(-1)
    assert all(torch.equal(ys[0], y) for y in ys[1:])


@functools.lru_cache(maxsize=None)
def stat_data(name):
    inp = O.make_inputs(O.BY_NAME[name], O.STAT_BATCH[name])
    s = inp["spec"]
    return {"spec": s, "stat": O.forward(inp["xs"], inp["w"], None, s), "xs": O.banded(inp["xs"], torch.bfloat16, DEV),
            "w": O.banded(inp["w"], torch.float32, DEV)}


def _rows_of_several_tiles(d, slab, dims, what):
    """The static partition gave every slab row three tiles or more, and each row's fp32 sums
    are exact (rows x the largest tile sum < 2^24 steps): the rows add up to the oracle's sums."""
    s = d["spec"]
    nt, rows = O.tile_count(s, dims), slab.shape[0]
    assert nt >= 3 * rows, (nt, rows)
    sa, sq = O.max_tile_sums(bf16_round(d["stat"]["y"]), s, dims)
    per_row = -(-nt // rows)
    assert per_row * sa / O.STEPS["sum_v"] < 2 ** 24 and per_row * sq / O.STEPS["sum_v2"] < 2 ** 24
    tot = slab.double().sum(0).cpu()
    check_exact(tot[0], d["stat"]["sum_v"], f"{what} sum_v over {rows} rows of {per_row} tiles")
    check_exact(tot[1], d["stat"]["sum_v2"], f"{what} sum_v2 over {rows} rows of {per_row} tiles")


@pytest.mark.parametrize("name", sorted(O.STAT_BATCH))
def test_statistics_rows_of_several_tiles(name):
    """The one-GPU production path of the BN statistics: the static schedule with several tiles
    per workgroup, hence per slab row (O.STAT_BATCH) -- conv_tile.hip, and conv_halo.hip's static
    partition.  (Chunks of more than one tile need over 8192 tiles: not covered.)"""
    d = stat_data(name)
    s = d["spec"]
    Kn = _native.kernels()
    ct._PLANS.clear()
    p = ct.fwd_plan(s)
    try:
        Kn.conv_tile_set_schedule(0)
        y, slab = launch(lambda: ct.conv_fwd(d["xs"], d["w"], None, s, NONE, True, p))
    finally:
        Kn.conv_tile_set_schedule(-1)
    check_exact(y, bf16_round(d["stat"]["y"]), f"{name}: tile y at batch {s.N}")
    _rows_of_several_tiles(d, slab, (p.TD, p.TH, p.TW), f"{name}: tile static")
    assert int(ct.sched(y.device, _native.stream(y)).abs().sum()) == 0
    if name in O.STAT_HALO:
        hp = C.halo_fwd_plan(s)
        y, slab = launch(lambda: C.halo_conv_fwd(d["xs"], d["w"], None, s, NONE, True, hp))
        check_exact(y, bf16_round(d["stat"]["y"]), f"{name}: halo y at batch {s.N}")
        _rows_of_several_tiles(d, slab, hp, f"{name}: halo static")


@pytest.mark.parametrize("name", names(O.TILE_CASES))
def test_tile_forward(name, monkeypatch):
    d = data(name)
    s = d["spec"]
    monkeypatch.delenv("FN_TILE_CS", raising=False)
    ct._PLANS.clear()
    p = ct.fwd_plan(s)
    assert p is not None, s
    _tile_forward(d, p, f"{name}: tile CS {p.CS}")
    if name in O.CS32_CASES:                     # 32-channel slices: never the cost model's choice here
        try:
            monkeypatch.setenv("FN_TILE_CS", "32")
            ct._PLANS.clear()
            p32 = ct.fwd_plan(s)
            assert p32 is not None and p32.CS == 32, p32
            _tile_forward(d, p32, f"{name}: tile CS 32")
        finally:
            monkeypatch.delenv("FN_TILE_CS")
            ct._PLANS.clear()


@pytest.mark.parametrize("name", [c["name"] for c in O.STRIDE1_CASES if ct.dgrad_plan(O.make_spec(c)) is not None])
def test_tile_dgrad(name):
    d = data(name)
    s, dv = d["spec"], d["dev"]
    want = bf16_round(d["bwd"]["dx"])
    p = ct.dgrad_plan(s)
    assert p is not None, s
    plans = [p]
    if p.NT == 4:                                # the 32-column form of the same shape too
        plans.append(ct.plan(s.N, (s.D, s.H, s.W), (s.KD, s.KH, s.KW), s.K, s.C))
        assert plans[1] is not None and plans[1].NT == 2
    Kn = _native.kernels()
    try:
        for q in plans:
            for cap in (0, 1):
                Kn.conv_tile_grid_cap(cap)
                dx = launch(lambda: ct.conv_dgrad(dv["dy"], dv["w"], s, q))
                check_exact(dx, want, f"{name}: tile dgrad NT {q.NT} cap {cap}")
                assert int(ct.sched(dx.device, _native.stream(dx)).abs().sum()) == 0
    finally:
        Kn.conv_tile_grid_cap(0)


# ---------------------------------------------------------------------------
# conv_wtile.hip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(O.WTILE_N))
def test_wtile_wgrad(name, monkeypatch):
    """At the batch that gives every worker three jobs or more (O.WTILE_N): dW, three launches
    accumulated into ``out``, and every form of the plan."""
    inp = O.make_inputs(O.BY_NAME[name], O.WTILE_N[name])
    s = inp["spec"]
    want = O.backward(inp["x"], inp["w"], inp["dy"], s, want=("dW",))["dW"]
    x, dy = O.banded(inp["x"], torch.bfloat16, DEV), O.banded(inp["dy"], torch.bfloat16, DEV)
    for k in ("FN_WTILE_KS2", "FN_WTILE_NW"):
        monkeypatch.delenv(k, raising=False)
    cw._PLANS.clear()
    p = cw.plan(s)
    assert p is not None and O.wtile_jobs(p, s) >= 3, p
    dw = launch(lambda: cw.conv_wgrad(dy, x, s, p))
    check_exact(dw.reshape(want.shape), want, f"{name}: wtile dW")
    with Guard():
        out = torch.zeros(s.K, s.taps, s.C, dtype=torch.float32, device=DEV)
        for _ in range(3):
            cw.conv_wgrad(dy, x, s, p, out=out)
    check_exact(out, 3 * want, f"{name}: wtile three launches into out")
    seen = {(p.nw, p.ks2)}
    try:
        for key, val in (("FN_WTILE_KS2", "0"), ("FN_WTILE_KS2", "1"), ("FN_WTILE_NW", "4"), ("FN_WTILE_NW", "8")):
            for k in ("FN_WTILE_KS2", "FN_WTILE_NW"):
                monkeypatch.delenv(k, raising=False)
            monkeypatch.setenv(key, val)
            cw._PLANS.clear()
            q = cw.plan(s)
            if q is None or (q.nw, q.ks2) in seen:           # (the 8-channel form has no 4-wave plan)
                continue
            seen.add((q.nw, q.ks2))
            assert O.wtile_jobs(q, s) >= 3, q
            dw = launch(lambda: cw.conv_wgrad(dy, x, s, q))
            check_exact(dw.reshape(want.shape), want, f"{name}: wtile dW {key}={val} nw {q.nw} ks2 {q.ks2}")
    finally:
        cw._PLANS.clear()


# ---------------------------------------------------------------------------
# conv_halo.hip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", names(O.STRIDE1_CASES))
def test_halo(name):
    """Forward (bias + act, statistics), dgrad and wgrad; among the cases the 8-channel slices,
    the weights-resident short-K form (stem_c8_k4) and tiles narrower than the output."""
    d = data(name)
    s, dv = d["spec"], d["dev"]
    pf, pd, pw = C.halo_fwd_plan(s), C.halo_dgrad_plan(s), C.halo_wgrad_plan(s)
    assert pf is not None, s
    fwd_checks(lambda x, b, act, st: C.halo_conv_fwd(x, dv["w"], b, s, act, st, pf), d, f"{name}: halo")
    if pd is not None:
        dx = launch(lambda: C.halo_conv_dgrad(dv["dy"], dv["w"], s, pd))
        check_exact(dx, bf16_round(d["bwd"]["dx"]), f"{name}: halo dgrad")
    if pw is not None:
        for rep in range(2):                     # exact on these grids, hence repeatable to the bit
            dw = launch(lambda: C.halo_conv_wgrad(dv["dy"], dv["x"], s, pw))
            check_exact(dw.reshape(s.K, s.taps, s.C), d["bwd"]["dW"], f"{name}: halo wgrad, launch {rep}")
    assert int(C.halo_sched(dv["x"].device, _native.stream(dv["x"])).abs().sum()) == 0, "schedule counters left set"


# ---------------------------------------------------------------------------
# conv_igemm.hip
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", names(O.IGEMM_CASES))
def test_igemm(name):
    d = data(name)
    s, dv = d["spec"], d["dev"]
    wmat, ldw = launch(lambda: C.pack_weight_rows(dv["w"], s))
    fwd_checks(lambda x, b, act, st: C.native_conv_fwd(x, wmat, ldw, b, s, act, st), d, f"{name}: igemm")
    dx = launch(lambda: C.native_conv_dgrad(dv["dy"], dv["w"], s))
    check_exact(dx, bf16_round(d["bwd"]["dx"]), f"{name}: igemm dgrad")
    dw = launch(lambda: C.native_conv_wgrad(dv["dy"], dv["x"], s))
    check_exact(dw.reshape(s.K, s.taps, s.C), d["bwd"]["dW"], f"{name}: igemm wgrad")
    r = launch(lambda: C.igemm_wgrad_cropped(dv["dy"], dv["x"], s, s.C, with_db=True))
    assert r is not None
    check_exact(r[0].reshape(s.K, s.taps, s.C), d["bwd"]["dW"], f"{name}: igemm wgrad, cropped")
    check_exact(r[1], d["bwd"]["db"], f"{name}: igemm db")


def test_igemm_channel_padded():
    """12 input channels zero-padded to 16 (what ConvFn does with C % 8 != 0): the vector gather
    over the padded copy, the weight gradient cropped back to 12 channels in the epilogue."""
    name = "ig_lenet_c12_k120"
    d = data(name)
    s, dv, inp = d["spec"], d["dev"], d["inp"]
    sp = O.padded_channels(s, 16)
    assert C.gather_mode(sp) == C.GM_VEC and C.igemm_wgrad_takes(sp)
    xp = torch.zeros(s.N, s.D, s.H, s.W, 16, dtype=torch.float64)
    xp[..., : s.C] = inp["x"]
    xp = O.banded(xp, torch.bfloat16, DEV)
    wmat, ldw = launch(lambda: C.pack_weight_rows(dv["w"], sp))
    for act in (NONE, RELU):
        y, _ = launch(lambda: C.native_conv_fwd(xp, wmat, ldw, dv["b"], sp, act, False))
        check_exact(y, want_y(d, act), f"{name}: padded igemm y act {act}")
    dw = launch(lambda: C.igemm_wgrad_cropped(dv["dy"], xp, sp, s.C))
    assert dw is not None
    check_exact(dw.reshape(s.K, s.taps, s.C), d["bwd"]["dW"], f"{name}: padded igemm wgrad")


@pytest.mark.parametrize("name", O.TANH_CASES)
def test_tanh_epilogue(name):
    """The one bounded quantity: tanh of the exact sum, rounded once (O.BOUNDED)."""
    assert (name, "y_tanh") in O.BOUNDED
    d = data(name)
    s, dv, inp = d["spec"], d["dev"], d["inp"]
    r = torch.tanh(O.forward(inp["xs"], inp["w"], inp["b"], s)["y"])
    if name.startswith("ig_"):
        wmat, ldw = launch(lambda: C.pack_weight_rows(dv["w"], s))
        y, _ = launch(lambda: C.native_conv_fwd(dv["xs"], wmat, ldw, dv["b"], s, ACT_TANH, False))
    else:
        y, _ = launch(lambda: C.halo_conv_fwd(dv["xs"], dv["w"], dv["b"], s, ACT_TANH, False, C.halo_fwd_plan(s)))
    frac = check_one_rounding(y, r, r.abs(), f"{name}: tanh epilogue")
    print(f"{name}: tanh epilogue, worst error / bound {frac:.3f}")


# ---------------------------------------------------------------------------
# the dispatcher: packing, padding and cropping glue
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("act", [NONE, RELU])
@pytest.mark.parametrize("name", ["conv2_c32_k5", "c16_k48_same", "ig_s2_k7_c1", "ig_lenet_c12_k120",
                                  "ig_flat_c3_dil2"])
def test_dispatcher(name, act):
    """ConvFn forward and backward: a tile case, a case whose weight gradient falls to the halo
    kernel, the space-to-depth stem, and two channel-padded ones (C = 12, C = 3)."""
    d = data(name)
    s, dv, inp = d["spec"], d["dev"], d["inp"]
    pre = d["fwd"]["y"]
    g = inp["dy"] * (pre > 0) if act == RELU else inp["dy"]          # relu' at 0 is 0
    bw = O.backward(inp["x"], inp["w"], g, s)
    x = dv["x"].detach().requires_grad_(True)
    w = dv["w"].detach().requires_grad_(True)
    b = dv["b"].detach().requires_grad_(True)
    with Guard():
        y, _ = C.ConvFn.apply(x, w, b, s, act, False)
        assert_guarded(y)
        y.backward(dv["dy"])
    check_exact(y, want_y(d, act), f"{name}: ConvFn y act {act}")
    check_exact(x.grad, bf16_round(bw["dx"]), f"{name}: ConvFn dx act {act}")
    check_exact(w.grad.reshape(s.K, s.taps, s.C), bw["dW"], f"{name}: ConvFn dW act {act}")
    check_exact(b.grad, bw["db"], f"{name}: ConvFn db act {act}")


@pytest.mark.parametrize("name", ["ig_flat_c3_dil2", "ig_lenet_c12_k120"])
def test_dispatcher_first_layer(name):
    """No input gradient wanted (a first layer): the gather weight-gradient kernel applies the relu
    backward as it loads dy and sums the bias gradient itself."""
    d = data(name)
    s, dv, inp = d["spec"], d["dev"], d["inp"]
    bw = O.backward(inp["x"], inp["w"], inp["dy"] * (d["fwd"]["y"] > 0), s, want=("dW",))
    w = dv["w"].detach().requires_grad_(True)
    b = dv["b"].detach().requires_grad_(True)
    with Guard():
        y, _ = C.ConvFn.apply(dv["x"], w, b, s, RELU, False)
        assert_guarded(y)
        y.backward(dv["dy"])
    check_exact(y, want_y(d, RELU), f"{name}: first-layer ConvFn y")
    check_exact(w.grad.reshape(s.K, s.taps, s.C), bw["dW"], f"{name}: first-layer ConvFn dW")
    check_exact(b.grad, bw["db"], f"{name}: first-layer ConvFn db")


def test_one_changed_input_is_seen_through_the_kernels():
    """The comparisons have teeth on real kernel output: with one x value off by one, or one
    weight of one tap negated, at the largest case (4,000 terms per output), what the kernels
    give no longer equals the oracle of the unchanged inputs -- and equals that of the changed ones."""
    name = "conv2_c32_k5"
    d = data(name)
    s, dv, inp = d["spec"], d["dev"], d["inp"]
    x2 = inp["xs"].clone()
    x2[1, 5, 6, 7, 3] += 1.0
    y, slab = launch(lambda: ct.conv_fwd(O.banded(x2, torch.bfloat16, DEV), dv["w"], None, s, NONE, True, ct.fwd_plan(s)))
    with pytest.raises(AssertionError, match="differ"):
        check_exact(y, bf16_round(d["stat"]["y"]), "y, one x changed")
    with pytest.raises(AssertionError, match="differ"):
        check_stats(slab, d, f"{name}: one x changed")
    st2 = O.forward(x2, inp["w"], None, s)
    check_exact(y, bf16_round(st2["y"]), "y against the oracle of the changed x")
    check_stats(slab, {"stat": st2, "spec": s}, f"{name}: the oracle of the changed x")
    w2 = inp["w"].clone()
    w2[17, 2, 3, 1, 9] = -w2[17, 2, 3, 1, 9]
    dx = launch(lambda: ct.conv_dgrad(dv["dy"], O.banded(w2, torch.float32, DEV), s, ct.dgrad_plan(s)))
    with pytest.raises(AssertionError, match="differ"):
        check_exact(dx, bf16_round(d["bwd"]["dx"]), "dx, one weight changed")
    check_exact(dx, bf16_round(O.backward(inp["x"], w2, inp["dy"], s, want=("dx",))["dx"]), "dx against the changed w")
    x3 = inp["x"].clone()
    x3[0, 3, 4, 5, 6] += 1.0
    dw = launch(lambda: cw.conv_wgrad(dv["dy"], O.banded(x3, torch.bfloat16, DEV), s, cw.plan(s)))
    with pytest.raises(AssertionError, match="differ"):
        check_exact(dw.reshape(s.K, s.taps, s.C), d["bwd"]["dW"], "dW, one x changed")
