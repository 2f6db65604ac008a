"""The Dense kernels -- csrc/kernels/dense.hip -- against the float64 oracle of
tests/_dense_oracle.py, kernel family by kernel family, bit for bit.

Each family's own entry point is called (``Kn.dense_fwd`` with the test's own split count and
slabs, ``Kn.dense_dgrad``, ``Kn.dense_wgrad``), so the dispatcher cannot route around a path; the
dispatcher (``LinearFn``, ``linear_infer``) has a test of its own.  Inputs lie on the dyadic
grids of the oracle's docstring, which make every fp32 sum of the kernels exact in any order: y
and dx are ``bf16_round(oracle)`` (the oracle as fp32 with ``out_fp32``), dW and db the oracle
itself, and ``check_exact`` allows nothing else.  The fp32 master weights are not bf16 values:
a quarter of them is an exact tie that the kernels' conversion has to round to nearest even.
The bounded quantities are the tanh and the sigmoid forward epilogue (``O.BOUNDED``,
``check_one_rounding``; tests/test_dense_oracle_cpu.py keeps that list honest).

Guard bands (tests/_guard.py): inputs sit in the middle of flat buffers whose ends hold a large
finite sentinel (``O.banded``).  Every launch runs inside ``KeepGuard``: each device tensor
allocated through ``torch.empty`` / ``torch.zeros`` while it is open -- the outputs, the forward's
``part`` slabs and the weight gradient's slice workspace here, and in the dispatcher tests also
what ``LinearFn`` and ``linear_infer`` allocate that way themselves -- has a NaN middle and
pattern ends, and is held until the guard exits, so the bands of scratch that the callee has
already dropped are checked too (``test_guard_*`` below show both).  An output slot nobody wrote
is a NaN that fails the comparison, and a write outside any of these tensors fails the band check.

Not covered: ``dense_wgrad_kernel<2>`` (128 columns per workgroup) is unreachable -- ``nb`` is
the constant 1 in ``fn_dense_wgrad`` -- and is not tested; ``dn_ncw``'s second rule (K < 512
with 256 or more 128 x 128 tiles) needs 32,768 rows; the workload sizes themselves are the
business of tests/test_kernels_gpu.py.

``FN_DENSE_ORACLE_REPORT=<file>`` writes one JSON line per check (case, template instance, check,
observed / bound): the source of profiles/dense_oracle.md.
"""
import functools
import importlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import _dense_oracle as O  # noqa: E402
from _bn_pool_oracle import bf16_round, check_exact, check_one_rounding  # noqa: E402
import _guard  # noqa: E402
from _guard import KeepGuard, assert_guarded, launch_kept  # noqa: E402
from featurenet_amd import _native  # noqa: E402

L = importlib.import_module("featurenet_amd.ops.linear")    # (ops.linear itself is the function)
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
_REC = []


def _rec(case, inst, check, frac):
    _REC.append({"case": case, "instance": inst, "check": check, "frac": float(frac)})


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("FN_DENSE_ORACLE_REPORT")
    if path:
        with open(path, "w") as f:
            for r in _REC:
                f.write(json.dumps(r) + "\n")


def _ids(cases):
    return [c["name"] for c in cases]


@functools.lru_cache(maxsize=None)
def shape_data(M, N, K, need):
    """Inputs of a shape, on the CPU (float64) and banded on the device; worked out once."""
    inp = O.make_inputs({"M": M, "N": N, "K": K}, need=need)
    dv = {k: O.banded(v, F32 if k in ("w", "b") else BF, DEV) for k, v in inp.items()}
    if "w" in inp:
        dv["wh"] = O.banded(bf16_round(inp["w"]), BF, DEV)           # the inference copy
    return inp, dv


def _ya(c):
    if not c["ya"]:
        return None, None
    ya = O.make_inputs(c, need=("ya",))["ya"]
    return ya, O.banded(ya, BF, DEV)


def _check_y(y, f, c, what, inst):
    """y against the oracle: bit for bit, or the one-rounding bound for tanh / sigmoid."""
    r = f["y"]
    if (c["name"], "y") in O.BOUNDED:
        assert c["act"] in (O.TANH, O.SIGMOID)
        keep = r.abs() >= O.SOFT_TINY            # (a sigmoid below the normal range: see the oracle)
        frac = check_one_rounding(y, r, r.abs(), what, keep=keep.to(y.device))
        tiny = y.double().cpu()[~keep]
        assert bool(((tiny >= 0) & (tiny <= 2 * O.SOFT_TINY)).all()), f"{what}: outputs below the normal range"
        _rec(c["name"], inst, "y one rounding", frac)
        print(f"{what}: worst error / bound {frac:.4f}")
    else:
        assert c["act"] in (O.NONE, O.RELU)
        _rec(c["name"], inst, "y exact", check_exact(y, r.float().double() if c["out_fp32"] else bf16_round(r), what))


# ---------------------------------------------------------------------------
# the guard itself: scratch dropped inside a launch is still checked, and a band write is seen
# ---------------------------------------------------------------------------
def _live():
    return [f for f in (ref() for ref, _ in _guard._LIVE) if f is not None]


def test_guard_keeps_dropped_scratch_until_the_band_check():
    _guard.check_bands()
    before = len(_live())
    with KeepGuard():
        torch.empty(3, 5, dtype=F32, device=DEV)             # dropped at once, like a callee's workspace
        torch.empty(7, dtype=BF, device=DEV)
        assert len(_live()) == before + 2
    _guard.check_bands()                                     # (released after the guard has exited)
    assert len(_live()) == before


@pytest.mark.parametrize("where", ["front", "behind"])
def test_guard_sees_a_write_next_to_dropped_scratch(where):
    n = 24
    i = O.BAND - 1 if where == "front" else O.BAND + n
    with pytest.raises(AssertionError, match="wrote in front" if where == "front" else "wrote behind"):
        with KeepGuard():
            flat = torch.empty(n, dtype=F32, device=DEV)._base       # (the view itself is dropped at once)
            good = float(flat[i])
            flat[i] = 0.0
    flat[i] = good                               # (whatever still refers to the buffer, its bands are whole again)
    del flat
    _guard.check_bands()


# ---------------------------------------------------------------------------
# forward: dense_fwd_part_kernel<VEC, D, WB, NCW, FINAL> and dense_fwd_reduce_kernel
# ---------------------------------------------------------------------------
def _fwd_instance(c, S, wbf16):
    p = O.fwd_plan(c["M"], c["N"], c["K"], S)
    inst = (f"dense_fwd_part<{'true' if p['vec'] else 'false'}, {p['D']}, {'true' if wbf16 else 'false'}, "
            f"{p['ncw']}, {'true' if p['Sr'] == 1 else 'false'}>")
    return inst + (f" + dense_fwd_reduce (S {p['Sr']})" if p["Sr"] > 1 else "")


def _run_fwd(x, w, b, M, N, K, S, act, out_fp32, wbf16):
    Kn = _native.kernels()
    part = torch.empty(S, M, N, dtype=F32, device=DEV)
    y = torch.empty(M, N, dtype=F32 if out_fp32 else BF, device=DEV)
    Kn.dense_fwd(x.data_ptr(), w.data_ptr(), _native.ptr(b), y.data_ptr(), part.data_ptr(), M, N, K, S, act,
                 int(out_fp32), _native.stream(x), [x.numel(), w.numel(), y.numel(), part.numel()], wbf16)
    return y


@pytest.mark.parametrize("wbf16", [0, 1], ids=["w_fp32", "w_bf16"])
@pytest.mark.parametrize("c", O.FWD_CASES, ids=_ids(O.FWD_CASES))
def test_forward(c, wbf16):
    M, N, K = c["M"], c["N"], c["K"]
    Kn = _native.kernels()
    S = int(Kn.dense_splits(M, N, K)) if c["S"] is None else c["S"]
    inp, dv = shape_data(M, N, K, ("x", "w", "b"))
    f = O.forward(inp["x"], inp["w"], inp["b"] if c["bias"] else None, c["act"])
    y = launch_kept(lambda: _run_fwd(dv["x"], dv["wh" if wbf16 else "w"], dv["b"] if c["bias"] else None, M, N, K, S,
                                c["act"], c["out_fp32"], wbf16))
    _check_y(y, f, c, f"{c['name']} wbf16 {wbf16}", _fwd_instance(c, S, wbf16))


# ---------------------------------------------------------------------------
# dgrad: dense_dgrad_kernel
# ---------------------------------------------------------------------------
def _run_dgrad(g, w, M, N, K, ya, act):
    dx = torch.empty(M, K, dtype=BF, device=DEV)
    _native.kernels().dense_dgrad(g.data_ptr(), w.data_ptr(), dx.data_ptr(), M, N, K, _native.stream(g),
                                  [g.numel(), w.numel(), dx.numel()] + ([ya.numel()] if ya is not None else []),
                                  _native.ptr(ya), act if ya is not None else 0)
    return dx


@pytest.mark.parametrize("c", O.DGRAD_CASES, ids=_ids(O.DGRAD_CASES))
def test_dgrad(c):
    M, N, K = c["M"], c["N"], c["K"]
    inp, dv = shape_data(M, N, K, ("w", "dy"))
    ya64, ya = _ya(c)
    want = O.backward(None, inp["w"], O.g_prime(inp["dy"], ya64, c["ya"]), want=("dx",))["dx"]
    dx = launch_kept(lambda: _run_dgrad(dv["dy"], dv["w"], M, N, K, ya, c["ya"]))
    p = O.dgrad_plan(M, N, K)
    _rec(c["name"], f"dense_dgrad (mrep {p['mrep']}, NP {p['NP']}, LDS {p['lds']} B)", "dx exact",
         check_exact(dx, bf16_round(want), c["name"]))


def test_dgrad_refuses_what_does_not_fit_in_lds():
    """N = 1280 needs 164,864 B of LDS: the launcher returns -4, which the binding raises, and dx
    stays as it was."""
    M, N, K = O.DGRAD_REFUSED
    inp, dv = shape_data(M, N, K, ("w", "dy"))
    with KeepGuard():
        dx = torch.empty(M, K, dtype=BF, device=DEV)
        with pytest.raises(RuntimeError, match="-4"):
            _native.kernels().dense_dgrad(dv["dy"].data_ptr(), dv["w"].data_ptr(), dx.data_ptr(), M, N, K,
                                          _native.stream(dx), [M * N, N * K, M * K], 0, 0)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx).all()), "a refused launch wrote dx"


# ---------------------------------------------------------------------------
# wgrad: dense_wgrad_kernel<1> (+ fn_part_reduce2 over batch slices)
# ---------------------------------------------------------------------------
def _run_wgrad(g, x, M, N, K, S, with_db, ya, act):
    dw = torch.empty(N, K, dtype=F32, device=DEV)
    db = torch.empty(N, dtype=F32, device=DEV) if with_db else None
    part = torch.empty(S * (N * K + N), dtype=F32, device=DEV) if S > 1 else None    # (NaN beforehand)
    _native.kernels().dense_wgrad(g.data_ptr(), x.data_ptr(), dw.data_ptr(), _native.ptr(db), M, N, K,
                                  _native.stream(g), [g.numel(), x.numel(), dw.numel(), part.numel() if S > 1 else 0,
                                                      ya.numel() if ya is not None else 0],
                                  _native.ptr(part), S, _native.ptr(ya), act if ya is not None else 0)
    return (dw, db) if with_db else (dw,)


@pytest.mark.parametrize("c", O.WGRAD_CASES, ids=_ids(O.WGRAD_CASES))
def test_wgrad(c):
    M, N, K = c["M"], c["N"], c["K"]
    inp, dv = shape_data(M, N, K, ("x", "dy"))
    ya64, ya = _ya(c)
    gp = O.g_prime(inp["dy"], ya64, c["ya"])
    want = O.backward(inp["x"], None, gp, want=("dW",))
    out = launch_kept(lambda: _run_wgrad(dv["dy"], dv["x"], M, N, K, c["S"], c["db"], ya, c["ya"]))
    p = O.wgrad_plan(M, N, K, c["S"])
    inst = f"dense_wgrad<1> (slices {p['Sr']}, MCH {p['MCH']}, chunks {p['chunks'][0]}, LDS {p['lds']} B)"
    _rec(c["name"], inst, "dW exact", check_exact(out[0], want["dW"], f"{c['name']} dW"))
    if c["db"]:
        _rec(c["name"], inst, "db exact", check_exact(out[1], want["db"], f"{c['name']} db"))


# ---------------------------------------------------------------------------
# the host functions against their mirrors
# ---------------------------------------------------------------------------
def _all_shapes():
    cases = O.FWD_CASES + O.DGRAD_CASES + O.WGRAD_CASES + O.DISPATCH_CASES
    return sorted({(c["M"], c["N"], c["K"]) for c in cases} | set(O.INFER_SHAPES) | {O.SPLITS_FC1, O.DGRAD_REFUSED})


def test_dense_splits_matches_its_mirror():
    Kn = _native.kernels()
    assert Kn.dense_splits(*O.SPLITS_FC1) == 128             # FC1: 2 column tiles x 128 slices, a workgroup per CU
    for s in _all_shapes():
        assert Kn.dense_splits(*s) == O.dense_splits(*s), s


def test_dense_wgrad_slices_matches_its_mirror():
    Kn = _native.kernels()
    assert Kn.dense_wgrad_slices(*O.SPLITS_FC1) == 1
    for s in _all_shapes() + [(300, 24, 40), (1024, 84, 120), (16384, 84, 120)]:
        assert Kn.dense_wgrad_slices(*s) == O.dense_wgrad_slices(*s), s


# ---------------------------------------------------------------------------
# the dispatcher: LinearFn (forward and torch.autograd.grad) and linear_infer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", O.DISPATCH_CASES, ids=_ids(O.DISPATCH_CASES))
def test_dispatcher(c):
    """A ya-path layer, a layer above K = 4096 (the separate act_bwd pass) and an fp32-output layer
    without activation.  y comes from the kernel here, so relu or none only."""
    M, N, K = c["M"], c["N"], c["K"]
    inp, dv = shape_data(M, N, K, ("x", "w", "b", "dy"))
    f = O.forward(inp["x"], inp["w"], inp["b"] if c["bias"] else None, c["act"])
    gp = O.g_prime(inp["dy"], bf16_round(f["y"]) if c["act"] else None, c["act"])
    bw = O.backward(inp["x"], inp["w"], gp)
    x = dv["x"].detach().requires_grad_(True)
    w = dv["w"].detach().requires_grad_(True)
    b = dv["b"].detach().requires_grad_(True) if c["bias"] else None
    dy = O.banded(inp["dy"], F32 if c["out_fp32"] else BF, DEV)
    with KeepGuard():
        y = L.LinearFn.apply(x, w, b, c["act"], c["out_fp32"])
        assert_guarded(y)
        grads = torch.autograd.grad(y, (x, w) + ((b,) if b is not None else ()), dy)
        assert_guarded(grads)
    assert y.dtype == (F32 if c["out_fp32"] else BF)
    _check_y(y, f, c, f"{c['name']} y", "LinearFn")
    _rec(c["name"], "LinearFn", "dx exact", check_exact(grads[0], bf16_round(bw["dx"]), f"{c['name']} dx"))
    _rec(c["name"], "LinearFn", "dW exact", check_exact(grads[1], bw["dW"], f"{c['name']} dW"))
    if b is not None:
        _rec(c["name"], "LinearFn", "db exact", check_exact(grads[2], bw["db"], f"{c['name']} db"))


@pytest.mark.parametrize("shape", O.INFER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_infer(shape):
    M, N, K = shape
    inp, dv = shape_data(M, N, K, ("x", "w", "b"))
    f = O.forward(inp["x"], inp["w"], inp["b"], O.RELU)
    y = launch_kept(lambda: L.linear_infer(dv["x"], dv["wh"], dv["b"], "relu"))
    _rec(f"infer-{M}x{N}x{K}", f"linear_infer (NCW {O.dn_ncw(M, N, K)})", "y exact",
         check_exact(y, bf16_round(f["y"]), f"linear_infer {shape}"))
