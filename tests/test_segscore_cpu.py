"""Segmentation scoring on the CPU reference path: ``reference.confusion``, the ``SegScore`` metrics,
``fn.evaluate_segmentation`` / ``FeatureNet3DSeg.score`` through a module, a checkpoint and bit-packed
input, the CLI subcommand ``score``, and the Python <-> ``_C`` argument plumbing of
``ops.conv.pw_argmax_score``.  All counts are integers and compared exactly; the metrics are float64
ratios of those integers, compared at 1e-12.
"""
import json
import math
import re

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from featurenet_amd import _native
from featurenet_amd.models.featurenet3d import FeatureNet3D, FeatureNet3DConfig, FeatureNet3DSeg
from featurenet_amd.ops import reference
from featurenet_amd.utils.segmetrics import SegScore

S, NC, N = 16, 3, 5


def _loop_confusion(truth, pred, n, ignore=None):
    out = [0] * (n * n + 1)
    for t, p in zip(truth, pred):
        if ignore is not None and t == ignore:
            continue
        if t >= n:
            out[n * n] += 1
        else:
            out[t * n + p] += 1
    return out


def test_reference_confusion_against_a_double_loop():
    g = torch.Generator().manual_seed(0)
    n = 4
    truth = torch.randint(0, n + 3, (5, 41), generator=g)          # holds n, n + 1, n + 2: out of range
    pred = torch.randint(0, n, (5, 41), generator=g).to(torch.uint8)
    tl, pl = truth.reshape(-1).tolist(), pred.reshape(-1).tolist()
    for ignore in (None, 1, n, n + 2, 200):
        got = reference.confusion(truth, pred, n, ignore)
        assert got.dtype == torch.int64 and got.shape == (n * n + 1,)
        assert got.tolist() == _loop_confusion(tl, pl, n, ignore), ignore
    assert int(reference.confusion(truth, pred, n)[n * n]) == int((truth >= n).sum()) > 0
    assert reference.confusion(truth.to(torch.uint8), pred, n, 1).tolist() == _loop_confusion(tl, pl, n, 1)
    empty = reference.confusion(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.uint8), n)
    assert empty.tolist() == [0] * (n * n + 1)


def test_segscore_fields_against_their_definitions():
    rng = np.random.default_rng(1)
    n = 6
    truth = rng.integers(0, n - 1, 5000)                            # class n - 1 never occurs in truth ...
    pred = rng.integers(0, n, 5000)
    pred[pred == 2] = 3                                             # ... label 2 is never given
    cm = np.zeros((n, n), np.int64)
    np.add.at(cm, (truth, pred), 1)
    s = SegScore.from_confusion(cm)
    assert np.array_equal(s.confusion, cm) and s.confusion.dtype == np.int64
    assert s.voxels == 5000
    assert math.isclose(s.accuracy, float((truth == pred).mean()), rel_tol=0, abs_tol=1e-12)
    iou = []
    for c in range(n):
        tp = int(((truth == c) & (pred == c)).sum())
        sup, prd = int((truth == c).sum()), int((pred == c).sum())
        assert s.support[c] == sup and s.predicted[c] == prd
        for name, num, den in (("iou", tp, sup + prd - tp), ("precision", tp, prd), ("recall", tp, sup),
                               ("dice", 2 * tp, sup + prd)):
            got = getattr(s, name)[c]
            assert got.dtype == np.float64
            if den == 0:
                assert np.isnan(got), (name, c)
            else:
                assert np.allclose(got, num / den, rtol=0, atol=1e-12), (name, c)
        if sup + prd - tp > 0:
            iou.append(tp / (sup + prd - tp))
    assert np.isnan(s.precision[2]) and not np.isnan(s.recall[2])   # never predicted
    assert np.isnan(s.recall[n - 1]) and s.iou[n - 1] == 0.0        # only predicted: IoU 0, counted in mIoU
    assert len(iou) == n and np.allclose(s.miou, np.mean(iou), rtol=0, atol=1e-12)


def test_segscore_nan_handling_and_json():
    cm = np.zeros((4, 4), np.int64)
    cm[0, 0], cm[0, 1], cm[1, 1], cm[1, 3] = 7, 1, 5, 2            # class 2: nowhere; class 3: only predicted
    s = SegScore.from_confusion(cm)
    assert np.isnan(s.iou[2]) and np.isnan(s.precision[2]) and np.isnan(s.recall[2]) and np.isnan(s.dice[2])
    assert s.iou[3] == 0.0 and s.precision[3] == 0.0 and np.isnan(s.recall[3])
    want = (7 / 8 + 5 / 8 + 0.0) / 3                                # class 2 is excluded from the mean
    assert np.allclose(s.miou, want, rtol=0, atol=1e-12)
    d = json.loads(json.dumps(s.to_dict()))
    assert d["iou"][2] is None and d["iou"][3] == 0.0 and d["recall"][3] is None
    assert d["confusion"] == cm.tolist() and d["voxels"] == 15 and d["support"] == [8, 7, 0, 0]
    assert np.allclose(d["miou"], want, rtol=0, atol=1e-12) and np.allclose(d["accuracy"], 12 / 15, rtol=0, atol=1e-12)
    none = SegScore.from_confusion(np.zeros((2, 2), np.int64))      # nothing counted at all
    assert np.isnan(none.accuracy) and np.isnan(none.miou)
    assert json.loads(json.dumps(none.to_dict()))["miou"] is None
    with pytest.raises(ValueError):
        SegScore.from_confusion(np.zeros((2, 3), np.int64))


def _lowest_argmax(logits: torch.Tensor) -> torch.Tensor:
    """Explicit scan from class 0 with a strict > (independent of reference.lowest_argmax)."""
    best = logits[..., 0].clone()
    idx = torch.zeros(logits.shape[:-1], dtype=torch.uint8)
    for c in range(1, logits.shape[-1]):
        m = logits[..., c] > best
        best = torch.where(m, logits[..., c], best)
        idx = torch.where(m, torch.full_like(idx, c), idx)
    return idx


@pytest.fixture(scope="module")
def seg():
    torch.manual_seed(0)
    m = FeatureNet3DSeg(S, num_classes=NC).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for c in list(m.enc) + [m.dec]:          # running statistics / affine away from the identity
            c.running_mean.copy_(torch.randn(c.cout, generator=g) * 0.1)
            c.running_var.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.gamma.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.beta.copy_(torch.randn(c.cout, generator=g) * 0.1)
        m.head.bias.copy_(torch.randn(NC, generator=g) * 0.1)
    x = (torch.rand(N, S, S, S, generator=g) < 0.4)
    y = torch.randint(0, NC, (N, S, S, S), generator=g)
    with torch.no_grad():
        pred = _lowest_argmax(m(x.float())).numpy()
    cm = np.zeros((NC, NC), np.int64)
    np.add.at(cm, (y.numpy().reshape(-1), pred.reshape(-1)), 1)
    return m, x, y, pred, cm


def test_evaluate_segmentation_matches_model_argmax(seg, tmp_path):
    m, x, y, pred, cm = seg
    assert len(np.unique(pred)) > 1                       # (not a degenerate all-one-class model)
    s = fn.evaluate_segmentation(m, x.numpy().astype(np.uint8), y.numpy(), batch_size=2, device="cpu")
    assert isinstance(s, SegScore) and np.array_equal(s.confusion, cm)
    assert s.voxels == N * S ** 3 and np.allclose(s.accuracy, (pred == y.numpy()).mean(), rtol=0, atol=1e-12)
    # through a checkpoint, int32 labels
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    s2 = fn.evaluate_segmentation(str(path), x.numpy().astype(np.float32), y.numpy().astype(np.int32), device="cpu")
    assert np.array_equal(s2.confusion, cm)
    # bit-packed input, uint8 labels, ignore_index: that class's row is empty
    packed = np.packbits(x.numpy().reshape(N, -1), axis=1, bitorder="little")
    s3 = fn.evaluate_segmentation(m, packed, y.numpy().astype(np.uint8), batch_size=4, packed_size=S, ignore_index=1,
                                  device="cpu")
    want = cm.copy()
    want[1] = 0
    assert np.array_equal(s3.confusion, want) and s3.voxels == int(want.sum())
    # labels the model has no class for: refused, unless masked
    y_bad = y.numpy().copy()
    y_bad[0, 0, 0, :3] = NC + 4
    with pytest.raises(ValueError, match=r"3 voxels.*ignore_index"):
        fn.evaluate_segmentation(m, x.numpy().astype(np.uint8), y_bad, device="cpu")
    s4 = fn.evaluate_segmentation(m, x.numpy().astype(np.uint8), y_bad, ignore_index=NC + 4, device="cpu")
    assert s4.voxels == N * S ** 3 - 3
    for off in (-1, 256):                                  # values no uint8 label can hold
        y_bad[0, 0, 0, 0] = off
        with pytest.raises(ValueError, match="0..255"):
            fn.evaluate_segmentation(m, x.numpy().astype(np.uint8), y_bad, device="cpu")


def test_score_accumulates_and_returns_labels(seg):
    m, x, y, pred, cm = seg
    m = m.cpu()
    acc, labels = m.score(x[:2].float(), y[:2], want_labels=True)
    assert acc.dtype == torch.int64 and acc.shape == (NC * NC + 1,)
    assert labels.dtype == torch.uint8 and np.array_equal(labels.numpy(), pred[:2])
    out, none = m.score(x[2:].float(), y[2:], acc=acc)
    assert out is acc and none is None
    assert np.array_equal(acc[:-1].reshape(NC, NC).numpy(), cm) and int(acc[-1]) == 0
    with pytest.raises(ValueError):
        m.score(x[:1].float(), torch.full((1, S, S, S), 300))
    with pytest.raises(ValueError):
        m.score(x[:1].float(), y[:1].float())


def test_error_cases():
    clf = FeatureNet3D(FeatureNet3DConfig.tiny())
    with pytest.raises(ValueError):
        fn.evaluate_segmentation(clf, np.zeros((1, 16, 16, 16), np.float32), np.zeros((1, 16, 16, 16), np.uint8))
    m = FeatureNet3DSeg(S, num_classes=NC).train()
    with pytest.raises(RuntimeError):
        m.score(torch.zeros(1, S, S, S), torch.zeros(1, S, S, S, dtype=torch.long))
    assert "evaluate_segmentation" in fn.__all__


def test_cli_score(seg, tmp_path, capsys):
    from featurenet_amd.cli import main

    m, x, y, pred, cm = seg
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    np.save(tmp_path / "x.npy", x.numpy().astype(np.uint8))
    np.save(tmp_path / "y.npy", y.numpy().astype(np.uint8))
    out = tmp_path / "score.json"
    assert main(["score", str(path), str(tmp_path / "x.npy"), str(tmp_path / "y.npy"), "--json", str(out)]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary == json.loads(out.read_text())
    assert summary["voxels"] == N * S ** 3 and len(summary["iou"]) == NC
    assert np.array(summary["confusion"]).sum() == N * S ** 3
    if not torch.cuda.is_available():                    # (the checkpoint loads onto the GPU when there is one)
        assert summary["confusion"] == cm.tolist()
        assert np.allclose(summary["miou"], SegScore.from_confusion(cm).miou, rtol=0, atol=1e-12)
    assert main(["score", str(path), str(tmp_path / "x.npy"), str(tmp_path / "y.npy"), "--ignore-index", "2"]) == 0
    masked = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert masked["support"][2] == 0 and masked["voxels"] == N * S ** 3 - int((y == 2).sum())


# --- Python <-> _C plumbing of ops.conv.pw_argmax_score (the technique of tests/test_native_abi.py) -----
def _arity(fn_) -> tuple[int, int]:
    sig = fn_.__doc__.split("\n")[0]
    inner = sig[sig.index("(") + 1:sig.rindex(") ->")]
    depth, parts, cur = 0, [], ""
    for ch in inner:
        depth += ch in "[(" and 1 or 0
        depth -= ch in "])" and 1 or 0
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur)
    return sum("=" not in p for p in parts), len(parts)


class _FakeK:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        lo, hi = _arity(getattr(self.real, name))

        def f(*args):
            assert lo <= len(args) <= hi, f"{name}: called with {len(args)} args, binding takes {lo}..{hi}"
            self.calls.append((name, args))
            return 3 if re.search(r"_blocks$", name) else None
        return f


def test_pw_argmax_score_call_matches_binding(monkeypatch):
    if not _native.kernels_available():
        pytest.skip("_C not built")
    import importlib

    C = importlib.import_module("featurenet_amd.ops.conv")     # (ops.conv the attribute is the function)
    fk = _FakeK(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: fk)
    monkeypatch.setattr(_native, "stream", lambda t=None: 0)
    x = torch.zeros(264, 32, dtype=torch.bfloat16)
    w, b = torch.zeros(25, 32), torch.zeros(25)
    truth = torch.zeros(264, dtype=torch.int64)
    acc, labels = C.pw_argmax_score(x, w, b, truth)
    assert acc.dtype == torch.int64 and acc.shape == (626,) and labels is None
    mine = torch.zeros(626, dtype=torch.int64)
    acc, labels = C.pw_argmax_score(x, w, None, truth, pro=(torch.ones(32), torch.zeros(32), 1), ignore_index=7,
                                    acc=mine, want_labels=True)
    assert acc is mine and labels.dtype == torch.uint8 and labels.shape == (264,)
    assert [n for n, _ in fk.calls] == ["pw_argmax_cm_blocks", "pw_argmax_cm"] * 2
    assert fk.calls[0][1] == (264, 32, 25)
    a0, a1 = fk.calls[1][1], fk.calls[3][1]
    # x w bias truth labels part acc M K N ignore psc psh pact stream ext
    assert a0[2] != 0 and a0[3] != 0 and a0[4] == 0 and a0[5] != 0 and a0[6] != 0
    assert a0[7:11] == (264, 32, 25, -1) and a0[11] == 0 and a0[12] == 0
    assert a0[-1] == [264 * 32, 264, 0, 3 * 626, 626]
    assert a1[2] == 0 and a1[4] == labels.data_ptr() and a1[6] == mine.data_ptr()
    assert a1[10] == 7 and a1[11] != 0 and a1[12] != 0 and a1[13] == 1
    assert a1[-1] == [264 * 32, 264, 264, 3 * 626, 626]
    with pytest.raises(ValueError):                               # a wrong-sized running matrix
        C.pw_argmax_score(x, w, b, truth, acc=torch.zeros(625, dtype=torch.int64))


def test_pw_argmax_cm_extent_check():
    """bind.cpp checks the operand extents before any launch."""
    if not _native.kernels_available():
        pytest.skip("_C not built")
    K = _native.kernels()
    M, Kc, Nc = 264, 32, 25
    blocks = K.pw_argmax_cm_blocks(M, Kc, Nc)
    assert blocks == 2                                             # ceil(264 / 256) tiles, below any grid cap
    good = [M * Kc, M, 0, blocks * 626, 626]

    def call(ext, labels=0, shape=(M, Kc, Nc), ignore=-1):
        K.pw_argmax_cm(0, 0, 0, 16, labels, 16, 16, *shape, ignore, 0, 0, 0, 0, ext)

    for i, name in ((0, "x"), (1, "truth"), (3, "part"), (4, "acc")):
        ext = list(good)
        ext[i] -= 1
        with pytest.raises(RuntimeError, match=f"{name} has"):
            call(ext)
    with pytest.raises(RuntimeError, match="labels has"):
        call([M * Kc, M, M - 1, blocks * 626, 626], labels=16)
    for bad in ((264, 72, 25), (264, 32, 65), (260, 32, 25)):      # K / N > 64, M % 8: negative code
        Mb, Kb, Nb = bad
        ext = [Mb * Kb, Mb, 0, K.pw_argmax_cm_blocks(*bad) * (Nb * Nb + 1), Nb * Nb + 1]
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            call(ext, shape=bad)
    for ignore in (-2, 256):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            call(good, ignore=ignore)
