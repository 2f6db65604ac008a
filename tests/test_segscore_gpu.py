"""The scoring instances of the fused 1x1 head + arg-max kernel (``pw_argmax_kernel<.., CM>`` +
``cm_accumulate_kernel``) and what is built on them (``ops.conv.pw_argmax_score``,
``FeatureNet3DSeg.score``, ``fn.evaluate_segmentation``) on the GPU.

Every count is an integer, so every check is exact equality: the confusion matrix must be the
``bincount`` of (truth, label) pairs where the labels are what the unchanged ``pw_argmax`` returns for
the same inputs (its numerics are covered against the fp64 oracle in ``tests/test_segment_gpu.py``).
Shapes are the smallest that reach every path: one partial tile, exactly one tile, a tile plus an
8-row tail, and one more tile than the launch grid, so a workgroup walks two tiles and adds both into
its histogram.
"""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import reference, subpixel  # noqa: E402

C = importlib.import_module("featurenet_amd.ops.conv")

DEV = "cuda"
KN = [(32, 25), (32, 5), (8, 2), (64, 64)]
PRO = [None, 0, 1]                                # none, BN only, BN + ReLU


def make_inputs(M, K, N, pro, bias, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    b = (0.1 * torch.randn(N, generator=g)).to(DEV) if bias else None
    p = None
    if pro is not None:
        psc = (torch.rand(K, generator=g) + 0.5).to(DEV)
        psh = (0.3 * torch.randn(K, generator=g)).to(DEV)
        p = (psc, psh, pro)
    return x, w, b, p


def make_truth(M, hi, seed):
    """uint8 [M], uniform on [0, hi)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, hi, (M,), generator=g).to(torch.uint8).to(DEV)


def pair_counts(truth, labels, N):
    return torch.bincount(truth.long() * N + labels.long(), minlength=N * N)


def grid_blocks(K, N):
    return int(_native.kernels().pw_argmax_cm_blocks(1 << 30, K, N))


def m_values(K, N):
    return [8, 256, 264, 256 * (grid_blocks(K, N) + 1) + 8]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("pro", PRO, ids=["plain", "bn", "bnrelu"])
@pytest.mark.parametrize("kn", KN, ids=lambda kn: f"k{kn[0]}n{kn[1]}")
def test_matrix_is_the_bincount_of_pw_argmax_labels(kn, pro, bias):
    K, N = kn
    for i, M in enumerate(m_values(K, N)):
        x, w, b, p = make_inputs(M, K, N, pro, bias, 200 + i)
        truth = make_truth(M, N, 300 + i)
        assert C.pw_argmax_ok(M, K, N, p)
        L, _ = C.pw_argmax(x, w, b, pro=p)
        acc, none = C.pw_argmax_score(x, w, b, truth, pro=p)
        acc2, labels = C.pw_argmax_score(x, w, b, truth, pro=p, want_labels=True)
        torch.cuda.synchronize()
        assert none is None and acc.dtype == torch.int64 and acc.shape == (N * N + 1,)
        want = pair_counts(truth, L, N)
        assert torch.equal(acc[:N * N], want), (M, int((acc[:N * N] != want).sum()))
        assert int(acc[N * N]) == 0
        assert int(acc.sum()) == M
        assert labels.dtype == torch.uint8 and torch.equal(labels, L), (M, int((labels != L).sum()))
        assert torch.equal(acc2, acc)


@pytest.mark.parametrize("pro", [None, 1], ids=["plain", "bnrelu"])
@pytest.mark.parametrize("kn", KN, ids=lambda kn: f"k{kn[0]}n{kn[1]}")
def test_ignore_index_and_out_of_range(kn, pro):
    K, N = kn
    for i, M in enumerate(m_values(K, N)[2:]):
        x, w, b, p = make_inputs(M, K, N, pro, True, 400 + i)
        L, _ = C.pw_argmax(x, w, b, pro=p)
        # truth uniform on [0, N], N ignored: those rows appear nowhere
        truth = make_truth(M, N + 1, 500 + i)
        keep = truth < N
        acc, _ = C.pw_argmax_score(x, w, b, truth, pro=p, ignore_index=N)
        assert torch.equal(acc[:N * N], pair_counts(truth[keep], L[keep], N))
        assert int(acc[N * N]) == 0 and int(acc.sum()) == int(keep.sum()) and int(keep.sum()) < M
        # the same truth without ignore_index: the rows with truth == N are out of range
        acc, _ = C.pw_argmax_score(x, w, b, truth, pro=p)
        assert torch.equal(acc[:N * N], pair_counts(truth[keep], L[keep], N))
        assert int(acc[N * N]) == M - int(keep.sum()) and int(acc.sum()) == M
        # an ignore_index below N: that class's row is empty, the others are untouched
        ig = N // 2
        acc, _ = C.pw_argmax_score(x, w, b, truth, pro=p, ignore_index=ig)
        want = pair_counts(truth[keep], L[keep], N).reshape(N, N).clone()
        assert int(want[ig].sum()) > 0
        want[ig] = 0
        assert torch.equal(acc[:N * N].reshape(N, N), want)
        assert int(acc[N * N]) == M - int(keep.sum())
        # truth holding N + 1 (and no ignore_index): slot N*N and nowhere else
        t2 = make_truth(M, N, 600 + i)
        bad = torch.arange(M, device=DEV) % 7 == 3
        t2[bad] = N + 1
        acc, _ = C.pw_argmax_score(x, w, b, t2, pro=p)
        assert int(acc[N * N]) == int(bad.sum())
        assert torch.equal(acc[:N * N], pair_counts(t2[~bad], L[~bad], N))


@pytest.mark.parametrize("kn", [(32, 25), (64, 64)], ids=lambda kn: f"k{kn[0]}n{kn[1]}")
def test_contended_bin(kn):
    """All-zero input and bias: every class ties at 0, the label is 0; with truth 0 every row of every
    wave adds to the one slot 0."""
    K, N = kn
    M = m_values(K, N)[-1]
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    _, w, _, _ = make_inputs(8, K, N, None, False, 9)
    acc, _ = C.pw_argmax_score(x, w, torch.zeros(N, device=DEV), torch.zeros(M, dtype=torch.uint8, device=DEV))
    assert int(acc[0]) == M
    assert int(acc[1:].abs().sum()) == 0


def _raw_call(x, w, b, truth, part, acc, ignore=-1):
    M, K = x.shape
    N = w.shape[0]
    _native.kernels().pw_argmax_cm(x.data_ptr(), w.data_ptr(), b.data_ptr(), truth.data_ptr(), 0, part.data_ptr(),
                                   acc.data_ptr(), M, K, N, ignore, 0, 0, 0, _native.stream(x),
                                   [x.numel(), truth.numel(), 0, part.numel(), acc.numel()])


def test_accumulates_and_rewrites_the_whole_slab():
    K, N = 32, 25
    M = m_values(K, N)[-1]
    x, w, b, p = make_inputs(M, K, N, 1, True, 21)
    truth = make_truth(M, N, 22)
    once, _ = C.pw_argmax_score(x, w, b, truth, pro=p)
    acc = torch.zeros(N * N + 1, dtype=torch.int64, device=DEV)
    out, _ = C.pw_argmax_score(x, w, b, truth, pro=p, acc=acc)
    out, _ = C.pw_argmax_score(x, w, b, truth, pro=p, acc=acc)
    assert out is acc and torch.equal(acc, 2 * once)
    # the raw entry point with a slab full of 0xFF bytes (and one row to spare) and a small M whose grid
    # is a single workgroup as well: every launched workgroup rewrites every slot of its row
    for Ms in (M, 264):
        xs, ts = x[:Ms].contiguous(), truth[:Ms].contiguous()
        blocks = int(_native.kernels().pw_argmax_cm_blocks(Ms, K, N))
        clean = torch.zeros(blocks * (N * N + 1), dtype=torch.int32, device=DEV)
        dirty = torch.full(((blocks + 1) * (N * N + 1),), -1, dtype=torch.int32, device=DEV)
        a0 = torch.zeros(N * N + 1, dtype=torch.int64, device=DEV)
        a1 = torch.zeros(N * N + 1, dtype=torch.int64, device=DEV)
        _raw_call(xs, w, b, ts, clean, a0)
        _raw_call(xs, w, b, ts, dirty, a1)
        torch.cuda.synchronize()
        assert torch.equal(a0, a1) and int(a0.sum()) == Ms
        assert torch.all(dirty[blocks * (N * N + 1):] == -1)            # (and nothing beyond its rows)
        assert torch.equal(dirty[:blocks * (N * N + 1)], clean)


def test_kernel_is_repeatable():
    K, N = 32, 25
    M = m_values(K, N)[-1]
    x, w, b, p = make_inputs(M, K, N, 1, True, 11)
    truth = make_truth(M, N, 12)
    a1, _ = C.pw_argmax_score(x, w, b, truth, pro=p)
    a2, _ = C.pw_argmax_score(x, w, b, truth, pro=p)
    assert torch.equal(a1, a2)


class _Recorder:
    """Forwards to the real ``_C`` and records the entry points called."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


@pytest.mark.parametrize("shape", [(4096, 72, 25), (4100, 32, 25)], ids=["k72", "m4100"])
def test_unsupported_shape_takes_the_fallback(shape, monkeypatch):
    M, K, N = shape
    x, w, b, _ = make_inputs(M, K, N, None, True, 7)
    truth = make_truth(M, N + 1, 8)
    assert not C.pw_argmax_ok(M, K, N)
    Kn = _native.kernels()
    blocks = int(Kn.pw_argmax_cm_blocks(M, K, N))
    part = torch.zeros(blocks * (N * N + 1), dtype=torch.int32, device=DEV)
    acc = torch.zeros(N * N + 1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported configuration"):      # the kernel refuses it
        _raw_call(x, w, b, truth, part, acc)
    rec = _Recorder(Kn)
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    acc, labels = C.pw_argmax_score(x, w, b, truth, ignore_index=3, want_labels=True)
    torch.cuda.synchronize()
    assert "pw_argmax_cm" not in rec.calls and rec.calls
    assert labels.dtype == torch.uint8 and labels.shape == (M,)
    assert acc.dtype == torch.int64 and acc.is_cuda
    assert torch.equal(acc, reference.confusion(truth, labels, N, 3))
    assert int(acc[N * N]) == int((truth == N).sum()) > 0 and int(acc[3 * N:4 * N].sum()) == 0


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
S = 32


def make_model(nc: int, seed: int = 0) -> FeatureNet3DSeg:
    """A CPU fp32 model whose BN folds are not the identity."""
    torch.manual_seed(seed)
    m = FeatureNet3DSeg(S, num_classes=nc).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for c in list(m.enc) + [m.dec]:
            c.running_mean.copy_(torch.randn(c.cout, generator=g) * 0.1)
            c.running_var.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.gamma.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.beta.copy_(torch.randn(c.cout, generator=g) * 0.1)
        m.head.bias.copy_(torch.randn(nc, generator=g) * 0.1)
    return m


def voxels(n: int, seed: int = 3) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, S, S, S, generator=g) < 0.4)


def true_labels(n: int, nc: int, seed: int = 4) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, nc, (n, S, S, S), generator=g)


def gpu_copy(m: FeatureNet3DSeg) -> FeatureNet3DSeg:
    mg = FeatureNet3DSeg(S, num_classes=m.num_classes)
    mg.load_state_dict(m.state_dict())
    return mg.to(DEV).eval()


@pytest.mark.parametrize("subpix", [True, False], ids=["subpixel", "taps27"])
@pytest.mark.parametrize("nc", [25, 5])
def test_score_is_the_bincount_of_predict(nc, subpix, monkeypatch):
    if not subpix:
        monkeypatch.setenv("FN_SUBPIXEL", "0")
    mg = gpu_copy(make_model(nc))
    x = voxels(2).to(DEV).to(torch.bfloat16)
    y = true_labels(2, nc)                                    # int64, on the host
    with torch.no_grad():
        z = x.unsqueeze(-1)
        for c in mg.enc:
            z = c(z)
        assert subpixel.infer_ok(z, mg.dec.cout, z.shape[-1]) == subpix      # (the path under test is taken)
    rec = _Recorder(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    acc, none = mg.score(x, y)
    assert rec.calls.count("pw_argmax_cm") == 1 and "pw_argmax" not in rec.calls
    labels = mg.predict(x)
    torch.cuda.synchronize()
    assert none is None and acc.shape == (nc * nc + 1,) and acc.dtype == torch.int64
    want = pair_counts(y.to(DEV).reshape(-1), labels.reshape(-1), nc)
    assert torch.equal(acc[:nc * nc], want) and int(acc[nc * nc]) == 0
    assert len(labels.unique()) > 1
    acc2, lab2 = mg.score(x, y.to(torch.uint8).to(DEV), acc=acc.clone(), want_labels=True)
    assert torch.equal(lab2, labels) and torch.equal(acc2, 2 * acc)


@pytest.mark.parametrize("bs", [1, 3])
def test_evaluate_segmentation_end_to_end(bs, tmp_path):
    n, nc = 5, 5
    m = make_model(nc)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": nc})
    xb = voxels(n)
    y = true_labels(n, nc).numpy()
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    score = fn.evaluate_segmentation(str(path), packed, y, batch_size=bs, device=DEV, packed_size=S)
    labels, _ = fn.segment(str(path), packed, batch_size=bs, device=DEV, packed_size=S)
    want = np.bincount(y.reshape(-1) * nc + labels.reshape(-1).astype(np.int64), minlength=nc * nc).reshape(nc, nc)
    assert score.confusion.dtype == np.int64 and np.array_equal(score.confusion, want)
    assert score.voxels == n * S ** 3 and score.accuracy == np.trace(want) / want.sum()
    y_bad = y.copy()
    y_bad[1, 2, 3, 4] = nc + 2
    with pytest.raises(ValueError, match="ignore_index"):
        fn.evaluate_segmentation(str(path), packed, y_bad, batch_size=bs, device=DEV, packed_size=S)
    masked = fn.evaluate_segmentation(str(path), packed, y_bad, batch_size=bs, device=DEV, packed_size=S,
                                      ignore_index=nc + 2)
    assert masked.voxels == n * S ** 3 - 1
