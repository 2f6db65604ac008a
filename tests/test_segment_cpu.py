"""``fn.segment`` / ``FeatureNet3DSeg.predict`` on the CPU reference path: per-voxel labels with
the lowest-index tie rule, through a module, a checkpoint and bit-packed input, the CLI
subcommand, and the Python <-> ``_C`` argument plumbing of ``ops.conv.pw_argmax``.
"""
import json
import re

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from featurenet_amd import _native
from featurenet_amd.models.featurenet3d import FeatureNet3D, FeatureNet3DConfig, FeatureNet3DSeg
from featurenet_amd.ops import reference

S, NC, N = 16, 3, 5


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
    with torch.no_grad():
        logits = m(x.float())
    return m, x, logits


def test_segment_matches_model_argmax(seg, tmp_path):
    m, x, logits = seg
    want = _lowest_argmax(logits).numpy()
    labels, conf = fn.segment(m, x.numpy().astype(np.uint8), batch_size=2)
    assert conf is None
    assert labels.dtype == np.uint8 and labels.shape == (N, S, S, S)
    assert np.array_equal(labels, want)
    assert len(np.unique(labels)) > 1                     # (not a degenerate all-one-class model)
    # [N, S, S, S, 1] float input, confidence
    labels2, conf = fn.segment(m, x.float().unsqueeze(-1).numpy(), batch_size=3, return_confidence=True)
    assert np.array_equal(labels2, want)
    assert conf.dtype == np.float32 and conf.shape == (N, S, S, S)
    ref_conf = torch.softmax(logits, -1).max(-1).values.numpy()
    assert np.abs(conf - ref_conf).max() <= 1e-6
    # through a checkpoint
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    labels3, _ = fn.segment(str(path), x.numpy().astype(np.float32), device="cpu")
    assert np.array_equal(labels3, want)
    # bit-packed input
    packed = np.packbits(x.numpy().reshape(N, -1), axis=1, bitorder="little")
    labels4, _ = fn.segment(m, packed, batch_size=4, packed_size=S)
    assert np.array_equal(labels4, want)


def test_segment_rejects_classifiers():
    clf = FeatureNet3D(FeatureNet3DConfig.tiny())
    with pytest.raises(ValueError):
        fn.segment(clf, np.zeros((1, 16, 16, 16), np.float32))
    net, _ = fn.build_model("lenet5", (28, 28, 1), 10)
    with pytest.raises(ValueError):
        fn.segment(net, np.zeros((1, 28, 28, 1), np.float32))


def test_predict_needs_eval_mode():
    m = FeatureNet3DSeg(S, num_classes=NC).train()
    with pytest.raises(RuntimeError):
        m.predict(torch.zeros(1, S, S, S))


def test_head_argmax_ties_go_to_the_lowest_index():
    g = torch.Generator().manual_seed(3)
    K, Nc = 32, 12
    w = torch.randn(Nc, K, generator=g)
    b = torch.randn(Nc, generator=g) * 0.1
    w[3] = w[7] = w.abs().sum(0)                         # rows 3 and 7 identical ...
    b[3] = b[7] = b.max() + 1.0                          # ... equal bias, and the largest logit
    x = torch.rand(64, K, generator=g) + 0.5             # positive inputs: rows 3 / 7 dominate
    labels, conf = reference.head_argmax(x, w, b)
    assert labels.dtype == torch.uint8 and conf.dtype == torch.float32
    assert torch.all(labels == 3)
    labels, conf = reference.head_argmax(torch.zeros(8, K), w, torch.zeros(Nc))
    assert torch.all(labels == 0)
    assert torch.allclose(conf, torch.full((8,), 1.0 / Nc))
    # prologue: relu(x * scale + shift) with a shift that zeroes every channel -> all logits tie
    labels, _ = reference.head_argmax(x, w, None, pro=(torch.ones(K), torch.full((K,), -10.0), "relu"))
    assert torch.all(labels == 0)


def test_cli_segment_writes_labels(seg, tmp_path, capsys):
    from featurenet_amd.cli import main

    m, x, logits = seg
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    np.save(tmp_path / "x.npy", x.numpy().astype(np.uint8))
    out, cout = tmp_path / "labels.npy", tmp_path / "conf.npy"
    assert main(["segment", str(path), str(tmp_path / "x.npy"), "-o", str(out), "--confidence", str(cout)]) == 0
    labels = np.load(out)
    assert labels.dtype == np.uint8 and labels.shape == (N, S, S, S)
    conf = np.load(cout)
    assert conf.dtype == np.float32 and conf.shape == (N, S, S, S)
    if not torch.cuda.is_available():                    # (the checkpoint loads onto the GPU when there is one)
        assert np.array_equal(labels, _lowest_argmax(logits).numpy())
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["shape"] == [N, S, S, S]
    assert len(summary["counts"]) == NC and sum(summary["counts"]) == labels.size


# --- Python <-> _C plumbing of ops.conv.pw_argmax (the technique of tests/test_native_abi.py) ----------
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
            return 1 if re.search(r"_blocks$", name) else None
        return f


def test_pw_argmax_call_matches_binding(monkeypatch):
    if not _native.kernels_available():
        pytest.skip("_C not built")
    import importlib

    C = importlib.import_module("featurenet_amd.ops.conv")     # (ops.conv the attribute is the function)
    fk = _FakeK(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: fk)
    monkeypatch.setattr(_native, "stream", lambda t=None: 0)
    x = torch.zeros(264, 32, dtype=torch.bfloat16)
    w, b = torch.zeros(25, 32), torch.zeros(25)
    labels, conf = C.pw_argmax(x, w, b)
    assert labels.dtype == torch.uint8 and labels.shape == (264,) and conf is None
    labels, conf = C.pw_argmax(x, w, None, pro=(torch.ones(32), torch.zeros(32), 1), want_conf=True)
    assert conf.dtype == torch.bfloat16 and conf.shape == (264,)
    assert [n for n, _ in fk.calls] == ["pw_argmax", "pw_argmax"]
    a0, a1 = fk.calls[0][1], fk.calls[1][1]
    assert a0[4] == 0 and a0[8] == 0 and a0[9] == 0          # no conf, no prologue: null pointers
    assert a1[2] == 0 and a1[4] != 0 and a1[8] != 0 and a1[10] == 1
    assert a1[5:8] == (264, 32, 25) and a1[-1] == [264 * 32, 264, 264]


def test_pw_argmax_extent_check():
    """bind.cpp checks the operand extents before any HIP call."""
    if not _native.kernels_available():
        pytest.skip("_C not built")
    K = _native.kernels()
    with pytest.raises(RuntimeError, match="x has"):
        K.pw_argmax(0, 0, 0, 0, 0, 264, 32, 25, 0, 0, 0, 0, [264 * 32 - 1, 264, 0])
    with pytest.raises(RuntimeError, match="labels has"):
        K.pw_argmax(0, 0, 0, 0, 0, 264, 32, 25, 0, 0, 0, 0, [264 * 32, 263, 0])
    with pytest.raises(RuntimeError, match="conf has"):
        K.pw_argmax(0, 0, 0, 0, 16, 264, 32, 25, 0, 0, 0, 0, [264 * 32, 264, 8])
    for bad in ((264, 72, 25), (264, 32, 65), (260, 32, 25)):      # K / N > 64, M % 8: negative code
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.pw_argmax(0, 0, 0, 16, 0, *bad, 0, 0, 0, 0, [bad[0] * bad[1], bad[0], 0])
