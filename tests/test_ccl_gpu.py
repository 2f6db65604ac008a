"""The connected-component kernels (``ccl.hip``) and the feature-instance path built on them
(``FeatureNet3DSeg.instances``, ``fn.extract_features``, ``fn.label_components``) on the GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``ops.reference``), and for the
serpentine and the solid volume also against the closed form.  The shapes are built round the
kernel's tile ``ccl_tile() = (TD, TH, TW)``: one clipped tile with W under one 16-byte vector, exactly
one tile (the vector-load path), one voxel more than a tile on every axis, and a 3 x 2 x 3 tile grid
with odd edges; each for one and two samples."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _ccl_cases import PATTERNS, closed_form_table, expected, serpentine_mask, volume  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import ccl, reference  # noqa: E402

DEV = "cuda"


def shapes():
    TD, TH, TW = _native.kernels().ccl_tile()
    return [(3, 5, 7), (TD, TH, TW), (TD + 1, TH + 1, TW + 1), (2 * TD + 1, 2 * TH - 1, 2 * TW + 3)]


def run(lab: torch.Tensor, background, connectivity):
    roots = ccl.connected_components(lab, background, connectivity)
    ids, table, offsets = ccl.instance_table(lab, roots)
    return roots, ids, table, offsets


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("si", range(4), ids=["clipped", "tile", "tile+1", "grid"])
def test_kernels_against_the_oracle(si, N, pattern):
    D, H, W = shapes()[si]
    cpu = volume(pattern, N, D, H, W)
    lab = cpu.to(DEV)
    for connectivity in (6, 26):
        for background in (0, None):
            got = run(lab, background, connectivity)
            again = run(lab, background, connectivity)
            torch.cuda.synchronize()
            want = expected(pattern, N, D, H, W, connectivity, background)
            what = (pattern, N, (D, H, W), connectivity, background)
            for name, g, a, w in zip(("roots", "ids", "table", "offsets"), got, again, want):
                assert g.dtype == w.dtype and g.is_cuda, (what, name)
                diff = int((g.cpu() != w).sum()) if g.shape == w.shape else g.shape
                assert torch.equal(g.cpu(), w), (what, name, diff)
                assert torch.equal(g, a), (what, name, "second run differs")
            fg = cpu.numel() if background is None else int((cpu != background).sum())
            assert int(got[2][:, 2].sum()) == fg, what
            if pattern == "serpentine" and background == 0:         # closed form, no oracle
                m = serpentine_mask(D, H, W)
                rows = np.stack([closed_form_table(m, n, 1) for n in range(N)])
                assert np.array_equal(got[2].cpu().numpy(), rows), what
                assert np.array_equal(got[0].cpu().numpy(), np.broadcast_to(m, (N, D, H, W)).astype(np.int32)), what
            if pattern == "solid":
                rows = np.stack([closed_form_table(np.ones((D, H, W), bool), n, 7) for n in range(N)])
                assert np.array_equal(got[2].cpu().numpy(), rows) and bool((got[0] == 1).all()), what


@pytest.mark.parametrize("connectivity", [6, 26])
def test_outputs_are_fully_rewritten_and_nothing_past_their_end(connectivity):
    """The entry points on buffers pre-filled with -1 and one spare row behind each."""
    N, (D, H, W) = 2, shapes()[3]
    V = D * H * W
    cpu = volume("blobs", N, D, H, W)
    want_roots, want_ids, want_table, _ = expected("blobs", N, D, H, W, connectivity, 0)
    T = len(want_table)
    lab = cpu.to(DEV)
    K, st = _native.kernels(), _native.stream(lab)
    roots, flags, ids = (torch.full((N * V + W,), -1, dtype=torch.int32, device=DEV) for _ in range(3))
    table = torch.full((T + 1, 13), -1, dtype=torch.int64, device=DEV)
    K.ccl_local(lab.data_ptr(), roots.data_ptr(), N, D, H, W, 0, connectivity, st, [N * V, N * V])
    torch.cuda.synchronize()
    r1 = roots[:N * V].view(N, V).cpu()
    assert bool((r1 >= 0).all()) and bool((r1 <= torch.arange(1, V + 1)).all())      # parents never point up
    assert torch.equal(r1 == 0, cpu.view(N, V) == 0)
    K.ccl_merge(lab.data_ptr(), roots.data_ptr(), N, D, H, W, 0, connectivity, st, [N * V, N * V])
    K.ccl_flatten(roots.data_ptr(), flags.data_ptr(), N, D, H, W, st, [N * V, N * V])
    rank = torch.cumsum(flags[:N * V], 0, dtype=torch.int32)
    assert int(rank[-1]) == T
    K.ccl_stats(lab.data_ptr(), roots.data_ptr(), rank.data_ptr(), ids.data_ptr(), table.data_ptr(), N, D, H, W, T, st,
                [N * V, N * V, N * V, N * V, T * 13])
    torch.cuda.synchronize()
    assert torch.equal(roots[:N * V].view(N, D, H, W).cpu(), want_roots)
    assert torch.equal(flags[:N * V].cpu(), (want_roots.view(N, V) == torch.arange(1, V + 1)).view(-1).to(torch.int32))
    assert torch.equal(ids[:N * V].view(N, D, H, W).cpu(), want_ids)
    assert torch.equal(table[:T].cpu(), want_table)
    for buf in (roots, flags, ids):
        assert bool((buf[N * V:] == -1).all())
    assert bool((table[T] == -1).all())
    # the table alone (no ids), again into a dirty buffer
    table.fill_(-1)
    K.ccl_stats(lab.data_ptr(), roots.data_ptr(), rank.data_ptr(), 0, table.data_ptr(), N, D, H, W, T, st,
                [N * V, N * V, N * V, 0, T * 13])
    torch.cuda.synchronize()
    assert torch.equal(table[:T].cpu(), want_table) and bool((table[T] == -1).all())


def test_unsupported_arguments_are_refused():
    lab = torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device=DEV)
    roots = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    K, st = _native.kernels(), _native.stream(lab)
    for conn, bg in ((18, 0), (6, 256), (6, -2)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.ccl_local(lab.data_ptr(), roots.data_ptr(), 1, 4, 4, 4, bg, conn, st, [64, 64])
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.ccl_merge(lab.data_ptr(), roots.data_ptr(), 1, 4, 4, 4, bg, conn, st, [64, 64])
    with pytest.raises(ValueError, match="connectivity"):
        ccl.connected_components(lab, 0, 18)
    with pytest.raises(ValueError):
        ccl.connected_components(lab.float())


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
    return torch.rand(n, S, S, S, generator=g) < 0.4


def gpu_copy(m: FeatureNet3DSeg) -> FeatureNet3DSeg:
    mg = FeatureNet3DSeg(S, num_classes=m.num_classes)
    mg.load_state_dict(m.state_dict())
    return mg.to(DEV).eval()


class _Recorder:
    """Forwards to the real ``_C`` and records the entry points called."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


@pytest.mark.parametrize("subpixel", ["1", "0"], ids=["subpixel", "27tap"])
def test_instances_equal_the_oracle_on_the_predicted_labels(subpixel, monkeypatch):
    monkeypatch.setenv("FN_SUBPIXEL", subpixel)
    mg = gpu_copy(make_model(5))
    x = voxels(2).to(DEV).to(torch.bfloat16)
    labels = mg.predict(x)
    assert len(labels.unique()) > 1
    rec = _Recorder(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    copies = []
    real_cpu, real_to = torch.Tensor.cpu, torch.Tensor.to

    def spy_cpu(t, *a, **k):
        copies.append((t.dtype, tuple(t.shape)))
        return real_cpu(t, *a, **k)

    def spy_to(t, *a, **k):
        out = real_to(t, *a, **k)
        if t.is_cuda and not out.is_cuda:
            copies.append((t.dtype, tuple(t.shape)))
        return out

    monkeypatch.setattr(torch.Tensor, "cpu", spy_cpu)
    monkeypatch.setattr(torch.Tensor, "to", spy_to)
    for connectivity, background in ((6, 0), (26, None)):
        table, offsets, ids = mg.instances(x, background=background, connectivity=connectivity, want_ids=True)
        t2, o2, none = mg.instances(x, background=background, connectivity=connectivity)
        torch.cuda.synchronize()
        assert table.is_cuda and offsets.is_cuda and ids.is_cuda and none is None
        assert torch.equal(t2, table) and torch.equal(o2, offsets)
        cpu_labels = real_cpu(labels)
        roots = reference.connected_components(cpu_labels, background, connectivity)
        want_ids, want_table, want_offsets = reference.instance_table(cpu_labels, roots)
        assert torch.equal(real_cpu(table), want_table) and torch.equal(real_cpu(offsets), want_offsets)
        assert torch.equal(real_cpu(ids), want_ids)
    for name in ("pw_argmax", "ccl_local", "ccl_merge", "ccl_flatten", "ccl_stats"):
        assert rec.calls.count(name) == 4, (name, rec.calls)
    # no per-voxel tensor (labels, roots, ids ...) crossed to the host inside instances()
    assert not [c for c in copies if int(np.prod(c[1])) >= S ** 3], copies


@pytest.mark.parametrize("bs", [1, 3])
def test_extract_features_end_to_end(bs, tmp_path):
    n = 4
    m = make_model(5)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 5})
    xb = voxels(n)
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    feats, ids = fn.extract_features(str(path), packed, batch_size=bs, device=DEV, packed_size=S, return_ids=True)
    labels, _ = fn.segment(str(path), packed, batch_size=bs, device=DEV, packed_size=S)
    want_ids, want = fn.label_components(labels, device=DEV)
    assert len(feats) == n and feats == want
    assert ids.dtype == np.int32 and np.array_equal(ids, want_ids)
    cpu_ids, cpu_feats = fn.label_components(labels, device="cpu")
    assert want == cpu_feats and np.array_equal(want_ids, cpu_ids)
    assert sum(f.voxels for fs in feats for f in fs) == int((labels != 0).sum())
    big, none = fn.extract_features(str(path), packed, batch_size=bs, device=DEV, packed_size=S, min_voxels=10)
    assert none is None and big == [[f for f in fs if f.voxels >= 10] for fs in want]
