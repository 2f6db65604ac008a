"""The overlap-table kernel (``overlap.hip``) and the feature-matching path built on it
(``ops.overlap``, ``FeatureNet3DSeg.match``, ``fn.evaluate_features``, ``fn.match_features``) on the
GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``reference.overlap_table``), each
kernel result taken twice.  The ids come from the CPU oracle of the label patterns of
``_ccl_cases`` (volume ``a`` split with 6-connectivity, ``b`` with 26 -- with 6 where ``a`` is solid,
which keeps ``noise4`` in ~1,100 pieces) and are moved to the device.
The shapes are built round ``overlap_chunk() = (CHUNK, SLOTS)``: rows shorter than a wave, exactly
one chunk per sample, V no multiple of CHUNK (chunks straddle rows and the sample boundary) and
many chunks; each for one and two samples.

Pairs per chunk at the shapes with V >= CHUNK (from the oracle): ``noise4`` / ``blobs`` and
``solid`` / ``noise4`` 1,000-1,300 (more than SLOTS: LDS conflicts go straight to the global
table), ``checker`` / ``blobs`` ~3,000 with every run of length 1, ``blobs`` / ``blobs`` <= ~160
(everything meets in LDS).  ``checker`` / ``blobs`` has P = 50,616 at the largest shape with N = 2,
but ``checker`` alone has 66,810 instances there, so the wrapper's first table (2 x the instance
counts, rounded up) already holds it; ``slabs`` -- z planes against x planes, D + W instances but
D * W pairs per sample -- is the case that makes the table grow."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _ccl_cases import expected  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import overlap, reference  # noqa: E402
from featurenet_amd.utils.featscore import FeatureScore  # noqa: E402

DEV = "cuda"
PAIRS = [("noise4", "blobs"), ("solid", "noise4"), ("checker", "blobs"), ("blobs", "blobs"), ("solid", "solid"),
         ("empty", "blobs"), ("samples", "solid"), ("wrap", "solid"), ("slabs", "slabs")]


def conn_b(pa: str) -> int:
    return 6 if pa == "solid" else 26


def shapes():
    chunk, slots = _native.kernels().overlap_chunk()
    assert (chunk, slots) == (4096, 512)         # the shapes below are built round these
    return [(3, 5, 7), (8, 8, 64), (9, 9, 65), (17, 15, 131)]


def ids_of(pattern: str, side: int, N: int, D: int, H: int, W: int, connectivity: int | None = None):
    """(ids int32 [N, D, H, W], offsets int64 [N + 1], rows) on the CPU; side 0 = volume a (6-connectivity
    unless given), 1 = b (26).  ``slabs``: side 0 numbers the z planes, side 1 the x planes."""
    if pattern == "slabs":
        z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
        per = D if side == 0 else W
        ids = torch.from_numpy(np.broadcast_to((z if side == 0 else x) + 1, (N, D, H, W)).astype(np.int32))
        return ids.contiguous(), torch.arange(N + 1, dtype=torch.int64) * per, N * per
    _, ids, table, offsets = expected(pattern, N, D, H, W, connectivity or (6 if side == 0 else 26), 0)
    return ids, offsets, len(table)


class _Recorder:
    """Forwards to the real ``_C`` and records the entry points called."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


@pytest.mark.parametrize("pa,pb", PAIRS, ids=["-".join(p) for p in PAIRS])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("si", range(4), ids=["short-rows", "chunk", "chunk+", "many"])
def test_kernel_against_the_oracle(si, N, pa, pb, monkeypatch):
    D, H, W = shapes()[si]
    ids_a, off_a, Ta = ids_of(pa, 0, N, D, H, W)
    ids_b, off_b, Tb = ids_of(pb, 1, N, D, H, W, conn_b(pa))
    want = reference.overlap_table(ids_a, off_a, ids_b, off_b)
    what = (pa, pb, N, (D, H, W))
    rec = _Recorder(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    dev = [t.to(DEV) for t in (ids_a, off_a, ids_b, off_b)]
    got = overlap.overlap_table(*dev)
    launches = rec.calls.count("overlap_pairs")
    again = overlap.overlap_table(*dev, rows=(Ta, Tb))
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got.cpu(), want), (what, int((got.cpu() != want).sum()))
    assert torch.equal(got, again), (what, "second run differs")
    assert int(got[:, 2].sum()) == int(((ids_a > 0) & (ids_b > 0)).sum()), what
    assert launches >= 1, (what, rec.calls)
    if pa == "empty":
        assert len(got) == 0
    if (pa, pb) == ("solid", "solid"):           # one pair per sample; the samples' equal ids must not merge
        assert got.tolist() == [[n, n, D * H * W] for n in range(N)], what
    if pa == "slabs":
        assert len(got) == N * D * W and bool((got[:, 2] == H).all()), what
        if si == 3:                              # D * W = 2,227 pairs per sample in a first table of 1,024: it grows
            assert len(got) > max(overlap.MIN_CAP, overlap._next_pow2(2 * (Ta + Tb))) and launches > 1, what


def test_the_issues_counts():
    """The pair counts the cases were chosen for."""
    def P(pa, pb, N, shape):
        a, b = ids_of(pa, 0, N, *shape), ids_of(pb, 1, N, *shape, conn_b(pa))
        return len(reference.overlap_table(a[0], a[1], b[0], b[1]))

    assert P("noise4", "blobs", 2, (8, 8, 64)) == 2185 and P("checker", "blobs", 2, (17, 15, 131)) == 50616
    assert 1000 <= P("noise4", "blobs", 1, (8, 8, 64)) <= 1300 and 1000 <= P("solid", "noise4", 1, (8, 8, 64)) <= 1300
    assert P("blobs", "blobs", 1, (8, 8, 64)) <= 160 and P("checker", "blobs", 1, (8, 8, 64)) > 2500


def test_identical_volumes_give_the_diagonal():
    N, (D, H, W) = 2, shapes()[3]
    _, ids, table, off = expected("blobs", N, D, H, W, 26, 0)
    got = overlap.overlap_table(ids.to(DEV), off.to(DEV), ids.to(DEV), off.to(DEV))
    T = len(table)
    assert torch.equal(got.cpu(), torch.stack([torch.arange(T), torch.arange(T), table[:, 2]], 1))


# ---------------------------------------------------------------------------------------------
# binding level
# ---------------------------------------------------------------------------------------------
def launch(ids_a, off_a, ids_b, off_b, cap, probe, W=None, ext=None):
    """One ``overlap_pairs`` call into a zeroed table with one spare element (-1) behind keys and counts."""
    N, V = ids_a.shape[0], ids_a[0].numel()
    keys, counts = (torch.zeros(cap + 1, dtype=torch.int64, device=DEV) for _ in range(2))
    keys[cap], counts[cap] = -1, -1
    lost = torch.tensor([0, -1], dtype=torch.int64, device=DEV)
    K, st = _native.kernels(), _native.stream(ids_a)
    K.overlap_pairs(ids_a.data_ptr(), ids_b.data_ptr(), off_a.data_ptr(), off_b.data_ptr(), keys.data_ptr(),
                    counts.data_ptr(), lost.data_ptr(), N, V, ids_a.shape[-1] if W is None else W, cap, probe, st,
                    ext or [ids_a.numel(), ids_b.numel(), off_a.numel(), off_b.numel(), cap, cap, 1])
    torch.cuda.synchronize()
    assert int(keys[cap]) == -1 and int(counts[cap]) == -1 and int(lost[1]) == -1, "written past the end"
    return keys[:cap].cpu(), counts[:cap].cpu(), int(lost[0])


def oracle_keys(want: torch.Tensor) -> dict:
    return {((ra + 1) << 32) | (rb + 1): c for ra, rb, c in want.tolist()}


def test_a_table_that_is_large_enough_holds_every_pair_and_nothing_past_its_end():
    N, (D, H, W) = 2, shapes()[2]
    a, b = ids_of("noise4", 0, N, D, H, W), ids_of("blobs", 1, N, D, H, W)
    want = oracle_keys(reference.overlap_table(a[0], a[1], b[0], b[1]))
    cap = 8192
    assert len(want) < cap // 2
    keys, counts, lost = launch(a[0].to(DEV), a[1].to(DEV), b[0].to(DEV), b[1].to(DEV), cap, 256)
    assert lost == 0
    occupied = keys != 0
    assert dict(zip(keys[occupied].tolist(), counts[occupied].tolist())) == want
    assert bool((counts[~occupied] == 0).all())


def test_a_table_that_is_too_small_loses_voxels_and_says_so():
    N, (D, H, W) = 2, shapes()[1]
    a, b = ids_of("noise4", 0, N, D, H, W), ids_of("blobs", 1, N, D, H, W)
    want = oracle_keys(reference.overlap_table(a[0], a[1], b[0], b[1]))
    assert len(want) == 2185
    cap = 64
    keys, counts, lost = launch(a[0].to(DEV), a[1].to(DEV), b[0].to(DEV), b[1].to(DEV), cap, cap)
    both = int(((a[0] > 0) & (b[0] > 0)).sum())
    assert lost > 0
    assert int(counts.sum()) + lost == both      # conservation, whatever the order of the atomics
    occupied = keys != 0
    assert bool(occupied.all()) and len(set(keys.tolist())) == cap
    for k, c in zip(keys.tolist(), counts.tolist()):
        assert k in want and 0 < c <= want[k], (k, c)


def test_unsupported_arguments_are_refused():
    N, (D, H, W) = 1, shapes()[1]
    a, b = ids_of("blobs", 0, N, D, H, W), ids_of("blobs", 1, N, D, H, W)
    dev = [t.to(DEV) for t in (a[0], a[1], b[0], b[1])]
    for cap, probe, w in ((48, 48, W), (1, 1, W), (64, 64, 7), (64, 0, W)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            launch(*dev, cap, probe, W=w)
    with pytest.raises(RuntimeError, match="keys has 32 elements"):
        launch(*dev, 64, 64, ext=[D * H * W, D * H * W, 2, 2, 32, 64, 1])
    with pytest.raises(RuntimeError, match="off_b has 1 elements"):
        launch(*dev, 64, 64, ext=[D * H * W, D * H * W, 2, 1, 64, 64, 1])
    ids, off = dev[0], dev[1]
    with pytest.raises(ValueError, match="int32"):
        overlap.overlap_table(ids.long(), off, ids, off)
    with pytest.raises(ValueError, match="ids_b must be"):
        overlap.overlap_table(ids, off, ids[:, :4], off)
    with pytest.raises(ValueError, match="offsets"):
        overlap.overlap_table(ids, off[:1], ids, off)
    with pytest.raises(ValueError, match="ids_b must be"):
        overlap.overlap_table(ids, off, ids.cpu(), off)


# ---------------------------------------------------------------------------------------------
# model level (the model of test_ccl_gpu.py)
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


def truth_for(labels: torch.Tensor) -> torch.Tensor:
    """True labels that agree with ``labels`` in part: two slabs relabelled, one emptied."""
    y = labels.clone()
    y[:, :5] = 0
    y[:, 12:16, :, :16] = 2
    y[:, :, 20:23] = 1
    return y


def test_match_equals_the_oracle_on_the_predicted_labels(monkeypatch):
    mg = gpu_copy(make_model(5))
    x = voxels(2).to(DEV).to(torch.bfloat16)
    labels = mg.predict(x)
    assert len(labels.unique()) > 1
    y = truth_for(labels)
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
    cpu_labels, cpu_y = real_cpu(labels), real_cpu(y)
    for connectivity, background in ((6, 0), (26, None)):
        got = mg.match(x, y, background=background, connectivity=connectivity)
        torch.cuda.synchronize()
        want = []
        for vol in (cpu_labels, cpu_y):
            ids, table, off = reference.instance_table(vol, reference.connected_components(vol, background,
                                                                                           connectivity))
            want += [table, off, ids]
        pairs = reference.overlap_table(want[2], want[1], want[5], want[4])
        assert len(pairs) > 0
        for g, w in zip(got, (want[0], want[1], want[3], want[4], pairs)):
            assert g.is_cuda and g.dtype == torch.int64 and torch.equal(real_cpu(g), w), (connectivity, background)
    assert rec.calls.count("overlap_pairs") >= 2 and rec.calls.count("ccl_stats") == 4, rec.calls
    # no per-voxel tensor (labels, roots, ids ...) crossed to the host inside match()
    assert not [c for c in copies if int(np.prod(c[1])) >= S ** 3], copies
    with pytest.raises(ValueError, match="uint8"):
        mg.match(x, y.int())


@pytest.mark.parametrize("bs", [1, 3])
def test_evaluate_features_end_to_end(bs, tmp_path):
    n = 4
    m = make_model(5)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 5})
    xb = voxels(n)
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    labels, _ = fn.segment(str(path), packed, batch_size=bs, device=DEV, packed_size=S)
    y = truth_for(torch.from_numpy(labels)).numpy()
    for kw in ({}, {"connectivity": 26, "min_voxels": 4, "iou_threshold": 0.6}):
        got = fn.evaluate_features(str(path), packed, y.astype(np.int64), batch_size=bs, device=DEV, packed_size=S, **kw)
        want = fn.match_features(labels, y, device="cpu", **kw)
        assert isinstance(got, FeatureScore) and got.to_dict() == want.to_dict(), kw
        assert fn.match_features(labels, y, device=DEV, **kw).to_dict() == want.to_dict(), kw
        assert len(got.matches) == n and int(got.tp.sum()) > 0 and int(got.fp.sum()) > 0 and int(got.fn.sum()) > 0
    # the model's own labels as the truth: every instance finds itself
    own = fn.evaluate_features(str(path), packed, labels, batch_size=bs, device=DEV, packed_size=S)
    _, feats = fn.label_components(labels, device="cpu")
    assert int(own.tp.sum()) == sum(len(f) for f in feats) > 0
    assert not own.fp.any() and not own.fn.any()
    assert bool((own.sq[own.tp > 0] == 1.0).all()) and own.mpq == 1.0 and own.msq == 1.0
    with pytest.raises(ValueError, match="label volumes"):
        fn.evaluate_features(str(path), packed, y[:2], device=DEV, packed_size=S)
