"""The access-direction kernels (``access.hip``) and the paths built on them
(``FeatureNet3DSeg.instances(want_access=True)``, ``fn.extract_features(access=True)``,
``fn.label_components(occupancy=)``) on the GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``ops.reference``).  The shapes put a row
under one wave, on exactly one wave, one lane over, and on two 64-wide pieces plus a remainder; the
largest one also spans two workgroups' chunks of the flat voxel range, the first ending mid-row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _access_cases import expected_access, fully_open_toward_truth, occupancy, singles  # noqa: E402
from _ccl_cases import PATTERNS  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import access, reference  # noqa: E402

DEV = "cuda"
SHAPES = [(3, 5, 7), (4, 6, 64), (5, 3, 65), (9, 7, 130)]


def run_bindings(ids: torch.Tensor, offsets: torch.Tensor, occ: torch.Tensor, T: int, want_mask: bool = True):
    """The two entry points on buffers pre-filled with -1 (0xFF) with one spare row behind each ->
    (ex, ey, ez, acc, mask or None); asserts that nothing past the outputs' ends was touched."""
    N, D, H, W = ids.shape
    K, st = _native.kernels(), _native.stream(ids)
    sizes = (N * D * H * 2, N * D * W * 2, N * H * W * 2)
    ex, ey, ez = (torch.full((n + 2 * W,), -1, dtype=torch.int32, device=DEV) for n in sizes)
    acc = torch.full((T + 1, 8), -1, dtype=torch.int64, device=DEV)
    mask = torch.full((ids.numel() + W,), 255, dtype=torch.uint8, device=DEV) if want_mask else None
    K.access_extents(occ.data_ptr(), ex.data_ptr(), ey.data_ptr(), ez.data_ptr(), N, D, H, W, st,
                     [occ.numel(), *sizes])
    K.access_stats(ids.data_ptr(), offsets.data_ptr(), ex.data_ptr(), ey.data_ptr(), ez.data_ptr(), _native.ptr(mask),
                   acc.data_ptr(), N, D, H, W, T, st,
                   [ids.numel(), N + 1, *sizes, ids.numel() if want_mask else 0, T * 8])
    torch.cuda.synchronize()
    for buf, n in zip((ex, ey, ez), sizes):
        assert bool((buf[n:] == -1).all())
    assert bool((acc[T] == -1).all()) and (mask is None or bool((mask[ids.numel():] == 255).all()))
    return (ex[:sizes[0]].view(N, D, H, 2), ey[:sizes[1]].view(N, D, W, 2), ez[:sizes[2]].view(N, H, W, 2), acc[:T],
            mask[:ids.numel()].view(ids.shape) if want_mask else None)


def check_against(got, want, what):
    for name, g, w in zip(("ex", "ey", "ez", "acc", "mask"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.is_cuda, (what, name)
        assert torch.equal(g.cpu(), w), (what, name, int((g.cpu() != w).sum()))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("si", range(4), ids=["under-a-wave", "one-wave", "wave+1", "two-pieces+rest"])
def test_kernels_against_the_oracle(si, N, pattern):
    D, H, W = SHAPES[si]
    ids_c, table, offsets_c, occ_c, *want = expected_access(pattern, N, D, H, W)
    ids, offsets, occ = ids_c.to(DEV), offsets_c.to(DEV), occ_c.to(DEV)
    T, what = len(table), (pattern, N, (D, H, W))
    got = run_bindings(ids, offsets, occ, T)
    check_against(got, want, what)
    again = run_bindings(ids, offsets, occ, T)
    assert all(torch.equal(g, a) for g, a in zip(got, again)), (what, "second run differs")
    check_against(run_bindings(ids, offsets, occ, T, want_mask=False), want, what)
    acc, mask = got[3], got[4]
    assert torch.equal(acc[:, 7].cpu(), table[:, 2]), what
    # the table against the kernel's own mask, counted per bit over its own ids
    rows = (ids.to(torch.int64) + offsets[:-1].view(N, 1, 1, 1) - 1)[ids > 0]
    bits = mask[ids > 0].to(torch.int64)
    for k in range(6):
        assert torch.equal(acc[:, k], torch.bincount(rows[(bits >> k & 1) != 0], minlength=T)), (what, k)
    assert torch.equal(acc[:, 6], torch.bincount(rows[bits == 0], minlength=T)), what
    assert not bool(mask[ids == 0].any()), what
    # the op layer takes the same kernels
    acc2, mask2 = access.access_table(ids, offsets, occ, want_mask=True)
    assert torch.equal(acc2, acc) and torch.equal(mask2, mask), what
    assert all(torch.equal(a, b) for a, b in zip(access.column_extents(occ), got[:3])), what


@pytest.mark.parametrize("N", [1, 2])
def test_single_voxel_instances_overflow_the_lds_table(N):
    """More instances in one workgroup's chunk than its LDS table has slots: the updates that find
    their slot held by another row go to global memory directly."""
    D, H, W = SHAPES[3]
    chunk, slots = _native.kernels().access_chunk()
    assert chunk > slots and D * H * W > chunk and chunk % W != 0     # two chunks, the first ends mid-row
    ids_c, offsets_c = singles(N, D, H, W)
    occ_c = occupancy(N, D, H, W, density=0.1, seed=1)
    want_acc, want_mask = reference.access_table(ids_c, offsets_c, occ_c, want_mask=True)
    T = N * D * H * W
    assert len(want_acc) == T and bool((want_acc[:, 7] == 1).all()) and bool((want_acc[:, :7].sum(1) >= 1).all())
    got = run_bindings(ids_c.to(DEV), offsets_c.to(DEV), occ_c.to(DEV), T)
    check_against(got[3:], (want_acc, want_mask), ("singles", N))
    assert int(got[3][:, 7].sum()) == T


def test_rows_outside_the_table_count_nowhere():
    """ids that point past the table (offsets that do not belong to them) are dropped, not used as addresses."""
    D, H, W = SHAPES[2]
    ids_c, offsets_c = singles(1, D, H, W)
    occ_c = occupancy(1, D, H, W)
    T = 100
    want_acc, want_mask = reference.access_table(ids_c, torch.tensor([0, T]), occ_c, want_mask=True)
    assert not bool(want_mask.view(-1)[T:].any()) and int(want_acc[:, 7].sum()) == T
    got = run_bindings(ids_c.to(DEV), torch.tensor([0, T], device=DEV), occ_c.to(DEV), T)
    check_against(got[3:], (want_acc, want_mask), "short table")
    neg = run_bindings(ids_c.to(DEV), torch.tensor([-50, T - 50], device=DEV), occ_c.to(DEV), T)   # rows -49 .. 925
    assert bool((neg[3][:, 7] == 1).all()) and not bool(neg[4].view(-1)[:50].any())
    assert not bool(neg[4].view(-1)[T + 50:].any())


def test_unsupported_arguments_are_refused():
    ids = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    occ = torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device=DEV)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    ex, ey, ez = access.column_extents(occ)
    acc = torch.zeros(4, 8, dtype=torch.int64, device=DEV)
    K, st = _native.kernels(), _native.stream(ids)
    p = dict(ids=ids.data_ptr(), offsets=off.data_ptr(), ex=ex.data_ptr(), ey=ey.data_ptr(), ez=ez.data_ptr(), mask=0,
             acc=acc.data_ptr(), N=1, D=4, H=4, W=4, T=4, st=st, ext=[64, 2, 32, 32, 32, 0, 32])
    for bad in (dict(T=-1, ext=[]), dict(T=65, ext=[]), dict(ids=0), dict(offsets=0), dict(ey=0), dict(acc=0),
                dict(H=0), dict(ex=ex.data_ptr() + 4)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.access_stats(**{**p, **bad})
    with pytest.raises(RuntimeError, match="acc has"):
        K.access_stats(**{**p, "T": 5})
    q = dict(occ=occ.data_ptr(), ex=ex.data_ptr(), ey=ey.data_ptr(), ez=ez.data_ptr(), N=1, D=4, H=4, W=4, st=st,
             ext=[64, 32, 32, 32])
    for bad in (dict(occ=0), dict(ez=0), dict(W=0, ext=[]), dict(N=0, ext=[])):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.access_extents(**{**q, **bad})
    with pytest.raises(RuntimeError, match="ey has"):
        K.access_extents(**{**q, "W": 5, "ext": [80, 32, 32, 40]})
    with pytest.raises(ValueError, match="one device"):
        access.access_table(ids, off, occ.cpu())
    with pytest.raises(ValueError, match="int32"):
        access.access_table(ids.long(), off, occ)
    torch.cuda.synchronize()


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


def test_instances_with_access_equal_the_oracle_on_the_predicted_labels(monkeypatch):
    mg = gpu_copy(make_model(5))
    xc = voxels(2)
    x = xc.to(DEV).to(torch.bfloat16)
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
        table, offsets, none, acc = mg.instances(x, background=background, connectivity=connectivity, want_access=True)
        t2, o2, ids, a2 = mg.instances(x, background=background, connectivity=connectivity, want_ids=True,
                                       want_access=True)
        three = mg.instances(x, background=background, connectivity=connectivity)
        torch.cuda.synchronize()
        assert none is None and ids.is_cuda and acc.is_cuda and acc.dtype == torch.int64 and len(three) == 3
        assert torch.equal(t2, table) and torch.equal(o2, offsets) and torch.equal(a2, acc)
        assert torch.equal(three[0], table) and three[2] is None
        cpu_labels = real_cpu(labels)
        roots = reference.connected_components(cpu_labels, background, connectivity)
        want_ids, want_table, want_offsets = reference.instance_table(cpu_labels, roots)
        want_acc, _ = reference.access_table(want_ids, want_offsets, xc.to(torch.uint8))
        assert torch.equal(real_cpu(table), want_table) and torch.equal(real_cpu(ids), want_ids)
        assert torch.equal(real_cpu(acc), want_acc) and torch.equal(want_acc[:, 7], want_table[:, 2])
    for name, count in (("ccl_stats", 6), ("access_extents", 4), ("access_stats", 4)):
        assert rec.calls.count(name) == count, (name, rec.calls)
    # no per-voxel tensor (occupancy, labels, ids, mask ...) crossed to the host inside instances()
    assert not [c for c in copies if int(np.prod(c[1])) >= S ** 3], copies


def test_extract_features_with_access_end_to_end(tmp_path):
    n = 4
    m = make_model(5)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 5})
    xb = voxels(n)
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    feats, none = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S, access=True)
    labels, _ = fn.segment(str(path), packed, batch_size=3, device=DEV, packed_size=S)
    _, want = fn.label_components(labels, device="cpu", occupancy=xb.numpy())
    assert none is None and len(feats) == n and feats == want
    _, on_gpu = fn.label_components(labels, device=DEV, occupancy=xb.numpy())
    assert on_gpu == want and sum(len(fs) for fs in want) > n
    plain, _ = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S)
    assert all(f.access is None for fs in plain for f in fs)
    assert [[f.to_dict() for f in fs] for fs in plain] == \
        [[{k: v for k, v in f.to_dict().items() if k in ("id", "class", "voxels", "bbox", "centroid")} for f in fs]
         for fs in feats]


def test_generated_parts_are_open_toward_their_access_face():
    vox, labels, parts, slots = fn.generate_parts(96, size=32, seed=3, device=DEV, return_slots=True)
    ids, feats = fn.label_components(labels, device=DEV, occupancy=vox)
    n = fully_open_toward_truth(labels, vox, parts, slots, feats, ids)
    assert n == 246 and len({p.cls for ps in parts for p in ps}) == 24
