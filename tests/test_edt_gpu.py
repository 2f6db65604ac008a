"""The distance-transform kernels (``edt.hip``) and the paths built on them (``fn.distance_transform``,
``FeatureNet3DSeg.instances(want_dims=True)``, ``fn.extract_features(dimensions=True)``,
``fn.label_components(dimensions=True)``) on the GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``ops.reference``).  The shapes put a row under
one wave, on exactly one wave, one lane over, and on two 64-wide pieces plus a remainder, and each axis at
its limit of 256 (which fills the LDS staging of the column scans)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _access_cases import occupancy, singles  # noqa: E402
from _ccl_cases import PATTERNS  # noqa: E402
from _edt_cases import (LIMIT_SHAPES, PARTS_COMPONENTS, PARTS_SUM_CLEARANCE2, PARTS_SUM_WALL, SEEDS,  # noqa: E402
                        SHAPES, expected_d2, expected_dims, judge, loop_dimension_table, seeds)
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import edt, reference  # noqa: E402
from featurenet_amd.ops.reference import EDT_INF  # noqa: E402

DEV = "cuda"
SENTINEL = -7


def run_transform(s: torch.Tensor, border: bool):
    """``edt_transform`` pass by pass on buffers pre-filled with a sentinel, one spare row behind each ->
    (t, d2); asserts that every element was written and nothing past the outputs' ends was touched."""
    N, D, H, W = s.shape
    K, st, n = _native.kernels(), _native.stream(s), s.numel()
    t, d2 = (torch.full((n + W,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
    K.edt_transform(s.data_ptr(), t.data_ptr(), d2.data_ptr(), N, D, H, W, border, 1, st, [n, n, n])
    torch.cuda.synchronize()
    assert bool((d2 == SENTINEL).all()) and bool((t[:n] >= 0).all())
    K.edt_transform(s.data_ptr(), t.data_ptr(), d2.data_ptr(), N, D, H, W, border, 2, st, [n, n, n])
    torch.cuda.synchronize()
    assert bool((t[n:] == SENTINEL).all()) and bool((d2[n:] == SENTINEL).all()) and bool((d2[:n] >= 0).all())
    return t[:n].view(s.shape), d2[:n].view(s.shape)


def run_stats(ids: torch.Tensor, offsets: torch.Tensor, d2: torch.Tensor, T: int) -> torch.Tensor:
    """``edt_stats`` on a raw table pre-filled with a sentinel and a guard row behind it -> dim int64 [T, 4],
    decoded as the op layer decodes it."""
    N, D, H, W = ids.shape
    raw = torch.full((T + 1, 3), SENTINEL, dtype=torch.int64, device=DEV)
    _native.kernels().edt_stats(ids.data_ptr(), offsets.data_ptr(), d2.data_ptr(), raw.data_ptr(), N, D, H, W, T,
                                _native.stream(ids), [ids.numel(), N + 1, d2.numel(), T * 3])
    torch.cuda.synchronize()
    assert bool((raw[T] == SENTINEL).all()) and bool((raw[:T] >= 0).all())
    key, wall, vox = raw[:T].unbind(1)
    has = vox > 0
    assert bool((key[~has] == 0).all()) and bool((wall[~has] == 0).all())
    return torch.stack([torch.where(has, key >> 32, -1), torch.where(has, 0xFFFFFFFF - (key & 0xFFFFFFFF), -1),
                        wall, vox], 1)


@pytest.mark.parametrize("kind", SEEDS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("shape", SHAPES + LIMIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transform_against_the_oracle(shape, N, kind):
    D, H, W = shape
    s_c = seeds(kind, N, D, H, W)
    s = s_c.to(DEV)
    for border in (False, True):
        what = (shape, N, kind, border)
        want = expected_d2(kind, N, D, H, W, border)
        t, d2 = run_transform(s, border)
        assert torch.equal(d2.cpu(), want), (what, int((d2.cpu() != want).sum()))
        if kind == "none" and not border:
            assert bool((d2 == EDT_INF).all()), what
        if not border:                                     # the first pass alone: the transform of each plane
            planes = reference.distance_sq(s_c.view(N * D, 1, H, W)).view(N, D, H, W)
            assert torch.equal(t.cpu(), planes), what
        t2, again = run_transform(s, border)
        assert torch.equal(again, d2) and torch.equal(t2, t), (what, "second run differs")
        # the op layer runs both passes on one buffer
        assert torch.equal(edt.distance_sq(s, border), d2), what
    assert np.array_equal(fn.distance_transform(s_c.numpy(), device=DEV), expected_d2(kind, N, D, H, W, False).numpy())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("si", range(4), ids=["under-a-wave", "one-wave", "wave+1", "two-pieces+rest"])
def test_statistics_against_the_oracle(si, N, pattern):
    D, H, W = SHAPES[si]
    ids_c, table, offsets_c, occ_c, want_d2, want_dim = expected_dims(pattern, N, D, H, W)
    ids, offsets, occ = ids_c.to(DEV), offsets_c.to(DEV), occ_c.to(DEV)
    T, what = len(table), (pattern, N, (D, H, W))
    _, d2 = run_transform(occ, False)
    dim = run_stats(ids, offsets, d2, T)
    assert dim.is_cuda and judge(d2.cpu(), want_d2, dim.cpu(), want_dim), what
    assert torch.equal(run_stats(ids, offsets, d2, T), dim), (what, "second run differs")
    assert torch.equal(dim[:, 3].cpu(), table[:, 2]), what
    # the table against the kernel's own d2 volume, recounted in torch over its own ids
    fg = ids > 0
    rows = (ids.to(torch.int64) + offsets[:-1].view(N, 1, 1, 1) - 1)[fg]
    d = d2.to(torch.int64)[fg]
    lin = torch.arange(D * H * W, device=DEV).view(1, D, H, W).expand(ids.shape)[fg]
    if T:
        r2 = torch.full((T,), -1, dtype=torch.int64, device=DEV).scatter_reduce(0, rows, d, "amax")
        attains = d == r2[rows]
        at = torch.full((T,), 1 << 40, dtype=torch.int64, device=DEV).scatter_reduce(0, rows[attains], lin[attains],
                                                                                     "amin")
        assert torch.equal(dim[:, 0], r2) and torch.equal(dim[:, 1], at), what
        assert torch.equal(dim[:, 2], torch.bincount(rows[d == 1], minlength=T)), what
    # the op layer takes the same kernels
    dim2, d22 = edt.dimension_table(ids, offsets, occ, want_d2=True)
    assert torch.equal(dim2, dim) and torch.equal(d22, d2), what
    assert torch.equal(edt.dimension_table(ids, offsets, occ, rows=T)[0], dim), what


@pytest.mark.parametrize("N", [1, 2])
def test_single_voxel_instances_overflow_the_lds_table(N):
    """More instances in one workgroup's chunk than its LDS table has slots: the updates that find
    their slot held by another row go to global memory directly."""
    D, H, W = SHAPES[3]
    chunk, slots = _native.kernels().edt_chunk()
    assert chunk > slots and D * H * W > chunk and chunk % W != 0     # two chunks, the first ends mid-row
    ids_c, offsets_c = singles(N, D, H, W)
    occ_c = occupancy(N, D, H, W, density=0.1, seed=1)
    want_d2 = reference.distance_sq(occ_c)
    want = reference.dimension_table(ids_c, offsets_c, want_d2)
    T = N * D * H * W
    assert len(want) == T and bool((want[:, 3] == 1).all())
    assert torch.equal(want[:, 1], torch.arange(D * H * W).repeat(N)) and torch.equal(want[:, 0], want_d2.view(-1))
    _, d2 = run_transform(occ_c.to(DEV), False)
    dim = run_stats(ids_c.to(DEV), offsets_c.to(DEV), d2, T)
    assert judge(d2.cpu(), want_d2, dim.cpu(), want), ("singles", N)


def test_rows_outside_the_table_count_nowhere():
    """ids that point past the table (offsets that do not belong to them) are dropped, not used as addresses."""
    D, H, W = SHAPES[2]
    ids_c, _ = singles(1, D, H, W)
    occ_c = occupancy(1, D, H, W)
    d2_c = reference.distance_sq(occ_c)
    ids, d2 = ids_c.to(DEV), d2_c.to(DEV)
    T = 100
    short = run_stats(ids, torch.tensor([0, T], device=DEV), d2, T)
    assert torch.equal(short.cpu(), reference.dimension_table(ids_c, torch.tensor([0, T]), d2_c))
    assert int(short[:, 3].sum()) == T
    off = np.array([-50, T - 50])                          # rows -49 .. 925 of a table of 100
    neg = run_stats(ids, torch.tensor(off, device=DEV), d2, T)
    assert np.array_equal(neg.cpu().numpy(), loop_dimension_table(ids_c.numpy(), off, d2_c.numpy(), T))
    assert neg[:, 1].tolist() == list(range(50, T + 50)) and bool((neg[:, 3] == 1).all())
    two = np.array([0, 0, 7])                              # both samples' ids land on the same rows
    ids2 = ids_c.repeat(2, 1, 1, 1).contiguous()
    d22 = torch.cat([d2_c, d2_c.flip(3)]).contiguous()
    shared = run_stats(ids2.to(DEV), torch.tensor(two, device=DEV), d22.to(DEV), 7)
    assert np.array_equal(shared.cpu().numpy(), loop_dimension_table(ids2.numpy(), two, d22.numpy(), 7))


def test_unsupported_arguments_are_refused():
    s = torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device=DEV)
    ids = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    d2 = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    raw = torch.zeros(4, 3, dtype=torch.int64, device=DEV)
    K, st = _native.kernels(), _native.stream(ids)
    p = dict(seeds=s.data_ptr(), t=d2.data_ptr(), d2=d2.data_ptr(), N=1, D=4, H=4, W=4, border=False, passes=3, st=st,
             ext=[64, 64, 64])
    for bad in (dict(seeds=0), dict(t=0), dict(d2=0), dict(t=d2.data_ptr() + 2), dict(d2=d2.data_ptr() + 1),
                dict(D=0, ext=[]), dict(W=0, ext=[]), dict(N=0, ext=[]), dict(D=257, ext=[]), dict(H=257, ext=[]),
                dict(W=257, ext=[]), dict(passes=0), dict(passes=4)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.edt_transform(**{**p, **bad})
    with pytest.raises(RuntimeError, match="d2 has"):
        K.edt_transform(**{**p, "W": 5, "ext": [80, 80, 64]})
    with pytest.raises(RuntimeError, match="missing extent"):
        K.edt_transform(**{**p, "ext": [64, 64]})
    q = dict(ids=ids.data_ptr(), offsets=off.data_ptr(), d2=d2.data_ptr(), raw=raw.data_ptr(), N=1, D=4, H=4, W=4, T=4,
             st=st, ext=[64, 2, 64, 12])
    for bad in (dict(T=-1, ext=[]), dict(T=65, ext=[]), dict(ids=0), dict(offsets=0), dict(d2=0), dict(raw=0),
                dict(H=0, ext=[]), dict(W=257, ext=[]), dict(raw=raw.data_ptr() + 4), dict(ids=ids.data_ptr() + 2)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.edt_stats(**{**q, **bad})
    with pytest.raises(RuntimeError, match="raw has"):
        K.edt_stats(**{**q, "T": 5})
    with pytest.raises(RuntimeError, match="missing extent"):
        K.edt_stats(**{**q, "ext": [64, 2, 64]})
    with pytest.raises(ValueError, match="one device"):
        edt.dimension_table(ids, off, s.cpu())
    with pytest.raises(ValueError, match="int32"):
        edt.dimension_table(ids.long(), off, s)
    with pytest.raises(ValueError, match="at most 256"):
        edt.distance_sq(torch.zeros(1, 1, 1, 257, dtype=torch.uint8, device=DEV))
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


def test_instances_with_dims_equal_the_oracle_on_the_predicted_labels(monkeypatch):
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
        table, offsets, none, dim = mg.instances(x, background=background, connectivity=connectivity, want_dims=True)
        t2, o2, ids, acc, d2 = mg.instances(x, background=background, connectivity=connectivity, want_ids=True,
                                            want_access=True, want_dims=True)
        three = mg.instances(x, background=background, connectivity=connectivity)
        torch.cuda.synchronize()
        assert none is None and ids.is_cuda and dim.is_cuda and dim.dtype == torch.int64 and len(three) == 3
        assert torch.equal(t2, table) and torch.equal(o2, offsets) and torch.equal(d2, dim)
        assert torch.equal(three[0], table) and three[2] is None
        cpu_labels = real_cpu(labels)
        roots = reference.connected_components(cpu_labels, background, connectivity)
        want_ids, want_table, want_offsets = reference.instance_table(cpu_labels, roots)
        occ = xc.to(torch.uint8)
        want_dim = reference.dimension_table(want_ids, want_offsets, reference.distance_sq(occ))
        want_acc, _ = reference.access_table(want_ids, want_offsets, occ)
        assert torch.equal(real_cpu(table), want_table) and torch.equal(real_cpu(ids), want_ids)
        assert torch.equal(real_cpu(dim), want_dim) and torch.equal(want_dim[:, 3], want_table[:, 2])
        assert torch.equal(real_cpu(acc), want_acc)
    for name, count in (("ccl_stats", 6), ("edt_transform", 4), ("edt_stats", 4), ("access_extents", 2),
                        ("access_stats", 2)):
        assert rec.calls.count(name) == count, (name, rec.calls)
    # no per-voxel tensor (occupancy, labels, ids, d2 ...) crossed to the host inside instances()
    assert not [c for c in copies if int(np.prod(c[1])) >= S ** 3], copies


def test_extract_features_with_dimensions_end_to_end(tmp_path):
    n = 4
    m = make_model(5)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 5})
    xb = voxels(n)
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    feats, none = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S, access=True,
                                      dimensions=True)
    labels, _ = fn.segment(str(path), packed, batch_size=3, device=DEV, packed_size=S)
    _, want = fn.label_components(labels, device="cpu", occupancy=xb.numpy(), dimensions=True)
    assert none is None and len(feats) == n and feats == want
    _, on_gpu = fn.label_components(labels, device=DEV, occupancy=xb.numpy(), dimensions=True)
    assert on_gpu == want and sum(len(fs) for fs in want) > n
    assert all(f.clearance2 is not None and f.access is not None for fs in feats for f in fs)
    plain, _ = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S)
    assert all(f.clearance2 is None and f.access is None for fs in plain for f in fs)
    assert [[f.to_dict() for f in fs] for fs in plain] == \
        [[{k: v for k, v in f.to_dict().items() if k in ("id", "class", "voxels", "bbox", "centroid")} for f in fs]
         for fs in feats]


def test_generated_parts_on_the_gpu_equal_the_cpu_path():
    vox, labels, parts = fn.generate_parts(96, size=32, seed=3, device=DEV)
    ids, feats = fn.label_components(labels, device=DEV, occupancy=vox, dimensions=True)
    ids_c, want = fn.label_components(labels, device="cpu", occupancy=vox, dimensions=True)
    assert np.array_equal(ids, ids_c) and feats == want
    recs = [f for fs in feats for f in fs]
    assert len(recs) == PARTS_COMPONENTS
    assert sum(f.clearance2 for f in recs) == PARTS_SUM_CLEARANCE2
    assert sum(f.wall_voxels for f in recs) == PARTS_SUM_WALL
