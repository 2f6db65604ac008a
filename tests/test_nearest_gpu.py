"""The labelled-distance-transform kernels (``nearest.hip``) and the paths built on them (``fn.nearest_instances``,
``FeatureNet3DSeg.instances(want_walls=...)``, ``fn.extract_features(walls=...)``, ``fn.label_components(walls=...)``)
on the GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``ops.reference``).  The shapes put a row under one
wave, on exactly one wave, one lane into the second 64-wide piece and one lane short of two pieces, and each
axis at its limit of 128 (which fills the LDS staging of the column scans)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _access_cases import singles  # noqa: E402
from _ccl_cases import PATTERNS  # noqa: E402
from _nearest_cases import (IDS, LIMIT_SHAPES, PARTS, PARTS_TOUCHING, SHAPES, expected_nn, expected_walls,  # noqa: E402
                            ids as case_ids, judge, loop_wall_table, parts_summary)
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import nearest, reference  # noqa: E402
from featurenet_amd.ops.reference import NN_NONE  # noqa: E402

DEV = "cuda"
SENTINEL = -7


def run_transform(v: torch.Tensor):
    """``nn_transform`` pass by pass on buffers pre-filled with a sentinel, one spare row behind each -> (t, nn);
    asserts that every element was written and nothing past the outputs' ends was touched."""
    N, D, H, W = v.shape
    K, st, n = _native.kernels(), _native.stream(v), v.numel()
    t, nn = (torch.full((2 * n + W,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(2))
    K.nn_transform(v.data_ptr(), t.data_ptr(), nn.data_ptr(), N, D, H, W, 1, st, [n, 2 * n, 2 * n])
    torch.cuda.synchronize()
    assert bool((nn == SENTINEL).all()) and bool((t[:2 * n] > 0).all())
    K.nn_transform(v.data_ptr(), t.data_ptr(), nn.data_ptr(), N, D, H, W, 2, st, [n, 2 * n, 2 * n])
    torch.cuda.synchronize()
    assert bool((t[2 * n:] == SENTINEL).all()) and bool((nn[2 * n:] == SENTINEL).all()) and bool((nn[:2 * n] > 0).all())
    return t[:2 * n].view(N, 2, D, H, W), nn[:2 * n].view(N, 2, D, H, W)


def run_stats(v: torch.Tensor, offsets: torch.Tensor, nn: torch.Tensor, T: int, limit2: int) -> torch.Tensor:
    """``wall_stats`` on a raw table pre-filled with a sentinel and a guard row behind it -> the kernel's columns
    int64 [T, 4] = gap2, at, thin, voxels, decoded as the op layer decodes them."""
    N, D, H, W = v.shape
    raw = torch.full((T + 1, 3), SENTINEL, dtype=torch.int64, device=DEV)
    _native.kernels().wall_stats(v.data_ptr(), offsets.data_ptr(), nn.data_ptr(), raw.data_ptr(), N, D, H, W, T,
                                 limit2, _native.stream(v), [v.numel(), N + 1, nn.numel(), T * 3])
    torch.cuda.synchronize()
    assert bool((raw[T] == SENTINEL).all()) and bool((raw[:T, 1:] >= 0).all())
    key, thin, vox = raw[:T].unbind(1)
    assert bool((key[vox == 0] == -1).all()) and bool((thin[vox == 0] == 0).all()) and bool((key[vox > 0] > 0).all())
    has = (vox > 0) & ((key >> 32) < reference.EDT_INF)
    return torch.stack([torch.where(has, key >> 32, -1), torch.where(has, key & 0xFFFFFFFF, -1), thin, vox], 1)


@pytest.mark.parametrize("kind", IDS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("shape", SHAPES + LIMIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transform_against_the_oracle(shape, N, kind):
    D, H, W = shape
    v_c = case_ids(kind, N, D, H, W)
    v = v_c.to(DEV)
    what = (shape, N, kind)
    want = expected_nn(kind, N, D, H, W)
    t, nn = run_transform(v)
    assert torch.equal(nn.cpu(), want), (what, int((nn.cpu() != want).sum()))
    if kind == "none":
        assert bool((nn == NN_NONE).all()), what
    # the first pass alone: the transform of each plane
    planes = reference.nearest_labels(v_c.view(N * D, 1, H, W)).view(N, D, 2, H, W).transpose(1, 2)
    assert torch.equal(t.cpu(), planes), (what, int((t.cpu() != planes).sum()))
    t2, again = run_transform(v)
    assert torch.equal(again, nn) and torch.equal(t2, t), (what, "second run differs")
    # the op layer runs both passes on one buffer
    assert torch.equal(nearest.nearest_labels(v), nn), what
    d2, near = fn.nearest_instances(v_c.numpy(), device=DEV)
    assert np.array_equal(d2, (want >> 32).numpy()) and np.array_equal(near, (want & 0xFFFFFFFF).numpy())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("si", range(4), ids=["under-a-wave", "one-wave", "wave+1", "two-pieces-1"])
def test_statistics_against_the_oracle(si, N, pattern):
    D, H, W = SHAPES[si]
    limit2 = (0, 1, 4, 9)[si]
    v_c, table, offsets_c, want_nn, want = expected_walls(pattern, N, D, H, W, limit2)
    v, offsets = v_c.to(DEV), offsets_c.to(DEV)
    T, what = len(table), (pattern, N, (D, H, W))
    _, nn = run_transform(v)
    cols = run_stats(v, offsets, nn, T, limit2)
    assert cols.is_cuda and judge(nn.cpu(), want_nn, cols.cpu(), want[:, [0, 1, 3, 4]]), what
    assert torch.equal(run_stats(v, offsets, nn, T, limit2), cols), (what, "second run differs")
    assert torch.equal(cols[:, 3].cpu(), table[:, 2]), what
    # the table against the kernel's own nn volume, recounted in torch over its own ids
    fg = v > 0
    rows = (v.to(torch.int64) + offsets[:-1].view(N, 1, 1, 1) - 1)[fg]
    d = (nn[:, 1] >> 32)[fg]
    lin = torch.arange(D * H * W, device=DEV).view(1, D, H, W).expand(v.shape)[fg]
    if T:
        gap2 = torch.full((T,), 1 << 40, dtype=torch.int64, device=DEV).scatter_reduce(0, rows, d, "amin")
        attains = d == gap2[rows]
        at = torch.full((T,), 1 << 40, dtype=torch.int64, device=DEV).scatter_reduce(0, rows[attains], lin[attains],
                                                                                     "amin")
        has = gap2 < reference.EDT_INF
        assert torch.equal(cols[:, 0], torch.where(has, gap2, -1)) and torch.equal(cols[:, 1], torch.where(has, at, -1))
        assert torch.equal(cols[:, 2], torch.bincount(rows[d <= limit2], minlength=T)), what
    # the op layer takes the same kernels and adds `other`
    wall, nn2 = nearest.wall_table(v, offsets, limit2, want_nn=True)
    assert wall.is_cuda and judge(nn2.cpu(), want_nn, wall.cpu(), want), what
    assert torch.equal(nearest.wall_table(v, offsets, limit2, rows=T)[0], wall), what


@pytest.mark.parametrize("N", [1, 2])
def test_single_voxel_instances_overflow_the_lds_table(N):
    """More instances in one workgroup's chunk than its LDS table has slots: the updates that find
    their slot held by another row go to global memory directly."""
    D, H, W = SHAPES[2]
    chunk, slots = _native.kernels().nn_chunk()
    assert min(chunk, D * H * W) > slots                    # a chunk holds more instances than the table has slots
    v_c, offsets_c = singles(N, D, H, W)
    want_nn = reference.nearest_labels(v_c)
    want = reference.wall_table(v_c, offsets_c, want_nn, 1)
    T = N * D * H * W
    assert len(want) == T and bool((want[:, 4] == 1).all()) and bool((want[:, 0] == 1).all())
    assert torch.equal(want[:, 1], torch.arange(D * H * W).repeat(N)) and bool((want[:, 3] == 1).all())
    v, offsets = v_c.to(DEV), offsets_c.to(DEV)
    _, nn = run_transform(v)
    cols = run_stats(v, offsets, nn, T, 1)
    assert judge(nn.cpu(), want_nn, cols.cpu(), want[:, [0, 1, 3, 4]]), ("singles", N)
    assert torch.equal(nearest.wall_table(v, offsets, 1)[0].cpu(), want)


def test_rows_outside_the_table_count_nowhere():
    """ids that point past the table (offsets that do not belong to them) are dropped, not used as addresses."""
    D, H, W = SHAPES[2]
    v_c, _ = singles(1, D, H, W)
    nn_c = reference.nearest_labels(v_c)
    v, nn = v_c.to(DEV), nn_c.to(DEV)
    T = 100
    short = run_stats(v, torch.tensor([0, T], device=DEV), nn, T, 0)
    assert np.array_equal(short.cpu().numpy(), loop_wall_table(v_c.numpy(), np.array([0, T]), nn_c.numpy(), T, 0))
    assert int(short[:, 3].sum()) == T
    off = np.array([-50, T - 50])                          # rows -49 .. 925 of a table of 100
    neg = run_stats(v, torch.tensor(off, device=DEV), nn, T, 1)
    assert np.array_equal(neg.cpu().numpy(), loop_wall_table(v_c.numpy(), off, nn_c.numpy(), T, 1))
    assert neg[:, 1].tolist() == list(range(50, T + 50)) and bool((neg[:, 3] == 1).all())
    two = np.array([0, 0, 7])                              # both samples' ids land on the same rows
    v2 = torch.cat([v_c, v_c.flip(3)]).contiguous()
    nn2 = reference.nearest_labels(v2)
    nn2[1, 1] += (torch.arange(D * H * W).view(D, H, W) % 3) << 32          # (distances that differ between the two)
    shared = run_stats(v2.to(DEV), torch.tensor(two, device=DEV), nn2.to(DEV), 7, 2)
    assert np.array_equal(shared.cpu().numpy(), loop_wall_table(v2.numpy(), two, nn2.numpy(), 7, 2))


def test_unsupported_arguments_are_refused():
    v = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    nn = torch.zeros(1, 2, 4, 4, 4, dtype=torch.int64, device=DEV)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    raw = torch.zeros(4, 3, dtype=torch.int64, device=DEV)
    K, st = _native.kernels(), _native.stream(v)
    p = dict(ids=v.data_ptr(), t=nn.data_ptr(), nn=nn.data_ptr(), N=1, D=4, H=4, W=4, passes=3, st=st,
             ext=[64, 128, 128])
    for bad in (dict(ids=0), dict(t=0), dict(nn=0), dict(t=nn.data_ptr() + 4), dict(nn=nn.data_ptr() + 4),
                dict(ids=v.data_ptr() + 2), dict(D=0, ext=[]), dict(W=0, ext=[]), dict(N=0, ext=[]), dict(D=129, ext=[]),
                dict(H=129, ext=[]), dict(W=129, ext=[]), dict(passes=0), dict(passes=4)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.nn_transform(**{**p, **bad})
    with pytest.raises(RuntimeError, match="nn has"):
        K.nn_transform(**{**p, "W": 5, "ext": [80, 160, 128]})
    with pytest.raises(RuntimeError, match="t has"):
        K.nn_transform(**{**p, "ext": [64, 64, 128]})
    with pytest.raises(RuntimeError, match="missing extent"):
        K.nn_transform(**{**p, "ext": [64, 128]})
    q = dict(ids=v.data_ptr(), offsets=off.data_ptr(), nn=nn.data_ptr(), raw=raw.data_ptr(), N=1, D=4, H=4, W=4, T=4,
             limit2=0, st=st, ext=[64, 2, 128, 12])
    for bad in (dict(T=-1, ext=[]), dict(T=65, ext=[]), dict(ids=0), dict(offsets=0), dict(nn=0), dict(raw=0),
                dict(H=0, ext=[]), dict(W=129, ext=[]), dict(raw=raw.data_ptr() + 4), dict(nn=nn.data_ptr() + 4),
                dict(ids=v.data_ptr() + 2), dict(limit2=-1), dict(limit2=1 << 30)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.wall_stats(**{**q, **bad})
    with pytest.raises(RuntimeError, match="raw has"):
        K.wall_stats(**{**q, "T": 5})
    with pytest.raises(RuntimeError, match="nn has"):
        K.wall_stats(**{**q, "ext": [64, 2, 64, 12]})
    with pytest.raises(RuntimeError, match="missing extent"):
        K.wall_stats(**{**q, "ext": [64, 2, 128]})
    with pytest.raises(ValueError, match="one device"):
        nearest.wall_table(v, off.cpu())
    with pytest.raises(ValueError, match="int32"):
        nearest.wall_table(v.long(), off)
    with pytest.raises(ValueError, match="at most 128"):
        nearest.nearest_labels(torch.zeros(1, 1, 1, 129, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="at most 128"):
        fn.nearest_instances(np.zeros((1, 129, 1, 1), np.int32), device=DEV)
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


def voxels(n: int, seed: int = 3, density: float = 0.4) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, S, S, S, generator=g) < density


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


def test_instances_with_walls_equal_the_oracle_on_the_predicted_labels(monkeypatch):
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
        table, offsets, none, wall = mg.instances(x, background=background, connectivity=connectivity, want_walls=4)
        t2, o2, ids, dim, w2 = mg.instances(x, background=background, connectivity=connectivity, want_ids=True,
                                            want_dims=True, want_walls=4)
        three = mg.instances(x, background=background, connectivity=connectivity)
        four = mg.instances(x, background=background, connectivity=connectivity, want_dims=True)
        torch.cuda.synchronize()
        assert none is None and ids.is_cuda and wall.is_cuda and wall.dtype == torch.int64 and len(three) == 3
        assert torch.equal(t2, table) and torch.equal(o2, offsets) and torch.equal(w2, wall)
        assert torch.equal(three[0], table) and three[2] is None
        assert len(four) == 4 and torch.equal(four[3], dim)
        cpu_labels = real_cpu(labels)
        roots = reference.connected_components(cpu_labels, background, connectivity)
        want_ids, want_table, want_offsets = reference.instance_table(cpu_labels, roots)
        assert torch.equal(real_cpu(table), want_table) and torch.equal(real_cpu(ids), want_ids)
        assert torch.equal(real_cpu(offsets), want_offsets)
        # (thousands of instances: the label-by-label oracle in torch on the device's tensors, not on the host's)
        want_wall = reference.wall_table(ids, offsets, reference.nearest_labels(ids), 4)
        assert torch.equal(wall, want_wall) and torch.equal(real_cpu(want_wall)[:, 4], want_table[:, 2])
        assert bool((want_wall[:, 0] >= 1).any())
    for name, count in (("ccl_stats", 8), ("nn_transform", 4), ("wall_stats", 4), ("edt_transform", 4),
                        ("edt_stats", 4)):
        assert rec.calls.count(name) == count, (name, rec.calls)
    # no per-voxel tensor (labels, ids, nn ...) crossed to the host inside instances()
    assert not [c for c in copies if int(np.prod(c[1])) >= S ** 3], copies


def test_extract_features_with_walls_end_to_end(tmp_path):
    n = 3
    m = make_model(5)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 5})
    xb = voxels(n, density=0.1)                 # (sparser material: hundreds of instances a part, not thousands)
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    feats, none = fn.extract_features(str(path), packed, batch_size=2, device=DEV, packed_size=S, walls=2)
    labels, _ = fn.segment(str(path), packed, batch_size=2, device=DEV, packed_size=S)
    _, want = fn.label_components(labels, device="cpu", walls=2)
    assert none is None and len(feats) == n and feats == want
    _, on_gpu = fn.label_components(labels, device=DEV, walls=2)
    assert on_gpu == want and sum(len(fs) for fs in want) > n
    assert all(f.walls and f.thin_voxels is not None for fs in feats for f in fs)
    assert any(f.gap2 is not None for fs in feats for f in fs)
    # results without walls are field for field what they are with them, less the new fields
    plain, _ = fn.extract_features(str(path), packed, batch_size=2, device=DEV, packed_size=S)
    assert all(not f.walls and f.gap2 is None and f.thin_voxels is None for fs in plain for f in fs)
    assert [[f.to_dict() for f in fs] for fs in plain] == \
        [[{k: v for k, v in f.to_dict().items() if k in ("id", "class", "voxels", "bbox", "centroid")} for f in fs]
         for fs in feats]
    every, _ = fn.extract_features(str(path), packed, batch_size=2, device=DEV, packed_size=S, access=True,
                                   dimensions=True, tool=2, contacts=True)
    with_walls, _ = fn.extract_features(str(path), packed, batch_size=2, device=DEV, packed_size=S, access=True,
                                        dimensions=True, tool=2, contacts=True, walls=True)
    extra = ("gap2", "gap_at", "gap_to", "min_wall", "thin_voxels")
    assert [[f.to_dict() for f in fs] for fs in every] == \
        [[{k: v for k, v in f.to_dict().items() if k not in extra} for f in fs] for fs in with_walls]
    assert all((f.gap2 == 1) == bool(f.neighbors) and f.thin_voxels is None for fs in with_walls for f in fs)


@pytest.mark.parametrize("separate", [True, False])
def test_generated_parts_on_the_gpu_equal_the_cpu_path(separate):
    kw = {} if separate else {"separate": False}
    vox, labels, parts = fn.generate_parts(96, size=32, seed=3, device=DEV, **kw)
    ids, feats = fn.label_components(labels, device=DEV, walls=1)
    ids_c, want = fn.label_components(labels, device="cpu", walls=1)
    assert np.array_equal(ids, ids_c) and feats == want
    got, pins = parts_summary(feats), PARTS if separate else PARTS_TOUCHING
    assert {k: got[k] for k in pins} == pins
