"""The tool-reach kernels (``reach.hip``) and the paths built on them (``fn.tool_reach``,
``FeatureNet3DSeg.instances(want_reach=)``, ``fn.extract_features(tool=)``, ``fn.label_components(tool=)``)
on the GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``ops.reference``).  The shapes put a row under
one wave, on exactly one wave, one lane over, and on two 64-wide pieces plus a remainder, each axis at its
limit of 256, and columns of 3, 5 and 9 voxels that do not divide between the four waves that share one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _access_cases import occupancy, singles  # noqa: E402
from _ccl_cases import PATTERNS  # noqa: E402
from _edt_cases import LIMIT_SHAPES, SEEDS, SHAPES, expected_d2  # noqa: E402
from _reach_cases import (SYNTHETIC, TOOLS, check_scene, expected_reach, expected_scan, judge,  # noqa: E402
                          loop_reach_table, scene, synthetic)
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import edt, reach, reference  # noqa: E402
from featurenet_amd.ops.reference import EDT_INF  # noqa: E402

DEV = "cuda"
SENTINEL = -7


def run_scan(vol: torch.Tensor) -> torch.Tensor:
    """``reach_scan`` on a buffer pre-filled with a sentinel, one spare row behind it -> r6; asserts that
    every element was written and nothing past the output's end was touched (the inputs are >= 0)."""
    N, D, H, W = vol.shape
    n = vol.numel()
    buf = torch.full((6 * n + W,), SENTINEL, dtype=torch.int32, device=DEV)
    _native.kernels().reach_scan(vol.data_ptr(), buf.data_ptr(), N, D, H, W, _native.stream(vol), [n, 6 * n])
    torch.cuda.synchronize()
    assert bool((buf[6 * n:] == SENTINEL).all()) and bool((buf[:6 * n] >= 0).all())
    return buf[:6 * n].view(N, 6, D, H, W)


def run_stats(ids, offsets, r6, dc2, T: int, need2: int, cut2: int) -> torch.Tensor:
    """``reach_stats`` on a raw table pre-filled with a sentinel and a guard row behind it -> int64 [T, 15]."""
    N, D, H, W = ids.shape
    raw = torch.full((T + 1, 15), SENTINEL, dtype=torch.int64, device=DEV)
    _native.kernels().reach_stats(ids.data_ptr(), offsets.data_ptr(), r6.data_ptr(), dc2.data_ptr(), raw.data_ptr(),
                                  N, D, H, W, T, need2, cut2, _native.stream(ids),
                                  [ids.numel(), N + 1, r6.numel(), dc2.numel(), T * 15])
    torch.cuda.synchronize()
    assert bool((raw[T] == SENTINEL).all()) and bool((raw[:T] >= -1).all())
    has = raw[:T, 14] > 0
    assert bool((raw[:T][~has] == torch.tensor([-1] * 6 + [0] * 9, device=DEV)).all())
    return raw[:T]


@pytest.mark.parametrize("kind", SEEDS + SYNTHETIC)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("shape", SHAPES + LIMIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scan_against_the_oracle(shape, N, kind):
    D, H, W = shape
    what = (shape, N, kind)
    if kind in SEEDS:
        vol_c = expected_d2(kind, N, D, H, W, False)
        want = reference.reach_scan(vol_c)
    else:
        vol_c, want = synthetic(kind, N, D, H, W), expected_scan(kind, N, D, H, W)
    vol = vol_c.to(DEV)
    r6 = run_scan(vol)
    bad = r6.cpu() != want
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist())
    if kind == "none":
        assert bool((r6 == EDT_INF).all()), what
    assert torch.equal(run_scan(vol), r6), (what, "second run differs")
    assert torch.equal(reach.reach_scan(vol), r6), what            # the op layer takes the same kernel
    if kind == "dense":
        occ = (vol_c == 0).to(torch.uint8).numpy()
        assert np.array_equal(fn.tool_reach(occ, device=DEV), want.numpy()), what


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("si", range(4), ids=["under-a-wave", "one-wave", "wave+1", "two-pieces+rest"])
def test_statistics_against_the_oracle(si, N, pattern):
    D, H, W = SHAPES[si]
    for tool in (1, 3):
        need2, cut2 = TOOLS[tool]
        ids_c, table, offsets_c, occ_c, d2_c, want_r6, want_dc2, want = expected_reach(pattern, N, D, H, W, tool)
        ids, offsets, occ = ids_c.to(DEV), offsets_c.to(DEV), occ_c.to(DEV)
        T, what = len(table), (pattern, N, (D, H, W), tool)
        r6 = run_scan(edt.distance_sq(occ))
        dc2 = edt.distance_sq(reference.reach_seeds(r6, need2))
        assert torch.equal(dc2.cpu(), want_dc2), what
        got = run_stats(ids, offsets, r6, dc2, T, need2, cut2)
        assert got.is_cuda and judge(r6.cpu(), want_r6, got.cpu(), want), what
        assert torch.equal(run_stats(ids, offsets, r6, dc2, T, need2, cut2), got), (what, "second run differs")
        assert torch.equal(got[:, 14].cpu(), table[:, 2]), what
        # the table against the kernel's own r6 and dc2 volumes, recounted in torch over its own ids
        fg = ids > 0
        rows = (ids.to(torch.int64) + offsets[:-1].view(N, 1, 1, 1) - 1)[fg]
        if T:
            e = r6.permute(0, 2, 3, 4, 1)[fg].to(torch.int64)                # [voxels, 6]
            for k in range(6):
                top = torch.full((T,), -1, dtype=torch.int64, device=DEV).scatter_reduce(0, rows, e[:, k], "amax")
                assert torch.equal(got[:, k], top), (what, k)
                assert torch.equal(got[:, 6 + k], torch.bincount(rows[e[:, k] >= need2], minlength=T)), (what, k)
            assert torch.equal(got[:, 12], torch.bincount(rows[(e < need2).all(1)], minlength=T)), what
            assert torch.equal(got[:, 13], torch.bincount(rows[dc2[fg] <= cut2], minlength=T)), what
        # the op layer takes the same kernels, with and without the caller's d2
        got2, r62 = reach.reach_table(ids, offsets, occ, need2, cut2, want_r6=True)
        assert torch.equal(got2, got) and torch.equal(r62, r6), what
        assert torch.equal(reach.reach_table(ids, offsets, occ, need2, cut2, rows=T, d2=d2_c.to(DEV))[0], got), what


@pytest.mark.parametrize("N", [1, 2])
def test_single_voxel_instances_overflow_the_lds_table(N):
    """More instances in one workgroup's chunk than its LDS table has slots: the updates that find
    their slot held by another row go to global memory directly."""
    D, H, W = SHAPES[3]
    chunk, slots = _native.kernels().reach_chunk()
    assert chunk > slots and D * H * W > chunk and chunk % W != 0     # two chunks, the first ends mid-row
    ids_c, offsets_c = singles(N, D, H, W)
    occ_c = occupancy(N, D, H, W, density=0.1, seed=1)
    want_r6 = reference.reach_scan(reference.distance_sq(occ_c))
    want_dc2 = reference.distance_sq(reference.reach_seeds(want_r6, 4))
    want = reference.reach_table(ids_c, offsets_c, want_r6, want_dc2, 4, 2)
    T = N * D * H * W
    assert len(want) == T and bool((want[:, 14] == 1).all())
    assert torch.equal(want[:, :6], want_r6.permute(0, 2, 3, 4, 1).reshape(T, 6).to(torch.int64))
    r6 = run_scan(edt.distance_sq(occ_c.to(DEV)))
    got = run_stats(ids_c.to(DEV), offsets_c.to(DEV), r6, want_dc2.to(DEV), T, 4, 2)
    assert judge(r6.cpu(), want_r6, got.cpu(), want), ("singles", N)


def test_rows_outside_the_table_count_nowhere():
    """ids that point past the table (offsets that do not belong to them) are dropped, not used as addresses."""
    D, H, W = SHAPES[2]
    ids_c, _ = singles(1, D, H, W)
    r6_c = reference.reach_scan(reference.distance_sq(occupancy(1, D, H, W)))
    dc2_c = reference.distance_sq(reference.reach_seeds(r6_c, 4))
    ids, r6, dc2 = ids_c.to(DEV), r6_c.to(DEV), dc2_c.to(DEV)
    T = 100
    short = run_stats(ids, torch.tensor([0, T], device=DEV), r6, dc2, T, 4, 2)
    assert torch.equal(short.cpu(), reference.reach_table(ids_c, torch.tensor([0, T]), r6_c, dc2_c, 4, 2))
    assert int(short[:, 14].sum()) == T
    off = np.array([-50, T - 50])                          # rows -49 .. 925 of a table of 100
    neg = run_stats(ids, torch.tensor(off, device=DEV), r6, dc2, T, 4, 2)
    assert np.array_equal(neg.cpu().numpy(), loop_reach_table(ids_c.numpy(), off, r6_c.numpy(), dc2_c.numpy(), 4, 2, T))
    assert bool((neg[:, 14] == 1).all())
    two = np.array([0, 0, 7])                              # both samples' ids land on the same rows
    ids2 = ids_c.repeat(2, 1, 1, 1).contiguous()
    r62, dc22 = torch.cat([r6_c, r6_c.flip(4)]).contiguous(), torch.cat([dc2_c, dc2_c.flip(3)]).contiguous()
    shared = run_stats(ids2.to(DEV), torch.tensor(two, device=DEV), r62.to(DEV), dc22.to(DEV), 7, 4, 2)
    assert np.array_equal(shared.cpu().numpy(),
                          loop_reach_table(ids2.numpy(), two, r62.numpy(), dc22.numpy(), 4, 2, 7))
    assert bool((shared[:, 14] == 2).all())


def test_unsupported_arguments_are_refused():
    v = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    r6 = torch.zeros(1, 6, 4, 4, 4, dtype=torch.int32, device=DEV)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    raw = torch.zeros(4, 15, dtype=torch.int64, device=DEV)
    K, st = _native.kernels(), _native.stream(v)
    p = dict(vol=v.data_ptr(), r6=r6.data_ptr(), N=1, D=4, H=4, W=4, st=st, ext=[64, 384])
    for bad in (dict(vol=0), dict(r6=0), dict(vol=v.data_ptr() + 2), dict(r6=r6.data_ptr() + 1), dict(D=0, ext=[]),
                dict(W=0, ext=[]), dict(N=0, ext=[]), dict(D=257, ext=[]), dict(H=257, ext=[]), dict(W=257, ext=[])):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.reach_scan(**{**p, **bad})
    with pytest.raises(RuntimeError, match="r6 has"):
        K.reach_scan(**{**p, "W": 5, "ext": [80, 384]})
    with pytest.raises(RuntimeError, match="missing extent"):
        K.reach_scan(**{**p, "ext": [64]})
    q = dict(ids=v.data_ptr(), offsets=off.data_ptr(), r6=r6.data_ptr(), dc2=v.data_ptr(), raw=raw.data_ptr(), N=1, D=4,
             H=4, W=4, T=4, need2=1, cut2=0, st=st, ext=[64, 2, 384, 64, 60])
    for bad in (dict(T=-1, ext=[]), dict(T=65, ext=[]), dict(ids=0), dict(offsets=0), dict(r6=0), dict(dc2=0),
                dict(raw=0), dict(need2=0), dict(cut2=-1), dict(H=0, ext=[]), dict(W=257, ext=[]),
                dict(raw=raw.data_ptr() + 4), dict(r6=r6.data_ptr() + 2)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.reach_stats(**{**q, **bad})
    with pytest.raises(RuntimeError, match="raw has"):
        K.reach_stats(**{**q, "T": 5})
    with pytest.raises(RuntimeError, match="missing extent"):
        K.reach_stats(**{**q, "ext": [64, 2, 384, 64]})
    occ = torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="one device"):
        reach.reach_table(v, off, occ.cpu(), 1, 0)
    with pytest.raises(ValueError, match="need2"):
        reach.reach_table(v, off, occ, 0, 0)
    with pytest.raises(ValueError, match="d2 must be int32"):
        reach.reach_table(v, off, occ, 1, 0, d2=v.cpu())
    with pytest.raises(ValueError, match="at most 256"):
        reach.reach_scan(torch.zeros(1, 1, 1, 257, dtype=torch.int32, device=DEV))
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


def test_instances_with_reach_equal_the_oracle_on_the_predicted_labels(monkeypatch):
    mg = gpu_copy(make_model(5))
    xc = voxels(2)
    x = xc.to(DEV).to(torch.bfloat16)
    labels = mg.predict(x)
    assert len(labels.unique()) > 1
    rec = _Recorder(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    tool = TOOLS[3]
    table, offsets, none, rch = mg.instances(x, want_reach=tool)
    t2, o2, ids, acc, dim, r2 = mg.instances(x, want_ids=True, want_access=True, want_dims=True, want_reach=tool)
    torch.cuda.synchronize()
    assert none is None and ids.is_cuda and rch.is_cuda and rch.dtype == torch.int64
    assert torch.equal(t2, table) and torch.equal(o2, offsets) and torch.equal(r2, rch)
    cpu_labels = labels.cpu()
    want_ids, want_table, want_offsets = reference.instance_table(cpu_labels,
                                                                  reference.connected_components(cpu_labels, 0, 6))
    occ = xc.to(torch.uint8)
    d2 = reference.distance_sq(occ)
    r6 = reference.reach_scan(d2)
    want = reference.reach_table(want_ids, want_offsets, r6, reference.distance_sq(reference.reach_seeds(r6, tool[0])),
                                 *tool)
    assert torch.equal(table.cpu(), want_table) and torch.equal(ids.cpu(), want_ids) and torch.equal(rch.cpu(), want)
    assert torch.equal(dim.cpu(), reference.dimension_table(want_ids, want_offsets, d2))
    assert torch.equal(acc.cpu(), reference.access_table(want_ids, want_offsets, occ)[0])
    assert torch.equal(want[:, 14], want_table[:, 2]) and bool((want[:, :6] <= dim.cpu()[:, :1]).all())
    # alone: d2 and dc2; with the dimensions: their d2 is shared, so again two transforms and not three
    for name, count in (("reach_scan", 2), ("reach_stats", 2), ("edt_transform", 4), ("edt_stats", 1),
                        ("access_stats", 1)):
        assert rec.calls.count(name) == count, (name, rec.calls)


def test_features_with_a_tool_end_to_end(tmp_path):
    n = 4
    m = make_model(5)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 5})
    xb = voxels(n)
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    feats, none = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S, access=True,
                                      dimensions=True, tool=3)
    labels, _ = fn.segment(str(path), packed, batch_size=3, device=DEV, packed_size=S)
    _, want = fn.label_components(labels, device="cpu", occupancy=xb.numpy(), dimensions=True, tool=3)
    assert none is None and len(feats) == n and feats == want
    _, on_gpu = fn.label_components(labels, device=DEV, occupancy=xb.numpy(), dimensions=True, tool=3)
    assert on_gpu == want and sum(len(fs) for fs in want) > n
    assert all(f.reachable is not None and f.tool == (4, 2) and f.clearance2 is not None for fs in feats for f in fs)
    only, _ = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S, tool=3)
    assert [[(f.id, f.entry2, f.reachable, f.unreachable, f.machinable) for f in fs] for fs in only] == \
        [[(f.id, f.entry2, f.reachable, f.unreachable, f.machinable) for f in fs] for fs in want]
    assert all(f.clearance2 is None and f.access is None for fs in only for f in fs)


def test_the_pinned_scene():
    lab, occ = scene()
    feats = {}
    for t in TOOLS:
        _, (recs,) = fn.label_components(lab, device=DEV, occupancy=occ, dimensions=True, tool=t)
        feats[t] = recs
    check_scene(feats)
    r6 = fn.tool_reach(occ, device=DEV)
    assert np.array_equal(r6, reference.reach_scan(reference.distance_sq(torch.from_numpy(occ))).numpy())
