"""The watershed kernels (``watershed.hip``) and the paths built on them (``ops.watershed``, ``fn.split_features``,
``fn.recognize(split=...)``, ``fn.label_components(split=...)``) on the GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``ops.reference.watershed_*``, which
``test_watershed_cpu.py`` holds against per-voxel loops).  The shapes put a tile row under one wave, on exactly one
wave and one lane over, a volume inside one tile, on exactly one tile, one voxel over on every axis, and on three
tiles along x with a remainder; the largest ones also span several workgroups' chunks of the flat voxel range.
Every output buffer is pre-filled with a sentinel and sits between guard rows, and every launch runs twice."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _guard import KeepGuard, launch_kept  # noqa: E402
from _watershed_cases import KINDS, SHAPES, case, dumbbell, expected  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3D, FeatureNet3DConfig  # noqa: E402
from featurenet_amd.ops import ccl, isolate, reference, watershed  # noqa: E402

DEV = "cuda"
SENTINEL = -0x01234567
SENTINEL64 = -0x0123456789ABCDEF
GUARD = 64


class _Recorder:
    """Forwards to the real ``_C`` and records the entry points called."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


def kept(fn):
    """``fn()`` with guard bands round every buffer it allocates, its results (stacked and gathered by torch, not
    allocated by the entry point) as they are."""
    with KeepGuard():
        return fn()


def guarded(n: int) -> tuple:
    """An int32 buffer of ``n`` elements between two guard rows, all of it the sentinel -> (whole, live view)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def untouched(whole: torch.Tensor) -> bool:
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def run_ascend(ids: torch.Tensor, height: torch.Tensor, staged: int) -> torch.Tensor:
    N, D, H, W = ids.shape
    whole, parent = guarded(ids.numel())
    _native.kernels().ws_ascend(ids.data_ptr(), height.data_ptr(), parent.data_ptr(), N, D, H, W, staged,
                                _native.stream(ids), [ids.numel()] * 3)
    torch.cuda.synchronize()
    assert untouched(whole) and not bool((parent == SENTINEL).any())
    return parent.view(ids.shape)


def run_resolve(parent: torch.Tensor) -> tuple:
    N, D, H, W = parent.shape
    whole_r, roots = guarded(parent.numel())
    whole_f, flags = guarded(parent.numel())
    _native.kernels().ws_resolve(parent.data_ptr(), roots.data_ptr(), flags.data_ptr(), N, D, H, W,
                                 _native.stream(parent), [parent.numel()] * 3)
    torch.cuda.synchronize()
    assert untouched(whole_r) and untouched(whole_f)
    assert not bool((roots == SENTINEL).any()) and not bool((flags == SENTINEL).any())
    return roots.view(parent.shape), flags.view(parent.shape)


def run_saddle(ids, bids, offsets, height, T: int, cap: int, probe: int) -> tuple:
    """``ws_saddle`` on a table pre-filled with a sentinel, its live part zeroed as the kernel wants it, a guard row
    on either side -> (keys, counts, lost)."""
    N, D, H, W = ids.shape
    tab = torch.full((2 * cap + 1 + 2 * GUARD,), SENTINEL64, dtype=torch.int64, device=DEV)
    live = tab[GUARD:GUARD + 2 * cap + 1]
    live.zero_()
    keys, counts, lost = live[:cap], live[cap:2 * cap], live[2 * cap:]
    _native.kernels().ws_saddle(ids.data_ptr(), bids.data_ptr(), offsets.data_ptr(), height.data_ptr(), keys.data_ptr(),
                                counts.data_ptr(), lost.data_ptr(), N, D, H, W, T, cap, probe, _native.stream(ids),
                                [ids.numel(), bids.numel(), N + 1, height.numel(), cap, cap, 1])
    torch.cuda.synchronize()
    assert bool((tab[:GUARD] == SENTINEL64).all()) and bool((tab[-GUARD:] == SENTINEL64).all())
    return keys, counts, lost


def decode(keys: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """The occupied slots of the pair table as sorted ``pairs`` rows (in torch, apart from the op layer)."""
    slot = torch.nonzero(keys).squeeze(1)
    key, order = torch.sort(keys[slot])
    return torch.stack([(key >> 32) - 1, (key & 0xFFFFFFFF) - 1, counts[slot][order]], 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("si", range(6), ids=["one-voxel", "in-a-tile", "one-tile", "tile+1", "three-tiles+rest",
                                              "four-tiles-along-x"])
def test_kernels_against_the_oracle(si, N, kind):
    D, H, W = SHAPES[si]
    what = (kind, N, (D, H, W))
    ids_c, height_c = case(kind, N, D, H, W)
    want_parent, want_roots, want_flags, want_bids, want_table, want_offsets, want_pairs = expected(kind, N, D, H, W)
    ids, height = ids_c.to(DEV), height_c.to(DEV)
    # each kernel alone, on the oracle's version of what it reads
    for staged in (1, 0):
        parent = run_ascend(ids, height, staged)
        assert torch.equal(parent.cpu(), want_parent), (what, staged, int((parent.cpu() != want_parent).sum()))
        assert torch.equal(run_ascend(ids, height, staged), parent), (what, staged, "second run differs")
    roots, flags = run_resolve(want_parent.to(DEV))
    assert torch.equal(roots.cpu(), want_roots) and torch.equal(flags.cpu(), want_flags), what
    again = run_resolve(want_parent.to(DEV))
    assert torch.equal(again[0], roots) and torch.equal(again[1], flags), (what, "second run differs")
    bids, table, offsets = ccl.instance_table((ids > 0).to(torch.uint8), roots, flags=flags)
    assert torch.equal(bids.cpu(), want_bids) and torch.equal(table.cpu(), want_table), what
    assert torch.equal(offsets.cpu(), want_offsets), what
    T = len(want_table)
    cap = 1 << max(10, (13 * ids.numel() - 1).bit_length())          # a slot for every forward pair: nothing is lost
    keys, counts, lost = run_saddle(ids, want_bids.to(DEV), want_offsets.to(DEV), height, T, cap, cap)
    pairs = decode(keys, counts)
    assert int(lost) == 0 and torch.equal(pairs.cpu(), want_pairs), (what, pairs.shape, want_pairs.shape)
    assert not bool(counts[keys == 0].any()), what
    keys2, counts2, _ = run_saddle(ids, want_bids.to(DEV), want_offsets.to(DEV), height, T, cap, cap)
    assert torch.equal(decode(keys2, counts2), pairs), (what, "second run differs")
    # then through the op layer
    got_roots, got_flags = launch_kept(lambda: watershed.ascend(ids, height))
    assert torch.equal(got_roots, roots) and torch.equal(got_flags, flags), what
    plain = watershed.ascend(ids, height, staged=0)
    assert torch.equal(plain[0], roots) and torch.equal(plain[1], flags), what
    got_pairs = kept(lambda: watershed.saddle_pairs(ids, bids, offsets, height))
    assert got_pairs.is_cuda and torch.equal(got_pairs, pairs), what
    assert torch.equal(watershed.saddle_pairs(ids, bids, offsets, height, rows=T), pairs), what
    for merge in (0, 1):
        want = watershed.split_instances(ids_c, height_c, merge)
        got = kept(lambda: watershed.split_instances(ids, height, merge))
        twice = watershed.split_instances(ids, height, merge)
        for g, t, w in zip(got, twice, want):
            assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w) and torch.equal(t, g), (what, merge)
    if kind == "noise" and si >= 2:
        assert len(want_pairs) > T > 0, what
    if kind == "touching" and si >= 1:           # two ids that touch everywhere: no basin pair crosses them
        assert len(want_pairs) > 0 and bool((ids_c.reshape(-1)[want_table[want_pairs[:, 0], 0] * D * H * W
                                                                  + want_table[want_pairs[:, 0], 3] - 1]
                                                 == ids_c.reshape(-1)[want_table[want_pairs[:, 1], 0] * D * H * W
                                                                      + want_table[want_pairs[:, 1], 3] - 1]).all())


def test_an_ascent_does_not_cross_samples():
    """Sample 1 lies higher than sample 0 and both carry id 1 where they meet in memory: no root of sample 0 may
    come from sample 1's heights, and the two samples' results are those of each sample alone."""
    D, H, W = SHAPES[3]
    ids_c, height_c = case("noise", 2, D, H, W)
    assert bool((ids_c[0, -1] == 1).all() and (ids_c[1, 0] == 1).all()) and int(height_c[1].min()) > int(height_c[0].max())
    roots, _ = watershed.ascend(ids_c.to(DEV), height_c.to(DEV))
    for n in range(2):
        alone, _ = watershed.ascend(ids_c[n:n + 1].to(DEV), height_c[n:n + 1].to(DEV))
        assert torch.equal(roots[n:n + 1], alone)


def test_resolve_stops_at_words_that_are_no_parents():
    """A parent outside [1, V] ends the walk with root 0 and is never used as an address; a cycle (no real chain has
    one) ends after V reads, with root 0 too."""
    D, H, W = 3, 5, 7
    V = D * H * W
    g = torch.Generator().manual_seed(5)
    parent = torch.arange(1, V + 1, dtype=torch.int32).repeat(2, 1)
    up = torch.randint(0, V, (2, V), generator=g, dtype=torch.int32)
    parent = torch.where(up < torch.arange(V), up + 1, parent)          # chains that run down to lower indices
    parent[0, 10], parent[0, 20], parent[1, 5], parent[1, 30] = 0, -7, V + 1, 2 ** 31 - 1
    parent[1, 40], parent[1, 41] = 42, 41                               # 40 <-> 41: a cycle
    want = torch.zeros(2, V, dtype=torch.int32)
    for n in range(2):
        for v in range(V):
            a, r = v, 0
            for _ in range(V):
                p = int(parent[n, a])
                if p < 1 or p > V:
                    break
                if p - 1 == a:
                    r = p
                    break
                a = p - 1
            want[n, v] = r
    assert int((want == 0).sum()) >= 6
    roots, flags = run_resolve(parent.view(2, D, H, W).to(DEV))
    assert torch.equal(roots.cpu().view(2, V), want)
    assert torch.equal(flags.cpu().view(2, V), (want == torch.arange(1, V + 1)).to(torch.int32))


def test_the_pair_table_grows_when_updates_are_lost(monkeypatch):
    """Noise makes a basin of almost every other voxel and several pair rows per basin: a table of 1,024 slots
    probed 64 deep drops updates and counts them; the op layer sees the count and runs again with a larger one."""
    D, H, W = SHAPES[4]
    ids_c, height_c = case("noise", 1, D, H, W)
    _, _, _, bids_c, table, offsets_c, want = expected("noise", 1, D, H, W)
    T = len(table)
    assert len(want) > 4 * 1024
    ids, height, bids, offsets = (t.to(DEV) for t in (ids_c, height_c, bids_c, offsets_c))
    keys, counts, lost = run_saddle(ids, bids, offsets, height, T, 1024, 64)
    part = decode(keys, counts).cpu()
    assert int(lost) > 0 and 0 < len(part) <= 1024
    oracle = {(a, b): s for a, b, s in want.tolist()}
    assert all((a, b) in oracle and 0 <= s <= oracle[(a, b)] for a, b, s in part.tolist())
    rec = _Recorder(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    got = watershed.saddle_pairs(ids, bids, offsets, height, rows=T, cap=1024)
    assert rec.calls.count("ws_saddle") > 1
    assert torch.equal(got.cpu(), want)
    assert torch.equal(watershed.saddle_pairs(ids, bids, offsets, height).cpu(), want)


def test_rows_outside_the_table_are_dropped():
    """Basin ids that point past the table (offsets that do not belong to them) are dropped, not used in a key."""
    D, H, W = SHAPES[3]
    ids_c, height_c = case("noise", 1, D, H, W)
    _, _, _, bids_c, table, _, full = expected("noise", 1, D, H, W)
    T = 100
    assert len(table) > 500
    ids, height = ids_c.to(DEV), height_c.to(DEV)
    for off in ([0, T], [-50, T - 50], [1000, T], [0, 0]):
        off_c = torch.tensor(off)
        want = reference.watershed_saddles(ids_c, bids_c, off_c, height_c)
        keys, counts, lost = run_saddle(ids, bids_c.to(DEV), off_c.to(DEV), height, off[1], 4096, 4096)
        assert int(lost) == 0 and torch.equal(decode(keys, counts).cpu(), want), off
        assert len(want) < len(full) and (len(want) > 0) == (off in ([0, T], [-50, T - 50])), off
    big = bids_c.clone()
    big.view(-1)[::3] = 2 ** 31 - 1              # basin ids beyond the sample's range, and negative ones
    big.view(-1)[1::7] = -5
    off_c = torch.tensor([0, len(table)])
    want = reference.watershed_saddles(ids_c, big, off_c, height_c)
    cap = 1 << 16
    keys, counts, lost = run_saddle(ids, big.to(DEV), off_c.to(DEV), height, len(table), cap, cap)
    assert int(lost) == 0 and len(want) > 0 and torch.equal(decode(keys, counts).cpu(), want)
    two = torch.tensor([0, 7, len(table)])       # in sample 1 a negative id plus its offset lands in the table
    ids2, h2, big2 = (torch.cat([t, t]) for t in (ids_c, height_c, big))
    want = reference.watershed_saddles(ids2, big2, two, h2)
    keys, counts, lost = run_saddle(ids2.to(DEV), big2.to(DEV), two.to(DEV), h2.to(DEV), len(table), cap, cap)
    assert int(lost) == 0 and torch.equal(decode(keys, counts).cpu(), want)


def test_unsupported_arguments_are_refused():
    ids = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    buf = torch.zeros(2 * 1024 + 1, dtype=torch.int64, device=DEV)
    out = torch.zeros(3, 64, dtype=torch.int32, device=DEV)
    K, st = _native.kernels(), _native.stream(ids)
    a = dict(ids=ids.data_ptr(), height=ids.data_ptr(), parent=out[0].data_ptr(), N=1, D=4, H=4, W=4, staged=1, st=st,
             ext=[64, 64, 64])
    for bad in (dict(ids=0), dict(height=0), dict(parent=0), dict(staged=2), dict(D=0, ext=[]), dict(W=257, ext=[])):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.ws_ascend(**{**a, **bad})
    with pytest.raises(RuntimeError, match="parent has"):
        K.ws_ascend(**{**a, "ext": [64, 64, 63]})
    r = dict(parent=out[0].data_ptr(), roots=out[1].data_ptr(), flags=out[2].data_ptr(), N=1, D=4, H=4, W=4, st=st,
             ext=[64, 64, 64])
    for bad in (dict(parent=0), dict(roots=0), dict(flags=0), dict(roots=out[0].data_ptr()), dict(H=300, ext=[])):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.ws_resolve(**{**r, **bad})
    s = dict(ids=ids.data_ptr(), bids=ids.data_ptr(), offsets=off.data_ptr(), height=ids.data_ptr(),
             keys=buf.data_ptr(), counts=buf[1024:].data_ptr(), lost=buf[2048:].data_ptr(), N=1, D=4, H=4, W=4, T=4,
             cap=1024, probe=256, st=st, ext=[64, 64, 2, 64, 1024, 1024, 1])
    for bad in (dict(T=-1), dict(T=65), dict(ids=0), dict(bids=0), dict(offsets=0), dict(height=0), dict(keys=0),
                dict(counts=0), dict(lost=0), dict(cap=1000), dict(probe=0)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.ws_saddle(**{**s, **bad})
    with pytest.raises(RuntimeError, match="keys has"):
        K.ws_saddle(**{**s, "ext": [64, 64, 2, 64, 512, 1024, 1]})
    with pytest.raises(ValueError, match="height must be int32"):
        watershed.ascend(ids, ids.cpu())
    with pytest.raises(ValueError, match="int32"):
        watershed.ascend(ids.long(), ids)
    with pytest.raises(ValueError, match="power of two"):
        watershed.saddle_pairs(ids, ids, off, ids, cap=1000)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------
def plain(feats) -> list:
    """The records without the classifier's opinion (bf16 on the GPU, fp32 on the CPU: it may differ)."""
    out = []
    for fs in feats:
        rows = []
        for f in fs:
            d = f.to_dict()
            for k in ("class", "recognized", "recognized_prob", "agrees"):
                d.pop(k, None)
            rows.append(d)
        out.append(rows)
    return out


def test_split_features_and_recognize_equal_the_cpu_path():
    cfg = FeatureNet3DConfig.tiny()
    S = cfg.input_size
    vox, labels, _ = fn.generate_parts(8, size=S, seed=3, features=(2, 4), separate=False, device=DEV)
    torch.manual_seed(0)
    clf = FeatureNet3D(cfg).eval()
    clf_gpu = FeatureNet3D(cfg)
    clf_gpu.load_state_dict(clf.state_dict())
    clf_gpu = clf_gpu.to(DEV).eval()
    ids0, _ = fn.label_components((vox == 0).astype(np.uint8), device="cpu")
    for merge in (0, 1, 2.5):
        got_ids, got = fn.split_features(ids0, occupancy=vox, merge=merge, device=DEV)
        want_ids, want = fn.split_features(ids0, occupancy=vox, merge=merge, device="cpu")
        assert np.array_equal(got_ids, want_ids) and got == want, merge
    assert sum(map(len, want)) < sum(map(len, fn.split_features(ids0, occupancy=vox, merge=0, device=DEV)[1]))
    kw = dict(split=1, access=True, dimensions=True, tool=2, contacts=True, walls=1, return_ids=True, return_labels=True)
    feats, ids, lab = fn.recognize(clf_gpu, vox, device=DEV, **kw)
    cfeats, cids, clab = fn.recognize(clf, vox, device="cpu", **kw)
    assert np.array_equal(ids, cids) and plain(feats) == plain(cfeats) and np.array_equal(lab > 0, clab > 0)
    assert all(f.component is not None and f.peak2 == f.clearance2 for fs in feats for f in fs)
    # the classes are those of the classifier on each piece alone, on this device
    occ = torch.from_numpy(vox).to(DEV)
    d2 = fn.distance_transform(vox, device=DEV)
    new, table, offsets, comp, peak2 = watershed.split_instances(torch.from_numpy(ids0).to(DEV),
                                                                 torch.from_numpy(d2).to(DEV), 1)
    assert np.array_equal(new.cpu().numpy(), ids)
    cls, prob, _ = isolate.recognize_table(clf_gpu, new, table, offsets)
    assert [f.recognized for fs in feats for f in fs] == cls.tolist()
    assert [f.recognized_prob for fs in feats for f in fs] == prob.tolist()
    whole, _, _ = fn.recognize(clf_gpu, vox, device=DEV)
    again, _, _ = fn.recognize(clf_gpu, vox, device=DEV, split=None)
    assert whole == again and sum(map(len, feats)) > sum(map(len, whole)) and occ.is_cuda
    lids, recs = fn.label_components(labels, device=DEV, occupancy=vox, split=1, contacts=True, dimensions=True)
    cl, crecs = fn.label_components(labels, device="cpu", occupancy=vox, split=1, contacts=True, dimensions=True)
    assert np.array_equal(lids, cl) and recs == crecs


def test_dumbbell_on_the_device():
    ids, occ = dumbbell()
    new, feats = fn.split_features(ids, occupancy=occ, merge=1, device=DEV)
    want, cfeats = fn.split_features(ids, occupancy=occ, merge=1, device="cpu")
    assert np.array_equal(new, want) and feats == cfeats and len(feats[0]) == 2
    one, feats = fn.split_features(ids, occupancy=occ, merge=8, device=DEV)
    assert np.array_equal(one, ids.numpy()) and len(feats[0]) == 1
