"""The watershed split of touching features (``ops.watershed``, ``ops.reference.watershed_*``,
``fn.split_features``, the ``split`` option of ``fn.recognize`` / ``fn.label_components``, the CLI) on the CPU.

The oracle is held against per-voxel loops written from the definition, the merge test against exact rational
arithmetic, and the whole split against its properties and against pinned counts on generated parts."""
import functools
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from _watershed_cases import case, components, dumbbell, loop_ascend, loop_saddles, same_partition
from featurenet_amd.cli import main
from featurenet_amd.models.featurenet3d import FeatureNet3D, FeatureNet3DConfig
from featurenet_amd.ops import overlap, reference, watershed

SMALL = [(1, 1, 1, 1), (1, 1, 1, 9), (2, 3, 4, 5), (1, 6, 7, 9), (2, 5, 2, 7)]


def small_inputs(N, D, H, W):
    g = torch.Generator().manual_seed(D * 100 + H * 10 + W)
    noise_ids = torch.randint(0, 4, (N, D, H, W), generator=g, dtype=torch.int32)
    yield "ties", noise_ids, torch.randint(0, 5, (N, D, H, W), generator=g, dtype=torch.int32)
    yield "negative", noise_ids, torch.randint(-3, 3, (N, D, H, W), generator=g, dtype=torch.int32)
    occ = (torch.rand(N, D, H, W, generator=g) < 0.3).to(torch.uint8)
    yield "d2", components((occ == 0).to(torch.uint8), 26), reference.distance_sq(occ)
    yield "d2-noise-ids", noise_ids, reference.distance_sq(occ)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_the_oracle_against_a_per_voxel_loop(shape):
    for what, ids, height in small_inputs(*shape):
        roots = reference.watershed_ascend(ids, height)
        want_parent, want_roots = loop_ascend(ids, height)
        assert roots.dtype == torch.int32 and torch.equal(roots, want_roots), what
        assert torch.equal(reference.watershed_parents(ids, height), want_parent), what
        bids, table, offsets = reference.instance_table((ids > 0).to(torch.uint8), roots)
        pairs = reference.watershed_saddles(ids, bids, offsets, height)
        assert pairs.dtype == torch.int64 and torch.equal(pairs, loop_saddles(ids, bids, offsets, height)), what
        got_roots, flags = watershed.ascend(ids, height)             # the op layer's CPU path is the oracle
        assert torch.equal(got_roots, roots) and flags.shape == roots.shape and flags.dtype == torch.int32
        assert torch.equal(watershed.saddle_pairs(ids, bids, offsets, height), pairs)
        # rows that do not belong to the offsets are dropped, as the loop drops them
        off2 = offsets - 2
        assert torch.equal(reference.watershed_saddles(ids, bids, off2, height), loop_saddles(ids, bids, off2, height))


def test_saddle_pairs_exist_on_the_small_inputs():
    """The loop comparison above is not vacuous: the small volumes do hold touching basins."""
    ids, height = next(iter(small_inputs(1, 6, 7, 9)))[1:]
    roots = reference.watershed_ascend(ids, height)
    bids, table, offsets = reference.instance_table((ids > 0).to(torch.uint8), roots)
    assert len(reference.watershed_saddles(ids, bids, offsets, height)) > 10


def test_the_merge_rule_is_the_exact_inequality():
    """``2 sqrt(p) - 2 sqrt(s) <= m`` for integers, decided without a root.  With ``a = 4p - 4s - m^2`` it is ``a
    <= 4 m sqrt(s)``; a root-free second opinion in rationals: it holds iff ``a <= 0``, or ``a > 0`` and ``(a / (4
    m))^2 <= s`` (``m > 0`` there, since ``m = 0`` and ``a > 0`` mean ``p > s``).  Around every perfect-square pair the
    rule must flip exactly where ``sqrt(p) - sqrt(s)`` crosses ``m / 2``."""
    top = 3 * 255 ** 2
    peaks = sorted({0, 1, 2, 3, 4, 5, 8, 9, 10, 16, 24, 25, 26, 49, 50, 100, 101, 255 ** 2, 2 * 255 ** 2, top - 1, top})
    for m in (0, 1, 2, 3, 4, 7, 16, 100):
        for p in peaks:
            for s in [q for q in peaks if q <= p] + [p - 1 if p else 0]:
                a = Fraction(4 * p - 4 * s - m * m)
                want = a <= 0 or (m > 0 and (a / (4 * m)) ** 2 <= s)
                assert watershed.joins(p, s, m) == want, (p, s, m)
    for r in (1, 2, 5, 17, 255):                 # p = (r + k)^2 over s = r^2: the difference of the roots is k
        for k in (0, 1, 2, 3):
            p, s = (r + k) ** 2, r * r
            assert watershed.joins(p, s, 2 * k) and watershed.joins(p - 1, s, 2 * k) if k else True
            assert not watershed.joins(p + 1, s, 2 * k)
            if k:
                assert not watershed.joins(p, s, 2 * k - 1)
    for merge, m in ((0, 0), (0.5, 1), (1, 2), (1.0, 2), ("2.5", 5), (Fraction(7, 2), 7), (8, 16)):
        assert watershed.merge_steps(merge) == m
    for bad in (-1, 0.25, 1 / 3, float("nan"), float("inf"), True, "x", None):
        with pytest.raises(ValueError, match="merge"):
            watershed.merge_steps(bad)


def test_merging_visits_the_highest_saddle_first():
    """Three basins in a row, peaks 100, 36, 100, saddles 25 (rows 0-1) and 16 (rows 1-2): at m = 2 the middle one
    (2 sqrt 36 - 2 sqrt 25 = 2) joins row 0 over the higher saddle, and the group, now of peak 100, stays apart
    from row 2 (2 sqrt 100 - 2 sqrt 16 = 12); the representative is the higher member."""
    table = torch.zeros(3, 13, dtype=torch.int64)
    table[:, 3] = torch.tensor([5, 9, 2])
    peak = torch.tensor([100, 36, 100])
    pairs = torch.tensor([[0, 1, 25], [1, 2, 16]])
    group, rep = watershed.merge_groups(pairs, table, 2, peak)
    assert group.tolist() == [0, 0, 1] and rep.tolist() == [0, 2]
    group, rep = watershed.merge_groups(pairs, table, 12, peak)
    assert group.tolist() == [0, 0, 0] and rep.tolist() == [2]                  # equal peaks: the lower root stands
    group, rep = watershed.merge_groups(pairs, table, 0, peak)
    assert group.tolist() == [0, 1, 2] and rep.tolist() == [0, 1, 2]
    group, rep = watershed.merge_groups(pairs[:0], table, 5, peak)
    assert group.tolist() == [0, 1, 2]


KINDS = [("noise", 2, 5, 6, 7), ("edt", 2, 12, 13, 20), ("touching", 1, 4, 5, 9), ("edt", 1, 9, 9, 65)]


@pytest.mark.parametrize("kind,N,D,H,W", KINDS)
def test_properties_of_the_split(kind, N, D, H, W):
    ids, height = case(kind, N, D, H, W)
    V = D * H * W
    roots, flags = watershed.ascend(ids, height)
    # basins subdivide components: a voxel and its root carry one id; nothing without an id has a root
    assert torch.equal(roots > 0, ids > 0)
    at = (roots.view(N, V).to(torch.int64) - 1).clamp(min=0)
    assert torch.equal(torch.where(ids.view(N, V) > 0, ids.view(N, V).gather(1, at), 0), ids.view(N, V).clamp(min=0))
    # every root is a local key maximum among its neighbours of the same id
    lin = torch.arange(V).view(1, D, H, W)
    key = height.clamp(min=0).to(torch.int64) << 32 | (0xFFFFFFFF - lin)
    beaten = torch.zeros(ids.shape, dtype=torch.bool)
    for dst, src in reference._ws_shifts(D, H, W, False):
        beaten[dst] |= (ids[dst] == ids[src]) & (key[src] > key[dst])
    assert torch.equal(flags.bool(), (ids > 0) & ~beaten)
    for merge in (0, 1, 2.5):
        new, table, offsets, comp, peak2 = watershed.split_instances(ids, height, merge)
        what = (kind, merge)
        assert new.dtype == torch.int32 and torch.equal(new > 0, ids > 0), what
        # the new instances subdivide the components too, and say which one they came from
        row = (new.to(torch.int64) + offsets[:-1].view(N, 1, 1, 1) - 1)[new > 0]
        assert torch.equal(comp[row], ids[new > 0].to(torch.int64)), what
        assert torch.equal(peak2, torch.full_like(peak2, -1).scatter_reduce(
            0, row, height[new > 0].clamp(min=0).to(torch.int64), "amax")), what
        # the table is the instance table of the new ids: the rows are numbered by each group's lowest basin, the
        # oracle's by the root, which is the representative's here -- the same rows in another order
        rows = torch.zeros(new.shape, dtype=torch.int64)
        rows[new > 0] = row
        fake_roots = torch.where(new > 0, table[:, 3][rows], 0)
        _, want, want_off = reference.instance_table((new > 0).to(torch.uint8), fake_roots.to(torch.int32))
        order = torch.argsort(table[:, 0] * V + table[:, 3])
        assert torch.equal(table[order], want) and torch.equal(offsets, want_off), what
        assert int(height.view(N, V)[table[:, 0], table[:, 3] - 1].clamp(min=0).ne(peak2).sum()) == 0, what
    fewer = [watershed.split_instances(ids, height, m)[1].shape[0] for m in (0, 0.5, 1, 3, 300)]
    assert fewer == sorted(fewer, reverse=True) and fewer[-1] == reference.instance_table(
        (ids > 0).to(torch.uint8), reference.connected_components(ids.to(torch.uint8), 0, 26))[1].shape[0]


@pytest.mark.parametrize("value", [0, 7, reference.EDT_INF])
def test_constant_height_returns_the_input_partition(value):
    for kind, N, D, H, W in KINDS[:3]:
        ids = case(kind, N, D, H, W)[0]              # the partition: 6-components of the carved block, else the ids' 26-components
        ids = components((ids > 0).to(torch.uint8), 6) if kind == "edt" else components(ids.to(torch.uint8), 26)
        height = torch.full(ids.shape, value, dtype=torch.int32)
        for merge in (0, 1, 40):
            new, table, offsets, comp, peak2 = watershed.split_instances(ids, height, merge)
            assert same_partition(new, ids) and bool((peak2 == value).all()), (kind, value, merge)
            # both number a sample's sets by their lowest voxel: the very ids
            assert torch.equal(new, ids) and torch.equal(comp, torch.cat(
                [torch.arange(1, int(ids[n].max()) + 1) for n in range(N)])), (kind, value, merge)


def test_dumbbell():
    ids, occ = dumbbell()
    assert int(ids.max()) == 1
    for dev_fn in (lambda: fn.split_features(ids.numpy(), occupancy=occ.numpy(), merge=1, device="cpu"),
                   lambda: fn.split_features(ids, height=reference.distance_sq(occ), merge=1.0, device="cpu")):
        new, feats = dev_fn()
        assert new.dtype == np.int32 and len(feats) == 1 and len(feats[0]) == 2
        big, small = sorted(feats[0], key=lambda f: -f.voxels)
        assert big.component == small.component == 1 and big.peak2 > small.peak2 >= 16
        assert big.centroid[2] < 11 < small.centroid[2] and big.voxels + small.voxels == int((ids > 0).sum())
        assert set(big.to_dict()) >= {"component", "peak2"}
    one, feats = fn.split_features(ids, occupancy=occ, merge=8, device="cpu")
    assert len(feats[0]) == 1 and np.array_equal(one, ids.numpy()) and feats[0][0].peak2 == big.peak2
    with pytest.raises(ValueError, match="exactly one"):
        fn.split_features(ids, device="cpu")
    with pytest.raises(ValueError, match="exactly one"):
        fn.split_features(ids, occupancy=occ, height=occ, device="cpu")
    with pytest.raises(ValueError, match="merge"):
        fn.split_features(ids, occupancy=occ, merge=0.3, device="cpu")
    with pytest.raises(ValueError, match="integers"):
        fn.split_features(ids.float(), occupancy=occ, device="cpu")
    with pytest.raises(ValueError, match="but ids"):
        fn.split_features(ids, occupancy=occ[:, :5], device="cpu")


# ---------------------------------------------------------------------------------------------
# generated parts
# ---------------------------------------------------------------------------------------------
N_PARTS, SIZE = 96, 64


def matched(ids: torch.Tensor, offsets: torch.Tensor, voxels: torch.Tensor, slots: torch.Tensor) -> tuple:
    """``(instances, truth features, matches)``: class-agnostic matches at IoU > 0.5 of an id volume against the
    ``slots`` volume of ``generate_parts`` (truth id = slot), through ``ops.overlap``."""
    N = ids.shape[0]
    K = int(slots.max())
    off_b = torch.arange(N + 1, dtype=torch.int64) * K
    truth = torch.bincount((slots.reshape(N, -1).to(torch.int64) + off_b[:-1, None] - 1)[slots.reshape(N, -1) > 0],
                           minlength=N * K)
    pairs = overlap.overlap_table(ids, offsets, slots.to(torch.int32), off_b)
    inter = pairs[:, 2]
    hit = 3 * inter > voxels[pairs[:, 0]] + truth[pairs[:, 1]]                 # inter / union > 1 / 2
    return int(offsets[-1]), int((truth > 0).sum()), int(hit.sum())


@functools.lru_cache(maxsize=None)
def parts(separate: bool):
    vox, labels, _, slots = fn.generate_parts(N_PARTS, SIZE, seed=3, separate=separate, device="cpu", return_slots=True)
    occ = torch.from_numpy(vox)
    removed = (occ == 0).to(torch.uint8)
    ids, table, offsets = reference.instance_table(removed, reference.connected_components(removed, 0, 6))
    return occ, torch.from_numpy(slots), ids, table, offsets, reference.distance_sq(occ)


def test_separate_parts_come_back_unchanged():
    occ, slots, ids, table, offsets, d2 = parts(True)
    new, table2, offsets2, comp, peak2 = watershed.split_instances(ids, d2, 1)
    assert torch.equal(new, ids) and torch.equal(offsets2, offsets)
    assert torch.equal(table2[:, [0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12]], table[:, [0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12]])
    assert matched(ids, offsets, table[:, 2], slots) == (252, 246, 240)
    assert watershed.split_instances(ids, d2, 0)[1].shape[0] == 307


def test_touching_parts_match_the_truth_better_after_the_split():
    occ, slots, ids, table, offsets, d2 = parts(False)
    before = matched(ids, offsets, table[:, 2], slots)
    new, table2, offsets2, comp, peak2 = watershed.split_instances(ids, d2, 1)
    after = matched(new, offsets2, table2[:, 2], slots)
    print("before", before, "after", after)
    assert after[2] >= before[2]
    assert before == (206, 245, 189) and after == (219, 245, 199)
    assert watershed.split_instances(ids, d2, 0)[1].shape[0] == 267


# ---------------------------------------------------------------------------------------------
# API and CLI
# ---------------------------------------------------------------------------------------------
S = 16


def classifier(seed: int = 0) -> FeatureNet3D:
    torch.manual_seed(seed)
    return FeatureNet3D(FeatureNet3DConfig.tiny()).eval()


@functools.lru_cache(maxsize=None)
def touching_parts(n: int = 8):
    vox, labels, _ = fn.generate_parts(n, S, seed=3, features=(2, 4), separate=False, device="cpu")
    return vox, labels


def test_split_none_leaves_recognize_and_label_components_alone():
    vox, labels = touching_parts()
    clf = classifier()
    kw = dict(device="cpu", access=True, dimensions=True, tool=2, contacts=True, walls=1, return_ids=True,
              return_labels=True)
    feats, ids, lab = fn.recognize(clf, vox, **kw)
    feats2, ids2, lab2 = fn.recognize(clf, vox, split=None, **kw)
    assert feats2 == feats and np.array_equal(ids2, ids) and np.array_equal(lab2, lab)
    assert all(f.component is None and f.peak2 is None and "component" not in f.to_dict() for fs in feats for f in fs)
    ids3, recs = fn.label_components(labels, device="cpu", occupancy=vox, dimensions=True, contacts=True)
    ids4, recs2 = fn.label_components(labels, device="cpu", occupancy=vox, dimensions=True, contacts=True, split=None)
    assert recs2 == recs and np.array_equal(ids3, ids4)
    with pytest.raises(ValueError, match="split needs occupancy"):
        fn.label_components(labels, device="cpu", split=1)


def test_recognize_and_label_components_with_a_split():
    vox, labels = touching_parts()
    clf = classifier()
    plain, ids0, _ = fn.recognize(clf, vox, device="cpu", return_ids=True)
    feats, ids, lab = fn.recognize(clf, vox, device="cpu", split=1, dimensions=True, tool=2, contacts=True,
                                   return_ids=True, return_labels=True)
    want_ids, want = fn.split_features(ids0, occupancy=vox, merge=1, device="cpu")
    assert np.array_equal(ids, want_ids) and sum(map(len, feats)) > sum(map(len, plain))
    for fs, ws in zip(feats, want):
        assert [(f.id, f.voxels, f.bbox, f.component, f.peak2) for f in fs] == \
               [(w.id, w.voxels, w.bbox, w.component, w.peak2) for w in ws]
        assert all(f.recognized is not None and f.cls == f.recognized + 1 and f.clearance2 == f.peak2 for f in fs)
    assert np.array_equal(lab > 0, ids > 0)
    # every table describes the pieces: the same records come from the split ids as a label volume of their own
    d = feats[0][0].to_dict()
    assert d["component"] >= 1 and d["peak2"] == d["clearance2"] and json.dumps(d)
    ids5, recs = fn.label_components(labels, device="cpu", occupancy=vox, split=1, contacts=True)
    whole_ids, whole = fn.label_components(labels, device="cpu", occupancy=vox, contacts=True)
    assert sum(map(len, recs)) >= sum(map(len, whole))
    for n, fs in enumerate(recs):                # a piece keeps the class of the component it was cut from
        by_id = {w.id: w for w in whole[n]}
        assert all(f.cls == by_id[f.component].cls for f in fs)
        assert sum(f.voxels for f in fs) == sum(w.voxels for w in whole[n])
    assert same_partition(torch.from_numpy(ids5), torch.from_numpy(
        fn.split_features(whole_ids, occupancy=vox, merge=1, device="cpu")[0]))


def test_cli_round_trip(tmp_path, capsys):
    ids, occ = dumbbell()
    np.save(tmp_path / "ids.npy", ids.numpy())
    np.save(tmp_path / "vox.npy", occ.numpy())
    assert main(["split", str(tmp_path / "ids.npy"), str(tmp_path / "vox.npy"), "-o", str(tmp_path / "out.npy"),
                 "--merge", "1", "--device", "cpu", "--json", str(tmp_path / "out.json")]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert doc == json.loads((tmp_path / "out.json").read_text())
    want_ids, want = fn.split_features(ids, occupancy=occ, merge=1, device="cpu")
    assert np.array_equal(np.load(tmp_path / "out.npy"), want_ids)
    assert doc["samples"] == [[f.to_dict() for f in fs] for fs in want] and len(doc["samples"][0]) == 2
    assert main(["split", str(tmp_path / "ids.npy"), str(tmp_path / "vox.npy"), "-o", str(tmp_path / "one.npy"),
                 "--merge", "8", "--device", "cpu"]) == 0
    assert len(json.loads(capsys.readouterr().out)["samples"][0]) == 1
    vox, _ = touching_parts()
    clf = classifier()
    path = fn.save(clf, tmp_path / "clf.fnk", {"model_kind": "featurenet3d", "config": clf.cfg.to_dict()})
    np.save(tmp_path / "parts.npy", vox)
    assert main(["recognize", str(path), str(tmp_path / "parts.npy"), "--device", "cpu", "--split"]) == 0
    doc = json.loads(capsys.readouterr().out)
    want, _, _ = fn.recognize(str(path), vox, device="cpu", split=1.0)
    assert doc["samples"] == [[f.to_dict() for f in fs] for fs in want] and "component" in doc["samples"][0][0]
    assert main(["recognize", str(path), str(tmp_path / "parts.npy"), "--device", "cpu"]) == 0
    assert "component" not in json.loads(capsys.readouterr().out)["samples"][0][0]
