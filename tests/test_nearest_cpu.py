"""The labelled distance transform and the wall table on the CPU: the oracle (``ops.reference.nearest_labels``,
``wall_table``) against brute force, scipy and the definitions, its invariants, and the paths built on it
(``fn.nearest_instances``, ``fn.label_components(walls=...)``, ``fn.extract_features(walls=...)``, the CLI)."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from _ccl_cases import PATTERNS
from _nearest_cases import (BIG, IDS, PARTS, PARTS_TOUCHING, SHAPES, brute_nearest, expected_nn, expected_walls, ids,
                            judge, loop_other, loop_wall_table, parts_summary)
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg
from featurenet_amd.ops import nearest, reference
from featurenet_amd.ops.reference import EDT_INF, NN_MAX_S, NN_NONE
from featurenet_amd.utils.seginstances import FeatureInstance, wall_threshold

S, NC = 16, 4


# --- the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.02, 0.15, 0.6])
def test_oracle_against_all_pairs(density):
    rng = np.random.default_rng(int(density * 1000))
    for shape in ((6, 6, 6), (3, 5, 6), (1, 1, 6), (2, 6, 1), (4, 4, 4)):
        for top in (1, 2, 3):
            vol = np.where(rng.random(shape) < density, rng.integers(1, top + 1, shape), rng.integers(-1, 1, shape))
            got = reference.nearest_labels(torch.from_numpy(vol[None].astype(np.int32)))
            assert np.array_equal(got[0].numpy(), brute_nearest(vol)), (shape, top, density)


def test_rank_zero_distances_against_scipy():
    from scipy import ndimage

    for kind in ("dense", "sparse", "ends", "ties", "big"):
        for D, H, W in SHAPES:
            v, nn = ids(kind, 2, D, H, W), expected_nn(kind, 2, D, H, W)
            for n in range(2):
                if not bool((v[n] > 0).any()):
                    assert bool((nn[n] == NN_NONE).all())
                    continue
                # (exact: the squared distances are integers below 2^53)
                d = ndimage.distance_transform_edt(~(v[n] > 0).numpy())
                assert np.array_equal(np.rint(d * d).astype(np.int64), (nn[n, 0] >> 32).numpy()), (kind, D, H, W, n)


@pytest.mark.parametrize("kind", IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_invariants(shape, kind):
    D, H, W = shape
    for N in (1, 2):
        v, nn = ids(kind, N, D, H, W), expected_nn(kind, N, D, H, W)
        assert nn.shape == (N, 2, D, H, W) and nn.dtype == torch.int64 and bool((nn > 0).all())
        d, lab = nn >> 32, nn & 0xFFFFFFFF
        seed = v > 0
        assert torch.equal(d[:, 0].to(torch.int32), reference.distance_sq(seed.to(torch.uint8)))
        assert bool((d[:, 0][seed] == 0).all()) and torch.equal(lab[:, 0][seed], v[seed].to(torch.int64))
        assert bool((d[:, 1] >= d[:, 0]).all())
        assert bool(((lab[:, 0] != lab[:, 1]) | ((lab[:, 0] == 0) & (lab[:, 1] == 0))).all())
        for n in range(N):
            labels = torch.unique(v[n][v[n] > 0])
            assert bool((nn[n, 0] == NN_NONE).all()) == (len(labels) == 0)
            assert bool((nn[n, 1] == NN_NONE).all()) == (len(labels) < 2)
            assert set(lab[n].unique().tolist()) <= set(labels.tolist()) | {0}
        if kind == "none":
            assert bool((nn == NN_NONE).all())
        if kind in ("one", "same-ends"):
            assert bool((nn[:, 1] == NN_NONE).all()) and bool((nn[:, 0] < NN_NONE).all())
        if kind == "big":
            assert set(lab.unique().tolist()) == {BIG, BIG - 1}
        if kind == "ties":                                    # at equal distances the smaller id is rank 0
            tie = d[:, 0] == d[:, 1]
            assert bool(tie.any()) and bool((lab[:, 0][tie] < lab[:, 1][tie]).all())
        # samples never see each other
        if N == 2:
            for n in range(2):
                assert torch.equal(reference.nearest_labels(v[n:n + 1].contiguous())[0], nn[n])


@pytest.mark.parametrize("pattern", PATTERNS)
def test_wall_table_against_the_definitions(pattern):
    for (D, H, W), limit2 in zip(SHAPES, (0, 1, 4, 9)):
        v, table, offsets, nn, wall = expected_walls(pattern, 2, D, H, W, limit2)
        T = len(table)
        want = loop_wall_table(v.numpy(), offsets.numpy(), nn.numpy(), T, limit2)
        assert wall.shape == (T, 5) and np.array_equal(wall[:, [0, 1, 3, 4]].numpy(), want), (pattern, D, H, W)
        assert np.array_equal(wall[:, 2].numpy(), loop_other(v.numpy(), offsets.numpy(), nn.numpy(), wall.numpy()))
        assert torch.equal(wall[:, 4], table[:, 2])
        has = wall[:, 0] >= 0
        assert bool((wall[~has][:, :3] == -1).all()) and bool((wall[has][:, 0] >= 1).all())
        if bool(has.any()):                                   # the other's own gap is no larger, and it is another row
            other = wall[has][:, 2]
            assert bool((wall[other][:, 0] <= wall[has][:, 0]).all()) and bool((wall[other][:, 0] >= 1).all())
            assert bool((other != torch.arange(T)[has]).all())
            assert torch.equal(table[other][:, 0], table[has][:, 0])         # of the same sample
        assert bool((wall[:, 3] <= wall[:, 4]).all())
        assert torch.equal(wall[:, 3] > 0, has & (wall[:, 0] <= limit2))
        # the op layer on CPU tensors is the reference
        got, none = nearest.wall_table(v, offsets, limit2)
        assert none is None and torch.equal(got, wall)
        got, nn2 = nearest.wall_table(v, offsets, limit2, rows=T, want_nn=True)
        assert judge(nn2, nn, got, wall)


def test_rows_outside_the_table_count_nowhere():
    D, H, W = SHAPES[2]
    v = torch.arange(1, D * H * W + 1, dtype=torch.int32).view(1, D, H, W)
    nn = reference.nearest_labels(v)
    assert bool(((nn[:, 1] >> 32) == 1).all())
    for offsets in (torch.tensor([0, 100]), torch.tensor([-50, 50])):
        T = int(offsets[-1])
        got = reference.wall_table(v, offsets, nn, 0)
        want = loop_wall_table(v.numpy(), offsets.numpy(), nn.numpy(), T, 0)
        assert np.array_equal(got[:, [0, 1, 3, 4]].numpy(), want)
        assert bool((got[:, 0] == 1).all()) and bool((got[:, 4] == 1).all()) and bool((got[:, 3] == 0).all())
        assert got[:, 1].tolist() == list(range(-int(offsets[0]), T - int(offsets[0])))
    empty = reference.wall_table(v, torch.tensor([0, 0]), nn, 0)
    assert empty.shape == (0, 5)


def test_the_comparison_rejects_near_misses():
    v, table, offsets, nn, wall = expected_walls("blobs", 2, *SHAPES[3], 9)
    assert judge(nn.clone(), nn, wall.clone(), wall)
    off = nn.clone()
    off[1, 1, 2, 3, 77] += 1                                  # a label one too large
    assert not judge(off, nn, wall, wall)
    loose = wall.clone()
    loose[:, 3] = reference.wall_table(v, offsets, nn, 10)[:, 3]
    assert not torch.equal(loose, wall) and not judge(nn, nn, loose, wall)
    flat_ids, flat_d = v[0].reshape(-1), (nn[0, 1] >> 32).reshape(-1)
    moved = None
    for k in range(int(offsets[1])):                          # an `at` that took the last voxel of a tie
        tie = ((flat_ids == k + 1) & (flat_d == wall[k, 0])).nonzero().view(-1)
        if len(tie) > 1:
            moved = wall.clone()
            moved[k, 1] = tie[-1]
            assert int(tie[0]) == int(wall[k, 1])
            break
    assert moved is not None and not judge(nn, nn, moved, wall)


def test_arguments_are_checked():
    v = torch.zeros(1, 2, 3, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match=f"at most {NN_MAX_S}"):
        nearest.nearest_labels(torch.zeros(1, 1, 1, NN_MAX_S + 1, dtype=torch.int32))
    with pytest.raises(ValueError, match=f"at most {NN_MAX_S}"):
        reference.nearest_labels(torch.zeros(1, NN_MAX_S + 1, 1, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        nearest.nearest_labels(v.long())
    with pytest.raises(ValueError, match="int32"):
        nearest.wall_table(v[0], torch.tensor([0, 0]))
    with pytest.raises(ValueError, match="offsets"):
        nearest.wall_table(v, torch.tensor([0, 0, 0]))
    for bad in (-1, EDT_INF, 1.0, True):
        with pytest.raises(ValueError, match="limit2"):
            nearest.wall_table(v, torch.tensor([0, 0]), bad)
    assert nearest.nearest_labels(v[:0]).shape == (0, 2, 2, 3, 4)
    assert nearest.wall_table(v[:0], torch.tensor([0]))[0].shape == (0, 5)
    assert NN_MAX_S == 128 and NN_NONE == EDT_INF << 32


# --- records ----------------------------------------------------------------------------------------
def test_wall_threshold_is_exact():
    assert [wall_threshold(t) for t in (0, 1, 2, 0.5, "0.5", Fraction(1, 3), 1.9999)] == [1, 4, 9, 2, 2, 1, 8]
    # the double nearest to sqrt(2) lies above it, the one before it below: no rounding decides either
    assert wall_threshold(Fraction(1.4142135623730951) - 1) == 2 and wall_threshold(Fraction(1.4142135623730949) - 1) == 1
    assert wall_threshold(Fraction(41421, 100000)) == 1 and wall_threshold(Fraction(41422, 100000)) == 2
    for bad in (-1, True, "x", math.inf, math.nan, None, 1 << 20):
        with pytest.raises(ValueError, match="wall_threshold"):
            wall_threshold(bad)


def test_feature_instance_records():
    table = torch.tensor([[0, 3, 10, 1, 0, 1, 2, 4, 2, 3, 20, 15, 25], [0, 1, 4, 9, 1, 1, 1, 2, 2, 2, 6, 6, 6],
                          [1, 2, 5, 1, 0, 0, 0, 0, 0, 4, 0, 0, 10]])
    offsets = torch.tensor([0, 2, 3])
    walls = torch.tensor([[9, (2 * 4 + 1) * 5 + 3, 1, 6, 10], [1, 7, 0, 0, 4], [-1, -1, -1, 0, 5]])
    plain = FeatureInstance.from_table(table, offsets)
    rich = FeatureInstance.from_table(table, offsets, walls=walls, shape=(6, 4, 5))
    a, (b, c), (alone,) = plain[0][0], rich[0], rich[1]
    assert a == FeatureInstance(1, 3, 10, (0, 1, 2, 4, 2, 3), (2.0, 1.5, 2.5)) and not a.walls
    assert (a.gap2, a.gap_at, a.gap_to, a.thin_voxels, a.gap, a.min_wall) == (None,) * 6
    assert a.to_dict() == {"id": 1, "class": 3, "voxels": 10, "bbox": [0, 1, 2, 4, 2, 3], "centroid": [2.0, 1.5, 2.5]}
    assert (b.gap2, b.gap_at, b.gap_to, b.thin_voxels, b.gap, b.min_wall) == (9, (2, 1, 3), 2, 6, 3.0, 2.0) and b != a
    assert (c.gap2, c.gap_at, c.gap_to, c.thin_voxels, c.gap, c.min_wall) == (1, (0, 1, 2), 1, 0, 1.0, 0.0)
    assert alone.walls and (alone.gap2, alone.gap_at, alone.gap_to, alone.gap, alone.min_wall) == (None,) * 5
    assert alone.thin_voxels == 0
    d = b.to_dict()
    assert {k: d[k] for k in a.to_dict()} == a.to_dict() and json.loads(json.dumps(d)) == d
    assert {k: d[k] for k in d if k not in a.to_dict()} == \
        {"gap2": 9, "gap_at": [2, 1, 3], "gap_to": 2, "min_wall": 2.0, "thin_voxels": 6}
    assert {k: v for k, v in alone.to_dict().items() if k.startswith(("gap", "min_", "thin"))} == \
        {"gap2": None, "gap_at": None, "gap_to": None, "min_wall": None, "thin_voxels": 0}
    assert FeatureInstance(1, 1, 1, (0,) * 6, (0.0,) * 3, gap2=2).min_wall == math.sqrt(2) - 1
    unlimited = FeatureInstance.from_table(table, offsets, walls=walls, shape=(6, 4, 5), thin=False)
    assert all(f.thin_voxels is None and f.walls for fs in unlimited for f in fs) and unlimited[0][0].gap2 == 9
    assert unlimited[0][0].to_dict()["thin_voxels"] is None
    kept = FeatureInstance.from_table(table, offsets, min_voxels=5, walls=walls, shape=(6, 4, 5))
    assert [f.id for f in kept[0]] == [1] and kept[0][0].gap_to == 2
    with pytest.raises(ValueError, match="wall table"):
        FeatureInstance.from_table(table, offsets, walls=walls[:, [0, 1, 2, 4, 3]], shape=(6, 4, 5))
    with pytest.raises(ValueError, match="wall table"):
        FeatureInstance.from_table(table, offsets, walls=walls[:1], shape=(6, 4, 5))
    with pytest.raises(ValueError, match="shape"):
        FeatureInstance.from_table(table, offsets, walls=walls)


# --- public API on the CPU path ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg():
    torch.manual_seed(0)
    m = FeatureNet3DSeg(S, num_classes=NC).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for c in list(m.enc) + [m.dec]:
            c.running_mean.copy_(torch.randn(c.cout, generator=g) * 0.1)
            c.running_var.copy_(torch.rand(c.cout, generator=g) + 0.5)
        m.head.bias.copy_(torch.randn(NC, generator=g) * 0.1)
    x = torch.rand(3, S, S, S, generator=g) < 0.4
    return m, x


def test_nearest_instances_api():
    assert "nearest_instances" in fn.__all__
    v = ids("dense", 2, *SHAPES[0])
    want = expected_nn("dense", 2, *SHAPES[0])
    for arg in (v.numpy(), v, v.to(torch.int64), v.numpy().astype(np.int16)):
        d2, near = fn.nearest_instances(arg, device="cpu")
        assert d2.dtype == near.dtype == np.int32 and d2.shape == near.shape == (2, 2) + SHAPES[0]
        assert np.array_equal(d2, (want >> 32).numpy()) and np.array_equal(near, (want & 0xFFFFFFFF).numpy())
    d2, near = fn.nearest_instances(v[1].numpy(), device="cpu")
    assert d2.shape == (2,) + SHAPES[0] and np.array_equal(near, (want[1] & 0xFFFFFFFF).numpy())
    big = ids("big", 1, *SHAPES[0])
    d2, near = fn.nearest_instances(big.numpy().astype(np.int64), device="cpu")
    assert set(np.unique(near).tolist()) == {BIG, BIG - 1} and int(d2.max()) < EDT_INF
    for bad in (v.float(), v[0, 0], v > 0, np.full((1, 1, 1, 1), 2 ** 31, np.int64)):
        with pytest.raises(ValueError, match="nearest_instances"):
            fn.nearest_instances(bad, device="cpu")


def test_label_components_with_walls():
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 3, (2, 6, 7, 8), generator=g) * (torch.rand(2, 6, 7, 8, generator=g) < 0.5)
    occ = torch.rand(2, 6, 7, 8, generator=g) < 0.3
    ids0, plain = fn.label_components(lab.numpy(), device="cpu")
    ids1, feats = fn.label_components(lab.numpy(), device="cpu", walls=1)
    _, unlimited = fn.label_components(lab.numpy(), device="cpu", walls=True)
    _, with_all = fn.label_components(lab.numpy(), device="cpu", occupancy=occ.numpy(), dimensions=True, contacts=True,
                                      walls=1.0)
    _, without = fn.label_components(lab.numpy(), device="cpu", occupancy=occ.numpy(), dimensions=True, contacts=True)
    roots = reference.connected_components(lab.to(torch.uint8), 0, 6)
    want_ids, table, offsets = reference.instance_table(lab.to(torch.uint8), roots)
    nn = reference.nearest_labels(want_ids)
    wall = reference.wall_table(want_ids, offsets, nn, 4)
    assert np.array_equal(ids1, ids0) and np.array_equal(ids1, want_ids.numpy())
    assert feats == FeatureInstance.from_table(table, offsets, walls=wall, shape=(6, 7, 8))
    assert plain == FeatureInstance.from_table(table, offsets) and all(not f.walls for fs in plain for f in fs)
    extra = ("gap2", "gap_at", "gap_to", "min_wall", "thin_voxels")
    strip = lambda fss: [[{k: v for k, v in f.to_dict().items() if k not in extra} for f in fs] for fs in fss]  # noqa: E731
    assert [[f.to_dict() for f in fs] for fs in plain] == strip(feats)
    assert [[f.to_dict() for f in fs] for fs in without] == strip(with_all)
    assert all(set(extra) <= set(f.to_dict()) for fs in feats for f in fs)
    assert [[(f.gap2, f.gap_at, f.gap_to) for f in fs] for fs in unlimited] == \
        [[(f.gap2, f.gap_at, f.gap_to) for f in fs] for fs in feats]
    assert all(f.thin_voxels is None for fs in unlimited for f in fs)
    assert [[(f.gap2, f.thin_voxels) for f in fs] for fs in with_all] == [[(f.gap2, f.thin_voxels) for f in fs] for fs in feats]
    seen = 0
    for n, fs in enumerate(feats):
        for f in fs:
            if f.gap2 is None:
                assert len(fs) == 1 and f.thin_voxels == 0
                continue
            z, y, x = f.gap_at
            seen += 1
            assert ids1[n, z, y, x] == f.id and f.gap_to != f.id and 1 <= f.gap_to <= len(fs)
            # the gap is the smallest distance between the two instances' voxels, and no third one is nearer
            mine = np.argwhere(ids1[n] == f.id)
            for o in fs:
                if o.id != f.id:
                    theirs = np.argwhere(ids1[n] == o.id)
                    d = ((mine[:, None, :] - theirs[None, :, :]) ** 2).sum(-1).min()
                    assert d >= f.gap2 and (o.id != f.gap_to or d == f.gap2)
            assert (f.thin_voxels > 0) == (f.gap2 <= 4)
    assert seen > 4
    # gap2 == 1 exactly where the contacts name a neighbour
    assert all((f.gap2 == 1) == bool(f.neighbors) for fs in with_all for f in fs)
    for bad in (-1, "x"):
        with pytest.raises(ValueError, match="wall_threshold"):
            fn.label_components(lab.numpy(), device="cpu", walls=bad)


def test_extract_features_with_walls(seg):
    m, x = seg
    xs = x.numpy().astype(np.uint8)
    labels, _ = fn.segment(m, xs, device="cpu")
    _, want = fn.label_components(labels, device="cpu", walls=2)
    feats, ids_ = fn.extract_features(m, xs, batch_size=2, device="cpu", walls=2)
    assert ids_ is None and feats == want and any(f.gap2 is not None for fs in feats for f in fs)
    _, want_all = fn.label_components(labels, device="cpu", occupancy=xs, dimensions=True, tool=2, contacts=True, walls=2)
    every, _ = fn.extract_features(m, xs, batch_size=2, device="cpu", access=True, dimensions=True, tool=2,
                                   contacts=True, walls=2)
    assert every == want_all
    plain, _ = fn.extract_features(m, xs, batch_size=2, device="cpu")
    assert all(not f.walls and f.gap2 is None for fs in plain for f in fs)
    xf = x[:2].float()
    three = m.instances(xf, want_ids=True)
    wall = reference.wall_table(three[2], three[1], reference.nearest_labels(three[2]), 9)
    four = m.instances(xf, want_walls=9)
    six = m.instances(xf.unsqueeze(-1), want_ids=True, want_access=True, want_dims=True, want_walls=9)
    assert len(three) == 3 and len(four) == 4 and len(six) == 6 and four[2] is None
    assert torch.equal(four[0], three[0]) and torch.equal(four[3], wall) and torch.equal(six[5], wall)
    assert torch.equal(six[2], three[2]) and six[3].shape == (len(wall), 8) and six[4].shape == (len(wall), 4)
    assert len(m.instances(xf, want_walls=None)) == 3


def test_cli_features_walls_and_nearest(seg, tmp_path, capsys):
    from featurenet_amd.cli import main

    m, x = seg
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    np.save(tmp_path / "x.npy", x.numpy().astype(np.uint8))
    assert main(["features", str(path), str(tmp_path / "x.npy")]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    extra = ("gap2", "gap_at", "gap_to", "min_wall", "thin_voxels")
    for args, thin in ((["--walls"], False), (["--walls", "1.5"], True)):
        assert main(["features", str(path), str(tmp_path / "x.npy")] + args) == 0
        doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        for recs, base in zip(doc["samples"], plain["samples"]):
            assert [{k: v for k, v in r.items() if k not in extra} for r in recs] == base
            assert not any(set(b) & set(extra) for b in base)
            for r in recs:
                assert (r["thin_voxels"] is not None) == thin
                if r["gap2"] is not None:
                    assert r["min_wall"] == max(0.0, math.sqrt(r["gap2"]) - 1) and len(r["gap_at"]) == 3
                    assert not thin or (r["thin_voxels"] > 0) == (r["gap2"] <= 6)
        if not torch.cuda.is_available():                    # (the checkpoint loads onto the GPU when there is one)
            feats, _ = fn.extract_features(m, x.numpy().astype(np.uint8), device="cpu", walls=1.5 if thin else True)
            assert doc["samples"] == [[f.to_dict() for f in fs] for fs in feats]
    v = ids("dense", 2, *SHAPES[0])
    np.save(tmp_path / "ids.npy", v.numpy())
    assert main(["nearest", str(tmp_path / "ids.npy"), "-o", str(tmp_path / "nn.npz"), "--device", "cpu",
                 "--json", str(tmp_path / "nn.json")]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = expected_nn("dense", 2, *SHAPES[0])
    with np.load(tmp_path / "nn.npz") as z:
        assert np.array_equal(z["d2"], (want >> 32).numpy()) and np.array_equal(z["nearest"], (want & 0xFFFFFFFF).numpy())
    assert out == json.loads((tmp_path / "nn.json").read_text())
    assert out == {"shape": [2, 2, *SHAPES[0]], "instance_voxels": int((v > 0).sum()), "min_gap_sq": 1,
                   "voxels_without_other": 0}


@pytest.mark.parametrize("separate", [True, False])
def test_generated_parts_have_the_pinned_gaps(separate):
    kw = {} if separate else {"separate": False}
    voxels, labels, parts = fn.generate_parts(96, size=32, seed=3, device="cpu", **kw)
    ids_, feats = fn.label_components(labels, device="cpu", occupancy=voxels, contacts=True, walls=True)
    got, pins = parts_summary(feats), PARTS if separate else PARTS_TOUCHING
    assert {k: got[k] for k in pins} == pins
    for n, fs in enumerate(feats):
        for f in fs:
            assert (f.gap2 is None) == (len(fs) == 1), (n, f)
            assert (f.gap2 == 1) == bool(f.neighbors), (n, f)
            if f.gap2 is not None:
                z, y, x = f.gap_at
                assert ids_[n, z, y, x] == f.id and f.gap_to in {o.id for o in fs} - {f.id}, (n, f)
    # one distance_sq per instance: the gap is the smallest distance of its voxels to any other instance's
    it = torch.from_numpy(ids_)
    for n in range(0, 96, 7):
        for f in feats[n]:
            others = ((it[n] > 0) & (it[n] != f.id)).to(torch.uint8)[None]
            d = reference.distance_sq(others)[0][it[n] == f.id]
            assert (None if int(d.min()) >= EDT_INF else int(d.min())) == f.gap2, (n, f)


# --- Python <-> _C plumbing -------------------------------------------------------------------------
class _FakeK:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args))


def test_nearest_calls_match_bindings(monkeypatch):
    from featurenet_amd import _native

    fk = _FakeK()
    monkeypatch.setattr(_native, "kernels", lambda: fk)
    monkeypatch.setattr(_native, "stream", lambda t=None: 0)
    monkeypatch.setattr(_native, "use_native", lambda t: True)
    v = torch.zeros(2, 3, 4, 5, dtype=torch.int32)
    off = torch.tensor([0, 4, 7])
    wall, nn = nearest.wall_table(v, off, 4, want_nn=True)
    assert wall.shape == (7, 5) and wall.dtype == torch.int64 and nn.shape == (2, 2, 3, 4, 5) and nn.dtype == torch.int64
    assert [n for n, _ in fk.calls] == ["nn_transform", "wall_stats"]
    t, s = fk.calls[0][1], fk.calls[1][1]          # ids t nn N D H W passes st ext
    assert t[0] == v.data_ptr() and t[1] == t[2] == nn.data_ptr() and t[3:8] == (2, 3, 4, 5, 3)
    assert t[-1] == [120, 240, 240]
    assert s[0] == v.data_ptr() and s[1] == off.data_ptr() and s[2] == nn.data_ptr() and s[4:10] == (2, 3, 4, 5, 7, 4)
    assert s[-1] == [120, 3, 240, 21]
