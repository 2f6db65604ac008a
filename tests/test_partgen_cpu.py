"""The part generator without a GPU: the host path (``_rt.carve_parts``) against the torch oracle
(``reference.carve_parts``), the meaning of the outputs, and the sampler (``_rt.sample_parts``).

Every comparison is exact.  The sampler's conditions are taken over ``PARTS`` = 2,000 parts at
S = 64 with 2..4 features: at most 1 % of them may end below two features (none do: the count
histogram is in profiles/part_generate.md), grown boxes are pairwise disjoint, and the labels'
6-connected components number exactly one per feature (two for class 16, a step on each of two
opposite edges).  The component count runs the reference CCL in slices of ``SLICE`` parts.
"""
import functools
import json

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from _partgen_cases import (BLIND, S, THROUGH, border_features, expected_components, face, row, single_features,
                            single_features_tight, table, tighten, unused)
from featurenet_amd import _native
from featurenet_amd.ops import partgen, reference
from featurenet_amd.utils.partfeatures import PartFeature, from_params

PARTS, BIG, SLICE = 2000, 64, 50


def host(params: torch.Tensor, size: int, threads: int = 4):
    return tuple(torch.from_numpy(a) for a in _native.runtime().carve_parts(params.numpy(), size, threads))


def same(got, want) -> bool:
    return len(got) == len(want) and all(g.dtype == torch.uint8 and torch.equal(g, w) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def big_tables() -> torch.Tensor:
    return partgen.sample(PARTS, BIG, 0, (2, 4), threads=4)


@functools.lru_cache(maxsize=None)
def big_labels() -> torch.Tensor:
    return host(big_tables(), BIG)[1]


# ---------------------------------------------------------------------------------------------
# host path == oracle
# ---------------------------------------------------------------------------------------------
def test_host_path_equals_the_oracle_on_every_class_and_orientation():
    params, want = single_features()
    assert params.shape == (576, 1, 16)
    assert same(host(params, S), want)
    tight, _ = single_features_tight()
    assert not torch.equal(tight, params)
    assert same(host(tight, S), want)                # exact boxes change nothing
    assert same(host(params, S, threads=1), want)


def test_host_path_equals_the_oracle_on_border_features():
    params, want = border_features()
    assert same(host(params, S), want)
    assert int((want[2] == 2).sum()) > 0             # second slots are visible too


@pytest.mark.parametrize("separate", [True, False])
@pytest.mark.parametrize("size,n", [(8, 5), (24, 3), (64, 2)])
def test_host_path_equals_the_oracle_on_sampler_tables(size, n, separate):
    params = partgen.sample(n, size, 5, (1, 6), separate=separate)
    assert params.shape == (n, 6, 16) and params.dtype == torch.int32
    assert same(host(params, size), reference.carve_parts(params, size))
    vox, labels, slots = partgen.carve(params, size, want_slots=True)
    assert same((vox, labels, slots), reference.carve_parts(params, size))
    bits, labels2 = partgen.carve(params, size, packed=True)
    assert torch.equal(labels2, labels)
    assert np.array_equal(bits.numpy(), np.packbits(vox.numpy().reshape(n, -1), axis=1, bitorder="little"))
    assert np.array_equal(_native.runtime().unpack_bits(bits[0].numpy(), size ** 3), vox[0].numpy().reshape(-1))


# ---------------------------------------------------------------------------------------------
# semantics
# ---------------------------------------------------------------------------------------------
def test_labels_mark_exactly_the_removed_voxels():
    for params, (occ, labels, slots) in (single_features(), border_features()):
        assert torch.equal(labels != 0, occ == 0) and torch.equal(slots != 0, occ == 0)
        cls = params[..., 0].to(torch.int64)
        idx = (slots.to(torch.int64) - 1).clamp(min=0).reshape(len(params), -1)
        assert torch.equal(torch.where(slots.reshape(len(params), -1) > 0, cls.gather(1, idx) + 1, 0),
                           labels.reshape(len(params), -1).to(torch.int64))


def test_every_class_removes_something_but_not_everything():
    _, (occ, labels, _) = single_features()
    removed = (occ == 0).reshape(576, -1).sum(1)
    assert bool((removed > 0).all()) and bool((removed < S ** 3).all())
    for c in range(24):
        part = removed[24 * c:24 * c + 24]
        assert bool((part == part[0]).all()), c      # an orientation moves the feature, it does not resize it
        assert set(labels[24 * c:24 * c + 24].unique().tolist()) == {0, c + 1}


def test_slot_voxels_lie_inside_their_rows_boxes():
    tables = [(single_features_tight()[0], S), (border_features()[0], S), (big_tables()[:40], BIG),
              (partgen.sample(40, BIG, 3, (2, 6), separate=False), BIG)]
    for params, size in tables:
        slots = reference.carve_parts(params, size)[2]           # (the oracle does not read the boxes)
        for n, k in (params[..., 0] >= 0).nonzero().tolist():
            z, y, x = (slots[n] == k + 1).nonzero(as_tuple=True)
            if len(z) == 0:
                continue
            x0, x1, y0, y1, z0, z1 = params[n, k, 10:].tolist()
            assert x0 <= int(x.min()) and int(x.max()) <= x1 and y0 <= int(y.min()) and int(y.max()) <= y1 \
                and z0 <= int(z.min()) and int(z.max()) <= z1, (n, k, params[n, k].tolist())


def test_through_features_reach_both_faces_and_blind_ones_only_the_access_face():
    _, (occ, _, _) = single_features()
    for through, blind in zip(THROUGH, BLIND):
        for o in range(24):
            t, b = occ[24 * through + o], occ[24 * blind + o]
            assert int((face(t, o) == 0).sum()) > 0 and int((face(t, o, opposite=True) == 0).sum()) > 0, (through, o)
            assert torch.equal(face(t, o) == 0, face(b, o) == 0), (through, blind, o)   # one section, two depths
            assert int((face(b, o, opposite=True) == 0).sum()) == 0, (blind, o)
            assert int((b == 0).sum()) < int((t == 0).sum())


def test_access_faces_are_those_of_the_single_feature_generator():
    """orient o turns the canonical top face to +z, -z, +x, -x, +y, -y: a blind hole in the middle
    of the face opens at Z = S-1, Z = 0, X = S-1, X = 0, Y = S-1, Y = 0 (volumes are [Z, Y, X])."""
    params = table([[row(2, o, cu=30, cv=30)] for o in range(6)])
    occ = reference.carve_parts(params, S)[0]
    mid = S // 2
    opened = [occ[0, S - 1, mid, mid], occ[1, 0, mid, mid], occ[2, mid, mid, S - 1], occ[3, mid, mid, 0],
              occ[4, mid, S - 1, mid], occ[5, mid, 0, mid]]
    closed = [occ[0, 0, mid, mid], occ[1, S - 1, mid, mid], occ[2, mid, mid, 0], occ[3, mid, mid, S - 1],
              occ[4, mid, 0, mid], occ[5, mid, S - 1, mid]]
    assert [int(v) for v in opened] == [0] * 6 and [int(v) for v in closed] == [1] * 6


def test_mirrors_move_corner_features_to_the_other_corners():
    params = table([[row(14, 6 * m)] for m in range(4)])       # corner block, access face +z
    occ = reference.carve_parts(params, S)[0]
    corners = [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)]  # (y, x)
    want = [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)]     # fx mirrors x, fy mirrors y
    for m in range(4):
        empty = [c for c in corners if int(occ[m, S - 1, c[0], c[1]]) == 0]
        assert empty == [want[m]], (m, empty)


def test_an_empty_table_gives_a_solid_block():
    for params in (table([[unused(), unused()]] * 3), torch.zeros(2, 0, 16, dtype=torch.int32)):
        for occ, labels, slots in (host(params, S), reference.carve_parts(params, S)):
            assert occ.shape == (len(params), S, S, S) and bool((occ == 1).all())
            assert not labels.any() and not slots.any()
    assert host(torch.zeros(0, 3, 16, dtype=torch.int32), S)[0].shape == (0, S, S, S)


def test_the_lowest_slot_wins():
    pocket, hole = row(10, 0), row(2, 0, depth=40)
    for first, second in ((pocket, hole), (hole, pocket)):
        params = table([[first, unused(), second]])
        occ, labels, slots = host(params, S)
        assert same((occ, labels, slots), reference.carve_parts(params, S))
        a = reference.carve_parts(table([[first]]), S)[1][0] != 0
        b = reference.carve_parts(table([[second]]), S)[1][0] != 0
        assert int((a & b).sum()) > 0 and int((a & ~b).sum()) > 0 and int((b & ~a).sum()) > 0
        assert bool((labels[0][a] == first[0] + 1).all()) and bool((slots[0][a] == 1).all())
        assert bool((labels[0][b & ~a] == second[0] + 1).all()) and bool((slots[0][b & ~a] == 3).all())
        assert torch.equal(occ[0] == 0, a | b)


def test_a_box_that_is_too_small_clips_its_feature_in_the_host_path():
    """The contract says a box is never too small; the host path (and the kernel) read it as part
    of the volume, the oracle does not read it."""
    params = table([[row(10, 0, x0=8, x1=8)]])
    occ = host(params, S)[0]
    full = reference.carve_parts(params, S)[0]
    assert torch.equal(occ[0, :, :, 8], full[0, :, :, 8]) and int((occ == 0).sum()) < int((full == 0).sum())
    assert bool((occ[0, :, :, :8] == 1).all()) and bool((occ[0, :, :, 9:] == 1).all())


# ---------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_is_deterministic_per_seed_and_index():
    rt = _native.runtime()
    base = rt.sample_parts(12, 32, 7, 1, 4, threads=1)
    assert base.dtype == np.int32 and base.shape == (12, 4, 16)
    assert np.array_equal(rt.sample_parts(12, 32, 7, 1, 4, threads=5), base)
    assert np.array_equal(rt.sample_parts(5, 32, 7, 1, 4, threads=2), base[:5])
    assert np.array_equal(rt.sample_parts(40, 32, 7, 1, 4)[:12], base)
    assert not np.array_equal(rt.sample_parts(12, 32, 8, 1, 4), base)
    assert len({tuple(p.reshape(-1)) for p in base}) == 12


def test_sampler_counts():
    params = big_tables()
    used = params[..., 0] >= 0
    counts = used.sum(1)
    assert int(counts.max()) <= 4
    short = float((counts < 2).float().mean())
    print("feature-count histogram", torch.bincount(counts, minlength=5).tolist(), "short of 2:", short)
    assert short <= 0.01
    # used slots come first, unused rows are (-1, 0, ...), every class and orientation occurs
    assert bool((used.long().diff(dim=1) <= 0).all())
    assert not params[~used][:, 1:].any() and bool((params[~used][:, 0] == -1).all())
    assert set(params[used][:, 0].tolist()) == set(range(24)) and set(params[used][:, 1].tolist()) == set(range(24))
    partgen.check_params(params, BIG)
    for lo, hi in ((0, 0), (3, 3), (1, 6)):
        c = (partgen.sample(50, BIG, 1, (lo, hi), separate=False)[..., 0] >= 0).sum(1)
        assert c.shape == (50,) and int(c.min()) >= lo and int(c.max()) <= hi
    few = partgen.sample(50, BIG, 1, (1, 4), num_classes=3)
    assert set(few[..., 0].unique().tolist()) <= {-1, 0, 1, 2}


def test_sampler_separation():
    for gap in (1, 3):
        params = big_tables() if gap == 1 else partgen.sample(200, BIG, 2, (2, 4), gap=gap)
        box = params[..., 10:].to(torch.int64)
        used = params[..., 0] >= 0
        K = params.shape[1]
        for i in range(K):
            for j in range(K):
                if i == j:
                    continue
                both = used[:, i] & used[:, j]
                a, b = box[both, i], box[both, j]
                apart = torch.zeros(len(a), dtype=torch.bool)
                for d in range(3):                   # a grown by gap misses b along some axis
                    apart |= (a[:, 2 * d] - gap > b[:, 2 * d + 1]) | (a[:, 2 * d + 1] + gap < b[:, 2 * d])
                assert bool(apart.all()), (gap, i, j)
    loose = partgen.sample(200, BIG, 2, (4, 4), separate=False)
    assert bool(((loose[..., 0] >= 0).sum(1) == 4).all())       # nothing is turned away


@pytest.mark.parametrize("part", range(PARTS // SLICE))
def test_sampler_components(part):
    lo = part * SLICE
    params, labels = big_tables()[lo:lo + SLICE], big_labels()[lo:lo + SLICE]
    roots = reference.connected_components(labels, 0, 6).reshape(SLICE, -1)
    found = (roots == torch.arange(1, BIG ** 3 + 1, dtype=torch.int32)).sum(1)
    assert torch.equal(found, expected_components(params)), (found - expected_components(params)).nonzero().tolist()


# ---------------------------------------------------------------------------------------------
# arguments, records, public API
# ---------------------------------------------------------------------------------------------
def test_argument_errors():
    good = table([[row(2, 0)]])
    with pytest.raises(ValueError, match="int32"):
        partgen.carve(good.long(), S)
    with pytest.raises(ValueError, match="int32"):
        partgen.carve(good[0], S)
    with pytest.raises(ValueError, match="int32"):
        partgen.carve(good[..., :15], S)
    for size in (12, 0, 264, 512, 16.0):
        with pytest.raises(ValueError, match="multiple of 8"):
            partgen.carve(good, size)
    with pytest.raises(ValueError, match="at most 32"):
        partgen.carve(good.repeat(1, 33, 1), S)
    for cls in (-2, 24, 255):
        with pytest.raises(ValueError, match="cls"):
            partgen.carve(table([[[cls] + row(2, 0)[1:]]]), S)
    with pytest.raises(ValueError, match="orient"):
        partgen.carve(table([[row(2, 24)]]), S)
    with pytest.raises(ValueError, match="geometry field"):
        partgen.carve(table([[row(2, 0, r=8 * S + 1)]]), S)
    assert partgen.carve(good.repeat(1, 32, 1), S)[0].shape == (1, S, S, S)
    rt = _native.runtime()
    for bad in (lambda: rt.carve_parts(good.numpy(), 12), lambda: rt.carve_parts(good.numpy(), 264),
                lambda: rt.carve_parts(good.repeat(1, 33, 1).numpy(), S), lambda: rt.carve_parts(good[0].numpy(), S),
                lambda: rt.sample_parts(1, 12, 0, 1, 4), lambda: rt.sample_parts(1, 64, 0, 3, 2),
                lambda: rt.sample_parts(1, 64, 0, 1, 33), lambda: rt.sample_parts(1, 64, 0, 1, 4, num_classes=25)):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(ValueError, match="features"):
        partgen.sample(1, 64, 0, (3, 2))
    with pytest.raises(ValueError, match="class 24"):
        reference.carve_parts(table([[[24] + row(2, 0)[1:]]]), S)


def test_part_records():
    params = table([[row(2, 13, x0=1, x1=2, y0=3, y1=4, z0=5, z1=6), unused(), row(16, 4)]])
    (feats,) = from_params(params)
    assert feats[0] == PartFeature(slot=0, cls=2, orientation=13, bbox=(5, 3, 1, 6, 4, 2)) and feats[0].face == "-z"
    assert feats[1].slot == 2 and feats[1].cls == 16 and feats[1].face == "+y"
    assert json.loads(json.dumps(feats[0].to_dict()))["bbox"] == [5, 3, 1, 6, 4, 2]
    assert from_params(torch.zeros(2, 0, 16, dtype=torch.int32)) == [[], []]


def test_generate_parts_on_the_cpu():
    assert "generate_parts" in fn.__all__
    vox, labels, parts, slots = fn.generate_parts(4, size=64, seed=4, features=(2, 3), device="cpu", return_slots=True)
    assert vox.dtype == labels.dtype == slots.dtype == np.uint8 and vox.shape == labels.shape == (4, 64, 64, 64)
    params = partgen.sample(4, 64, 4, (2, 3))
    want = reference.carve_parts(params, 64)
    assert all(np.array_equal(g, w.numpy()) for g, w in zip((vox, labels, slots), want))
    assert parts == from_params(params) and all(2 <= len(p) <= 3 for p in parts)
    for n, feats in enumerate(parts):                # the records describe the volumes
        for f in feats:
            z, y, x = (slots[n] == f.slot + 1).nonzero()
            assert len(z) and set(labels[n][slots[n] == f.slot + 1].tolist()) == {f.cls + 1}
            assert f.bbox[0] <= z.min() and z.max() <= f.bbox[3] and f.bbox[2] <= x.min() and x.max() <= f.bbox[5]
    again = fn.generate_parts(3, size=64, seed=4, features=(2, 3), device="cpu")
    assert len(again) == 3 and np.array_equal(again[1], labels[:3])
    # instances of the labels are the features
    _, inst = fn.label_components(labels, device="cpu")
    for n, feats in enumerate(parts):
        assert sorted(i.cls for i in inst[n]) == sorted(f.cls + 1 for f in feats for _ in range(2 if f.cls == 16 else 1))


def test_voxel_seg_dataset_and_training_on_the_cpu():
    from featurenet_amd.training.data import load_dataset, voxel_seg_dataset

    ds = voxel_seg_dataset(12, 4, size=16, features=(1, 3), seed=2, device="cpu")
    assert ds.name == "voxel-seg" and ds.num_classes == 25 and ds.input_shape == (16, 16, 16, 1) and not ds.packed
    assert ds.x_train.dtype == ds.y_train.dtype == torch.uint8
    assert ds.x_train.shape == (12, 16, 16, 16, 1) and ds.y_test.shape == (4, 16, 16, 16)
    assert ds.meta["seed"] == 2 and "sample_parts" in ds.meta["generator"]
    assert torch.equal(ds.y_train, reference.carve_parts(ds.meta["params_train"], 16)[1])
    assert torch.equal(ds.x_train[..., 0] == 0, ds.y_train != 0)
    assert not torch.equal(ds.meta["params_train"][:4], ds.meta["params_test"])
    res = fn.train("segmentation", data=ds, epochs=2, batch_size=4, device="cpu", verbose=0)
    assert all(np.isfinite(v) for v in res.history["loss"]) and res.meta["dataset"] == "voxel-seg"
    small = load_dataset("voxel-seg", synthetic_sizes=(20, 10), seed=9)
    assert small.x_train.shape == (2, 64, 64, 64, 1) and small.x_test.shape == (1, 64, 64, 64, 1)
    assert small.y_train.dtype == torch.uint8 and small.num_classes == 25


def test_cli_generate_parts(tmp_path, capsys):
    from featurenet_amd.cli import main

    out, js = tmp_path / "parts.npz", tmp_path / "parts.json"
    assert main(["generate-parts", "-n", "3", "--size", "16", "--seed", "5", "--features", "1", "2", "-o", str(out),
                 "--json", str(js), "--device", "cpu"]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["shape"] == [3, 16, 16, 16] and sum(summary["features_per_part"]) == 3
    with np.load(out, allow_pickle=False) as d:
        vox, labels = d["voxels"], d["labels"]
    want = fn.generate_parts(3, size=16, seed=5, features=(1, 2), device="cpu")
    assert np.array_equal(vox, want[0]) and np.array_equal(labels, want[1])
    doc = json.loads(js.read_text())
    assert [[f["class"] for f in p] for p in doc["parts"]] == [[f.cls for f in p] for p in want[2]]
