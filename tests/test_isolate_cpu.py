"""Instance isolation on the CPU: the oracle (``ops.reference.isolate_instances``) against a per-voxel loop in
exact fractions and against the part generator, and the paths built on it (``ops.isolate``,
``fn.isolate_features``, the ``classifier`` option of ``fn.label_components``, ``fn.recognize``, the CLI).
Every comparison is exact."""
import json

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from _isolate_cases import (LOOP_CASES, generator_parts, grid_window, inner_window, loop_part, pattern_ids, random_ids,
                            random_sel, table_sel)
from featurenet_amd import _native
from featurenet_amd.models.featurenet3d import FeatureNet3D, FeatureNet3DConfig, FeatureNet3DSeg
from featurenet_amd.ops import isolate, reference

S = 16


def loop_parts(ids, sel, size):
    return torch.from_numpy(np.stack([loop_part(ids, row, size) for row in sel.tolist()]))


@pytest.mark.parametrize("shape,size", LOOP_CASES, ids=[f"{s}-to-{z}" for s, z in LOOP_CASES])
def test_oracle_against_a_per_voxel_loop(shape, size):
    ids = random_ids(2, *shape)
    sel = random_sel(2, shape, 2, grid_window(shape))[:4]
    got = reference.isolate_instances(ids, sel, size, 1)
    want = loop_parts(ids, sel, size)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    if shape == (5, 12, 9):                                  # the short axes leave free space around the stock
        assert not bool(got[:, 0].any()) and not bool(got[:, :, :, 0].any()) and bool(got[:, 3].any())


def test_the_issues_example_of_a_short_axis():
    """``L = 5`` of ``Lmax = 12`` into 8 looks at -3 -2 0 1 3 4 6 7."""
    o = torch.arange(8)
    s = torch.div((2 * o + 1) * 12 - (12 - 5) * 8, 16, rounding_mode="floor")
    assert s.tolist() == [-3, -2, 0, 1, 3, 4, 6, 7]
    ids = torch.ones(1, 5, 12, 9, dtype=torch.int32)
    part = reference.isolate_instances(ids, torch.tensor([[0, 2, 0, 0, 0, 4, 11, 8, 0, 0, 0, 5, 12, 9]],
                                                         dtype=torch.int32), 8, 1)
    # no voxel carries id 2, so the stock is solid: material where 0 <= s < 5, free space around it
    assert part[0, :, 4, 4].tolist() == [0, 0, 1, 1, 1, 1, 0, 0]


def test_oracle_with_a_window_strictly_inside_the_grid():
    shape = (9, 10, 12)
    ids = random_ids(2, *shape)
    win = inner_window(shape)
    assert all(w > 0 for w in win[:3]) and all(w + l < s for w, l, s in zip(win[:3], win[3:], shape))
    sel = random_sel(2, shape, 2, win)[:4]
    for size in (8, 16):
        assert torch.equal(reference.isolate_instances(ids, sel, size, 1), loop_parts(ids, sel, size))


@pytest.mark.parametrize("pattern", ["blobs", "noise4", "wrap", "solid", "empty"])
def test_identity_is_the_instance_mask(pattern):
    ids, table, offsets = pattern_ids(pattern, 2, 8, 8, 8)
    sel = table_sel(table, offsets, grid_window((8, 8, 8)))
    parts = reference.isolate_instances(ids, sel, 8, 1)
    assert len(parts) == len(table)
    for row, part in zip(sel.tolist(), parts):
        assert torch.equal(part, (ids[row[0]] != row[1]).to(torch.uint8))
    assert torch.equal((parts == 0).flatten(1).sum(1), table[:, 2])


@pytest.mark.parametrize("size", [8, 16])
def test_the_box_is_part_of_the_definition(size):
    shape = (8, 8, 8)
    ids, table, offsets = pattern_ids("blobs", 2, *shape)
    true = reference.isolate_instances(ids, table_sel(table, offsets, grid_window(shape)), size, 1)
    wide = reference.isolate_instances(ids, table_sel(table, offsets, grid_window(shape), "wide"), size, 1)
    assert torch.equal(true, wide) and bool((true == 0).any())
    half_sel = table_sel(table, offsets, grid_window(shape), "half")
    half = reference.isolate_instances(ids, half_sel, size, 1)
    assert torch.equal(half, loop_parts(ids, half_sel, size))
    cut = 0
    for row, h, t in zip(half_sel.tolist(), half, true):
        keep = (row[7] + 1) * size // 8                      # output columns whose source lies in the low half
        assert torch.equal(h[:, :, :keep], t[:, :, :keep]) and bool(h[:, :, keep:].all())
        cut += int((t[:, :, keep:] == 0).sum())
    assert cut > 0                                           # some feature did lose its other half


@pytest.mark.parametrize("shape,size", [((8, 8, 8), 8), ((5, 12, 9), 8), ((8, 8, 8), 16)])
def test_formats(shape, size):
    ids = random_ids(2, *shape)
    sel = random_sel(2, shape, 3, grid_window(shape))
    dense = reference.isolate_instances(ids, sel, size, 1)
    bits = reference.isolate_instances(ids, sel, size, 0)
    bf = reference.isolate_instances(ids, sel, size, 2)
    M = len(sel)
    assert bits.dtype == torch.uint8 and bits.shape == (M, size ** 3 // 8)
    packed = np.stack([_native.runtime().pack_bits(p.numpy().reshape(-1)) for p in dense])
    assert np.array_equal(bits.numpy(), packed)
    assert bf.dtype == torch.bfloat16 and bf.shape == (M, size, size, size, 1)
    assert torch.equal(bf, dense.to(torch.bfloat16).unsqueeze(-1))
    for fmt, want in ((0, bits), (1, dense), (2, bf)):       # the op layer's CPU path is the oracle
        assert torch.equal(isolate.isolate_instances(ids, sel, size, fmt), want)
        none = isolate.isolate_instances(ids, sel[:0], size, fmt)
        assert none.shape == (0, *want.shape[1:]) and none.dtype == want.dtype


@pytest.mark.parametrize("size", [16, 32])
def test_the_generator_is_an_exact_oracle(size):
    slots, sel, want = generator_parts(size)
    assert len(sel) > 6 and len(set(sel[:, 1].tolist())) > 1         # parts with more than one feature
    got = isolate.isolate_instances(slots, sel, size, 1)
    assert torch.equal(got, want)
    assert all(bool((p == 0).any()) for p in got)            # every used slot removed something


# ---------------------------------------------------------------------------------------------
# op-layer helpers
# ---------------------------------------------------------------------------------------------
def test_selection_and_material_window():
    shape = (8, 8, 8)
    ids, table, offsets = pattern_ids("blobs", 2, *shape)
    sel, keep = isolate.selection(table, offsets, shape=shape)
    assert torch.equal(sel, table_sel(table, offsets, grid_window(shape))) and torch.equal(keep, torch.arange(len(table)))
    k = int(table[:, 2].max())
    big, kept = isolate.selection(table, offsets, rows=len(table), min_voxels=k, shape=shape)
    assert torch.equal(kept, torch.nonzero(table[:, 2] >= k).squeeze(1)) and torch.equal(big, sel[kept])
    assert 0 < len(kept) < len(table)
    occ = torch.zeros(3, 6, 7, 9, dtype=torch.uint8)
    occ[0, 1:4, 2:3, 5:9] = 1
    occ[2, 5, 6, 0] = 3
    win = isolate.material_window(occ)
    assert win.tolist() == [[1, 2, 5, 3, 1, 4], [0, 0, 0, 6, 7, 9], [5, 6, 0, 1, 1, 1]]
    with pytest.raises(ValueError, match="shape"):
        isolate.selection(table, offsets)
    wsel, _ = isolate.selection(table, offsets, window=torch.tensor([[1, 1, 1, 6, 6, 6], [0, 2, 0, 8, 4, 8]]))
    assert wsel[:, 8:].tolist() == [[1, 1, 1, 6, 6, 6] if n == 0 else [0, 2, 0, 8, 4, 8] for n in table[:, 0].tolist()]


def test_errors():
    ids = torch.zeros(1, 8, 8, 8, dtype=torch.int32)
    row = [0, 1, 0, 0, 0, 7, 7, 7, 0, 0, 0, 8, 8, 8]
    sel = torch.tensor([row], dtype=torch.int32)
    for size in (12, 4, 264, True, 8.0):
        with pytest.raises(ValueError, match="size"):
            isolate.isolate_instances(ids, sel, size, 1)
    with pytest.raises(ValueError, match="fmt"):
        isolate.isolate_instances(ids, sel, 8, 3)
    with pytest.raises(ValueError, match="int32"):
        isolate.isolate_instances(ids.long(), sel, 8, 1)
    with pytest.raises(ValueError, match="sel"):
        isolate.isolate_instances(ids, sel[:, :13], 8, 1)
    with pytest.raises(ValueError, match="at most 256"):
        isolate.isolate_instances(torch.zeros(1, 1, 1, 257, dtype=torch.int32), sel, 8, 1)
    for col, bad in ((0, 1), (0, -1), (8, 1), (9, -1), (13, 9), (11, 0), (12, -3)):
        wrong = list(row)
        wrong[col] = bad
        with pytest.raises(ValueError, match="outside the grid"):
            isolate.isolate_instances(ids, torch.tensor([row, wrong], dtype=torch.int32), 8, 1)
    with pytest.raises(ValueError, match="no cube"):
        fn.isolate_features(np.zeros((1, 8, 8, 16), np.int32), device="cpu")
    with pytest.raises(ValueError, match="size"):
        fn.isolate_features(np.zeros((1, 8, 8, 8), np.int32), size=12, device="cpu")
    with pytest.raises(ValueError, match="occupancy"):
        fn.isolate_features(np.zeros((1, 8, 8, 8), np.int32), stock="bbox", device="cpu")
    seg = FeatureNet3DSeg(S, num_classes=3)
    y = np.zeros((1, S, S, S), np.uint8)
    with pytest.raises(ValueError, match="FeatureNet3D"):
        fn.label_components(y, classifier=seg, device="cpu")
    with pytest.raises(ValueError, match="FeatureNet3D"):
        fn.recognize(seg, y, device="cpu")
    with pytest.raises(ValueError, match="FeatureNet3D"):
        isolate.recognize_table(seg, torch.zeros(1, S, S, S, dtype=torch.int32), torch.zeros(0, 13, dtype=torch.int64),
                                torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="stock"):
        fn.recognize(tiny(), y, stock="hull", device="cpu")


# ---------------------------------------------------------------------------------------------
# plumbing, with the tiny classifier at 16^3
# ---------------------------------------------------------------------------------------------
def tiny(seed: int = 0) -> FeatureNet3D:
    torch.manual_seed(seed)
    m = FeatureNet3D(FeatureNet3DConfig.tiny()).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                    # (running statistics that are not the identity)
        for c in m.convs:
            c.running_mean.copy_(torch.randn(c.cout, generator=g) * 0.1)
            c.running_var.copy_(torch.rand(c.cout, generator=g) + 0.5)
    return m


@pytest.fixture(scope="module")
def parts():
    """(voxels, labels) of 4 generated parts at 16^3, uint8 arrays."""
    vox, labels, _ = fn.generate_parts(4, size=S, seed=3, device="cpu")
    return vox, labels


def test_label_components_with_a_classifier(parts):
    vox, labels = parts
    m = tiny()
    ids, feats = fn.label_components(labels, device="cpu", classifier=m)
    plain_ids, plain = fn.label_components(labels, device="cpu")
    assert np.array_equal(ids, plain_ids) and not m.training
    recs = [f for fs in feats for f in fs]
    assert len(recs) > 4 and all(p.recognized is None and p.agrees is None for fs in plain for p in fs)
    lt = torch.from_numpy(labels)
    tid, table, offsets = reference.instance_table(lt, reference.connected_components(lt, 0, 6))
    assert np.array_equal(tid.numpy(), ids)
    cls, prob, probs = isolate.recognize_table(m, tid, table, offsets, want_probs=True)
    assert [f.recognized for f in recs] == cls.tolist() and [f.recognized_prob for f in recs] == prob.tolist()
    assert probs.shape == (len(recs), 2) and torch.equal(probs.gather(1, cls[:, None]).squeeze(1), prob)
    assert isolate.recognize_table(m, tid, table, offsets)[2] is None
    for f, p in zip(recs, (p for fs in plain for p in fs)):  # every earlier field is untouched
        assert f.agrees == (f.cls == f.recognized + 1)
        assert {**f.to_dict(), "recognized": None, "recognized_prob": None, "agrees": None} == \
            {**p.to_dict(), "recognized": None, "recognized_prob": None, "agrees": None}
        assert f.to_dict()["recognized"] == f.recognized and "recognized" not in p.to_dict()
    # the classifier run directly on what isolate_features gives, in the same batches
    for bs in (256, 3):
        _, small = fn.label_components(labels, device="cpu", classifier=m, batch_size=bs)
        cut, index = fn.isolate_features(ids, features=small, device="cpu")
        assert cut.shape == (len(recs), S, S, S) and cut.dtype == np.uint8
        assert index.tolist() == [[n, f.id] for n, fs in enumerate(small) for f in fs]
        want, p = fn.classify(m, cut, batch_size=bs)
        got = [f for fs in small for f in fs]
        assert [f.recognized for f in got] == want.tolist()
        assert [f.recognized_prob for f in got] == [float(p[i, c]) for i, c in enumerate(want)]
    everything, index_all = fn.isolate_features(ids, device="cpu")
    assert np.array_equal(everything, cut) and np.array_equal(index_all, index)
    bits, _ = fn.isolate_features(ids, device="cpu", packed=True)
    assert np.array_equal(bits, np.packbits(cut.reshape(len(cut), -1), axis=1, bitorder="little"))
    up, _ = fn.isolate_features(ids, size=32, device="cpu")
    assert np.array_equal(up, cut.repeat(2, 1).repeat(2, 2).repeat(2, 3))


def test_min_voxels_leaves_none(parts):
    vox, labels = parts
    m = tiny()
    _, feats = fn.label_components(labels, device="cpu", classifier=m)
    recs = [f for fs in feats for f in fs]
    k = sorted(f.voxels for f in recs)[len(recs) // 2]
    _, some = fn.label_components(labels, device="cpu", classifier=m, min_voxels=k)
    for f, g in zip(recs, (g for fs in some for g in fs)):
        assert (g.id, g.cls, g.voxels, g.bbox) == (f.id, f.cls, f.voxels, f.bbox)
        if f.voxels >= k:
            assert g.recognized == f.recognized          # (other batches: the last bits of the probability may differ)
            assert g.recognized_prob == pytest.approx(f.recognized_prob, rel=1e-5)
        else:
            assert g.recognized is None and g.recognized_prob is None and g.agrees is None
    assert any(g.recognized is None for fs in some for g in fs) and any(g.recognized is not None for fs in some for g in fs)
    cut, index = fn.isolate_features(fn.label_components(labels, device="cpu")[0], min_voxels=k, device="cpu")
    assert index.tolist() == [[n, g.id] for n, fs in enumerate(some) for g in fs if g.recognized is not None]


def test_recognize(parts):
    vox, labels = parts
    m = tiny()
    feats, ids, lab = fn.recognize(m, vox, device="cpu", return_ids=True, return_labels=True)
    none = fn.recognize(m, vox, device="cpu")
    assert none[1] is None and none[2] is None and none[0] == feats
    # separate=True parts: the components of the removed volume are the components of the labels
    want_ids, truth = fn.label_components(labels, device="cpu", classifier=m)
    assert np.array_equal(ids, want_ids) and ids.dtype == np.int32 and lab.dtype == np.uint8
    for fs, ts in zip(feats, truth):
        assert [(f.id, f.voxels, f.bbox, f.centroid, f.recognized, f.recognized_prob) for f in fs] == \
            [(t.id, t.voxels, t.bbox, t.centroid, t.recognized, t.recognized_prob) for t in ts]
        assert all(f.cls == f.recognized + 1 and f.agrees for f in fs)
    mapped = np.zeros_like(lab)
    for n, fs in enumerate(feats):
        for f in fs:
            mapped[n][ids[n] == f.id] = f.cls
    assert np.array_equal(lab, mapped) and np.array_equal(lab != 0, vox == 0)
    # the geometric options run through the same path as label_components
    full, _, _ = fn.recognize(m, vox, device="cpu", access=True, dimensions=True, tool=2, contacts=True, walls=1)
    relabelled = np.where(ids > 0, 1, 0).astype(np.uint8)
    _, geo = fn.label_components(relabelled, device="cpu", occupancy=vox, dimensions=True, tool=2, contacts=True, walls=1)
    for fs, gs in zip(full, geo):
        for f, g in zip(fs, gs):
            a, b = f.to_dict(), g.to_dict()
            assert {k: v for k, v in a.items() if k in b and k != "class"} == {k: v for k, v in b.items() if k != "class"}
    k = 1 + min(f.voxels for fs in feats for f in fs)
    fewer, _, fewer_lab = fn.recognize(m, vox, device="cpu", min_voxels=k, return_labels=True)
    key = lambda f: (f.id, f.cls, f.voxels, f.bbox, f.recognized)      # noqa: E731 (other batches: the last bits of prob)
    assert [[key(f) for f in fs if f.voxels >= k] for fs in feats] == [[key(f) for f in fs] for fs in fewer]
    assert int((fewer_lab != 0).sum()) == sum(f.voxels for fs in fewer for f in fs) < int((lab != 0).sum())


def test_stock_bbox_ignores_empty_margins(parts):
    vox, _ = parts
    m = tiny()
    pad = (3, 1, 2)                                          # empty voxels in front of z, y, x; 1, 3, 2 behind
    big = np.zeros((len(vox), S + 4, S + 4, S + 4), np.uint8)
    big[:, pad[0]:pad[0] + S, pad[1]:pad[1] + S, pad[2]:pad[2] + S] = vox
    want, _, _ = fn.recognize(m, vox, device="cpu")
    got, ids, _ = fn.recognize(m, big, stock="bbox", device="cpu", return_ids=True)
    for v in vox:                                            # material on every face: its box is the whole block
        assert all(v.take([0, -1], axis=a).any(axis=tuple(b for b in range(3) if b != a)).all() for a in range(3))
    for fs, ws in zip(got, want):
        assert [(f.id, f.cls, f.voxels, f.recognized, f.recognized_prob) for f in fs] == \
            [(w.id, w.cls, w.voxels, w.recognized, w.recognized_prob) for w in ws]
        assert [f.bbox for f in fs] == [tuple(b + pad[i % 3] for i, b in enumerate(w.bbox)) for w in ws]
    assert not ids[:, :pad[0]].any() and not ids[:, :, :, pad[2] + S:].any()
    grid, gids, _ = fn.recognize(m, big, stock="grid", device="cpu", return_ids=True)
    # with the grid as stock the margin is removed volume too: one more component, which takes in every
    # feature that opens on a face of the block
    for fs, ws, g in zip(grid, want, gids):
        assert fs[0].bbox == (0, 0, 0, S + 3, S + 3, S + 3) and fs[0].voxels >= (S + 4) ** 3 - S ** 3
        assert len(fs) <= len(ws) + 1 and sum(f.voxels for f in fs) == int((g > 0).sum())
        assert sum(f.voxels for f in fs) == (S + 4) ** 3 - S ** 3 + sum(w.voxels for w in ws)
    # features that open on no face stay apart from the margin: it is exactly one extra component, the first
    closed = np.ones((1, S, S, S), np.uint8)
    closed[0, 4:8, 4:8, 4:8] = 0
    closed[0, 10:13, 9:14, 3:6] = 0
    padded = np.zeros((1, S + 4, S + 4, S + 4), np.uint8)
    padded[:, pad[0]:pad[0] + S, pad[1]:pad[1] + S, pad[2]:pad[2] + S] = closed
    (alone,), _, _ = fn.recognize(m, closed, device="cpu")
    (grid,), _, _ = fn.recognize(m, padded, stock="grid", device="cpu")
    (bbox,), _, _ = fn.recognize(m, padded, stock="bbox", device="cpu")
    assert len(alone) == 2 and len(grid) == 3 and grid[0].voxels == (S + 4) ** 3 - S ** 3
    shifted = [(f.id + 1, f.voxels, tuple(b + pad[i % 3] for i, b in enumerate(f.bbox))) for f in alone]
    assert [(f.id, f.voxels, f.bbox) for f in grid[1:]] == shifted
    assert [(f.id, f.cls, f.voxels, f.recognized, f.recognized_prob) for f in bbox] == \
        [(f.id, f.cls, f.voxels, f.recognized, f.recognized_prob) for f in alone]


def test_cli_round_trips(parts, tmp_path, capsys):
    from featurenet_amd.cli import main

    vox, labels = parts
    m = tiny()
    clf = fn.save(m, tmp_path / "clf.fnk", {"model_kind": "featurenet3d", "config": m.cfg.to_dict()})
    np.save(tmp_path / "x.npy", vox)
    assert main(["recognize", str(clf), str(tmp_path / "x.npy"), "--json", str(tmp_path / "out.json"), "--labels",
                 str(tmp_path / "labels.npy"), "--device", "cpu", "--min-voxels", "2", "--stock", "bbox"]) == 0
    doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert doc == json.loads((tmp_path / "out.json").read_text())
    feats, _, lab = fn.recognize(m, vox, stock="bbox", min_voxels=2, device="cpu", return_labels=True)
    assert doc["samples"] == [[f.to_dict() for f in fs] for fs in feats]
    assert np.array_equal(np.load(tmp_path / "labels.npy"), lab)
    assert all(r["agrees"] and r["class"] == r["recognized"] + 1 for rs in doc["samples"] for r in rs)
    torch.manual_seed(1)
    seg = FeatureNet3DSeg(S, num_classes=3).eval()
    sp = fn.save(seg, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 3})
    assert main(["features", str(sp), str(tmp_path / "x.npy")]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert main(["features", str(sp), str(tmp_path / "x.npy"), "--classifier", str(clf)]) == 0
    doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    extra = ("recognized", "recognized_prob", "agrees")
    n = 0
    for recs, base in zip(doc["samples"], plain["samples"]):
        assert [{k: v for k, v in r.items() if k not in extra} for r in recs] == base
        for r in recs:
            assert r["recognized"] in (0, 1) and 0.5 <= r["recognized_prob"] <= 1 and \
                r["agrees"] == (r["class"] == r["recognized"] + 1)
            n += 1
    assert n > 0
    if not torch.cuda.is_available():                        # (the checkpoints load onto the GPU when there is one)
        want, _ = fn.extract_features(seg, vox, device="cpu", classifier=m)
        assert doc["samples"] == [[f.to_dict() for f in fs] for fs in want]
