"""Tool reach on the CPU path: the oracle (``ops.reference.reach_scan`` / ``reach_table``) against plain
loops, the identity with the access mask, the bounds that tie it to the dimension table, ``tool_thresholds``,
the pinned scene, the record type, ``fn.tool_reach``, ``fn.label_components(tool=)``,
``fn.extract_features(tool=)``, the CLI, the generated parts, and the Python <-> ``_C`` plumbing of
``ops.reach``.  Everything is an exact integer comparison."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from _access_cases import occupancy, singles
from _ccl_cases import PATTERNS
from _edt_cases import PARTS_COMPONENTS, SEEDS, expected_d2
from _reach_cases import (PARTS_SUM_ENTRY2, PARTS_SUM_MACHINABLE, SYNTHETIC, TOOLS, check_scene, expected_reach,
                          expected_scan, judge, loop_reach_scan, loop_reach_table, scene, synthetic)
from featurenet_amd import _native
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg
from featurenet_amd.ops import reach, reference
from featurenet_amd.ops.reference import EDT_INF
from featurenet_amd.utils.partfeatures import FACES
from featurenet_amd.utils.seginstances import FeatureInstance, tool_thresholds

S, NC = 16, 5


# --- the scan ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SYNTHETIC)
def test_scan_oracle_against_a_loop_on_synthetic_volumes(kind):
    for N, (D, H, W) in ((2, (3, 4, 5)), (1, (2, 5, 9))):
        vol = synthetic(kind, N, D, H, W)
        r6 = expected_scan(kind, N, D, H, W)
        assert r6.dtype == torch.int32 and np.array_equal(r6.numpy(), loop_reach_scan(vol.numpy())), (kind, N)
        assert torch.equal(reach.reach_scan(vol), r6)
    vol, r6 = synthetic(kind, 1, 3, 4, 5), expected_scan(kind, 1, 3, 4, 5)
    if kind == "increasing":                               # the minimum sits at the low end of every path
        assert torch.equal(r6[:, 0::2], vol[:, None].expand(1, 3, 3, 4, 5))
        assert torch.equal(r6[0, 1], vol[0, :1].expand(3, 4, 5)) and torch.equal(r6[0, 3], vol[0, :, :, :1].expand(3, 4, 5))
    if kind == "constant":
        assert bool((r6 == 12345).all())


@pytest.mark.parametrize("kind", SEEDS)
def test_scan_oracle_against_a_loop_on_distances(kind):
    d2 = expected_d2(kind, 2, 3, 5, 7, False)
    r6 = reference.reach_scan(d2)
    assert np.array_equal(r6.numpy(), loop_reach_scan(d2.numpy()))
    if kind == "none":
        assert bool((r6 == EDT_INF).all())
    if kind == "all":
        assert bool((r6 == 0).all())
    assert bool((r6 <= d2[:, None]).all())


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 5, 3, 65), (1, 9, 7, 130)], ids=str)
def test_open_voxels_are_the_access_mask(shape):
    """``r6[:, k] >= 1`` holds exactly where the voxel is free and open toward face ``k``."""
    occ = occupancy(*shape)
    ids = torch.ones(shape, dtype=torch.int32)             # one instance per sample: the mask of every voxel
    _, mask = reference.access_table(ids, torch.arange(shape[0] + 1), occ, want_mask=True)
    r6 = reference.reach_scan(reference.distance_sq(occ))
    for k in range(6):
        assert torch.equal(r6[:, k] >= 1, (occ == 0) & ((mask >> k & 1) != 0)), (shape, FACES[k])
    assert bool((r6.permute(1, 0, 2, 3, 4)[:, occ != 0] == 0).all())                  # material gives 0


# --- the table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_reach_table_against_a_per_voxel_loop(pattern):
    for tool, N, (D, H, W) in ((1, 2, (3, 5, 7)), (3, 1, (5, 3, 65))):
        ids, table, offsets, occ, d2, r6, dc2, want = expected_reach(pattern, N, D, H, W, tool)
        need2, cut2 = TOOLS[tool]
        loop = loop_reach_table(ids.numpy(), offsets.numpy(), r6.numpy(), dc2.numpy(), need2, cut2, len(table))
        assert want.dtype == torch.int64 and np.array_equal(want.numpy(), loop), (pattern, tool)
        got, got_r6 = reach.reach_table(ids, offsets, occ, need2, cut2, want_r6=True)
        assert judge(got_r6, r6, got, want)
        again, none = reach.reach_table(ids, offsets, occ, need2, cut2, rows=len(table), d2=d2)
        assert none is None and torch.equal(again, want)
        # the bounds that tie it to the other tables
        dim = reference.dimension_table(ids, offsets, d2)
        assert torch.equal(want[:, 14], table[:, 2])
        assert bool((want[:, :6] <= dim[:, :1]).all())                     # entry2 <= clearance2
        assert bool((want[:, 13] >= want[:, 14] - want[:, 12]).all())      # a reached centre is cleared
        assert bool((want[:, 6:12].sum(1) >= want[:, 14] - want[:, 12]).all())
        assert bool((want[:, 6:13] <= want[:, 14:]).all())


def test_rows_outside_the_table_count_nowhere():
    D, H, W = 5, 3, 65
    ids, _ = singles(1, D, H, W)
    d2 = reference.distance_sq(occupancy(1, D, H, W))
    r6 = reference.reach_scan(d2)
    dc2 = reference.distance_sq(reference.reach_seeds(r6, 4))
    T = 100
    for off in ([0, T], [-50, T]):                         # (the oracle's table has offsets[-1] rows)
        got = reference.reach_table(ids, torch.tensor(off), r6, dc2, 4, 2)
        assert np.array_equal(got.numpy(), loop_reach_table(ids.numpy(), np.array(off), r6.numpy(), dc2.numpy(), 4, 2, T))
        assert len(got) == T and bool((got[:, 14] == 1).all())
        assert torch.equal(got[:, :6], r6[0].reshape(6, -1)[:, -off[0]:T - off[0]].T.to(torch.int64))
    two = torch.tensor([0, 0, 7])                          # both samples' ids land on the same rows
    ids2 = ids.repeat(2, 1, 1, 1)
    r62, dc22 = torch.cat([r6, r6.flip(4)]), torch.cat([dc2, dc2.flip(3)])
    got = reference.reach_table(ids2, two, r62, dc22, 4, 2)
    assert np.array_equal(got.numpy(), loop_reach_table(ids2.numpy(), two.numpy(), r62.numpy(), dc22.numpy(), 4, 2, 7))
    empty = reference.reach_table(torch.zeros(1, 2, 2, 2, dtype=torch.int32), torch.tensor([0, 3]),
                                  torch.zeros(1, 6, 2, 2, 2, dtype=torch.int32),
                                  torch.zeros(1, 2, 2, 2, dtype=torch.int32), 1, 0)
    assert empty.tolist() == [[-1] * 6 + [0] * 9] * 3


def test_the_comparison_rejects_near_misses():
    ids, table, offsets, occ, d2, r6, dc2, want = expected_reach("blobs", 2, 9, 7, 130, 3)
    assert judge(r6.clone(), r6, want.clone(), want)
    for k in range(6):
        bad = r6.clone()
        bad[1, k, 8, 6, 129] += 1
        assert not judge(bad, r6, want, want)
    for col in range(15):
        bad = want.clone()
        bad[len(want) // 2, col] += 1
        assert not judge(r6, r6, bad, want)


def test_empty_and_refused_inputs():
    assert reference.reach_scan(torch.zeros(0, 3, 4, 5, dtype=torch.int32)).shape == (0, 6, 3, 4, 5)
    assert reach.reach_scan(torch.zeros(2, 0, 4, 5, dtype=torch.int32)).shape == (2, 6, 0, 4, 5)
    ids = torch.zeros(2, 3, 4, 5, dtype=torch.int32)
    occ = torch.zeros(2, 3, 4, 5, dtype=torch.uint8)
    off = torch.tensor([0, 0, 0])
    got, none = reach.reach_table(ids, off, occ, 1, 0)
    assert got.shape == (0, 15) and got.dtype == torch.int64 and none is None
    e_ids = torch.zeros(0, 3, 4, 5, dtype=torch.int32)
    assert reach.reach_table(e_ids, torch.tensor([0]), e_ids.to(torch.uint8), 1, 0, want_r6=True)[1].shape == (0, 6, 3, 4, 5)
    for need2, cut2 in ((0, 0), (-1, 0), (1, -1), (1.0, 0), (True, 0), (EDT_INF, 0)):
        with pytest.raises(ValueError, match="need2"):
            reach.reach_table(ids, off, occ, need2, cut2)
    with pytest.raises(ValueError, match="need2"):
        reference.reach_table(ids, off, torch.zeros(2, 6, 3, 4, 5, dtype=torch.int32), ids, 0, 0)
    with pytest.raises(ValueError, match="int32"):
        reach.reach_scan(occ)
    with pytest.raises(ValueError, match="int32"):
        reach.reach_scan(ids[0])
    with pytest.raises(ValueError, match="int32"):
        reference.reach_scan(ids.long())
    with pytest.raises(ValueError, match="uint8"):
        reach.reach_table(ids, off, ids, 1, 0)
    with pytest.raises(ValueError, match="ids must be int32"):
        reach.reach_table(ids.long(), off, occ, 1, 0)
    with pytest.raises(ValueError, match="ids must be int32"):
        reach.reach_table(ids[:1], off, occ, 1, 0)
    with pytest.raises(ValueError, match="offsets must be int64"):
        reach.reach_table(ids, off[:2], occ, 1, 0)
    with pytest.raises(ValueError, match="d2 must be int32"):
        reach.reach_table(ids, off, occ, 1, 0, d2=ids.long())
    with pytest.raises(ValueError, match="d2 must be int32"):
        reach.reach_table(ids, off, occ, 1, 0, d2=ids[:1])
    for shape in ((1, 257, 1, 1), (1, 1, 257, 1), (1, 1, 1, 257)):
        with pytest.raises(ValueError, match="at most 256"):
            reach.reach_scan(torch.zeros(shape, dtype=torch.int32))
        with pytest.raises(ValueError, match="at most 256"):
            reference.reach_scan(torch.zeros(shape, dtype=torch.int32))
        with pytest.raises(ValueError, match="at most 256"):
            reach.reach_table(torch.zeros(shape, dtype=torch.int32), torch.tensor([0, 0]),
                              torch.zeros(shape, dtype=torch.uint8), 1, 0)


# --- tools and records ------------------------------------------------------------------------------
def test_tool_thresholds():
    for t, want in TOOLS.items():
        assert tool_thresholds(t) == want == tool_thresholds(float(t)) == tool_thresholds(Fraction(t))
    assert tool_thresholds(0) == (1, 0) and tool_thresholds(2.5) == (4, 1) and tool_thresholds("2.5") == (4, 1)
    assert tool_thresholds(2) == (3, 1) and tool_thresholds(Fraction(1, 3)) == (1, 0)
    for t in range(0, 40):
        need2, cut2 = tool_thresholds(t)
        assert isinstance(need2, int) and isinstance(cut2, int) and 0 <= cut2 < need2
        assert (need2 - 1) * 4 < (t + 1) ** 2 <= need2 * 4 and cut2 * 4 <= t * t < (cut2 + 1) * 4
    for bad in (-1, -0.5, math.inf, math.nan, None, "wide", True, 1 << 17):
        with pytest.raises(ValueError, match="tool diameter|wider than any grid"):
            tool_thresholds(bad)


def test_feature_instance_records():
    table = torch.tensor([[0, 3, 10, 1, 0, 1, 2, 4, 2, 3, 20, 15, 25], [0, 1, 4, 9, 1, 1, 1, 2, 2, 2, 6, 6, 6]])
    offsets = torch.tensor([0, 2])
    rch = torch.tensor([[9, 0, 4, 4, 0, 0, 10, 0, 5, 4, 0, 0, 0, 10, 10],
                        [EDT_INF, EDT_INF, 1, 1, 2, 2, 4, 4, 0, 0, 0, 0, 0, 4, 4]])
    (a, b), = FeatureInstance.from_table(table, offsets, reach=rch, tool=(4, 2))
    assert a.entry2 == (9, 0, 4, 4, 0, 0) and a.reachable == (10, 0, 5, 4, 0, 0) and a.tool == (4, 2)
    assert (a.unreachable, a.machinable, a.residual) == (0, 10, 0) and a.access is None and a.clearance2 is None
    assert a.entry_diameter("+z") == 5.0 and a.entry_diameter("-z") == 0.0 and a.entry_diameter("+x") == 3.0
    assert a.tool_faces() == ("+z",) and a.tool_faces(0.5) == ("+z", "+x") and a.tool_faces(0.4) == ("+z", "+x", "-x")
    assert b.entry_diameter("+z") == math.inf and b.entry_diameter("+x") == 1.0 and b.tool_faces() == ("+z", "-z")
    d = a.to_dict(0.5)
    assert d["tool"] == [4, 2] and d["entry2"] == dict(zip(FACES, a.entry2)) and d["tool_faces"] == ["+z", "+x"]
    assert d["reachable"]["+x"] == 5 and (d["unreachable"], d["machinable"], d["residual"]) == (0, 10, 0)
    assert json.loads(json.dumps(b.to_dict()))["entry2"]["+z"] == EDT_INF
    plain, = FeatureInstance.from_table(table, offsets)
    assert all(f.entry2 is None and f.reachable is None and f.unreachable is None and f.machinable is None
               and f.tool is None and f.residual is None and f.entry_diameter("+z") is None for f in plain)
    assert not set(plain[0].to_dict()) & {"tool", "entry2", "reachable", "tool_faces", "unreachable", "machinable",
                                          "residual"}
    with pytest.raises(ValueError, match="no reach counts"):
        plain[0].tool_faces()
    with pytest.raises(ValueError, match="face must be"):
        a.entry_diameter("up")
    wrong = rch.clone()
    wrong[1, 14] = 5
    with pytest.raises(ValueError, match="reach table does not belong"):
        FeatureInstance.from_table(table, offsets, reach=wrong, tool=(4, 2))
    with pytest.raises(ValueError, match="reach table does not belong"):
        FeatureInstance.from_table(table, offsets, reach=rch[:1], tool=(4, 2))
    with pytest.raises(ValueError, match="tool ="):
        FeatureInstance.from_table(table, offsets, reach=rch)


def test_the_pinned_scene():
    lab, occ = scene()
    feats = {}
    for t in TOOLS:
        ids, (recs,) = fn.label_components(lab, device="cpu", occupancy=occ, dimensions=True, tool=t)
        feats[t] = recs
    check_scene(feats)
    hole, slot, pocket = feats[5][2], feats[5][1], feats[5][0]
    assert hole.tool_faces(0.1) == ("+z",) and hole.tool_faces() == () and hole.residual == 276
    assert slot.tool_faces(0.1) == ("+x", "-x", "+y") and hole.entry_diameter("+z") == 2 * math.sqrt(46) - 1
    assert pocket.tool_diameter == 5.0 and pocket.machinable == 0          # wide enough, but no way in
    # the counterbore: the wide tool that fits the hole's mouth never reaches its narrow part
    assert hole.tool_diameter > 7 and feats[7][2].machinable < feats[5][2].machinable < feats[3][2].machinable
    r6 = fn.tool_reach(occ, device="cpu")
    assert r6.shape == (1, 6, 32, 32, 32) and int(r6[0, 0][ids[0] == 3].max()) == 46


# --- the public paths -------------------------------------------------------------------------------
def test_tool_reach_api():
    assert "tool_reach" in fn.__all__
    g = torch.Generator().manual_seed(4)
    vol = torch.rand(2, 4, 5, 6, generator=g) < 0.1
    want = reference.reach_scan(reference.distance_sq(vol.to(torch.uint8))).numpy()
    for v in (vol.numpy(), vol.numpy().astype(np.int64) * 7, vol):
        got = fn.tool_reach(v, device="cpu")
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(fn.tool_reach(vol[1].numpy(), device="cpu"), want[1])
    with pytest.raises(ValueError, match="integers or bools"):
        fn.tool_reach(vol.float().numpy(), device="cpu")
    with pytest.raises(ValueError, match=r"\[D, H, W\]"):
        fn.tool_reach(np.zeros((4, 4), np.uint8), device="cpu")
    with pytest.raises(ValueError, match="at most 256"):
        fn.tool_reach(np.zeros((1, 1, 257), np.uint8), device="cpu")


def test_label_components_with_a_tool():
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 3, (2, 6, 7, 8), generator=g)
    occ = torch.rand(2, 6, 7, 8, generator=g) < 0.3
    ids, feats = fn.label_components(lab.numpy(), device="cpu", occupancy=occ.numpy(), dimensions=True, tool=3)
    ids0, no_dims = fn.label_components(lab.numpy(), device="cpu", occupancy=occ.numpy(), tool=3)
    _, no_tool = fn.label_components(lab.numpy(), device="cpu", occupancy=occ.numpy(), dimensions=True)
    roots = reference.connected_components(lab.to(torch.uint8), 0, 6)
    want_ids, table, offsets = reference.instance_table(lab.to(torch.uint8), roots)
    o8 = occ.to(torch.uint8)
    acc, _ = reference.access_table(want_ids, offsets, o8)
    d2 = reference.distance_sq(o8)
    r6 = reference.reach_scan(d2)
    rch = reference.reach_table(want_ids, offsets, r6, reference.distance_sq(reference.reach_seeds(r6, 4)), 4, 2)
    assert np.array_equal(ids, ids0)
    assert feats == FeatureInstance.from_table(table, offsets, access=acc, dims=reference.dimension_table(
        want_ids, offsets, d2), shape=(6, 7, 8), reach=rch, tool=(4, 2))
    assert no_dims == FeatureInstance.from_table(table, offsets, access=acc, reach=rch, tool=(4, 2))
    assert all(f.reachable is None and f.tool is None for fs in no_tool for f in fs)
    extra = ("tool", "entry2", "reachable", "tool_faces", "unreachable", "machinable", "residual")
    assert [[f.to_dict() for f in fs] for fs in no_tool] == \
        [[{k: v for k, v in f.to_dict().items() if k not in extra} for f in fs] for fs in feats]
    for fs in feats:
        for f in fs:
            assert max(f.entry2) <= f.clearance2 and f.machinable >= f.voxels - f.unreachable
    with pytest.raises(ValueError, match="occupancy"):
        fn.label_components(lab.numpy(), device="cpu", tool=3)
    with pytest.raises(ValueError, match="tool diameter"):
        fn.label_components(lab.numpy(), device="cpu", occupancy=occ.numpy(), tool=-1)


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


def test_extract_features_with_a_tool(seg):
    m, x = seg
    xs = x.numpy().astype(np.uint8)
    labels, _ = fn.segment(m, xs, device="cpu")
    _, want = fn.label_components(labels, device="cpu", occupancy=xs, dimensions=True, tool=3)
    feats, ids = fn.extract_features(m, xs, batch_size=2, device="cpu", access=True, dimensions=True, tool=3)
    assert ids is None and feats == want and any(f.voxels > 1 for fs in feats for f in fs)
    only, _ = fn.extract_features(m, xs, batch_size=2, device="cpu", tool=3.0)
    assert all(f.access is None and f.clearance2 is None for fs in only for f in fs)
    assert [[(f.id, f.entry2, f.reachable, f.unreachable, f.machinable, f.tool) for f in fs] for fs in only] == \
        [[(f.id, f.entry2, f.reachable, f.unreachable, f.machinable, f.tool) for f in fs] for fs in want]
    plain, _ = fn.extract_features(m, xs, batch_size=2, device="cpu", dimensions=True)
    assert all(f.reachable is None and f.clearance2 is not None for fs in plain for f in fs)
    xf = x[:2].float()
    three = m.instances(xf, want_ids=True)
    r6 = reference.reach_scan(reference.distance_sq(x[:2].to(torch.uint8)))
    rch = reference.reach_table(three[2], three[1], r6, reference.distance_sq(reference.reach_seeds(r6, 4)), 4, 2)
    four = m.instances(xf, want_reach=(4, 2))
    six = m.instances(xf.unsqueeze(-1), want_ids=True, want_access=True, want_dims=True, want_reach=(4, 2))
    assert len(four) == 4 and len(six) == 6 and four[2] is None and torch.equal(four[0], three[0])
    assert torch.equal(four[3], rch) and torch.equal(six[5], rch) and torch.equal(six[2], three[2])
    assert six[3].shape == (len(rch), 8) and six[4].shape == (len(rch), 4)
    assert bool((rch[:, :6] <= six[4][:, :1]).all()) and torch.equal(rch[:, 14], three[0][:, 2])
    with pytest.raises(ValueError, match="need2"):
        m.instances(xf, want_reach=(0, 0))


def test_cli_features_tool_and_reach(seg, tmp_path, capsys):
    from featurenet_amd.cli import main

    m, x = seg
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    np.save(tmp_path / "x.npy", x.numpy().astype(np.uint8))
    assert main(["features", str(path), str(tmp_path / "x.npy")]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert main(["features", str(path), str(tmp_path / "x.npy"), "--tool", "3", "--access-fraction", "0.5"]) == 0
    doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    extra = ("tool", "entry2", "reachable", "tool_faces", "unreachable", "machinable", "residual")
    for recs, base in zip(doc["samples"], plain["samples"]):
        assert [{k: v for k, v in r.items() if k not in extra} for r in recs] == base
        assert not any(set(b) & set(extra) for b in base)
        for r in recs:
            assert r["tool"] == [4, 2] and r["residual"] == r["voxels"] - r["machinable"] >= 0
            assert r["tool_faces"] == [f for f in FACES if r["reachable"][f] >= 0.5 * r["voxels"]]
            assert r["machinable"] >= r["voxels"] - r["unreachable"] and list(r["entry2"]) == list(FACES)
    if not torch.cuda.is_available():                    # (the checkpoint loads onto the GPU when there is one)
        feats, _ = fn.extract_features(m, x.numpy().astype(np.uint8), device="cpu", tool=3)
        assert doc["samples"] == [[f.to_dict(0.5) for f in fs] for fs in feats]
    args = ["reach", str(tmp_path / "x.npy"), "-o", str(tmp_path / "r6.npy"), "--device", "cpu", "--json",
            str(tmp_path / "r6.json")]
    assert main(args) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    r6 = np.load(tmp_path / "r6.npy")
    want = reference.reach_scan(reference.distance_sq(x.to(torch.uint8))).numpy()
    assert np.array_equal(r6, want) and r6.dtype == np.int32 and out == json.loads((tmp_path / "r6.json").read_text())
    assert out == {"shape": [3, 6, S, S, S], "material": int(x.sum()),
                   "open_voxels": {f: int((want[:, k] >= 1).sum()) for k, f in enumerate(FACES)},
                   "max_entry_sq": {f: int(want[:, k].max()) for k, f in enumerate(FACES)}}
    np.save(tmp_path / "one.npy", x[0].numpy())
    assert main(["reach", str(tmp_path / "one.npy"), "-o", str(tmp_path / "one_r6.npy"), "--device", "cpu"]) == 0
    capsys.readouterr()
    assert np.array_equal(np.load(tmp_path / "one_r6.npy"), want[0])


def test_generated_parts_are_reached_from_their_access_face():
    if not _native.runtime_available():
        pytest.skip("_rt not built")
    voxels, labels, parts, slots = fn.generate_parts(96, size=32, seed=3, device="cpu", return_slots=True)
    ids, one = fn.label_components(labels, device="cpu", occupancy=voxels, dimensions=True, tool=1)
    checked, seen = 0, set()
    for n, recs in enumerate(one):
        by_slot = {p.slot: p for p in parts[n]}
        for f in recs:
            carried = np.unique(slots[n][ids[n] == f.id])
            assert f.machinable >= f.voxels - f.unreachable and max(f.entry2) <= f.clearance2, (n, f)
            assert len(carried) == 1 and carried[0] >= 1, (n, f, carried)
            p = by_slot[int(carried[0]) - 1]
            assert f.reachable[p.orientation % 6] == f.voxels and p.face in f.tool_faces(), (n, f, p)
            checked += 1
            seen.add((n, p.slot))
    assert checked == PARTS_COMPONENTS and len(seen) == sum(len(ps) for ps in parts)   # no feature is left out
    _, three = fn.label_components(labels, device="cpu", occupancy=voxels, tool=3)
    recs = [f for fs in three for f in fs]
    assert tuple(sum(f.entry2[k] for f in recs) for k in range(6)) == PARTS_SUM_ENTRY2
    assert sum(f.machinable for f in recs) == PARTS_SUM_MACHINABLE


# --- Python <-> _C plumbing -------------------------------------------------------------------------
class _FakeK:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args))


def test_reach_calls_match_bindings(monkeypatch):
    if not _native.kernels_available():
        pytest.skip("_C not built")
    K = _native.kernels()
    chunk, slots = K.reach_chunk()
    assert chunk % 256 == 0 and slots == 512
    fk = _FakeK()
    monkeypatch.setattr(_native, "kernels", lambda: fk)
    monkeypatch.setattr(_native, "stream", lambda t=None: 0)
    monkeypatch.setattr(_native, "use_native", lambda t: True)
    ids = torch.zeros(2, 3, 4, 5, dtype=torch.int32)
    occ = torch.zeros(2, 3, 4, 5, dtype=torch.uint8)
    d2 = torch.zeros(2, 3, 4, 5, dtype=torch.int32)
    rch, r6 = reach.reach_table(ids, torch.tensor([0, 4, 7]), occ, 4, 2, d2=d2, want_r6=True)
    assert rch.shape == (7, 15) and rch.dtype == torch.int64 and r6.shape == (2, 6, 3, 4, 5) and r6.dtype == torch.int32
    # the caller's d2 is not computed again: one transform only, that of the reached centres
    assert [n for n, _ in fk.calls] == ["reach_scan", "edt_transform", "reach_stats"]
    sc, st = fk.calls[0][1], fk.calls[2][1]        # vol r6 N D H W st ext | ids offsets r6 dc2 raw N D H W T need2 cut2
    assert sc[0] == d2.data_ptr() and sc[1] == r6.data_ptr() and sc[2:6] == (2, 3, 4, 5) and sc[-1] == [120, 720]
    assert st[0] == ids.data_ptr() and st[2] == r6.data_ptr() and st[4] == rch.data_ptr()
    assert st[5:12] == (2, 3, 4, 5, 7, 4, 2) and st[-1] == [120, 3, 720, 120, 105]
    fk.calls.clear()
    reach.reach_table(ids, torch.tensor([0, 4, 7]), occ, 1, 0, rows=7)
    assert [n for n, _ in fk.calls] == ["edt_transform", "reach_scan", "edt_transform", "reach_stats"]
    # the real bindings take exactly these arguments, and check extents and geometry before any launch
    for i, name in enumerate(("vol", "r6")):
        ext = [120, 720]
        ext[i] -= 1
        with pytest.raises(RuntimeError, match=f"{name} has"):
            K.reach_scan(16, 16, 2, 3, 4, 5, 0, ext)
    for i, name in enumerate(("ids", "offsets", "r6", "dc2", "raw")):
        ext = [120, 3, 720, 120, 105]
        ext[i] -= 1
        with pytest.raises(RuntimeError, match=f"{name} has"):
            K.reach_stats(16, 16, 16, 16, 16, 2, 3, 4, 5, 7, 4, 2, 0, ext)
    with pytest.raises(RuntimeError, match="missing extent"):
        K.reach_stats(16, 16, 16, 16, 16, 2, 3, 4, 5, 7, 4, 2, 0, [120, 3, 720, 120])
    p = dict(vol=16, r6=16, N=2, D=3, H=4, W=5, st=0, ext=[])
    for bad in (dict(D=0), dict(N=0), dict(W=257), dict(H=257), dict(D=257), dict(vol=0), dict(r6=0), dict(vol=18),
                dict(r6=17), dict(N=1 << 8, D=256, H=256, W=256)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.reach_scan(**{**p, **bad})
    q = dict(ids=16, offsets=16, r6=16, dc2=16, raw=16, N=2, D=3, H=4, W=5, T=7, need2=4, cut2=2, st=0, ext=[])
    for bad in (dict(T=-1), dict(T=121), dict(ids=0), dict(offsets=0), dict(r6=0), dict(dc2=0), dict(raw=0),
                dict(need2=0), dict(cut2=-1), dict(W=257), dict(H=0), dict(raw=20), dict(offsets=20), dict(r6=18)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.reach_stats(**{**q, **bad})
