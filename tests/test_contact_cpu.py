"""Feature contacts on the CPU path: the oracle (``ops.reference.contact_table``) against a hand-worked scene and
a plain loop, the identities that tie it to the instance and dimension tables, the pinned generated parts
(separated and intersecting), the record type, ``fn.label_components(contacts=True)``,
``fn.extract_features(contacts=True)``, the CLI, and the Python <-> ``_C`` plumbing of ``ops.contact``.
Everything is an exact integer comparison."""
import json

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from _ccl_cases import PATTERNS
from _contact_cases import (HAND_ADJ, HAND_CONTACT, check_identities, expected_contacts, hand_scene,
                            loop_contact_table)
from _edt_cases import PARTS_COMPONENTS
from featurenet_amd import _native
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg
from featurenet_amd.ops import contact, reference
from featurenet_amd.utils.partfeatures import FACES
from featurenet_amd.utils.seginstances import FeatureInstance

S, NC = 16, 5
SHAPES = [(1, 1, 1), (1, 1, 64), (1, 5, 1), (3, 5, 7), (4, 6, 64)]


def tables_of(labels: torch.Tensor):
    roots = reference.connected_components(labels, 0, 6)
    return reference.instance_table(labels, roots)


# --- the oracle -------------------------------------------------------------------------------------
def test_hand_worked_scene():
    lab, occ = hand_scene()
    ids, table, offsets = tables_of(lab)
    assert table[:, 1].tolist() == [2, 1] and table[:, 2].tolist() == [20, 72]    # the hole is row 0
    con, adj = reference.contact_table(ids, offsets, occ)
    assert con.dtype == adj.dtype == torch.int64
    assert con.tolist() == HAND_CONTACT and adj.tolist() == HAND_ADJ
    again, adj2 = contact.contact_table(ids, offsets, occ, rows=2)
    assert torch.equal(again, con) and torch.equal(adj2, adj)
    _, (recs,) = fn.label_components(lab, device="cpu", occupancy=occ, contacts=True)
    hole, pocket = recs
    assert hole.neighbors == ((2, "+z", 4),) and pocket.neighbors == ((1, "-z", 4),)
    assert hole.entered_through("+z") == (2,) and hole.entered_through("-z") == () and pocket.entered_through("-z") == (1,)
    assert hole.floor("-z") == 0 and not hole.blind("-z") and not hole.blind("+z")   # through: bottom to pocket
    assert pocket.floor("+z") == 20 and pocket.blind("+z")                          # 24 less the hole's 4
    assert hole.surface == 48 and pocket.surface == 80 + 24 + 4


@pytest.mark.parametrize("pattern", PATTERNS)
def test_oracle_against_a_per_voxel_loop(pattern):
    for N in (1, 2):
        for D, H, W in SHAPES:
            for kind in ("complement", "random"):
                ids, table, offsets, occ, con, adj = expected_contacts(pattern, N, D, H, W, kind)
                lc, la = loop_contact_table(ids.numpy(), offsets.numpy(), occ.numpy(), len(table))
                what = (pattern, N, (D, H, W), kind)
                assert con.shape == (len(table), 19) and np.array_equal(con.numpy(), lc), what
                assert adj.shape == la.shape and np.array_equal(adj.numpy(), la), what
                got, got_adj = contact.contact_table(ids, offsets, occ)
                assert torch.equal(got, con) and torch.equal(got_adj, adj), what


def test_samples_do_not_meet():
    """The last plane of a sample and the first of the next are no neighbours: two solid samples of different
    instances have every outer face open and share nothing."""
    ids = torch.ones(2, 2, 3, 4, dtype=torch.int32)
    occ = torch.zeros(2, 2, 3, 4, dtype=torch.uint8)
    con, adj = reference.contact_table(ids, torch.tensor([0, 1, 2]), occ)
    assert adj.shape == (0, 4) and con.tolist() == [[0] * 6 + [12, 12, 6, 6, 8, 8] + [0] * 6 + [24]] * 2
    lc, la = loop_contact_table(ids.numpy(), np.array([0, 1, 2]), occ.numpy(), 2)
    assert np.array_equal(lc, con.numpy()) and len(la) == 0


def test_rows_outside_the_table_and_empty_inputs():
    ids = torch.tensor([[[[1, 2, 3, 0, -4]]]], dtype=torch.int32)
    occ = torch.tensor([[[[0, 0, 0, 1, 1]]]], dtype=torch.uint8)
    for off, T in (([0, 2], 2), ([-1, 1], 1), ([0, 0], 0)):
        con, adj = reference.contact_table(ids, torch.tensor(off), occ)
        lc, la = loop_contact_table(ids.numpy(), np.array(off), occ.numpy(), T)
        assert np.array_equal(con.numpy(), lc) and np.array_equal(adj.numpy(), la), off
    con, adj = reference.contact_table(ids, torch.tensor([0, 2]), occ)
    # id 3 has no row: still a shared face of id 2, but no pair; ids <= 0 carry no instance
    assert con[1, 12 + 2] == 1 and con[1, 12 + 3] == 1 and adj.tolist() == [[0, 1, 2, 1]]
    e = torch.zeros(0, 3, 4, 5, dtype=torch.int32)
    con, adj = contact.contact_table(e, torch.tensor([0]), e.to(torch.uint8))
    assert con.shape == (0, 19) and adj.shape == (0, 4)
    with pytest.raises(ValueError, match="int32"):
        contact.contact_table(ids.long(), torch.tensor([0, 2]), occ)
    with pytest.raises(ValueError, match="uint8"):
        contact.contact_table(ids, torch.tensor([0, 2]), ids)
    with pytest.raises(ValueError, match="offsets"):
        contact.contact_table(ids, torch.tensor([0, 1, 2]), occ)


@pytest.mark.parametrize("pattern", ["blobs", "noise4", "checker"])
def test_identities(pattern):
    for N, (D, H, W) in ((1, (3, 5, 7)), (2, (4, 6, 64)), (2, (9, 7, 130))):
        ids, table, offsets, occ, con, adj = expected_contacts(pattern, N, D, H, W)
        what = (pattern, N, (D, H, W))
        check_identities(con, adj, table, what)
        # no instance voxel is material here: a voxel with a material face neighbour has 1..6 wall faces
        assert not bool(occ[ids > 0].any()), what
        dim = reference.dimension_table(ids, offsets, reference.distance_sq(occ))
        walls = con[:, 0:6].sum(1)
        assert bool((dim[:, 2] <= walls).all()) and bool((walls <= 6 * dim[:, 2]).all()), what
        if pattern == "checker":                 # every voxel its own instance: nothing but shared and open faces
            assert int(con[:, :6].sum()) == 0 and bool((con[:, 6:18].sum(1) == 6 * con[:, 18]).all()), what


# --- generated parts --------------------------------------------------------------------------------
def parts_records(separate: bool):
    if not _native.runtime_available():
        pytest.skip("_rt not built")
    voxels, labels, parts, slots = fn.generate_parts(96, size=32, seed=3, device="cpu", separate=separate,
                                                     return_slots=True)
    ids, feats = fn.label_components(labels, device="cpu", occupancy=voxels, contacts=True)
    return voxels, labels, parts, slots, ids, feats


def sums(recs, field):
    return tuple(sum(getattr(f, field)[k] for f in recs) for k in range(6))


def test_separated_parts_share_nothing():
    voxels, labels, parts, slots, ids, feats = parts_records(True)
    recs = [f for fs in feats for f in fs]
    assert len(recs) == PARTS_COMPONENTS == 253
    assert all(f.shared_area == (0,) * 6 and f.neighbors == () for f in recs)
    assert sums(recs, "wall_area") == (19846, 21915, 27234, 28663, 15777, 16105)
    assert sums(recs, "open_area") == (10647, 8578, 11054, 9625, 7866, 7538)
    assert sum(f.voxels for f in recs) == 230783
    # every true feature is open at its recorded access face, and a through feature has no floor there
    checked = through = along = 0
    for n, fs in enumerate(feats):
        by_slot = {p.slot: p for p in parts[n]}
        for f in fs:
            carried = np.unique(slots[n][ids[n] == f.id])
            assert len(carried) == 1 and carried[0] >= 1, (n, f)
            p = by_slot[int(carried[0]) - 1]
            assert f.open_area[p.orientation % 6] > 0, (n, f, p)
            if f.through:                        # open toward two opposite faces: no wall on either of those sides
                pairs = [k for k in (0, 2, 4) if FACES[k] in f.open_faces() and FACES[k + 1] in f.open_faces()]
                assert pairs and all(f.floor(FACES[k]) == 0 and f.floor(FACES[k + 1]) == 0 for k in pairs), (n, f, p)
                through += 1
                if p.orientation % 6 // 2 * 2 in pairs:          # ... through along the axis of its access face
                    assert f.floor(p.face) == 0 and not f.blind(p.face), (n, f, p)
                    along += 1
            checked += 1
    assert checked == 253 and through >= along > 0


def test_intersecting_parts():
    voxels, labels, parts, slots, ids, feats = parts_records(False)
    recs = [f for fs in feats for f in fs]
    assert len(recs) == 253
    lt = torch.as_tensor(labels)
    tids, table, offsets = tables_of(lt)
    con, adj = reference.contact_table(tids, offsets, (torch.as_tensor(voxels) != 0).to(torch.uint8))
    assert adj.shape == (109, 4) and int(adj[:, 3].sum()) == 2974
    assert sums(recs, "shared_area") == (993, 993, 1121, 1121, 860, 860)
    assert sums(recs, "wall_area") == (19883, 21958, 27210, 27464, 16665, 16049)
    assert sums(recs, "open_area") == (10901, 8826, 10823, 10569, 7488, 8104)
    assert sum(f.voxels for f in recs) == 242795
    check_identities(con, adj, table, "intersecting parts")
    # the records mirror adj in both directions, with the opposite face on the higher row
    told = sorted((n, f.id, i, face, c) for n, fs in enumerate(feats) for f in fs for i, face, c in f.neighbors)
    off = offsets.tolist()
    want = []
    for a, b, k, c in adj.tolist():
        n = int(table[a, 0])
        assert n == int(table[b, 0])
        want += [(n, a - off[n] + 1, b - off[n] + 1, FACES[k], c), (n, b - off[n] + 1, a - off[n] + 1, FACES[k ^ 1], c)]
    assert told == sorted(want) and len(told) == 218
    for fs in feats:
        for f in fs:
            assert list(f.neighbors) == sorted(f.neighbors, key=lambda t: (t[0], FACES.index(t[1])))
            for k, face in enumerate(FACES):
                assert f.shared_area[k] == sum(c for _, fc, c in f.neighbors if fc == face)


# --- records, API, CLI ------------------------------------------------------------------------------
def test_record_plumbing():
    lab, occ = hand_scene()
    ids, table, offsets = tables_of(lab)
    pair = reference.contact_table(ids, offsets, occ)
    (hole, pocket), = FeatureInstance.from_table(table, offsets, contacts=pair)
    assert hole.wall_area == (0, 0, 10, 10, 10, 10) and hole.open_area == (0, 4, 0, 0, 0, 0)
    assert pocket.shared_area == (0, 4, 0, 0, 0, 0) and pocket.neighbors == ((1, "-z", 4),)
    d = json.loads(json.dumps(hole.to_dict()))
    assert d["wall_area"] == dict(zip(FACES, hole.wall_area)) and d["open_area"]["-z"] == 4
    assert d["shared_area"]["+z"] == 4 and d["surface"] == 48 and d["floor"]["+z"] == 0 and d["floor"]["+x"] == 10
    assert d["neighbors"] == [{"id": 2, "face": "+z", "faces": 4}]
    plain, = FeatureInstance.from_table(table, offsets)
    assert all(f.wall_area is None and f.neighbors is None and f.surface is None for f in plain)
    assert not {"wall_area", "open_area", "shared_area", "neighbors", "surface", "floor"} & set(plain[0].to_dict())
    # min_voxels drops records from the lists only: the pocket still names the hole
    (only,), = FeatureInstance.from_table(table, offsets, min_voxels=21, contacts=pair)
    assert only.id == 2 and only.neighbors == ((1, "-z", 4),)
    wrong = pair[0].clone()
    wrong[0, 18] += 1
    with pytest.raises(ValueError, match="contact table"):
        FeatureInstance.from_table(table, offsets, contacts=(wrong, pair[1]))
    with pytest.raises(ValueError, match="contact pairs"):
        FeatureInstance.from_table(table, offsets, contacts=(pair[0], torch.tensor([[0, 2, 0, 4]])))
    with pytest.raises(ValueError, match="contacts=True needs occupancy"):
        fn.label_components(lab, device="cpu", contacts=True)
    with pytest.raises(ValueError, match="no contact"):
        plain[0].floor("+z")
    with pytest.raises(ValueError, match="face must be"):
        hole.floor("up")


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


def test_extract_features_with_contacts(seg):
    m, x = seg
    xs = x.numpy().astype(np.uint8)
    labels, _ = fn.segment(m, xs, device="cpu")
    _, want = fn.label_components(labels, device="cpu", occupancy=xs, dimensions=True, tool=3, contacts=True)
    feats, ids = fn.extract_features(m, xs, batch_size=2, device="cpu", access=True, dimensions=True, tool=3,
                                     contacts=True)
    assert ids is None and feats == want and any(f.neighbors for fs in feats for f in fs)
    only, _ = fn.extract_features(m, xs, batch_size=2, device="cpu", contacts=True)
    assert all(f.access is None and f.clearance2 is None and f.reachable is None for fs in only for f in fs)
    key = lambda f: (f.id, f.wall_area, f.open_area, f.shared_area, f.neighbors)      # noqa: E731
    assert [[key(f) for f in fs] for fs in only] == [[key(f) for f in fs] for fs in want]
    plain, _ = fn.extract_features(m, xs, batch_size=2, device="cpu", access=True)
    assert all(f.wall_area is None and f.access is not None for fs in plain for f in fs)
    xf = x[:2].float()
    three = m.instances(xf, want_ids=True)
    con, adj = reference.contact_table(three[2], three[1], x[:2].to(torch.uint8))
    five = m.instances(xf, want_contacts=True)
    eight = m.instances(xf.unsqueeze(-1), want_ids=True, want_access=True, want_dims=True, want_reach=(4, 2),
                        want_contacts=True)
    assert len(five) == 5 and len(eight) == 8 and five[2] is None and torch.equal(five[0], three[0])
    assert torch.equal(five[3], con) and torch.equal(five[4], adj) and len(adj) > 0
    assert torch.equal(eight[6], con) and torch.equal(eight[7], adj) and eight[5].shape == (len(con), 15)
    check_identities(con, adj, three[0], "model")


def test_cli_features_contacts(seg, tmp_path, capsys):
    from featurenet_amd.cli import main

    m, x = seg
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    np.save(tmp_path / "x.npy", x.numpy().astype(np.uint8))
    assert main(["features", str(path), str(tmp_path / "x.npy")]) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert main(["features", str(path), str(tmp_path / "x.npy"), "--contacts"]) == 0
    doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    extra = ("wall_area", "open_area", "shared_area", "floor", "surface", "neighbors")
    for recs, base in zip(doc["samples"], plain["samples"]):
        assert [{k: v for k, v in r.items() if k not in extra} for r in recs] == base
        assert not any(set(b) & set(extra) for b in base)
        by_id = {r["id"]: r for r in recs}
        for r in recs:
            assert all(list(r[k]) == list(FACES) for k in extra[:4])
            assert r["surface"] == sum(sum(r[k].values()) for k in extra[:3])
            assert r["floor"] == {f: r["wall_area"][FACES[k ^ 1]] for k, f in enumerate(FACES)}
            for nb in r["neighbors"]:
                back = FACES[FACES.index(nb["face"]) ^ 1]
                assert {"id": r["id"], "face": back, "faces": nb["faces"]} in by_id[nb["id"]]["neighbors"]
    if not torch.cuda.is_available():                    # (the checkpoint loads onto the GPU when there is one)
        feats, _ = fn.extract_features(m, x.numpy().astype(np.uint8), device="cpu", contacts=True)
        assert doc["samples"] == [[f.to_dict() for f in fs] for fs in feats]


# --- Python <-> _C plumbing -------------------------------------------------------------------------
class _FakeK:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args))


def test_contact_calls_match_bindings(monkeypatch):
    if not _native.kernels_available():
        pytest.skip("_C not built")
    K = _native.kernels()
    chunk, slots = K.contact_chunk()
    assert chunk % 256 == 0 and slots == 512
    fk = _FakeK()
    monkeypatch.setattr(_native, "kernels", lambda: fk)
    monkeypatch.setattr(_native, "stream", lambda t=None: 0)
    monkeypatch.setattr(_native, "use_native", lambda t: True)
    ids = torch.zeros(2, 3, 4, 5, dtype=torch.int32)
    occ = torch.zeros(2, 3, 4, 5, dtype=torch.uint8)
    con, adj = contact.contact_table(ids, torch.tensor([0, 4, 7]), occ)
    assert con.shape == (7, 19) and con.dtype == torch.int64 and adj.shape == (0, 4) and adj.dtype == torch.int64
    (name, c), = fk.calls       # ids occ offsets contact keys counts lost N D H W T cap probe st ext
    assert name == "contact_stats" and c[0] == ids.data_ptr() and c[1] == occ.data_ptr() and c[3] == con.data_ptr()
    assert c[7:14] == (2, 3, 4, 5, 7, 1024, 1024)      # (the smallest table is the full one here: probed to its end)
    assert c[-1] == [120, 120, 3, 133, 1024, 1024, 1]
    assert c[5] == c[4] + 8 * 1024 and c[6] == c[5] + 8 * 1024
    with pytest.raises(ValueError, match="2\\^30"):
        contact.contact_table(ids, torch.tensor([0, 4, 7]), occ, rows=1 << 30)
    # the real bindings take exactly these arguments, and check extents and geometry before any launch
    buf = torch.zeros(7 * 19 + 2 * 1024 + 1, dtype=torch.int64)
    p = dict(ids=ids.data_ptr(), occ=occ.data_ptr(), offsets=buf.data_ptr(), contact=buf.data_ptr(),
             keys=buf.data_ptr(), counts=buf.data_ptr(), lost=buf.data_ptr(), N=2, D=3, H=4, W=5, T=7, cap=1024,
             probe=256, st=0, ext=[120, 120, 3, 133, 1024, 1024, 1])
    for i, name in enumerate(("ids", "occ", "offsets", "contact", "keys", "counts", "lost")):
        ext = list(p["ext"])
        ext[i] -= 1
        with pytest.raises(RuntimeError, match=f"{name} has"):
            K.contact_stats(**{**p, "ext": ext})
    for bad in (dict(T=-1, ext=[]), dict(T=121, ext=[]), dict(ids=0), dict(occ=0), dict(offsets=0), dict(contact=0),
                dict(keys=0), dict(lost=0), dict(H=0, ext=[]), dict(cap=1000), dict(cap=1), dict(probe=0)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.contact_stats(**{**p, **bad})
