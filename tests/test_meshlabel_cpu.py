"""Mesh labels without a GPU: the torch oracle (``reference.mesh_votes``) against the closed form
for boundary meshes and against a plain Python reading of the rule, the host path
(``_rt.mesh_votes``) against the oracle bit for bit, ``ops.meshlabel``'s argument checks,
``fn.label_mesh``, ``FeatureInstance.faces`` and the CLI.
"""
import json

import numpy as np
import pytest
import torch

import featurenet_amd as fn
import _mesh_cases as mc
import _meshlabel_cases as lc
from featurenet_amd import _native
from featurenet_amd.ops import meshlabel, reference
from featurenet_amd.utils.voxelmesh import voxels_to_mesh, write_labelled_obj

needs_rt = pytest.mark.skipif(not _native.runtime_available(), reason="_rt is not built")


def oracle(meshes, vols, size):
    tris, off = mc.batch(meshes)
    return reference.mesh_votes(tris, off, torch.from_numpy(np.stack(vols)), size).numpy()


def multiset(rows):
    return sorted(map(tuple, np.asarray(rows).tolist()))


@pytest.mark.parametrize("size", [8, 16])
def test_oracle_gives_boundary_triangles_the_air_voxel_across_the_face(size):
    occ, ids, meshes = lc.volumes_case(size)
    for o, i, tris in zip(occ, ids, meshes):
        rows = oracle([tris], [i], size)
        assert np.array_equal(rows[:, 0], lc.boundary_expectation(tris, o, i))
        # the quad's diagonal passes through the column centre: the tie rule gives it to one of the two
        assert set(rows[:, 2].tolist()) == {0, 1} and 2 * int(rows[:, 2].sum()) == len(tris)
        assert np.array_equal(rows[:, 1], (rows[:, 0] != 0).astype(np.int32))          # one vote, or none
        # order, vertex rotation and winding do not matter, per triangle and as a multiset
        plain = mc.boundary_tris(o, seed=None)
        g = np.random.default_rng(size)
        perm, turn, flip = g.permutation(len(plain)), g.integers(0, 3, len(plain)), g.integers(0, 2, len(plain)) > 0
        t = plain.reshape(-1, 3, 3)[perm]
        t = np.stack([t[np.arange(len(t)), (turn + k) % 3] for k in range(3)], 1)
        t[flip] = t[flip][:, [0, 2, 1]]
        base = oracle([plain], [i], size)
        assert np.array_equal(oracle([t.reshape(-1, 9)], [i], size), base[perm])
        assert multiset(rows) == multiset(base) == multiset(oracle([mc.scramble(plain, 11)], [i], size))


def test_oracle_boundary_winners_follow_the_grid_symmetries():
    size = 8
    occ, ids, _ = lc.volumes_case(size)
    plain = mc.boundary_tris(occ[0], seed=None)
    base = oracle([plain], [ids[0]], size)
    for move, move_vol in zip(mc.symmetries(size), lc.volume_symmetries(size)):
        rows = oracle([move(plain)], [move_vol(ids[0])], size)
        assert np.array_equal(rows[:, :2], base[:, :2])
        assert np.array_equal(move_vol(occ[0]), fn.voxelize(move(plain).reshape(-1, 3, 3) / 16, size=size,
                                                            fit=((0, 0, 0), 1.0), device="cpu")[0])


@pytest.mark.parametrize("name", ["ties", "degenerate", "normal_tie", "vote_tie", "large", "large_axis", "outside"])
def test_oracle_equals_the_rule_read_in_python(name):
    _, size, tris, off, vol = next(c for c in lc.suite() if c[0] == name)
    want = np.concatenate([lc.slow_votes(tris[a:b].numpy(), vol[n].numpy())
                           for n, (a, b) in enumerate(zip(off[:-1].tolist(), off[1:].tolist()))])
    assert np.array_equal(lc.expected(name, "int32").numpy(), want)


def test_oracle_on_the_hand_made_cases():
    rows = lc.expected("large", "int32").numpy()
    assert rows[0, 2] == 120 and rows[0, 1] == 1                    # 120 columns, all values distinct: one vote
    _, _, _, _, vol = next(c for c in lc.suite() if c[0] == "large")
    assert rows[0, 0] == lc.slow_votes(np.array([lc.LARGE]), vol[0].numpy())[0, 0]
    tie = lc.expected("vote_tie", "int32").numpy()
    assert tie[0, 0] == 4 and tie[0, 1] == tie[0, 2] > 1            # 9 and 4 tie in votes: the lower wins
    deg = lc.expected("degenerate", "int32").numpy()
    assert deg[0].tolist() == [0, 0, 0] and deg[-1].tolist() == [0, 0, 0] and deg[1, 2] > 0
    # |n_x| = |n_y|: the rays run along x.  The triangle lies in the plane x + y = 120 over z 10..120, so
    # with x it covers the (y, z) columns of rows y = 1..5; with y it would count (z, x) columns instead
    _, _, tris, off, vol = next(c for c in lc.suite() if c[0] == "normal_tie")
    tie_rows = lc.expected("normal_tie", "int32")
    assert tie_rows.dtype == torch.int32 and tie_rows[0, 2] == lc.slow_votes(tris.numpy(), vol[0].numpy())[0, 2] > 0
    for s, sub, cen, r in mc.SPHERES:                                # no degenerate triangle, few centroid votes
        rows = oracle([mc.sphere(sub, cen, r)[0]], [lc.random_values(s, 1, 1, 9)], s)
        assert 0 <= (rows[:, 2] == 0).mean() < 0.08
        inside = np.abs(np.asarray(cen) - s / 2).max() + r < s / 2                   # the third one leaves the grid
        assert (rows[:, 1] > 0).all() == inside


@needs_rt
@pytest.mark.parametrize("dtype", ["int32", "uint8"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_host_path_equals_the_oracle(name, dtype):
    _, size, tris, off, vol = next(c for c in lc.suite() if c[0] == name)
    v = lc.volume(vol, dtype)
    want = lc.expected(name, dtype)
    for threads in (1, 5):
        got = torch.from_numpy(_native.runtime().mesh_votes(tris.numpy(), off.numpy(), v.numpy(), threads))
        assert got.dtype == torch.int32 and torch.equal(got, want), (name, int((got != want).any(1).sum()))
    assert torch.equal(meshlabel.mesh_votes(tris, off, v), want)
    assert torch.equal(meshlabel.mesh_votes(tris, off, v, form="wave"), want)       # (no forms on the host)


@needs_rt
def test_argument_checks():
    _, size, tris, off, vol = next(c for c in lc.suite() if c[0] == "volumes8")
    for bad in (vol.long(), vol.float(), vol[:2], vol[:, :, :, :4], vol[0], vol.numpy()):
        with pytest.raises(ValueError, match="mesh_votes"):
            meshlabel.mesh_votes(tris, off, bad)
    with pytest.raises(ValueError, match="size"):
        meshlabel.mesh_votes(tris, off, torch.zeros(3, 12, 12, 12, dtype=torch.int32))
    with pytest.raises(ValueError, match="form"):
        meshlabel.mesh_votes(tris, off, vol, form="lane")
    with pytest.raises(ValueError, match="mesh_votes: tris"):
        meshlabel.mesh_votes(tris.long(), off, vol)
    with pytest.raises(ValueError, match="8192"):
        meshlabel.mesh_votes(tris + 9000, off, vol)
    rt, t, o, v = _native.runtime(), tris.numpy(), off.numpy(), vol.numpy()
    for call in (lambda: rt.mesh_votes(t[:, :8], o, v, 1), lambda: rt.mesh_votes(t, o + 1, v, 1),
                 lambda: rt.mesh_votes(t, o[::-1].copy(), v, 1), lambda: rt.mesh_votes(t + 8100, o, v, 1),
                 lambda: rt.mesh_votes(t, o, v[:2], 1), lambda: rt.mesh_votes(t, o, v.astype(np.int64), 1),
                 lambda: rt.mesh_votes(t, o, v[:, :, :, :4], 1), lambda: rt.mesh_votes(t, o, v[:, ::1, ::1, ::-1], 1)):
        with pytest.raises(RuntimeError, match="mesh_votes"):
            call()
    with pytest.raises(ValueError, match="mesh_votes"):
        reference.mesh_votes(tris, off, vol.long(), size)


def small_part():
    """A 16^3 part with a pocket, a through hole and a blind hole -> occupancy uint8 [16, 16, 16]."""
    occ = np.ones((16, 16, 16), np.uint8)
    occ[10:, 3:9, 2:13] = 0                      # a pocket open to +z
    occ[:, 11:14, 4:7] = 0                       # a hole through z
    occ[4:8, 0:5, 9:12] = 0                      # a blind hole from -y
    return occ


@needs_rt
def test_label_mesh_round_trip():
    assert "label_mesh" in fn.__all__
    occ = small_part()
    mesh = voxels_to_mesh(occ) * 0.25 + np.float32([3.0, -2.0, 1.0])
    vox, info = fn.voxelize(mesh, size=16, device="cpu", return_info=True)
    assert np.array_equal(vox[0], occ)
    ids, feats = fn.label_components(1 - vox, device="cpu")
    assert len(feats[0]) == 3
    # the air voxel a boundary triangle bounds: half a voxel from the face's centre, along the outward normal
    normal = np.cross(mesh[:, 1] - mesh[:, 0], mesh[:, 2] - mesh[:, 0]).astype(np.float64)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    at = ((mesh.mean(1) - np.float32([3.0, -2.0, 1.0])) / 0.25 + 0.4 * normal)
    cell = np.floor(at).astype(int)
    inside = ((cell >= 0) & (cell < 16)).all(1)
    c = np.clip(cell, 0, 15)
    want = np.where(inside, ids[0][c[:, 2], c[:, 1], c[:, 0]], 0)
    winners, rows = fn.label_mesh(mesh, ids[0], device="cpu", return_votes=True)
    assert winners.dtype == np.int32 and winners.shape == (len(mesh),) and rows.shape == (len(mesh), 3)
    assert np.array_equal(winners, want) and np.array_equal(rows[:, 0], winners)
    assert set(np.unique(winners)) == {0, 1, 2, 3}
    again = fn.label_mesh([mesh], ids, fit=(info["origin"][0], info["voxel_size"][0]), device="cpu")
    assert isinstance(again, list) and np.array_equal(again[0], winners)
    assert np.array_equal(fn.label_mesh(mesh, ids[0].astype(np.int64), device="cpu"), winners)
    labels = (ids[0] > 0).astype(np.uint8) * 7                       # uint8 labels vote as they are
    assert np.array_equal(fn.label_mesh(mesh, labels, device="cpu"), np.where(winners > 0, 7, 0))
    for bad, match in ((ids[0].astype(np.float32), "integers"), (ids[0][:8], "volume"), (np.stack([ids[0]] * 2), "meshes")):
        with pytest.raises(ValueError, match=match):
            fn.label_mesh(mesh, bad, device="cpu")


@needs_rt
def test_recognize_and_extract_features_fill_faces():
    from featurenet_amd.models.featurenet3d import FeatureNet3D, FeatureNet3DConfig, FeatureNet3DSeg

    occ = small_part()
    mesh = voxels_to_mesh(occ)
    torch.manual_seed(0)
    clf = FeatureNet3D(FeatureNet3DConfig.tiny()).eval()                 # (16^3)
    plain, _, _ = fn.recognize(clf, occ[None], device="cpu")
    assert all(f.faces is None for f in plain[0])
    feats, ids, _ = fn.recognize(clf, occ[None], device="cpu", return_ids=True, meshes=[mesh], fit=((0, 0, 0), 1.0))
    winners = fn.label_mesh(mesh, ids[0], fit=((0, 0, 0), 1.0), device="cpu")
    assert len(feats[0]) == 3
    held = np.concatenate([f.faces for f in feats[0]] + [np.nonzero(winners == 0)[0]])
    assert np.array_equal(np.sort(held), np.arange(len(mesh)))
    for f in feats[0]:
        assert len(f.faces) and (winners[f.faces] == f.id).all() and (np.diff(f.faces) > 0).all()
        assert f.to_dict()["faces"] == f.faces.tolist()
    seg = FeatureNet3DSeg(16, num_classes=5).eval()
    feats, ids = fn.extract_features(seg, torch.from_numpy(occ[None]), device="cpu", return_ids=True, meshes=[mesh], fit=((0, 0, 0), 1.0))
    winners = fn.label_mesh(mesh, ids[0], fit=((0, 0, 0), 1.0), device="cpu")
    shown = {f.id for f in feats[0]}
    held = np.concatenate([f.faces for f in feats[0]] + [np.nonzero(~np.isin(winners, list(shown)))[0]])
    assert np.array_equal(np.sort(held), np.arange(len(mesh)))
    assert all((winners[f.faces] == f.id).all() for f in feats[0])
    with pytest.raises(ValueError, match="meshes"):
        fn.recognize(clf, occ[None], device="cpu", meshes=[mesh, mesh])


def parse_obj(path):
    verts, groups, name = [], {}, None
    for line in open(path).read().splitlines():
        kind, *rest = line.split() or [""]
        if kind == "v":
            verts.append([float(x) for x in rest])
        elif kind == "g":
            name = rest[0]
            groups.setdefault(name, [])
        elif kind == "f":
            groups[name].append([int(x) - 1 for x in rest])
    return np.asarray(verts), groups


@needs_rt
def test_cli_label_mesh(tmp_path, capsys):
    from featurenet_amd.cli import main

    occ = small_part()
    mesh = (voxels_to_mesh(occ) * 0.5).astype(np.float32)
    stl, npy, out, js, obj = (str(tmp_path / n) for n in ("part.stl", "ids.npy", "faces.npy", "faces.json", "part.obj"))
    _native.runtime().write_stl(stl, mesh, True)
    ids, _ = fn.label_components(1 - occ[None], device="cpu")
    np.save(npy, ids)
    winners = fn.label_mesh(mesh, ids[0], device="cpu")
    assert main(["label-mesh", stl, npy, "-o", out, "--json", js, "--obj", obj, "--device", "cpu"]) == 0
    assert np.array_equal(np.load(out), winners)
    doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert doc == json.load(open(js)) and doc["triangles"] == len(mesh) and doc["labelled"] == int((winners != 0).sum())
    assert doc["faces"] == {str(k): int((winners == k).sum()) for k in (1, 2, 3)}
    verts, groups = parse_obj(obj)
    assert set(groups) == {"feature_1", "feature_2", "feature_3", "unlabelled"}
    seen = np.zeros(len(mesh), bool)
    for name, faces in groups.items():
        value = 0 if name == "unlabelled" else int(name.split("_")[1])
        index = [f[0] // 3 for f in faces]
        assert all(f == [3 * i, 3 * i + 1, 3 * i + 2] for f, i in zip(faces, index))
        assert (winners[index] == value).all() and not seen[index].any()
        seen[index] = True
    assert seen.all() and np.array_equal(verts.reshape(-1, 3, 3).astype(np.float32), mesh)
    assert main(["label-mesh", stl, npy, "-o", out, "--fit", "0", "0", "0", "0.5", "--device", "cpu"]) == 0
    assert np.array_equal(np.load(out), winners)
    write_labelled_obj(obj, mesh[:2], np.array([5, 5]))
    assert list(parse_obj(obj)[1]) == ["feature_5", "unlabelled"]
