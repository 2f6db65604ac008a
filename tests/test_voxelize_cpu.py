"""The voxelizer without a GPU: the host path (``_rt.voxelize_tris``) against the torch oracle
(``reference.voxelize_tris``), what the rule promises (the boundary mesh of a volume gives the
volume back, a mesh listed twice cancels, order, vertex rotation and winding do not matter, ties
on edges and vertices leave no column open), ``quantize``, STL files, ``fn.voxelize`` and the CLI.
"""
import json

import numpy as np
import pytest
import torch

import featurenet_amd as fn
import _mesh_cases as mc
from featurenet_amd import _native
from featurenet_amd.ops import reference
from featurenet_amd.ops import voxelize as vx
from featurenet_amd.utils.voxelmesh import icosphere, voxels_to_mesh


def host(tris, off, size, threads=3):
    occ, leaks = _native.runtime().voxelize_tris(tris.numpy(), off.numpy(), size, threads)
    return torch.from_numpy(occ), torch.from_numpy(leaks)


def both(meshes, size):
    """Oracle and host path on a batch, asserted equal -> ``(occ, leaks)``."""
    tris, off = mc.batch(meshes)
    occ, leaks = reference.voxelize_tris(tris, off, size)
    got = host(tris, off, size)
    assert torch.equal(got[0], occ) and torch.equal(got[1], leaks)
    assert occ.dtype == torch.uint8 and leaks.dtype == torch.int64 and occ.shape == (len(meshes),) + (size,) * 3
    return occ, leaks


@pytest.mark.parametrize("size", [8, 16, 24])
def test_host_path_equals_the_oracle(size):
    for name, tris, off, occ, leaks in mc.suite(size):
        for threads in (1, 5):
            got = host(tris, off, size, threads)
            assert torch.equal(got[0], occ) and torch.equal(got[1], leaks), name
        dev_occ, dev_leaks = vx.voxelize(tris, off, size)
        assert torch.equal(dev_occ, occ) and torch.equal(dev_leaks, leaks)
        bits, _ = vx.voxelize(tris, off, size, packed=True)
        assert torch.equal(bits.reshape(-1), torch.from_numpy(np.packbits(occ.numpy().reshape(-1), bitorder="little")))


@pytest.mark.parametrize("size,source", [(8, "random"), (16, "random"), (16, "parts"), (24, "parts")])
def test_boundary_mesh_gives_the_volume_back(size, source):
    vols = [mc.random_volume(size, s, d) for s, d in ((1, 0.5), (2, 0.15), (3, 0.85))] if source == "random" \
        else list(mc.parts(size, 3, 4))
    occ, leaks = both([mc.boundary_tris(v, seed=i) for i, v in enumerate(vols)], size)
    assert np.array_equal(occ.numpy(), np.stack(vols)) and not leaks.any()
    # the same meshes, twice as large
    occ2, leaks2 = both([mc.boundary_tris(v, scale=2, seed=i) for i, v in enumerate(vols)], 2 * size)
    want = np.stack(vols).repeat(2, 1).repeat(2, 2).repeat(2, 3)
    assert np.array_equal(occ2.numpy(), want) and not leaks2.any()


def test_a_mesh_listed_twice_cancels():
    v = mc.parts(16)[0]
    occ, leaks = both([np.concatenate([mc.boundary_tris(v, seed=1), mc.boundary_tris(v, seed=2)]),
                       np.concatenate([mc.octahedron(), mc.box(), mc.octahedron(), mc.box()])], 16)
    assert not occ.any() and not leaks.any()


def test_order_rotation_and_winding_do_not_matter():
    plain = [mc.boundary_tris(mc.parts(16)[1], seed=None), mc.sphere(2, (8.0, 7.0, 9.0), 6.1)[0], mc.octahedron()]
    want = both(plain, 16)
    for seed in (1, 2, 3):
        got = both([mc.scramble(m, seed) for m in plain], 16)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert want[0].any() and not want[1].any()


def test_ties_the_box():
    occ, leaks = both([mc.box()], 8)
    want = np.zeros((8, 8, 8), np.uint8)
    want[2:7, 1:5, 0:6] = 1                          # x 0..5, y 1..4, z 2..6
    assert np.array_equal(occ[0].numpy(), want) and leaks.tolist() == [0]


@pytest.mark.parametrize("solid,volume", [(mc.box, 120), (mc.octahedron, 38)], ids=["box", "octahedron"])
def test_ties_under_the_48_symmetries(solid, volume):
    syms = mc.symmetries(8)
    assert len(syms) == 48
    occ, leaks = both([sym(solid()) for sym in syms], 8)
    assert leaks.tolist() == [0] * 48
    assert occ.reshape(48, -1).sum(1).tolist() == [volume] * 48


def test_open_meshes_report_their_columns():
    for face in (0, 1):
        occ, leaks = both([mc.box(skip_face=face)], 8)
        assert leaks.tolist() == [4 * 5]             # the columns of the missing x face: y 1..4, z 2..6
        cols = occ[0].numpy()[2:7, 1:5]
        if face == 1:                                # entered and never left: solid to the end of the grid
            assert cols[:, :, 0:].all() and occ.sum() == 20 * 8
        else:                                        # never entered: the far face starts the material
            assert not cols[:, :, :6].any() and cols[:, :, 6:].all() and occ.sum() == 20 * 2


@pytest.mark.parametrize("size,sub,centre,radius", mc.SPHERES, ids=["16-80", "24-320", "16-320-outside"])
def test_icospheres(size, sub, centre, radius):
    for seed in (1, 2):
        tris, e = mc.sphere(sub, centre, radius, seed)
        assert len(tris) == 20 * 4 ** sub
        occ, leaks = both([tris], size)
        solid, empty = mc.sphere_bounds(size, centre, radius, e)
        filled = occ[0].numpy().astype(bool)
        assert filled[solid].all() and not filled[empty].any()
        undecided = 1 - (solid | empty).mean()
        assert undecided <= 0.08, undecided
        assert leaks.tolist() == [0]                 # (the part outside the grid is open towards -x only)


def test_quantize():
    g = np.random.default_rng(0)
    v = g.normal(size=(50, 3)) * (3.0, 1.0, 0.5) + (10.0, -4.0, 2.0)
    for size, margin in ((64, 0), (64, 2), (24, 1.5)):
        q, origin, vs = vx.quantize(v, size, "bbox", margin)
        assert q.dtype == np.int32 and q.shape == v.shape
        lo, hi = q.min(0), q.max(0)
        assert lo[0] == 16 * margin and hi[0] == 16 * (size - margin)        # the longest side spans it exactly
        for axis in (1, 2):                                                 # the others are centred to a unit
            assert abs((lo[axis] + hi[axis]) - 16 * size) <= 1
        assert np.abs((origin + q * (vs / 16)) - v).max() <= vs / 32 * (1 + 1e-9)        # the transform, back
        again, o2, vs2 = vx.quantize(v, size, (origin, vs))
        assert np.array_equal(again, q) and np.array_equal(o2, origin) and vs2 == vs
    q, origin, vs = vx.quantize(voxels_to_mesh(mc.parts(16)[0]), 16)                    # a part fills the grid
    assert np.array_equal(q, 16 * voxels_to_mesh(mc.parts(16)[0])) and vs == 1 and not origin.any()
    tri = vx.quantize(np.zeros((4, 3, 3)) + np.arange(3)[:, None], 8, ((0, 0, 0), 0.5))[0]
    assert tri.shape == (4, 3, 3) and tri.max() == 64
    with pytest.raises(ValueError, match="lattice ends"):
        vx.quantize(v, 64, ((0.0, 0.0, 0.0), 0.01))
    with pytest.raises(ValueError, match="no extent"):
        vx.quantize(np.ones((3, 3)), 64)
    with pytest.raises(ValueError, match="margin"):
        vx.quantize(v, 64, "bbox", 32)
    with pytest.raises(ValueError, match="fit"):
        vx.quantize(v, 64, "sphere")
    with pytest.raises(ValueError, match="not finite"):
        vx.quantize(np.array([[0.0, np.nan, 1.0]]), 64)
    with pytest.raises(ValueError, match="multiple of 8"):
        vx.quantize(v, 20)


def test_stl_files(tmp_path):
    rt = _native.runtime()
    v, f = icosphere(1)
    tris = (v[f] * 3.25 + 0.1).astype(np.float32)
    for binary in (True, False):
        p = str(tmp_path / f"s{int(binary)}.stl")
        rt.write_stl(p, tris, binary)
        back = rt.read_stl(p)
        assert back.dtype == np.float32 and back.shape == (80, 3, 3) and np.array_equal(back, tris)
    raw = (tmp_path / "s1.stl").read_bytes()
    assert len(raw) == 84 + 50 * 80 and (tmp_path / "s0.stl").read_text().startswith("solid")
    sly = tmp_path / "solid.stl"                     # a binary file whose header begins with "solid"
    sly.write_bytes(b"solid but binary".ljust(80) + raw[80:])
    assert np.array_equal(rt.read_stl(str(sly)), tris)
    rt.write_stl(str(tmp_path / "none.stl"), np.zeros((0, 3, 3), np.float32), True)
    assert rt.read_stl(str(tmp_path / "none.stl")).shape == (0, 3, 3)
    text = (tmp_path / "s0.stl").read_text()
    bad = {"cut": raw[:-7], "lying": raw[:80] + (81).to_bytes(4, "little") + raw[84:], "short": raw[:50],
           "junk": bytes(range(256)) * 3, "empty": b"", "half": text[:len(text) // 2].encode(),
           "word": text.replace("vertex", "vertx", 1).encode(), "number": text.replace("vertex ", "vertex x", 1).encode(),
           "open": text.replace("endsolid", "").encode()}
    for name, data in bad.items():
        p = tmp_path / f"bad_{name}.stl"
        p.write_bytes(data)
        with pytest.raises(RuntimeError, match="read_stl"):
            rt.read_stl(str(p))
    with pytest.raises(RuntimeError, match="cannot open"):
        rt.read_stl(str(tmp_path / "missing.stl"))
    with pytest.raises(RuntimeError, match=r"\[F, 3, 3\]"):
        rt.write_stl(str(tmp_path / "x.stl"), np.zeros((4, 3), np.float32), True)


def test_check_tris_refusals():
    tris, off = mc.batch([mc.box(), mc.octahedron()])
    vx.check_tris(tris, off)
    for bad_t, bad_o, msg in ((tris.long(), off, "int32"), (tris[:, :8], off, "int32"), (tris.numpy(), off, "ndarray"),
                              (tris, off.long(), "offsets"), (tris, off[None], "offsets"),
                              (tris, off + 1, "run from 0"), (tris, off[:2], "run from 0"),
                              (tris, torch.tensor([0, 14, 12, 20], dtype=torch.int32), "decrease"),
                              (tris + 8100, off, "8192"), (-tris - 8100, off, "8192")):
        with pytest.raises(ValueError, match=msg):
            vx.voxelize(bad_t, bad_o, 16)
    for size in (12, 4, 264, 16.0, True):
        with pytest.raises(ValueError, match="multiple of 8"):
            vx.voxelize(tris, off, size)
    rt = _native.runtime()
    t, o = tris.numpy(), off.numpy()
    for call in (lambda: rt.voxelize_tris(t, o, 12, 1), lambda: rt.voxelize_tris(t[:, :8], o, 16, 1),
                 lambda: rt.voxelize_tris(t, o + 1, 16, 1), lambda: rt.voxelize_tris(t, o[::-1].copy(), 16, 1),
                 lambda: rt.voxelize_tris(t + 8100, o, 16, 1)):
        with pytest.raises(RuntimeError, match="voxelize_tris"):
            call()
    with pytest.raises(ValueError, match="int32"):
        reference.voxelize_tris(tris.long(), off, 16)


def test_voxels_to_mesh():
    one = voxels_to_mesh(np.ones((1, 1, 1)))
    assert one.dtype == np.float32 and one.shape == (12, 3, 3) and one.min() == 0 and one.max() == 1
    normals = np.cross(one[:, 1] - one[:, 0], one[:, 2] - one[:, 0])
    assert (np.einsum("fd,fd->f", normals, one.mean(1) - 0.5) > 0).all()             # outward
    v = mc.random_volume(8, 5)
    tris = voxels_to_mesh(v)
    faces = sum(int((np.diff(np.pad(v, 1).astype(np.int8), axis=a) != 0).sum()) for a in range(3))
    assert len(tris) == 2 * faces
    ids = (tris.astype(np.int64) * (1, 9, 81)).sum(-1)                                # vertex -> number (0..8 per axis)
    edges = np.sort(np.concatenate([ids[:, [i, (i + 1) % 3]] for i in range(3)]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts % 2 == 0).all()                                                   # closed: every edge an even count
    assert voxels_to_mesh(np.zeros((4, 4, 4))).shape == (0, 3, 3)
    with pytest.raises(ValueError, match="D, H, W"):
        voxels_to_mesh(np.zeros((4, 4)))


def test_voxelize_on_the_cpu(tmp_path):
    assert "voxelize" in fn.__all__
    rt = _native.runtime()
    part = mc.parts(16)[0]
    mesh = voxels_to_mesh(part)
    stl, txt = tmp_path / "part.stl", tmp_path / "part_ascii.stl"
    rt.write_stl(str(stl), mesh, True)
    rt.write_stl(str(txt), mesh, False)
    for m in (str(stl), txt, mesh, torch.from_numpy(mesh), [mesh]):
        vox = fn.voxelize(m, size=16, device="cpu")
        assert vox.dtype == np.uint8 and vox.shape == (1, 16, 16, 16) and np.array_equal(vox[0], part)
    verts, inverse = np.unique(mesh.reshape(-1, 3), axis=0, return_inverse=True)
    pair = (verts, inverse.reshape(-1, 3))
    vox, info = fn.voxelize([pair, str(stl), mesh * 2.5 - 7], size=16, device="cpu", return_info=True)
    assert vox.shape == (3, 16, 16, 16) and all(np.array_equal(v, part) for v in vox)
    assert info["leaks"].tolist() == [0, 0, 0] and info["origin"].shape == (3, 3)
    assert np.allclose(info["voxel_size"], [1, 1, 2.5]) and np.allclose(info["origin"][2], -7)
    bits = fn.voxelize(mesh, size=16, device="cpu", packed=True)
    assert bits.shape == (1, 512) and np.array_equal(np.unpackbits(bits[0], bitorder="little"), part.reshape(-1))
    big = fn.voxelize(mesh, size=32, device="cpu")                         # bbox: the part fills any grid
    assert np.array_equal(big[0], part.repeat(2, 0).repeat(2, 1).repeat(2, 2))
    inset, info = fn.voxelize(mesh, size=32, margin=8, device="cpu", return_info=True)
    assert np.array_equal(inset[0, 8:24, 8:24, 8:24], part) and inset.sum() == part.sum()
    assert info["voxel_size"][0] == 1 and info["origin"].tolist() == [[-8, -8, -8]]
    v, f = icosphere(2)
    ball, info = fn.voxelize((v, f), size=24, fit=((-1.5, -1.5, -1.5), 0.125), device="cpu", return_info=True)
    assert abs(ball.sum() / (4 / 3 * np.pi * 8 ** 3) - 1) < 0.08 and info["leaks"].tolist() == [0]
    holed, info = fn.voxelize(v[f[5:]], size=24, fit=((-1.5, -1.5, -1.5), 0.125), device="cpu", return_info=True)
    assert info["leaks"][0] > 0                                            # not watertight: the user is told
    assert fn.voxelize([], size=8, device="cpu").shape == (0, 8, 8, 8)
    with pytest.raises(ValueError, match="STL path"):
        fn.voxelize(np.zeros((4, 3)), size=8, device="cpu")
    with pytest.raises(ValueError, match="outside"):
        fn.voxelize((verts, inverse.reshape(-1, 3) + len(verts)), size=8, device="cpu")
    with pytest.raises(RuntimeError, match="cannot open"):
        fn.voxelize(str(tmp_path / "missing.stl"), size=8, device="cpu")


def test_cli_voxelize_and_export_stl(tmp_path, capsys):
    from featurenet_amd.cli import main

    parts = mc.parts(16)
    np.save(tmp_path / "parts.npy", parts)
    stls = [str(tmp_path / f"p{i}.stl") for i in range(2)]
    assert main(["export-stl", str(tmp_path / "parts.npy"), "-o", stls[0]]) == 0
    assert main(["export-stl", str(tmp_path / "parts.npy"), "--index", "1", "-o", stls[1], "--ascii",
                 "--voxel-size", "0.5", "--origin", "1", "2", "3"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[0])["voxels"] == int(parts[0].sum()) and json.loads(lines[1])["triangles"] > 0
    assert open(stls[1]).read().startswith("solid") and len(open(stls[0], "rb").read()) % 50 == 34
    out, js, bv = tmp_path / "vox.npy", tmp_path / "info.json", tmp_path / "bv"
    assert main(["voxelize", *stls, "--size", "16", "-o", str(out), "--json", str(js), "--binvox", str(bv),
                 "--device", "cpu"]) == 0
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["shape"] == [2, 16, 16, 16] and summary["leaks"] == [0, 0]
    assert summary["filled_voxels"] == parts.reshape(2, -1).sum(1).tolist()
    assert np.allclose(summary["voxel_size"], [1, 0.5]) and np.allclose(summary["origin"], [[0, 0, 0], [1, 2, 3]])
    assert json.loads(js.read_text()) == summary
    vox = np.load(out, allow_pickle=False)
    assert vox.dtype == np.uint8 and np.array_equal(vox, parts)
    grid, translate, scale = _native.runtime().read_binvox(str(bv / "p1.binvox"))
    assert np.array_equal(grid, parts[1]) and np.allclose(translate, [1, 2, 3]) and np.isclose(scale, 8.0)
    assert main(["voxelize", stls[1], "--size", "16", "--origin", "1", "2", "3", "--voxel-size", "0.5", "-o", str(out),
                 "--device", "cpu"]) == 0
    assert np.array_equal(np.load(out)[0], parts[1])
    labels = fn.generate_parts(1, size=16, seed=2, features=(1, 2), device="cpu")[1]
    np.save(tmp_path / "labels.npy", labels)
    value = int(labels.max())
    assert main(["export-stl", str(tmp_path / "labels.npy"), "--value", str(value), "-o", stls[0]]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["voxels"] == int((labels == value).sum())
