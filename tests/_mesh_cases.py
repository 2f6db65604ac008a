"""Meshes for the voxelizer's tests (CPU and GPU), on the lattice of 16 units per voxel, and the
oracle's results for them, computed once per process.

Boundary meshes of volumes come shuffled, with every triangle's vertices rotated and its winding
flipped at random: the rule must not see any of that.  The box and the octahedron have edges and
vertices that pass through column centres (``16 k + 8``), so they live on the tie rule; the 48
symmetries of the cube move them through every orientation of it.
"""
import functools
import itertools

import numpy as np
import torch

from featurenet_amd.ops import partgen, reference
from featurenet_amd.utils.voxelmesh import icosphere, voxels_to_mesh

U = 16
BOX = ((8, 24, 40), (104, 88, 120))              # at 8^3: voxels x 0..5, y 1..4, z 2..6
OCTA = ((72, 56, 72), 48)                        # centre, radius (8^3)


def scramble(tris: np.ndarray, seed: int) -> np.ndarray:
    """``[T, 9]`` -> the same triangles in another order, each with its vertices rotated and, one
    in two, its winding flipped."""
    g = np.random.default_rng(seed)
    t = tris.reshape(-1, 3, 3)[g.permutation(len(tris))]
    turn = g.integers(0, 3, len(t))
    t = np.stack([t[np.arange(len(t)), (turn + i) % 3] for i in range(3)], 1)
    flip = g.integers(0, 2, len(t)).astype(bool)
    t[flip] = t[flip][:, [0, 2, 1]]
    return np.ascontiguousarray(t.reshape(-1, 9))


def boundary_tris(occ, scale: int = 1, seed: int | None = 0) -> np.ndarray:
    """The boundary mesh of a volume on the lattice, int32 ``[T, 9]``, scrambled by ``seed``."""
    t = np.rint(voxels_to_mesh(np.asarray(occ)) * (U * scale)).astype(np.int32).reshape(-1, 9)
    return t if seed is None else scramble(t, seed)


def batch(meshes):
    """List of ``[T_i, 9]`` arrays -> ``(tris int32 [T, 9], offsets int32 [N + 1])`` tensors."""
    meshes = [np.asarray(m, np.int32).reshape(-1, 9) for m in meshes]
    tris = np.concatenate(meshes) if meshes else np.zeros((0, 9), np.int32)
    off = np.concatenate([[0], np.cumsum([len(m) for m in meshes])]).astype(np.int32)
    return torch.from_numpy(tris), torch.from_numpy(off)


def random_volume(size: int, seed: int, density: float = 0.45) -> np.ndarray:
    return (np.random.default_rng(seed).random((size,) * 3) < density).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def parts(size: int, n: int = 2, seed: int = 3) -> np.ndarray:
    """Occupancy of ``n`` sampled parts, uint8 ``[n, S, S, S]`` (the torch oracle's carving)."""
    return reference.carve_parts(partgen.sample(n, size, seed, (2, 4)), size)[0].numpy()


def from_faces(vertices, faces) -> np.ndarray:
    return np.asarray(vertices, np.int64)[np.asarray(faces)].reshape(-1, 9).astype(np.int32)


def box(lo=BOX[0], hi=BOX[1], skip_face: int | None = None) -> np.ndarray:
    """12 triangles, outward wound; ``skip_face`` 0 / 1 leaves out the face at x = lo / x = hi."""
    v = list(itertools.product(*zip(lo, hi)))                                 # index = 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [f for i, q in enumerate(quads) if i != skip_face for f in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return from_faces(v, faces)


def octahedron(centre=OCTA[0], radius=OCTA[1]) -> np.ndarray:
    c = np.asarray(centre)
    v = [c + radius * np.eye(3, dtype=np.int64)[i] * s for i in range(3) for s in (1, -1)]     # +x -x +y -y +z -z
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return from_faces(v, faces)


def symmetries(size: int):
    """The 48 symmetries of the grid as functions on ``[T, 9]`` lattice triangles."""
    out = []
    for perm in itertools.permutations(range(3)):
        for mirror in itertools.product((False, True), repeat=3):
            def apply(tris, perm=perm, mirror=mirror):
                t = tris.reshape(-1, 3, 3)[:, :, list(perm)].copy()
                for axis, m in enumerate(mirror):
                    if m:
                        t[:, :, axis] = U * size - t[:, :, axis]
                return np.ascontiguousarray(t.reshape(-1, 9))
            out.append(apply)
    return out


def rotation(seed: int) -> np.ndarray:
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def sphere(subdivisions: int, centre, radius: float, seed: int = 0):
    """A rotated icosphere snapped to the lattice -> ``(tris int32 [T, 9], longest edge of the
    unit mesh)``; ``centre`` and ``radius`` in voxels."""
    v, f = icosphere(subdivisions)
    v = v @ rotation(seed).T
    e = float(np.linalg.norm(v[f] - v[f][:, [1, 2, 0]], axis=-1).max())
    return from_faces(np.rint((v * radius + np.asarray(centre, np.float64)) * U), f), e


SPHERES = ((16, 1, (8.0, 8.0, 8.0), 6.3), (24, 2, (12.0, 12.0, 12.0), 10.7), (16, 2, (5.0, 8.0, 11.0), 9.5))


def sphere_bounds(size: int, centre, radius: float, e: float):
    """``(must be solid, must be empty)`` bool ``[S, S, S]`` for a sphere's voxelization: a voxel
    whose centre is nearer than the inscribed radius of the faceted, snapped mesh is solid, one
    farther than the radius plus the snap is empty."""
    ax = np.arange(size) + 0.5
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return d < radius * np.sqrt(1 - e * e / 3) - 1 / 16, d > radius + 1 / 16


@functools.lru_cache(maxsize=None)
def suite(size: int):
    """The cases that every path runs at ``size`` (8, 16 or 24): ``(name, tris, offsets, occ,
    leaks)`` with the oracle's results."""
    s = size
    vol = [random_volume(s, 7), random_volume(s, 8, 0.2)] if s <= 16 else list(parts(s))
    half = [random_volume(s // 2, 9)] if s >= 16 else []
    meshes = {
        "volumes": [boundary_tris(v, seed=i) for i, v in enumerate(vol)],
        "doubled": [boundary_tris(v, scale=2, seed=5) for v in half],
        "twice": [np.concatenate([boundary_tris(vol[0], seed=1), boundary_tris(vol[0], seed=2)])],
        "ties": [sym(box()) + 0 for sym in symmetries(8)[::7]] + [sym(octahedron()) for sym in symmetries(8)[::5]],
        "open": [box(skip_face=0), box(skip_face=1)],
        "uneven": [boundary_tris(vol[0]), np.zeros((0, 9), np.int32), box(), octahedron(), sphere(1, (s / 2,) * 3, 0.4 * s)[0]],
        "three": [box(), np.zeros((0, 9), np.int32), boundary_tris(vol[-1], seed=6)],
        "outside": [sphere(2, (0.3 * s, 0.5 * s, 0.7 * s), 0.6 * s, seed=4)[0]],
        "single": [octahedron()],
        "empty": [np.zeros((0, 9), np.int32)],
        "none": [],
    }
    out = []
    for name, ms in meshes.items():
        if name == "doubled" and not ms:
            continue
        tris, off = batch(ms)
        occ, leaks = reference.voxelize_tris(tris, off, s)
        out.append((name, tris, off, occ, leaks))
    return out
