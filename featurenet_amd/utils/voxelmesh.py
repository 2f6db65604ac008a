"""The boundary of a voxel volume as a triangle mesh: what ``fn.voxelize`` inverts exactly, and
how a part or one feature instance (a mask of ``ids == k``) leaves the project as an STL file."""
from __future__ import annotations

import numpy as np


def voxels_to_mesh(occ) -> np.ndarray:
    """Boundary quads of ``occ`` ``[S0, S1, S2]`` (indexed ``[z, y, x]``, non-zero = material) ->
    float32 ``[F, 3, 3]``: two triangles per voxel face between material and not, vertices
    ``(x, y, z)`` in voxel units (voxel ``(x, y, z)`` is the cube ``[x, x + 1] x [y, y + 1] x
    [z, z + 1]``), wound counter-clockwise seen from outside.  The mesh is closed: every edge
    belongs to an even number of triangles."""
    occ = np.asarray(occ)
    if occ.ndim != 3:
        raise ValueError(f"voxels_to_mesh: occ must be [D, H, W], not {occ.shape}")
    solid = np.pad(occ != 0, 1)
    out = []
    for axis in range(3):                        # 0 = x, 1 = y, 2 = z; array axis 2 - axis
        u, v = (axis + 1) % 3, (axis + 2) % 3    # e_u x e_v = e_axis
        for sign in (1, -1):
            face = solid & ~np.roll(solid, -sign, axis=2 - axis)
            z, y, x = np.nonzero(face[1:-1, 1:-1, 1:-1])
            p = np.stack([x, y, z], 1).astype(np.float32)
            if sign > 0:
                p[:, axis] += 1
            eu, ev = np.zeros(3, np.float32), np.zeros(3, np.float32)
            eu[u], ev[v] = 1, 1
            quad = [p, p + eu, p + eu + ev, p + ev]
            if sign < 0:
                quad = quad[::-1]
            out.append(np.stack([quad[0], quad[1], quad[2]], 1))
            out.append(np.stack([quad[0], quad[2], quad[3]], 1))
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 3, 3), np.float32)


def write_labelled_obj(path, tris, winners) -> None:
    """Triangles float ``[F, 3, 3]`` (model units) and their winners ``[F]`` (``fn.label_mesh``) ->
    a Wavefront OBJ: three ``v`` lines per triangle in the order given, then one group
    ``g feature_<id>`` per winner, ascending, and last ``g unlabelled`` for winner 0 (there even if
    empty); a group's ``f`` lines name the triangles it holds (triangle ``i`` is ``f 3i+1 3i+2 3i+3``)."""
    tris, winners = np.asarray(tris, np.float64), np.asarray(winners)
    if tris.ndim != 3 or tris.shape[1:] != (3, 3) or winners.shape != (len(tris),):
        raise ValueError(f"write_labelled_obj: tris must be [F, 3, 3] and winners [F], not {tris.shape} and "
                         f"{winners.shape}")
    with open(path, "w") as f:
        f.write("# featurenet_amd label-mesh\n")
        for x, y, z in tris.reshape(-1, 3):
            f.write(f"v {x:.9g} {y:.9g} {z:.9g}\n")
        values = np.unique(winners)
        for value in [*values[values != 0], 0]:             # (unlabelled comes last, and always)
            f.write("g unlabelled\n" if value == 0 else f"g feature_{int(value)}\n")
            for i in np.nonzero(winners == value)[0]:
                f.write(f"f {3 * i + 1} {3 * i + 2} {3 * i + 3}\n")


def icosphere(subdivisions: int = 2):
    """A unit sphere as ``(vertices float64 [V, 3], faces int64 [F, 3])``: an icosahedron whose
    triangles are split in four ``subdivisions`` times (``F = 20 * 4 ** subdivisions``), the new
    vertices pushed out to the sphere.  Closed, outward wound."""
    g = (1 + 5 ** 0.5) / 2
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
             (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
             (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11),
             (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in verts]
    for _ in range(int(subdivisions)):
        mid, split = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            split += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = split
    return np.asarray(verts, np.float64), np.asarray(faces, np.int64)
