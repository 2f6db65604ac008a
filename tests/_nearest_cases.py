"""Inputs of the labelled-distance-transform and wall-table tests (CPU and GPU) and their cached oracle results."""
import functools

import numpy as np
import torch

from _ccl_cases import expected
from featurenet_amd.ops import reference
from featurenet_amd.ops.reference import EDT_INF, NN_NONE

# under a wave, one wave, a second piece of one lane, two pieces less one lane
SHAPES = [(3, 5, 7), (4, 6, 64), (5, 3, 65), (3, 4, 127)]
LIMIT_SHAPES = [(2, 3, 128), (2, 128, 3), (128, 2, 64)]                  # each axis at its limit
IDS = ("none", "one", "ends", "same-ends", "dense", "sparse", "ties", "big")
BIG = 2 ** 31 - 1

# fn.generate_parts(96, size=32, seed=3) through the CPU oracle path (test_nearest_cpu.py pins them there):
# instances, those with another feature in their part, the smallest gap2, the sum of gap2; with separate=False
# the instances with gap2 == 1 instead of the smallest
PARTS = {"instances": 253, "with_other": 234, "alone": 19, "min_gap2": 4, "sum_gap2": 21218}
PARTS_TOUCHING = {"instances": 253, "with_other": 234, "touching": 83, "sum_gap2": 17996}


@functools.lru_cache(maxsize=None)
def ids(kind: str, N: int, D: int, H: int, W: int) -> torch.Tensor:
    """int32 [N, D, H, W]; the samples differ in every kind but ``none``.
    none: no seed (0 and negative values); one: a single label, so rank 1 is missing everywhere; ends: one id at
    the first voxel and another at the last; same-ends: one id at both ends (two seeds, rank 1 still missing);
    dense: density 0.3, ids 1..3; sparse: density 0.002, ids 1..50 (the nearest other lies far off, often in the
    other 64-wide piece of the row); ties: two labels mirrored about the volume's centre, the larger id first in
    raster order (equal distances on a whole plane: the smaller id must win); big: ids 2^31 - 1 and 2^31 - 2 among
    negative non-seeds."""
    rng = np.random.default_rng(sum(map(ord, kind)) * 1000003 + N * 7919 + D * 131 + H * 17 + W)
    shape, V = (N, D, H, W), D * H * W
    out = np.zeros((N, V), np.int64)
    if kind == "none":
        out[:] = rng.choice(np.array([0, -1, -(2 ** 31)]), (N, V))
    elif kind == "one":
        for n in range(N):
            out[n, rng.random(V) < 0.05] = 3 + n
            out[n, rng.integers(V)] = 3 + n
    elif kind == "ends":
        for n in range(N):
            out[n, 0], out[n, -1] = 1 + n, 2 + n
    elif kind == "same-ends":
        for n in range(N):
            out[n, 0] = out[n, -1] = 5 + n
    elif kind in ("dense", "sparse"):
        density, top = (0.3, 3) if kind == "dense" else (0.002, 50)
        out = np.where(rng.random((N, V)) < density, rng.integers(1, top + 1, (N, V)), 0)
    elif kind == "ties":
        for n in range(N):
            first = np.flatnonzero(rng.random(V // 2) < 0.02)
            first = first if len(first) else np.array([rng.integers(V // 2)])
            out[n, first], out[n, V - 1 - first] = 2 + n, 1 + n
    elif kind == "big":
        u = rng.random((N, V))
        out = np.where(u < 0.05, BIG, np.where(u < 0.1, BIG - 1, np.where(u < 0.5, -1, 0)))
        out[:, 0] = -(2 ** 31)
    else:
        raise KeyError(kind)
    return torch.from_numpy(out.reshape(shape).astype(np.int32))


@functools.lru_cache(maxsize=None)
def expected_nn(kind: str, N: int, D: int, H: int, W: int) -> torch.Tensor:
    """``reference.nearest_labels`` of :func:`ids`; computed once, never modified."""
    return reference.nearest_labels(ids(kind, N, D, H, W))


@functools.lru_cache(maxsize=None)
def expected_walls(pattern: str, N: int, D: int, H: int, W: int, limit2: int):
    """(ids, table, offsets, nn, wall) of the CPU oracle for the ``pattern`` label volume of ``_ccl_cases``
    (6-connectivity, background 0); computed once, never modified."""
    _, ids_, table, offsets = expected(pattern, N, D, H, W, 6, 0)
    nn = reference.nearest_labels(ids_)
    return ids_, table, offsets, nn, reference.wall_table(ids_, offsets, nn, limit2)


def brute_nearest(vol: np.ndarray) -> np.ndarray:
    """The two ranks of one small volume [D, H, W] from all pairs (voxel, seed), straight from the definitions ->
    int64 [2, D, H, W]."""
    D, H, W = vol.shape
    out = np.full((2, D, H, W), NN_NONE, np.int64)
    seeds = [(z, y, x, int(vol[z, y, x])) for z in range(D) for y in range(H) for x in range(W) if vol[z, y, x] > 0]
    for z in range(D):
        for y in range(H):
            for x in range(W):
                per = {}
                for sz, sy, sx, L in seeds:
                    d2 = (z - sz) ** 2 + (y - sy) ** 2 + (x - sx) ** 2
                    per[L] = min(per.get(L, d2), d2)
                keys = sorted(d2 << 32 | L for L, d2 in per.items())
                for r, k in enumerate(keys[:2]):
                    out[r, z, y, x] = k
    return out


def loop_wall_table(ids_: np.ndarray, offsets: np.ndarray, nn: np.ndarray, T: int, limit2: int) -> np.ndarray:
    """The kernel's columns of the wall table -- gap2, at, thin, voxels -- instance by instance, straight from the
    definitions (``other`` needs offsets that belong to the ids: :func:`loop_other`)."""
    N = ids_.shape[0]
    out = np.tile(np.array([-1, -1, 0, 0], np.int64), (T, 1))
    for n in range(N):
        flat_ids, flat_d = ids_[n].reshape(-1), (nn[n, 1] >> 32).reshape(-1)
        for i in np.unique(flat_ids):
            row = int(offsets[n]) + int(i) - 1
            if i <= 0 or not 0 <= row < T:
                continue
            where = np.flatnonzero(flat_ids == i)
            d = flat_d[where]
            out[row, 2] += int((d <= limit2).sum())
            out[row, 3] += len(where)
            gap2 = int(d.min())
            if gap2 >= EDT_INF:
                continue
            if out[row, 0] >= 0:                           # (rows shared by two samples: foreign offsets)
                gap2 = min(gap2, int(out[row, 0]))
            first = [int(w) for w, v in zip(where, d) if v == gap2]
            if out[row, 0] == gap2:
                first.append(int(out[row, 1]))
            out[row, :2] = gap2, min(first)
    return out


def loop_other(ids_: np.ndarray, offsets: np.ndarray, nn: np.ndarray, wall: np.ndarray) -> np.ndarray:
    """``other`` of every row from the table's own ``at``: the row of the id that rank 1 names there."""
    out = np.full(len(wall), -1, np.int64)
    for n in range(ids_.shape[0]):
        for r in range(int(offsets[n]), int(offsets[n + 1])):
            if wall[r, 0] >= 0:
                out[r] = int(offsets[n]) + int(nn[n, 1].reshape(-1)[wall[r, 1]] & 0xFFFFFFFF) - 1
    return out


def parts_summary(feats) -> dict:
    recs = [f for fs in feats for f in fs]
    gaps = [f.gap2 for f in recs if f.gap2 is not None]
    return {"instances": len(recs), "with_other": len(gaps), "alone": len(recs) - len(gaps),
            "min_gap2": min(gaps), "touching": sum(g == 1 for g in gaps), "sum_gap2": sum(gaps)}


def judge(got_nn, want_nn, got_wall, want_wall) -> bool:
    """The comparison every test of the kernels uses: exact equality of both results."""
    return torch.equal(got_nn, want_nn) and torch.equal(got_wall, want_wall)
