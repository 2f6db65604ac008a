"""Inputs of the distance-transform and dimension-table tests (CPU and GPU) and their cached oracle results."""
import functools

import numpy as np
import torch

from _access_cases import occupancy
from _ccl_cases import expected
from featurenet_amd.ops import reference

SHAPES = [(3, 5, 7), (4, 6, 64), (5, 3, 65), (9, 7, 130)]                # as test_access_gpu.py
LIMIT_SHAPES = [(2, 3, 256), (2, 256, 3), (256, 2, 64)]                  # each axis at its limit
SEEDS = ("dense", "sparse", "ends", "none", "all")

# fn.generate_parts(96, size=32, seed=3) through the CPU oracle path (test_edt_cpu.py pins them there)
PARTS_COMPONENTS = 253
PARTS_SUM_CLEARANCE2 = 4340
PARTS_SUM_WALL = 96478


@functools.lru_cache(maxsize=None)
def seeds(kind: str, N: int, D: int, H: int, W: int) -> torch.Tensor:
    """uint8 [N, D, H, W] with values 0, 1 and 255: density 0.3, density 0.002 (the nearest seed then lies
    far off, often in another 64-wide piece of the row), the first and the last voxel, none, all."""
    rng = np.random.default_rng(sum(map(ord, kind)) * 1000003 + N * 7919 + D * 131 + H * 17 + W)
    shape = (N, D, H, W)
    if kind in ("dense", "sparse"):
        m = rng.random(shape) < (0.3 if kind == "dense" else 0.002)
    elif kind == "ends":
        m = np.zeros(shape, bool)
        m[:, 0, 0, 0] = m[:, -1, -1, -1] = True
    elif kind in ("none", "all"):
        m = np.full(shape, kind == "all")
    else:
        raise KeyError(kind)
    return torch.from_numpy(np.where(m, rng.choice(np.array([1, 255], np.uint8), shape), 0).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def expected_d2(kind: str, N: int, D: int, H: int, W: int, border: bool) -> torch.Tensor:
    """``reference.distance_sq`` of :func:`seeds`; computed once, never modified."""
    return reference.distance_sq(seeds(kind, N, D, H, W), border)


@functools.lru_cache(maxsize=None)
def expected_dims(pattern: str, N: int, D: int, H: int, W: int):
    """(ids, table, offsets, occ, d2, dim) of the CPU oracle for the ``pattern`` label volume of ``_ccl_cases``
    (6-connectivity, background 0) under the random material of ``_access_cases``; computed once, never modified."""
    _, ids, table, offsets = expected(pattern, N, D, H, W, 6, 0)
    occ = occupancy(N, D, H, W)
    d2 = reference.distance_sq(occ)
    return ids, table, offsets, occ, d2, reference.dimension_table(ids, offsets, d2)


def loop_dimension_table(ids: np.ndarray, offsets: np.ndarray, d2: np.ndarray, T: int) -> np.ndarray:
    """The dimension table instance by instance, straight from the definitions."""
    N, D, H, W = ids.shape
    out = np.tile(np.array([-1, -1, 0, 0], np.int64), (T, 1))
    for n in range(N):
        flat_ids, flat_d = ids[n].reshape(-1), d2[n].reshape(-1).astype(np.int64)
        for i in np.unique(flat_ids):
            row = int(offsets[n]) + int(i) - 1
            if i <= 0 or not 0 <= row < T:
                continue
            where = np.flatnonzero(flat_ids == i)
            d = flat_d[where]
            r2 = max(int(d.max()), int(out[row, 0]))       # (rows shared by two samples: foreign offsets)
            first = [int(w) for w, v in zip(where, d) if v == r2]
            if out[row, 0] == r2:
                first.append(int(out[row, 1]))
            out[row] = r2, min(first), out[row, 2] + int((d == 1).sum()), out[row, 3] + len(where)
    return out


def judge(got_d2, want_d2, got_dim, want_dim) -> bool:
    """The comparison every test of the kernels uses: exact equality of both results."""
    return torch.equal(got_d2, want_d2) and torch.equal(got_dim, want_dim)
