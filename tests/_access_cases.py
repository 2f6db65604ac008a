"""Inputs of the access-direction tests (CPU and GPU) and their cached oracle results."""
import functools

import numpy as np
import torch

from _ccl_cases import expected, volume
from featurenet_amd.ops import reference


@functools.lru_cache(maxsize=None)
def occupancy(N: int, D: int, H: int, W: int, density: float = 0.3, seed: int = 0) -> torch.Tensor:
    """Random material, drawn independently of every label volume; values 0, 1 and 255."""
    rng = np.random.default_rng(977 * seed + N * 7919 + D * 131 + H * 17 + W + int(density * 1000))
    m = rng.random((N, D, H, W)) < density
    return torch.from_numpy(np.where(m, rng.choice(np.array([1, 255], np.uint8), m.shape), 0).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def expected_access(pattern: str, N: int, D: int, H: int, W: int):
    """(ids, table, offsets, occ, ex, ey, ez, acc, mask) of the CPU oracle for the ``pattern`` label volume
    of ``_ccl_cases`` (6-connectivity, background 0) under independent random material; computed once, never
    modified."""
    _, ids, table, offsets = expected(pattern, N, D, H, W, 6, 0)
    occ = occupancy(N, D, H, W)
    ex, ey, ez = reference.column_extents(occ)
    acc, mask = reference.access_table(ids, offsets, occ, want_mask=True)
    return ids, table, offsets, occ, ex, ey, ez, acc, mask


def singles(N: int, D: int, H: int, W: int):
    """Every voxel its own instance: (ids, offsets) with ids 1..V in raster order in each sample."""
    V = D * H * W
    ids = torch.arange(1, V + 1, dtype=torch.int32).view(1, D, H, W).repeat(N, 1, 1, 1).contiguous()
    return ids, torch.arange(N + 1, dtype=torch.int64) * V


def fully_open_toward_truth(labels, voxels, parts, slots, feats, ids) -> int:
    """Checks that every component of ``labels`` is fully open toward the access face of the generated
    feature whose slot it carries, and that no feature is left without a component -> features checked."""
    seen = set()
    for n, recs in enumerate(feats):
        by_slot = {p.slot: p for p in parts[n]}
        for f in recs:
            carried = np.unique(slots[n][ids[n] == f.id])
            assert len(carried) == 1 and carried[0] >= 1, (n, f, carried)
            p = by_slot[int(carried[0]) - 1]
            assert f.cls == p.cls + 1, (n, f, p)
            assert f.access[p.orientation % 6] == f.voxels, (n, f, p)
            assert p.face in f.open_faces(), (n, f, p)
            seen.add((n, p.slot))
    carved = {(n, int(s) - 1) for n in range(len(parts)) for s in np.unique(slots[n]) if s}
    assert seen == carved and len(seen) == sum(len(ps) for ps in parts), (len(seen), len(carved))
    return len(seen)
