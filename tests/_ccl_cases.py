"""Label volumes for the connected-component tests (CPU and GPU) and their cached oracle results."""
import functools

import numpy as np
import torch

from featurenet_amd.ops import reference

PATTERNS = ("noise2", "noise4", "blobs", "checker", "solid", "empty", "serpentine", "samples", "wrap")


def serpentine_mask(D: int, H: int, W: int) -> np.ndarray:
    """One path through every even plane: full rows at even y joined at alternating ends, the planes
    joined at alternating ends of the plane's path.  It starts at voxel 0."""
    m = np.zeros((D, H, W), bool)
    m[::2, ::2, :] = True
    for j, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            x = W - 1 if j % 2 == 0 else 0
            m[::2, y, x] = True
    rows = (H + 1) // 2                                   # full rows per plane; the path ends on the last
    end = (2 * (rows - 1), W - 1 if rows % 2 == 1 else 0)
    for k, z in enumerate(range(1, D, 2)):
        if z + 1 < D:
            y, x = end if k % 2 == 0 else (0, 0)
            m[z, y, x] = True
    return m


@functools.lru_cache(maxsize=None)
def volume(pattern: str, N: int, D: int, H: int, W: int) -> torch.Tensor:
    rng = np.random.default_rng(sum(map(ord, pattern)) * 1000003 + N * 7919 + D * 131 + H * 17 + W)
    shape = (N, D, H, W)
    if pattern in ("noise2", "noise4"):
        v = rng.integers(0, int(pattern[-1]), shape)
    elif pattern == "blobs":                               # block-upsampled coarse noise, odd block so it
        b = 3                                              # never lines up with the tile faces
        coarse = rng.integers(0, 4, (N, -(-D // b), -(-H // b), -(-W // b)))
        v = np.kron(coarse, np.ones((1, b, b, b), np.int64))[:, :D, :H, :W]
    elif pattern == "checker":                             # two non-background classes
        z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
        v = np.broadcast_to(1 + (z + y + x) % 2, shape)
    elif pattern == "solid":
        v = np.full(shape, 7)
    elif pattern == "empty":
        v = np.zeros(shape)
    elif pattern == "serpentine":
        v = np.broadcast_to(serpentine_mask(D, H, W), shape)
    elif pattern == "samples":                             # facing end planes of consecutive samples
        v = np.zeros(shape)
        v[:-1, D - 1] = 3
        v[1:, 0] = 3
    elif pattern == "wrap":                                # end of a row / plane and the start of the next
        v = np.zeros(shape)
        v[:, 0, 0, W - 1] = 2
        if H > 1:
            v[:, 0, 1, 0] = 2
            v[:, 0, H - 1, W - 1] = 5
        if D > 1:
            v[:, 1, 0, 0] = 5
    else:
        raise KeyError(pattern)
    return torch.from_numpy(np.ascontiguousarray(v).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def expected(pattern: str, N: int, D: int, H: int, W: int, connectivity: int, background):
    """(roots, ids, table, offsets) of the CPU oracle; computed once, never modified."""
    lab = volume(pattern, N, D, H, W)
    roots = reference.connected_components(lab, background, connectivity)
    ids, table, offsets = reference.instance_table(lab, roots, True)
    return roots, ids, table, offsets


def closed_form_table(mask: np.ndarray, sample: int, cls: int) -> np.ndarray:
    """The table row of ONE component that is exactly ``mask`` [D, H, W], straight from its voxels."""
    z, y, x = np.nonzero(mask)
    root = int(np.flatnonzero(mask.reshape(-1))[0]) + 1
    return np.array([sample, cls, z.size, root, z.min(), y.min(), x.min(), z.max(), y.max(), x.max(),
                     z.sum(), y.sum(), x.sum()], np.int64)
