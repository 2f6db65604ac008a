"""Id volumes, selections and oracles for the instance-isolation tests (CPU and GPU).

``loop_part`` is the definition read literally, voxel by voxel in ``fractions.Fraction``; ``cases`` gives the
(ids, sel) pairs that both suites run; ``generator_parts`` is the part generator as an exact oracle: isolating
slot ``k`` of a ``separate=True`` part must give the part carved from slot ``k`` alone."""
import functools
import math
from fractions import Fraction

import numpy as np
import torch

from _ccl_cases import PATTERNS, expected
from featurenet_amd.ops import partgen, reference

# (source grid, S, why): the smallest shapes at which an output row stops fitting the kernel's lane mapping
SHAPES = [((8, 8, 8), 8, "one byte per row"),
          ((64, 64, 64), 64, "identity, a row exactly one wave of voxels"),
          ((3, 5, 130), 72, "a row one byte over a wave, non-cubic, two 64-wide source pieces plus a rest"),
          ((16, 16, 16), 8, "down"),
          ((8, 8, 8), 16, "up"),
          ((5, 12, 9), 8, "centred short axes, out-of-stock voxels")]
LOOP_CASES = [((8, 8, 8), 8), ((16, 16, 16), 8), ((8, 8, 8), 16), ((5, 12, 9), 8)]


def loop_part(ids: torch.Tensor, row, S: int) -> np.ndarray:
    """One part uint8 [S, S, S] of one ``sel`` row, by the definition: the centre of output voxel ``o`` lies at
    ``(o + 1/2) Lmax / S - (Lmax - L) / 2`` in window coordinates, and the voxel looks at the source voxel
    that holds it (a centre on a boundary: the higher one)."""
    n, ident, bz0, by0, bx0, bz1, by1, bx1, wz0, wy0, wx0, Lz, Ly, Lx = (int(v) for v in row)
    Lmax = max(Lz, Ly, Lx)
    src = [[math.floor(Fraction(2 * o + 1, 2) * Fraction(Lmax, S) - Fraction(Lmax - L, 2)) for o in range(S)]
           for L in (Lz, Ly, Lx)]
    vol = ids[n].numpy()
    out = np.zeros((S, S, S), np.uint8)
    for Z, sz in enumerate(src[0]):
        for Y, sy in enumerate(src[1]):
            for X, sx in enumerate(src[2]):
                if not (0 <= sz < Lz and 0 <= sy < Ly and 0 <= sx < Lx):
                    continue                                 # outside the stock: free space
                z, y, x = wz0 + sz, wy0 + sy, wx0 + sx
                feature = bz0 <= z <= bz1 and by0 <= y <= by1 and bx0 <= x <= bx1 and vol[z, y, x] == ident
                out[Z, Y, X] = 0 if feature else 1
    return out


def grid_window(shape) -> list:
    return [0, 0, 0, *shape]


def table_sel(table: torch.Tensor, offsets: torch.Tensor, window, boxes: str = "true") -> torch.Tensor:
    """``sel`` int32 [T, 14] of every table row with one window ``(z0, y0, x0, Lz, Ly, Lx)``.  ``boxes``:
    ``true`` the table's, ``wide`` the whole window's grid (0 .. 255), ``half`` the table's cut in half along
    x (the low half is kept)."""
    rows = []
    off = offsets.tolist()
    for k, r in enumerate(table.tolist()):
        n = r[0]
        box = r[4:10]
        if boxes == "wide":
            box = [0, 0, 0, 255, 255, 255]
        elif boxes == "half":
            box = box[:5] + [(box[2] + box[5]) // 2]
        rows.append([n, k - off[n] + 1, *box, *window])
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 14)


@functools.lru_cache(maxsize=None)
def pattern_ids(pattern: str, N: int, D: int, H: int, W: int):
    """(ids, table, offsets) of a ``_ccl_cases`` pattern (6-connected, background 0), read-only."""
    _, ids, table, offsets = expected(pattern, N, D, H, W, 6, 0)
    return ids, table, offsets


@functools.lru_cache(maxsize=None)
def random_ids(N: int, D: int, H: int, W: int, top: int = 5, seed: int = 0) -> torch.Tensor:
    """ids drawn at random from 0..top: instances that are no components, everywhere in the grid."""
    g = torch.Generator().manual_seed(seed + D * 131 + H * 17 + W)
    return torch.randint(0, top + 1, (N, D, H, W), generator=g, dtype=torch.int32)


def random_sel(N: int, shape, top: int, window, empty: int | None = None) -> torch.Tensor:
    """Every id 1..top + 1 (the last one carried by no voxel) of every sample but ``empty``, whole-grid boxes,
    then two rows again (duplicates)."""
    rows = [[n, i, 0, 0, 0, shape[0] - 1, shape[1] - 1, shape[2] - 1, *window]
            for n in range(N) if n != empty for i in range(1, top + 2)]
    return torch.tensor(rows + rows[:2], dtype=torch.int32).reshape(-1, 14)


def inner_window(shape) -> list:
    """A window strictly inside the grid (a voxel off every low face, two off every high one where there is room)."""
    w0 = [1 if s > 2 else 0 for s in shape]
    L = [max(1, s - 3) if s > 2 else s for s in shape]
    return w0 + L


@functools.lru_cache(maxsize=None)
def generator_parts(S: int, n: int = 6, seed: int = 3, features=(1, 4)):
    """``(slots int32 [n, S, S, S], sel int32 [M, 14], want uint8 [M, S, S, S])``: the ``slots`` volume of
    ``separate=True`` parts as ids (slot k is id k + 1), one row per used slot with the whole grid as box and
    window, and the occupancy carved from a table in which every other slot is unused."""
    tab = partgen.sample(n, S, seed, features, separate=True)
    _, _, slots = reference.carve_parts(tab, S)
    rows, alone = [], []
    for p in range(n):
        for k in range(tab.shape[1]):
            if int(tab[p, k, 0]) < 0:
                continue
            one = tab[p:p + 1].clone()
            one[0, :, 0] = -1
            one[0, k, 0] = tab[p, k, 0]
            alone.append(one)
            rows.append([p, k + 1, 0, 0, 0, S - 1, S - 1, S - 1, 0, 0, 0, S, S, S])
    want, _, _ = reference.carve_parts(torch.cat(alone), S)
    return slots.to(torch.int32), torch.tensor(rows, dtype=torch.int32), want


__all__ = ["PATTERNS", "SHAPES", "LOOP_CASES", "loop_part", "grid_window", "table_sel", "pattern_ids", "random_ids",
           "random_sel", "inner_window", "generator_parts"]
