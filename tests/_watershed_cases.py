"""Inputs and expectations shared by the watershed tests (``test_watershed_cpu.py``, ``test_watershed_gpu.py``)."""
import functools

import torch

from featurenet_amd.ops import reference

KINDS = ("noise", "edt", "flat", "touching")
SHAPES = [(1, 1, 1), (3, 5, 7), (8, 8, 64), (9, 9, 65), (16, 17, 130), (5, 6, 256)]
OFFSETS26 = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


def carved(N: int, D: int, H: int, W: int, seed: int) -> torch.Tensor:
    """Occupancy uint8 ``[N, D, H, W]``: a solid block with boxes and balls removed, the more the larger it is, so
    that some of them touch or overlap."""
    g = torch.Generator().manual_seed(seed)
    occ = torch.ones(N, D, H, W, dtype=torch.uint8)
    z, y, x = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    for n in range(N):
        for k in range(6 + D * H * W // 600):
            c = [int(torch.randint(0, s, (1,), generator=g)) for s in (D, H, W)]
            r = int(torch.randint(1, max(2, min(max(D, H, W) // 3, 9)), (1,), generator=g))
            if k % 2:
                hole = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
            else:
                hole = ((z - c[0]).abs() <= r) & ((y - c[1]).abs() <= r // 2) & ((x - c[2]).abs() <= 2 * r)
            occ[n][hole] = 0
    return occ


def components(removed: torch.Tensor, connectivity: int = 6) -> torch.Tensor:
    """The component ids int32 of a uint8 volume's non-zero voxels (the CPU oracle of ``ops.ccl``)."""
    return reference.instance_table(removed, reference.connected_components(removed, 0, connectivity))[0]


@functools.lru_cache(maxsize=None)
def case(kind: str, N: int, D: int, H: int, W: int, seed: int = 0):
    """``(ids, height)`` int32 ``[N, D, H, W]`` on the CPU (shared: do not write into them).

    noise: random ids in 0..3 and heights in 0..4, so ties are everywhere; edt: the components of a carved block
    over the squared distance to its material; flat: those components over a constant; touching: two
    components that are 26-adjacent (stripes of ids 1 and 2 with a diagonal boundary) over random heights.
    With two samples the last plane of sample 0 and the first of sample 1 carry id 1, and all of sample 1 lies
    higher than sample 0: an ascent that crossed the sample boundary would climb into it."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * D + 3 * H + W + N)
    if kind == "noise":
        ids = torch.randint(0, 4, (N, D, H, W), generator=g, dtype=torch.int32)
        height = torch.randint(0, 5, (N, D, H, W), generator=g, dtype=torch.int32)
    elif kind in ("edt", "flat"):
        occ = carved(N, D, H, W, seed + 11)
        ids = components((occ == 0).to(torch.uint8))
        height = reference.distance_sq(occ) if kind == "edt" else torch.full((N, D, H, W), 7, dtype=torch.int32)
        if kind == "edt" and int(height.max()) >= reference.EDT_INF:     # (a sample without material: keep it small)
            height = height.clamp(max=50)
    elif kind == "touching":
        z, y, x = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
        ids = (1 + ((x + y + z) // 3) % 2).to(torch.int32).expand(N, D, H, W).clone()
        height = torch.randint(-2, 9, (N, D, H, W), generator=g, dtype=torch.int32)
    else:
        raise ValueError(kind)
    if N == 2:
        ids[0, -1], ids[1, 0] = 1, 1
        height[1] += int(height[0].max()) + 1
    return ids, height


@functools.lru_cache(maxsize=None)
def expected(kind: str, N: int, D: int, H: int, W: int, seed: int = 0):
    """``(parent, roots, flags, basin_ids, table, offsets, pairs)`` of :func:`case` by the oracle, on the CPU."""
    ids, height = case(kind, N, D, H, W, seed)
    parent, roots = reference.watershed_parents(ids, height), reference.watershed_ascend(ids, height)
    V = D * H * W
    flags = (roots.view(N, V) == torch.arange(1, V + 1, dtype=torch.int32)).to(torch.int32).view(N, D, H, W)
    bids, table, offsets = reference.instance_table((ids > 0).to(torch.uint8), roots)
    return parent, roots, flags, bids, table, offsets, reference.watershed_saddles(ids, bids, offsets, height)


def loop_ascend(ids: torch.Tensor, height: torch.Tensor) -> tuple:
    """``(parent, roots)`` by a per-voxel loop written from the definition (small volumes only)."""
    N, D, H, W = ids.shape
    I, Hh = ids.tolist(), height.tolist()
    roots, parents = torch.zeros_like(ids), torch.zeros_like(ids)
    for n in range(N):
        def key(z, y, x):
            return (max(Hh[n][z][y][x], 0) << 32) | (0xFFFFFFFF - ((z * H + y) * W + x))

        def parent(z, y, x):
            best, at = key(z, y, x), (z, y, x)
            for dz, dy, dx in OFFSETS26:
                u = (z + dz, y + dy, x + dx)
                if 0 <= u[0] < D and 0 <= u[1] < H and 0 <= u[2] < W and I[n][u[0]][u[1]][u[2]] == I[n][z][y][x]:
                    if key(*u) > best:
                        best, at = key(*u), u
            return at
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    if I[n][z][y][x] <= 0:
                        continue
                    v, steps = (z, y, x), 0
                    u = parent(z, y, x)
                    parents[n, z, y, x] = (u[0] * H + u[1]) * W + u[2] + 1
                    while parent(*v) != v:
                        v, steps = parent(*v), steps + 1
                        assert steps < D * H * W
                    roots[n, z, y, x] = (v[0] * H + v[1]) * W + v[2] + 1
    return parents, roots


def loop_saddles(ids: torch.Tensor, bids: torch.Tensor, offsets: torch.Tensor, height: torch.Tensor) -> torch.Tensor:
    """``pairs`` by a loop over every voxel and its 26 neighbours, written from the definition."""
    N, D, H, W = ids.shape
    T = int(offsets[-1])
    I, B, Hh, off = ids.tolist(), bids.tolist(), height.tolist(), offsets.tolist()
    best = {}
    for n in range(N):
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    for dz, dy, dx in OFFSETS26:
                        uz, uy, ux = z + dz, y + dy, x + dx
                        if not (0 <= uz < D and 0 <= uy < H and 0 <= ux < W):
                            continue
                        if I[n][z][y][x] <= 0 or I[n][uz][uy][ux] != I[n][z][y][x]:
                            continue
                        if B[n][z][y][x] <= 0 or B[n][uz][uy][ux] <= 0:
                            continue
                        a, b = off[n] + B[n][z][y][x] - 1, off[n] + B[n][uz][uy][ux] - 1
                        if not (0 <= a < T and 0 <= b < T) or a >= b:
                            continue
                        s = min(max(Hh[n][z][y][x], 0), max(Hh[n][uz][uy][ux], 0))
                        best[(a, b)] = max(best.get((a, b), -1), s)
    rows = [(a, b, s) for (a, b), s in sorted(best.items())]
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


def dumbbell() -> tuple:
    """``(ids, occ)`` ``[1, 24, 24, 24]``: balls of radius 6 and 4 joined by a neck of radius 2, one component."""
    z, y, x = torch.meshgrid(torch.arange(24), torch.arange(24), torch.arange(24), indexing="ij")
    a = (z - 11) ** 2 + (y - 11) ** 2 + (x - 7) ** 2 <= 36
    b = (z - 11) ** 2 + (y - 11) ** 2 + (x - 18) ** 2 <= 16
    neck = ((z - 11) ** 2 + (y - 11) ** 2 <= 4) & (x >= 7) & (x <= 18)
    removed = (a | b | neck)[None]
    return components(removed.to(torch.uint8)), (~removed).to(torch.uint8)


def same_partition(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Two id volumes cut each sample into the same sets of voxels, whatever the numbers."""
    if not torch.equal(a > 0, b > 0):
        return False
    N = a.shape[0]
    top = int(max(a.max(), b.max())) + 1
    for n in range(N):
        fa, fb = a[n].reshape(-1).to(torch.int64), b[n].reshape(-1).to(torch.int64)
        pairs = torch.unique(fa * top + fb)
        if len(pairs) != len(torch.unique(fa)) or len(pairs) != len(torch.unique(fb)):
            return False
    return True
