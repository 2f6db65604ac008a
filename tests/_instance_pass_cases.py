"""One volume through all four instance-table ops (``ccl``, ``overlap``, ``access``, ``edt``) on a device, the
results tied to each other and to the CPU oracle (used by the CPU and the GPU test of the instance pass)."""
import functools

import torch

from _access_cases import occupancy
from _ccl_cases import expected, volume
from featurenet_amd.ops import access, ccl, edt, overlap, reference

PATTERNS = ("blobs", "noise4", "solid")
SHAPES = [(3, 5, 7), (9, 7, 130)]        # rows under one wave, one partial chunk; V = 8190: two chunks, the first
#                                          ends mid-row, rows of two 64-lane pieces plus a remainder


@functools.lru_cache(maxsize=None)
def oracle(pattern: str, N: int, D: int, H: int, W: int):
    """(table, acc, dim, pairs) of the CPU oracle; computed once, never modified."""
    _, ids, table, offsets = expected(pattern, N, D, H, W, 6, 0)
    occ = occupancy(N, D, H, W)
    acc, _ = reference.access_table(ids, offsets, occ)
    dim = reference.dimension_table(ids, offsets, reference.distance_sq(occ))
    return table, acc, dim, reference.overlap_table(ids, offsets, ids, offsets)


def check_identities(pattern: str, N: int, shape, device: str) -> None:
    D, H, W = shape
    what = (pattern, N, shape)
    lab, occ = volume(pattern, N, D, H, W).to(device), occupancy(N, D, H, W).to(device)
    ids, table, offsets = ccl.instance_table(lab, ccl.connected_components(lab, 0, 6))
    acc, _ = access.access_table(ids, offsets, occ)
    dim, _ = edt.dimension_table(ids, offsets, occ)
    pairs = overlap.overlap_table(ids, offsets, ids, offsets)
    T = len(table)
    assert T >= N and int(table[:, 2].sum()) == int((lab != 0).sum()), what
    # the voxel counts of three kernels are one vector
    assert torch.equal(acc[:, 7], table[:, 2]) and torch.equal(dim[:, 3], table[:, 2]), what
    # a volume against itself: every instance meets itself in all its voxels and nothing else
    r = torch.arange(T, dtype=torch.int64, device=device)
    assert torch.equal(pairs, torch.stack([r, r, table[:, 2]], 1)), what
    for name, got, want in zip(("table", "acc", "dim", "pairs"), (table, acc, dim, pairs), oracle(pattern, N, D, H, W)):
        assert got.dtype == want.dtype and got.device.type == torch.device(device).type, (what, name)
        assert torch.equal(got.cpu(), want), (what, name)
