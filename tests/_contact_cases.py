"""Inputs of the feature-contact tests (CPU and GPU), a plain-Python oracle, and cached oracle results."""
import functools

import numpy as np
import torch

from _access_cases import occupancy
from _ccl_cases import expected
from featurenet_amd.ops import reference

STEPS = ((1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0))    # (dz, dy, dx) of +z -z +x -x +y -y


def loop_contact_table(ids: np.ndarray, offsets: np.ndarray, occ: np.ndarray, T: int):
    """``(contact [T, 19], adj [P, 4])`` voxel by voxel and face by face, straight from the definitions."""
    N, D, H, W = ids.shape
    contact = np.zeros((T, 19), np.int64)
    pairs = {}
    for n in range(N):
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    me = int(ids[n, z, y, x])
                    row = int(offsets[n]) + me
                    if me <= 0 or not 1 <= row <= T:
                        continue
                    contact[row - 1, 18] += 1
                    for k, (dz, dy, dx) in enumerate(STEPS):
                        uz, uy, ux = z + dz, y + dy, x + dx
                        if not (0 <= uz < D and 0 <= uy < H and 0 <= ux < W):
                            contact[row - 1, 6 + k] += 1
                            continue
                        other = int(ids[n, uz, uy, ux])
                        if other == me:
                            continue
                        if other <= 0:
                            contact[row - 1, (0 if occ[n, uz, uy, ux] != 0 else 6) + k] += 1
                            continue
                        contact[row - 1, 12 + k] += 1
                        mate = int(offsets[n]) + other
                        if row < mate <= T:
                            pairs[(row - 1, mate - 1, k)] = pairs.get((row - 1, mate - 1, k), 0) + 1
    adj = np.array([(*key, pairs[key]) for key in sorted(pairs)], np.int64).reshape(-1, 4)
    return contact, adj


def hand_scene():
    """(labels uint8 [1, 8, 8, 8], occ uint8): a pocket (label 1) on z 5..7, y 2..5, x 1..6 with a 2 x 2 hole
    (label 2) on z 0..4, y 3..4, x 3..4 through its floor and the bottom; material exactly where no label is."""
    lab = np.zeros((1, 8, 8, 8), np.uint8)
    lab[0, 5:8, 2:6, 1:7] = 1
    lab[0, 0:5, 3:5, 3:5] = 2
    return torch.from_numpy(lab), torch.from_numpy((lab == 0).astype(np.uint8))


HAND_CONTACT = [[0, 0, 10, 10, 10, 10, 0, 4, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 20],
                [0, 20, 12, 12, 18, 18, 24, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 72]]
HAND_ADJ = [[0, 1, 0, 4]]


def material(kind: str, ids: torch.Tensor) -> torch.Tensor:
    """``complement``: material exactly where no instance is; ``random``: drawn independently of the labels (so
    that faces open through unlabelled free voxels occur, and instance voxels that are material)."""
    if kind == "complement":
        return (ids == 0).to(torch.uint8)
    return occupancy(*ids.shape)


@functools.lru_cache(maxsize=None)
def expected_contacts(pattern: str, N: int, D: int, H: int, W: int, kind: str = "complement"):
    """(ids, table, offsets, occ, contact, adj) of the CPU oracle for the ``pattern`` label volume of
    ``_ccl_cases`` (6-connectivity, background 0); computed once, never modified."""
    _, ids, table, offsets = expected(pattern, N, D, H, W, 6, 0)
    occ = material(kind, ids)
    contact, adj = reference.contact_table(ids, offsets, occ)
    return ids, table, offsets, occ, contact, adj


def check_identities(contact: torch.Tensor, adj: torch.Tensor, table: torch.Tensor, what) -> None:
    """The identities between the two tables and the instance table (any device)."""
    T = len(table)
    assert contact.shape == (T, 19) and adj.shape[1] == 4, what
    assert torch.equal(contact[:, 18], table[:, 2]), what
    a, b, k, f = adj.unbind(1)
    assert bool((a < b).all()) and bool((f > 0).all()), what
    key = (a * T + b) * 6 + k
    assert bool((key[1:] > key[:-1]).all()), what                  # sorted by (a, b, k), each triple once
    seen = torch.zeros(T * 6, dtype=torch.int64, device=contact.device)
    seen.index_add_(0, a * 6 + k, f)                                # a sees b toward k ...
    seen.index_add_(0, b * 6 + (k ^ 1), f)                          # ... and b sees a toward the opposite side
    assert torch.equal(contact[:, 12:18], seen.view(T, 6)), what
    total = contact[:, 12:18].sum(0)
    assert total[0] == total[1] and total[2] == total[3] and total[4] == total[5], what
