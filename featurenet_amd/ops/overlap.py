"""The overlap table of two instance-id volumes: which predicted instance shares how many voxels
with which true one.

``overlap_table`` takes the ``ids`` volumes and ``offsets`` that ``ops.ccl.instance_table`` gives
for two label volumes of one shape and returns ``pairs`` int64 ``[P, 3]``, rows ``(row_a, row_b,
voxels)`` sorted by ``(row_a, row_b)`` (``reference.overlap_table`` has the exact definition).
Device tensors run ``overlap_pairs`` (``overlap.hip``): runs of one pair along a row are combined
in the wave, then in an LDS table, then counted in an open-addressing hash table in global memory.
Which slot a pair lands in depends on the order of the atomics; the set of (pair, count) does not,
and only that set, sorted, leaves this module.  CPU tensors run the reference.

The hash table's capacity is a guess from the instance counts (a pair list can be longer than both
tables: slabs against crossing slabs).  A pair that finds no slot is not lost silently: the kernel
counts its voxels in ``lost`` and the table is rebuilt four times as large.  A table with a slot
per voxel, probed to its end, always holds every pair, so this ends.
"""
from __future__ import annotations

import torch

from .. import _native
from . import ccl, reference
from ._volumes import check_batch, check_volume

MIN_CAP = 1024
PROBE = 256        # slots an update tries before it counts as lost (the last, full-size table: all)


def _check(ids_a, off_a, ids_b, off_b) -> None:
    check_volume(ids_a, "overlap_table", "ids_a", torch.int32)
    check_volume(ids_b, "overlap_table", "ids_b", torch.int32)
    if ids_b.shape != ids_a.shape or ids_b.device != ids_a.device:
        raise ValueError(f"overlap_table: ids_b must be int32 {tuple(ids_a.shape)} on {ids_a.device}, not "
                         f"{ids_b.dtype} {tuple(ids_b.shape)} on {ids_b.device}")
    N = ids_a.shape[0]
    for name, t in (("off_a", off_a), ("off_b", off_b)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or t.numel() != N + 1 \
                or t.device != ids_a.device:
            got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"overlap_table: {name} must be int64 [{N + 1}] (N + 1 offsets) on {ids_a.device}, "
                             f"not {got}")
    check_batch(ids_a, "overlap_table")


def instance_overlap(labels_a: torch.Tensor, labels_b: torch.Tensor, background: int | None = 0,
                     connectivity: int = 6):
    """The instances of two label volumes (uint8 ``[N, D, H, W]``, one shape, one device) and their
    overlap table -> ``(table_a, off_a, table_b, off_b, pairs)`` on that device: ``ops.ccl`` on
    each, with ids, then :func:`overlap_table`.  The ids stay inside."""
    if labels_b.shape != labels_a.shape or labels_b.device != labels_a.device:
        raise ValueError(f"instance_overlap: the label volumes are {tuple(labels_a.shape)} on {labels_a.device} and "
                         f"{tuple(labels_b.shape)} on {labels_b.device}")
    out = []
    for lab in (labels_a, labels_b):
        lab = lab.contiguous()
        roots, flags = ccl.connected_components(lab, background, connectivity, return_flags=True)
        out.append(ccl.instance_table(lab, roots, want_ids=True, flags=flags))
    (ids_a, table_a, off_a), (ids_b, table_b, off_b) = out
    pairs = overlap_table(ids_a, off_a, ids_b, off_b, rows=(table_a.shape[0], table_b.shape[0]))
    return table_a, off_a, table_b, off_b, pairs


def _next_pow2(n: int) -> int:
    return 1 << max(0, int(n) - 1).bit_length()


def overlap_table(ids_a: torch.Tensor, off_a: torch.Tensor, ids_b: torch.Tensor, off_b: torch.Tensor,
                  rows: tuple[int, int] | None = None) -> torch.Tensor:
    """``pairs`` int64 ``[P, 3]`` of two id volumes and their offsets (``reference.overlap_table``),
    on the inputs' device.  ``rows``: the two instance tables' row counts when the caller has them
    on the host (they size the first hash table; read from the offsets when not given)."""
    _check(ids_a, off_a, ids_b, off_b)
    dev = ids_a.device
    if ids_a.numel() == 0:
        return torch.zeros(0, 3, dtype=torch.int64, device=dev)
    if not _native.use_native(ids_a):
        return reference.overlap_table(ids_a, off_a, ids_b, off_b)
    N, D, H, W = ids_a.shape
    V = D * H * W
    ids_a, ids_b, off_a, off_b = ids_a.contiguous(), ids_b.contiguous(), off_a.contiguous(), off_b.contiguous()
    if rows is None:
        rows = torch.stack([off_a[-1], off_b[-1]]).tolist()
    K_, st = _native.kernels(), _native.stream(ids_a)
    # full: a slot per voxel and as many again (<= 2^32) -- probed to its end it holds any pair list
    full = max(MIN_CAP, _next_pow2(2 * N * V))
    cap = min(full, max(MIN_CAP, _next_pow2(2 * (int(rows[0]) + int(rows[1])))))
    while True:
        buf = torch.zeros(2 * cap + 1, dtype=torch.int64, device=dev)      # keys | counts | lost, one fill
        keys, counts, lost = buf[:cap], buf[cap:2 * cap], buf[2 * cap:]
        K_.overlap_pairs(ids_a.data_ptr(), ids_b.data_ptr(), off_a.data_ptr(), off_b.data_ptr(), keys.data_ptr(),
                         counts.data_ptr(), lost.data_ptr(), N, V, W, cap, cap if cap >= full else PROBE, st,
                         [ids_a.numel(), ids_b.numel(), off_a.numel(), off_b.numel(), cap, cap, 1])
        if int(lost) == 0:                       # (with P below: the values read back before the result)
            break
        if cap >= full:
            raise RuntimeError(f"overlap_table: {int(lost)} voxels found no slot in a table of {cap} for {N * V} "
                               "voxels (corrupt ids or offsets?)")
        cap = min(full, 4 * cap)
    slot = torch.nonzero(keys).squeeze(1)
    key, order = torch.sort(keys[slot])          # (keys < 2^63: the int64 order is the uint64 order)
    return torch.stack([(key >> 32) - 1, (key & 0xffffffff) - 1, counts[slot][order]], 1)
