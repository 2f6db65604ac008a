"""Contacts of feature instances: what each instance borders, face by face.

``contact_table`` counts, for every row of an instance table, the voxel faces toward each of the six
sides ``+z, -z, +x, -x, +y, -y`` (``utils.partfeatures.FACES``; ``+z`` is the high-index end of z)
that meet material (*wall*), free space or the outside of the grid (*open*) and another instance
(*shared*), and lists which instances share faces, on which side and how many (see
:mod:`featurenet_amd.ops.reference` for the exact definitions).  Device tensors run ``contact_stats``
(``contact.hip``): one lane per voxel reads its six neighbours, runs along x are combined by ballot,
then in an LDS table, then added to ``contact``; the instance pairs go through the open-addressing
hash table of ``ops.overlap`` (``pair_table.h``).  Which slot a pair lands in depends on the order of
the atomics; the set of (pair, faces) does not, and only that set, sorted, leaves this module.  CPU
tensors and empty batches run the reference.

The hash table's capacity is a guess from the instance count.  A pair update that finds no slot is
not lost silently: the kernel counts its faces in ``lost`` and the pass runs again with four
times the capacity.  A table with a slot for every face of every voxel, probed to its end, always
holds every pair, so this ends.
"""
from __future__ import annotations

import torch

from .. import _native
from . import reference
from ._volumes import check_batch, check_ids_offsets, check_volume
from .overlap import MIN_CAP, PROBE, _next_pow2

NCOL = reference.CONTACT_NCOL    # wall x 6, open x 6, shared x 6, voxels
MAX_T = reference.CONTACT_MAX_T
MAX_CAP = 1 << 32


def contact_table(ids: torch.Tensor, offsets: torch.Tensor, occ: torch.Tensor, rows: int | None = None):
    """``(contact, adj)`` of an id volume, its instance table's ``offsets`` and the occupancy
    (``reference.contact_table``): contact int64 ``[T, 19]``, adj int64 ``[P, 4]`` with rows
    ``(row_a, row_b, face, faces)`` sorted by ``(row_a, row_b, face)``, on the ids' device.
    ``rows``: the table's row count ``T = offsets[-1]`` when the caller knows it (it saves the
    device-to-host read that sizes ``contact``)."""
    check_volume(occ, "contact_table", "occ")
    check_ids_offsets(ids, offsets, occ, "contact_table")
    if not _native.use_native(ids) or ids.numel() == 0:
        return reference.contact_table(ids, offsets, occ)
    check_batch(ids, "contact_table")
    ids, offsets, occ = ids.contiguous(), offsets.contiguous(), occ.contiguous()
    N, D, H, W = ids.shape
    dev = ids.device
    T = int(offsets[-1]) if rows is None else int(rows)
    if T >= MAX_T:
        raise ValueError(f"contact_table: the instance table must have fewer than 2^30 rows, not {T}")
    K_, st = _native.kernels(), _native.stream(ids)
    # full: a slot for every face of every voxel (<= 2^32) -- probed to its end it holds any pair list
    full = min(MAX_CAP, max(MIN_CAP, _next_pow2(6 * ids.numel())))
    cap = min(full, max(MIN_CAP, _next_pow2(2 * T)))
    while True:
        contact = torch.zeros(T, NCOL, dtype=torch.int64, device=dev)      # (the kernel adds: zeroed every round)
        buf = torch.zeros(2 * cap + 1, dtype=torch.int64, device=dev)      # keys | counts | lost, one fill
        keys, counts, lost = buf[:cap], buf[cap:2 * cap], buf[2 * cap:]
        K_.contact_stats(ids.data_ptr(), occ.data_ptr(), offsets.data_ptr(), contact.data_ptr(), keys.data_ptr(),
                         counts.data_ptr(), lost.data_ptr(), N, D, H, W, T, cap, cap if cap >= full else PROBE, st,
                         [ids.numel(), occ.numel(), offsets.numel(), contact.numel(), cap, cap, 1])
        if int(lost) == 0:                       # (with P below: the values read back before the result)
            break
        if cap >= full:
            raise RuntimeError(f"contact_table: {int(lost)} faces found no slot in a table of {cap} for "
                               f"{ids.numel()} voxels (corrupt ids or offsets?)")
        cap = min(full, 4 * cap)
    slot = torch.nonzero(keys).squeeze(1)
    key, order = torch.sort(keys[slot])          # (keys < 2^63: the int64 order is the uint64 order)
    adj = torch.stack([(key >> 33) - 1, ((key >> 3) & (MAX_T - 1)) - 1, key & 7, counts[slot][order]], 1)
    return contact, adj
