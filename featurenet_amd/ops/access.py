"""Access directions of feature instances: from which faces of the grid each instance is open.

``column_extents`` turns an occupancy volume ``uint8 [N, D, H, W]`` (material: ``occ != 0``) into
the first and last material index of every column along x, y and z; ``access_table`` counts, for
every row of an instance table, the voxels of that instance that are open toward each of the six
faces ``+z, -z, +x, -x, +y, -y`` (``utils.partfeatures.FACES``; ``+z`` is the high-index end of z),
toward none, and in all (see :mod:`featurenet_amd.ops.reference` for the exact definitions).
Device tensors run the ``access.hip`` kernels -- ``access_extents`` (one launch, each table element
written by one workgroup), ``access_stats`` (one lane per voxel, runs along x combined by ballot,
then in an LDS table, then added to the table) -- CPU tensors and empty batches the reference
twins.  Everything is an exact integer that does not depend on execution order.
"""
from __future__ import annotations

import torch

from .. import _native
from . import reference
from ._volumes import check_batch, check_ids_offsets, check_volume

NCOL = 8           # +z -z +x -x +y -y none voxels


def column_extents(occ: torch.Tensor):
    """``(ex, ey, ez)`` int32 ``[N, D, H, 2]``, ``[N, D, W, 2]``, ``[N, H, W, 2]`` of ``occ`` uint8
    ``[N, D, H, W]`` (``reference.column_extents``), on its device."""
    check_volume(occ, "column_extents", "occ")
    if not _native.use_native(occ) or occ.numel() == 0:
        return reference.column_extents(occ)
    check_batch(occ, "column_extents")
    occ = occ.contiguous()
    N, D, H, W = occ.shape
    ex = torch.empty(N, D, H, 2, dtype=torch.int32, device=occ.device)
    ey = torch.empty(N, D, W, 2, dtype=torch.int32, device=occ.device)
    ez = torch.empty(N, H, W, 2, dtype=torch.int32, device=occ.device)
    _native.kernels().access_extents(occ.data_ptr(), ex.data_ptr(), ey.data_ptr(), ez.data_ptr(), N, D, H, W,
                                     _native.stream(occ), [occ.numel(), ex.numel(), ey.numel(), ez.numel()])
    return ex, ey, ez


def access_table(ids: torch.Tensor, offsets: torch.Tensor, occ: torch.Tensor, want_mask: bool = False,
                 rows: int | None = None):
    """``(acc, mask or None)`` of an id volume, its instance table's ``offsets`` and the occupancy
    (``reference.access_table``): acc int64 ``[T, 8]``, mask uint8 ``[N, D, H, W]``, on the ids'
    device.  ``rows``: the table's row count ``T = offsets[-1]`` when the caller knows it (it
    saves the device-to-host read that sizes ``acc``)."""
    check_volume(occ, "access_table", "occ")
    check_ids_offsets(ids, offsets, occ, "access_table")
    if not _native.use_native(ids) or ids.numel() == 0:
        return reference.access_table(ids, offsets, occ, want_mask)
    check_batch(ids, "access_table")
    ids, offsets = ids.contiguous(), offsets.contiguous()
    N, D, H, W = ids.shape
    ex, ey, ez = column_extents(occ)
    T = int(offsets[-1]) if rows is None else int(rows)
    acc = torch.empty(T, NCOL, dtype=torch.int64, device=ids.device)
    mask = torch.empty(ids.shape, dtype=torch.uint8, device=ids.device) if want_mask else None
    _native.kernels().access_stats(ids.data_ptr(), offsets.data_ptr(), ex.data_ptr(), ey.data_ptr(), ez.data_ptr(),
                                   _native.ptr(mask), acc.data_ptr(), N, D, H, W, T, _native.stream(ids),
                                   [ids.numel(), offsets.numel(), ex.numel(), ey.numel(), ez.numel(),
                                    mask.numel() if want_mask else 0, acc.numel()])
    return acc, mask
