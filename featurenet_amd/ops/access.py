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

NCOL = 8           # +z -z +x -x +y -y none voxels


def _check_occ(occ, what: str) -> None:
    if not isinstance(occ, torch.Tensor) or occ.dtype != torch.uint8 or occ.dim() != 4:
        got = f"{occ.dtype} {tuple(occ.shape)}" if isinstance(occ, torch.Tensor) else type(occ).__name__
        raise ValueError(f"{what}: occ must be a uint8 [N, D, H, W] tensor, not {got}")


def column_extents(occ: torch.Tensor):
    """``(ex, ey, ez)`` int32 ``[N, D, H, 2]``, ``[N, D, W, 2]``, ``[N, H, W, 2]`` of ``occ`` uint8
    ``[N, D, H, W]`` (``reference.column_extents``), on its device."""
    _check_occ(occ, "column_extents")
    if not _native.use_native(occ) or occ.numel() == 0:
        return reference.column_extents(occ)
    if occ.numel() >= 1 << 31:
        raise ValueError("column_extents: a batch must have fewer than 2^31 voxels; split it by samples")
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
    _check_occ(occ, "access_table")
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.shape != occ.shape:
        got = f"{ids.dtype} {tuple(ids.shape)}" if isinstance(ids, torch.Tensor) else type(ids).__name__
        raise ValueError(f"access_table: ids must be int32 {tuple(occ.shape)}, not {got}")
    N = occ.shape[0]
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or tuple(offsets.shape) != (N + 1,):
        got = f"{offsets.dtype} {tuple(offsets.shape)}" if isinstance(offsets, torch.Tensor) else type(offsets).__name__
        raise ValueError(f"access_table: offsets must be int64 [{N + 1}], not {got}")
    if ids.device != occ.device or offsets.device != occ.device:
        raise ValueError(f"access_table: ids ({ids.device}), offsets ({offsets.device}) and occ ({occ.device}) must "
                         "be on one device")
    if not _native.use_native(ids) or ids.numel() == 0:
        return reference.access_table(ids, offsets, occ, want_mask)
    if ids.numel() >= 1 << 31:
        raise ValueError("access_table: a batch must have fewer than 2^31 voxels; split it by samples")
    ids, offsets = ids.contiguous(), offsets.contiguous()
    _, D, H, W = ids.shape
    ex, ey, ez = column_extents(occ)
    T = int(offsets[-1]) if rows is None else int(rows)
    acc = torch.empty(T, NCOL, dtype=torch.int64, device=ids.device)
    mask = torch.empty(ids.shape, dtype=torch.uint8, device=ids.device) if want_mask else None
    _native.kernels().access_stats(ids.data_ptr(), offsets.data_ptr(), ex.data_ptr(), ey.data_ptr(), ez.data_ptr(),
                                   _native.ptr(mask), acc.data_ptr(), N, D, H, W, T, _native.stream(ids),
                                   [ids.numel(), offsets.numel(), ex.numel(), ey.numel(), ez.numel(),
                                    mask.numel() if want_mask else 0, acc.numel()])
    return acc, mask
