"""Dimensions of feature instances: how far each voxel lies from the nearest material.

``distance_sq`` is the exact squared Euclidean distance transform of a seed volume ``uint8 [N, D,
H, W]`` (a seed: ``seeds != 0``; with ``border`` the positions just outside the grid too);
``dimension_table`` gives, for every row of an instance table, the largest squared distance to the
material over the instance's voxels (the radius of the largest ball that fits), the voxel where it
is attained, the voxels that touch material, and the voxels (see
:mod:`featurenet_amd.ops.reference` for the exact definitions).  Device tensors run the ``edt.hip``
kernels -- ``edt_xy`` and ``edt_z`` (two launches, each element written by one workgroup, no
atomics), ``edt_stats`` (one lane per voxel, an LDS table, then 64-bit max / add) -- CPU tensors and
empty batches the reference twins.  Everything is an exact integer that does not depend on
execution order.
"""
from __future__ import annotations

import torch

from .. import _native
from . import reference
from ._volumes import check_batch, check_ids_offsets, check_volume
from .reference import EDT_INF, EDT_MAX_S  # noqa: F401

NCOL = 4           # r2 at wall voxels


def _check_seeds(seeds, what: str, name: str = "seeds") -> None:
    check_volume(seeds, what, name)
    if max(seeds.shape[1:]) > EDT_MAX_S:
        raise ValueError(f"{what}: each of D, H, W is at most {EDT_MAX_S}, not {tuple(seeds.shape[1:])}")


def distance_sq(seeds: torch.Tensor, border: bool = False) -> torch.Tensor:
    """int32 ``[N, D, H, W]`` squared distance of every voxel to the nearest seed of ``seeds`` uint8
    ``[N, D, H, W]`` (``reference.distance_sq``), on its device."""
    _check_seeds(seeds, "distance_sq")
    if not _native.use_native(seeds) or seeds.numel() == 0:
        return reference.distance_sq(seeds, border)
    check_batch(seeds, "distance_sq")
    seeds = seeds.contiguous()
    N, D, H, W = seeds.shape
    d2 = torch.empty(seeds.shape, dtype=torch.int32, device=seeds.device)
    # the z pass stages what it reads before it writes: one buffer serves as t and as d2
    _native.kernels().edt_transform(seeds.data_ptr(), d2.data_ptr(), d2.data_ptr(), N, D, H, W, bool(border), 3,
                                    _native.stream(seeds), [seeds.numel(), d2.numel(), d2.numel()])
    return d2


def dimension_table(ids: torch.Tensor, offsets: torch.Tensor, occ: torch.Tensor, rows: int | None = None,
                    want_d2: bool = False, d2: torch.Tensor | None = None):
    """``(dim, d2 or None)`` of an id volume, its instance table's ``offsets`` and the occupancy:
    dim int64 ``[T, 4]`` = ``r2, at, wall, voxels`` (``reference.dimension_table`` over
    ``distance_sq(occ)``: the material is the seed, the grid's border is not), d2 int32 ``[N, D, H,
    W]``, on the ids' device.  ``rows``: the table's row count ``T = offsets[-1]`` when the caller
    knows it (it saves the device-to-host read that sizes the table).  ``d2``: ``distance_sq(occ)`` when the
    caller already has it."""
    _check_seeds(occ, "dimension_table", "occ")
    check_ids_offsets(ids, offsets, occ, "dimension_table")
    if d2 is not None and (d2.shape != occ.shape or d2.dtype != torch.int32 or d2.device != occ.device):
        raise ValueError(f"dimension_table: d2 must be int32 {tuple(occ.shape)} on {occ.device}")
    if not _native.use_native(ids) or ids.numel() == 0:
        d2 = reference.distance_sq(occ) if d2 is None else d2
        return reference.dimension_table(ids, offsets, d2), (d2 if want_d2 else None)
    check_batch(ids, "dimension_table")
    ids, offsets = ids.contiguous(), offsets.contiguous()
    N, D, H, W = ids.shape
    d2 = distance_sq(occ) if d2 is None else d2.contiguous()
    T = int(offsets[-1]) if rows is None else int(rows)
    raw = torch.empty(T, 3, dtype=torch.int64, device=ids.device)
    _native.kernels().edt_stats(ids.data_ptr(), offsets.data_ptr(), d2.data_ptr(), raw.data_ptr(), N, D, H, W, T,
                                _native.stream(ids), [ids.numel(), offsets.numel(), d2.numel(), raw.numel()])
    key, wall, vox = raw.unbind(1)
    has = vox > 0
    dim = torch.stack([torch.where(has, key >> 32, -1), torch.where(has, 0xFFFFFFFF - (key & 0xFFFFFFFF), -1),
                       wall, vox], 1)
    return dim, (d2 if want_d2 else None)
