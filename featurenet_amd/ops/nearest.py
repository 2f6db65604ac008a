"""Walls between feature instances: how close each instance comes to another one.

``nearest_labels`` is the labelled distance transform of an id volume int32 ``[N, D, H, W]`` (a seed
of label ``ids``: ``ids > 0``): per voxel the keys ``d2 << 32 | label`` of the nearest label and of
the nearest other label; ``wall_table`` gives, for every row of an instance table, the smallest
squared distance from one of the instance's voxels to a voxel of another instance of its sample,
the voxel where it is attained, the row of that other instance, the voxels that have another
instance within ``limit2``, and the voxels (see :mod:`featurenet_amd.ops.reference` for the exact
definitions).  Device tensors run the ``nearest.hip`` kernels -- ``nn_xy`` and ``nn_z`` (two launches,
each element written by one workgroup, no atomics), ``wall_stats`` (one lane per voxel, an LDS table,
then 64-bit min / add) -- CPU tensors and empty batches the reference twins.  Everything is an exact
integer that does not depend on execution order.
"""
from __future__ import annotations

import torch

from .. import _native
from . import reference
from ._volumes import check_batch, check_ids_offsets, check_volume
from .reference import EDT_INF, NN_MAX_S, NN_NONE  # noqa: F401

NCOL = reference.WALL_NCOL     # gap2 at other thin voxels


def _check_ids(ids, what: str) -> None:
    check_volume(ids, what, "ids", torch.int32)
    if max(ids.shape[1:]) > NN_MAX_S:
        raise ValueError(f"{what}: each of D, H, W is at most {NN_MAX_S}, not {tuple(ids.shape[1:])}")


def nearest_labels(ids: torch.Tensor) -> torch.Tensor:
    """int64 ``[N, 2, D, H, W]`` keys ``d2 << 32 | label`` of the nearest and the nearest other label of
    every voxel of ``ids`` int32 ``[N, D, H, W]`` (``reference.nearest_labels``), on its device."""
    _check_ids(ids, "nearest_labels")
    if not _native.use_native(ids) or ids.numel() == 0:
        return reference.nearest_labels(ids)
    check_batch(ids, "nearest_labels")
    ids = ids.contiguous()
    N, D, H, W = ids.shape
    nn = torch.empty((N, 2, D, H, W), dtype=torch.int64, device=ids.device)
    # the z pass stages what it reads before it writes: one buffer serves as t and as nn
    _native.kernels().nn_transform(ids.data_ptr(), nn.data_ptr(), nn.data_ptr(), N, D, H, W, 3, _native.stream(ids),
                                   [ids.numel(), nn.numel(), nn.numel()])
    return nn


def wall_table(ids: torch.Tensor, offsets: torch.Tensor, limit2: int = 0, rows: int | None = None,
               want_nn: bool = False):
    """``(wall, nn or None)`` of an id volume and its instance table's ``offsets``: wall int64 ``[T,
    5]`` = ``gap2, at, other, thin, voxels`` (``reference.wall_table`` over ``nearest_labels(ids)``),
    nn int64 ``[N, 2, D, H, W]``, on the ids' device.  ``limit2``: the squared distance up to which a
    voxel counts as thin, ``0 <= limit2 < EDT_INF``.  ``rows``: the table's row count ``T =
    offsets[-1]`` when the caller knows it (it saves the device-to-host read that sizes the table)."""
    _check_ids(ids, "wall_table")
    check_ids_offsets(ids, offsets, ids, "wall_table")
    if isinstance(limit2, bool) or not isinstance(limit2, int) or not 0 <= limit2 < EDT_INF:
        raise ValueError(f"wall_table: limit2 must be an int in [0, {EDT_INF}), not {limit2!r}")
    if not _native.use_native(ids) or ids.numel() == 0:
        nn = reference.nearest_labels(ids)
        return reference.wall_table(ids, offsets, nn, limit2), (nn if want_nn else None)
    check_batch(ids, "wall_table")
    ids, offsets = ids.contiguous(), offsets.contiguous()
    N, D, H, W = ids.shape
    nn = nearest_labels(ids)
    T = int(offsets[-1]) if rows is None else int(rows)
    raw = torch.empty(T, 3, dtype=torch.int64, device=ids.device)
    _native.kernels().wall_stats(ids.data_ptr(), offsets.data_ptr(), nn.data_ptr(), raw.data_ptr(), N, D, H, W, T,
                                 limit2, _native.stream(ids), [ids.numel(), offsets.numel(), nn.numel(), raw.numel()])
    return reference.wall_decode(raw, offsets, nn), (nn if want_nn else None)
