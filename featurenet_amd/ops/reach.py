"""Tool reach of feature instances: which tool comes in from which face, and what it clears.

``reach_scan`` turns an int32 volume ``[N, D, H, W]`` into its six directional running minima
``r6 [N, 6, D, H, W]``: over ``d2 = distance_sq(occ)`` the squared clearance of the largest ball
whose centre travels in a straight line from outside each face ``+z, -z, +x, -x, +y, -y`` of the grid
to the voxel.  ``reach_table`` gives, for every row of an instance table and one tool ``(need2,
cut2)``, the largest ``r6`` per face, the centres the tool reaches from each face and from none,
the voxels the tool clears from those centres, and the voxels (see
:mod:`featurenet_amd.ops.reference` for the exact definitions).  Device tensors run the
``reach.hip`` kernels -- ``reach_scan`` (one launch, each element written by one workgroup, no
atomics), ``reach_stats`` (one lane per voxel, an LDS table, then 64-bit max / add) -- and between
them the existing ``edt`` kernels on the reached centres; CPU tensors and empty batches the
reference twins.  Everything is an exact integer that does not depend on execution order.
"""
from __future__ import annotations

import torch

from .. import _native
from . import edt, reference
from ._volumes import check_batch, check_ids_offsets, check_volume, got
from .reference import EDT_INF, EDT_MAX_S  # noqa: F401

NCOL = reference.REACH_NCOL    # entry2 x 6, reached x 6, unreached, machinable, voxels


def _check_axes(t, what: str) -> None:
    if max(t.shape[1:]) > EDT_MAX_S:
        raise ValueError(f"{what}: each of D, H, W is at most {EDT_MAX_S}, not {tuple(t.shape[1:])}")


def reach_scan(vol: torch.Tensor) -> torch.Tensor:
    """int32 ``[N, 6, D, H, W]`` directional minima of ``vol`` int32 ``[N, D, H, W]``
    (``reference.reach_scan``), on its device."""
    check_volume(vol, "reach_scan", "vol", torch.int32)
    _check_axes(vol, "reach_scan")
    if not _native.use_native(vol) or vol.numel() == 0:
        return reference.reach_scan(vol)
    check_batch(vol, "reach_scan")
    vol = vol.contiguous()
    N, D, H, W = vol.shape
    r6 = torch.empty(N, 6, D, H, W, dtype=torch.int32, device=vol.device)
    _native.kernels().reach_scan(vol.data_ptr(), r6.data_ptr(), N, D, H, W, _native.stream(vol),
                                 [vol.numel(), r6.numel()])
    return r6


def reach_table(ids: torch.Tensor, offsets: torch.Tensor, occ: torch.Tensor, need2: int, cut2: int,
                rows: int | None = None, d2: torch.Tensor | None = None, want_r6: bool = False):
    """``(reach, r6 or None)`` of an id volume, its instance table's ``offsets``, the occupancy and a
    tool: reach int64 ``[T, 15]`` (``reference.reach_table`` over ``r6 = reach_scan(distance_sq(occ))``
    and the squared distance to the centres the tool reaches), r6 int32 ``[N, 6, D, H, W]``, on the
    ids' device.  ``need2 >= 1`` and ``cut2 >= 0`` as ``utils.seginstances.tool_thresholds`` gives
    them.  ``rows``: the table's row count when the caller knows it; ``d2``: ``distance_sq(occ)``
    when the caller has it already (``dimension_table(..., want_d2=True)``)."""
    if isinstance(need2, bool) or isinstance(cut2, bool) or not isinstance(need2, int) or not isinstance(cut2, int):
        raise ValueError(f"reach_table: need2 and cut2 must be ints, not {need2!r}, {cut2!r}")
    if need2 < 1 or cut2 < 0 or need2 >= EDT_INF or cut2 >= EDT_INF:
        raise ValueError(f"reach_table: 1 <= need2 and 0 <= cut2 (both below {EDT_INF}), not {need2}, {cut2}")
    check_volume(occ, "reach_table", "occ")
    _check_axes(occ, "reach_table")
    check_ids_offsets(ids, offsets, occ, "reach_table")
    if d2 is not None and (not isinstance(d2, torch.Tensor) or d2.dtype != torch.int32 or d2.shape != occ.shape
                           or d2.device != occ.device):
        raise ValueError(f"reach_table: d2 must be int32 {tuple(occ.shape)} on {occ.device}, not {got(d2)}")
    native = _native.use_native(ids) and ids.numel() > 0
    if d2 is None:
        d2 = edt.distance_sq(occ) if native else reference.distance_sq(occ)
    if not native:
        r6 = reference.reach_scan(d2)
        dc2 = reference.distance_sq(reference.reach_seeds(r6, need2))
        return reference.reach_table(ids, offsets, r6, dc2, need2, cut2), (r6 if want_r6 else None)
    check_batch(ids, "reach_table")
    ids, offsets = ids.contiguous(), offsets.contiguous()
    N, D, H, W = ids.shape
    r6 = reach_scan(d2)
    dc2 = edt.distance_sq(reference.reach_seeds(r6, need2))
    T = int(offsets[-1]) if rows is None else int(rows)
    reach = torch.empty(T, NCOL, dtype=torch.int64, device=ids.device)
    _native.kernels().reach_stats(ids.data_ptr(), offsets.data_ptr(), r6.data_ptr(), dc2.data_ptr(), reach.data_ptr(),
                                  N, D, H, W, T, need2, cut2, _native.stream(ids),
                                  [ids.numel(), offsets.numel(), r6.numel(), dc2.numel(), reach.numel()])
    return reach, (r6 if want_r6 else None)
