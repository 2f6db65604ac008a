"""Connected components of a label volume and the per-component instance table.

``connected_components`` turns ``uint8 [N, D, H, W]`` labels into ``roots`` (1 + the smallest
linear index of each voxel's component, 0 = background); ``instance_table`` turns labels + roots
into dense ids, one table row per component and the row range of each sample (see
:mod:`featurenet_amd.ops.reference` for the exact definitions).  Device tensors run the
``ccl.hip`` kernels -- ``ccl_local`` (one tile per workgroup, in LDS), ``ccl_merge`` (across tile
faces), ``ccl_flatten`` (roots + root flags), one ``torch.cumsum`` over the flags, ``ccl_stats``
(ids + table) -- CPU tensors the reference twins.  Everything is an exact integer that does not
depend on execution order.

Why ``ccl_local`` may skip links.  A tile row starts as runs of equal class along x (every voxel
under its run's first voxel).  Against an earlier row ``r'`` a voxel at ``x`` touches
``r'[x-1], r'[x], r'[x+1]`` (26-connectivity; ``r'[x]`` alone for 6); those of its class are
``cm, c0, cp``; ``L`` says its left neighbour is in its run.  It unions with ``r'[x]`` when ``c0
and not L``, with ``r'[x-1]`` when ``cm and not c0 and not L``, with ``r'[x+1]`` when ``cp and not
c0``.  Every linked pair still ends in one set, by induction on ``x``: equal-class neighbours
inside ``r'`` are one run already, so ``c0`` covers ``cm`` and ``cp``; and with ``L`` the left
voxel -- same set as ``x`` -- has already met ``r'[x-1]`` or ``r'[x]`` directly or through its own
left neighbour.  For 6-connectivity the same argument drops the union when ``L and cm``.  A solid
tile therefore makes one union per row, not one per voxel.  ``ccl_merge`` walks each tile face in
rows the same way (along y on an x face) and applies the rule where it rests on links inside one
tile and on earlier unions of the same row only: ``L`` also needs the previous voxel in this
voxel's tile, and ``c0`` covers ``cm`` / ``cp`` only where they lie in the facing voxel's tile.
"""
from __future__ import annotations

import torch

from .. import _native
from . import reference
from ._volumes import check_batch, check_volume

NCOL = 13          # sample class voxels root z0 y0 x0 z1 y1 x1 sum_z sum_y sum_x


def _check(labels: torch.Tensor, connectivity: int, what: str) -> None:
    if connectivity not in (6, 26):
        raise ValueError(f"{what}: connectivity must be 6 (faces) or 26 (faces, edges and corners), "
                         f"not {connectivity!r}")
    check_volume(labels, what, "labels")
    if labels.shape[1] * labels.shape[2] * labels.shape[3] >= 1 << 31:
        raise ValueError(f"{what}: a sample must have fewer than 2^31 voxels")


def _root_flags(roots: torch.Tensor) -> torch.Tensor:
    N = roots.shape[0]
    r = roots.reshape(N, -1)
    return (r == torch.arange(1, r.shape[1] + 1, dtype=torch.int32, device=roots.device)).to(torch.int32)


def connected_components(labels: torch.Tensor, background: int | None = 0, connectivity: int = 6,
                         return_flags: bool = False):
    """``roots`` int32 ``[N, D, H, W]`` of ``labels`` uint8 ``[N, D, H, W]``
    (``reference.connected_components``); with ``return_flags`` also the int32 root flags
    ``roots[v] == v + 1`` that ``ccl_flatten`` writes anyway (:func:`instance_table` takes them)."""
    _check(labels, connectivity, "connected_components")
    if background is not None and not 0 <= int(background) <= 255:
        background = None                        # (no uint8 voxel carries it)
    if not _native.use_native(labels) or labels.numel() == 0:
        roots = reference.connected_components(labels, background, connectivity)
        return (roots, _root_flags(roots)) if return_flags else roots
    labels = labels.contiguous()
    N, D, H, W = labels.shape
    roots = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    K_, st = _native.kernels(), _native.stream(labels)
    bg = -1 if background is None else int(background)
    ext = [labels.numel(), roots.numel()]
    K_.ccl_local(labels.data_ptr(), roots.data_ptr(), N, D, H, W, bg, connectivity, st, ext)
    K_.ccl_merge(labels.data_ptr(), roots.data_ptr(), N, D, H, W, bg, connectivity, st, ext)
    flags = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    K_.ccl_flatten(roots.data_ptr(), flags.data_ptr(), N, D, H, W, st, [roots.numel(), flags.numel()])
    return (roots, flags) if return_flags else roots


def instance_table(labels: torch.Tensor, roots: torch.Tensor, want_ids: bool = True,
                   flags: torch.Tensor | None = None):
    """``(ids or None, table, offsets)`` of ``labels`` and their ``roots``
    (``reference.instance_table``): ids int32 ``[N, D, H, W]``, table int64 ``[T, 13]``, offsets
    int64 ``[N + 1]``, all on the labels' device.  ``flags``: the root flags of
    ``connected_components(..., return_flags=True)``, compared out of ``roots`` when not given."""
    _check(labels, 6, "instance_table")
    if roots.shape != labels.shape or roots.dtype != torch.int32 or roots.device != labels.device:
        raise ValueError(f"instance_table: roots must be int32 {tuple(labels.shape)} on {labels.device}, not "
                         f"{roots.dtype} {tuple(roots.shape)} on {roots.device}")
    if not _native.use_native(labels):
        return reference.instance_table(labels, roots, want_ids)
    N, D, H, W = labels.shape
    dev = labels.device
    if labels.numel() == 0:
        return (torch.zeros(labels.shape, dtype=torch.int32, device=dev) if want_ids else None,
                torch.zeros(0, NCOL, dtype=torch.int64, device=dev), torch.zeros(N + 1, dtype=torch.int64, device=dev))
    check_batch(labels, "instance_table")        # (the kernel ranks the batch's roots in int32)
    labels = labels.contiguous()
    K_, st = _native.kernels(), _native.stream(labels)
    roots = roots.contiguous()
    if flags is None:
        flags = _root_flags(roots)
    elif flags.numel() != labels.numel() or flags.dtype != torch.int32 or flags.device != dev:
        raise ValueError(f"instance_table: flags must be int32 with {labels.numel()} elements on {dev}")
    rank = torch.cumsum(flags.reshape(-1), 0, dtype=torch.int32)
    offsets = torch.cat([rank.new_zeros(1), rank.view(N, -1)[:, -1]]).to(torch.int64)
    T = int(rank[-1])                            # the one device-to-host read: it sizes the table
    ids = torch.empty(labels.shape, dtype=torch.int32, device=dev) if want_ids else None
    table = torch.empty(T, NCOL, dtype=torch.int64, device=dev)
    K_.ccl_stats(labels.data_ptr(), roots.data_ptr(), rank.data_ptr(), _native.ptr(ids), table.data_ptr(), N, D, H, W,
                 T, st, [labels.numel(), roots.numel(), rank.numel(), ids.numel() if want_ids else 0, table.numel()])
    return ids, table, offsets

