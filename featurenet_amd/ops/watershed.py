"""Watershed split of touching feature instances.

A component of the removed volume can hold several features: a hole drilled into a pocket floor, a slot that
crosses a step.  On the squared distance to the material each of them is a hill of its own, joined to the next
over a pass.  ``split_instances`` cuts every component of an id volume along those passes:

* ``ascend`` sends every voxel uphill inside its component (26 neighbours, ties to the lower index) and
  gives ``roots`` and the root flags; the voxels of one root are a *basin*.  ``ccl.instance_table`` turns them
  into basin ids and a basin table, as it does for connected components.
* ``saddle_pairs`` lists, for every two basins of one component that touch, the height of the pass between
  them.
* ``merge_groups`` joins, on the host and over that list alone, the basins whose lower peak rises less than
  ``merge`` voxels of clearance above the pass; what is left are the new instances.

See :mod:`featurenet_amd.ops.reference` for the exact definitions.  Device tensors run the ``watershed.hip``
kernels -- ``ws_ascend`` (every parent written by one lane, from 27 cached reads or from a tile and its halo staged
in LDS: :data:`STAGED`), ``ws_resolve``
(each voxel walks its parents), ``ws_saddle`` (one lane per voxel over the 13 forward neighbours, into the
hash table of ``pair_table.h`` with a maximum) -- CPU tensors and empty batches the reference twins.
Everything is an exact integer that does not depend on execution order; nothing per-voxel crosses to the host.

The hash table grows as in ``ops.contact``: an update that finds no slot is counted in ``lost`` and the pass
runs again with four times the capacity, up to a table with a slot for every forward neighbour of every voxel.
"""
from __future__ import annotations

from fractions import Fraction

import torch

from .. import _native
from . import ccl, reference
from ._volumes import check_batch, check_ids_offsets, check_volume
from .overlap import MIN_CAP, PROBE, _next_pow2
from .reference import WS_MAX_S

NCOL = ccl.NCOL
MAX_CAP = 1 << 32
# ws_ascend's kernel: 27 reads from global memory (0) or the LDS tile (1).  The same parents; on generated parts, where
# nine voxels in ten are material and leave at once, the plain form measured faster (100 against 124 us for 32 x 64^3),
# on a volume where every voxel ascends the tile does (128 against 203 us): profiles/feature_split.md
STAGED = 0


def _check(ids, height, what: str) -> None:
    check_volume(ids, what, "ids", torch.int32)
    if not isinstance(height, torch.Tensor) or height.dtype != torch.int32 or height.shape != ids.shape \
            or height.device != ids.device:
        raise ValueError(f"{what}: height must be int32 {tuple(ids.shape)} on {ids.device}")
    if max(ids.shape[1:]) > WS_MAX_S:
        raise ValueError(f"{what}: each of D, H, W is at most {WS_MAX_S}, not {tuple(ids.shape[1:])}")


def ascend(ids: torch.Tensor, height: torch.Tensor, staged: int | None = None):
    """``(roots, flags)`` int32 ``[N, D, H, W]`` of an id volume and a height volume, both int32 ``[N, D, H,
    W]`` (``reference.watershed_ascend``; flags: ``roots[v] == v + 1``), on their device.  ``staged``: which
    ``ws_ascend`` kernel runs (default: :data:`STAGED`; the result is the same)."""
    _check(ids, height, "ascend")
    if not _native.use_native(ids) or ids.numel() == 0:
        roots = reference.watershed_ascend(ids, height)
        return roots, ccl._root_flags(roots).view(roots.shape)
    check_batch(ids, "ascend")
    ids, height = ids.contiguous(), height.contiguous()
    N, D, H, W = ids.shape
    K_, st = _native.kernels(), _native.stream(ids)
    parent = torch.empty(ids.shape, dtype=torch.int32, device=ids.device)
    roots = torch.empty(ids.shape, dtype=torch.int32, device=ids.device)
    flags = torch.empty(ids.shape, dtype=torch.int32, device=ids.device)
    ext = [ids.numel()] * 3
    K_.ws_ascend(ids.data_ptr(), height.data_ptr(), parent.data_ptr(), N, D, H, W, STAGED if staged is None else staged,
                 st, ext)
    K_.ws_resolve(parent.data_ptr(), roots.data_ptr(), flags.data_ptr(), N, D, H, W, st, ext)
    return roots, flags


def saddle_pairs(ids: torch.Tensor, basin_ids: torch.Tensor, offsets: torch.Tensor, height: torch.Tensor,
                 rows: int | None = None, cap: int | None = None) -> torch.Tensor:
    """``pairs`` int64 ``[P, 3]``, rows ``(row_a, row_b, saddle)`` sorted by ``(row_a, row_b)``, of an id
    volume, the basin ids and ``offsets`` of its basin table and the height (``reference.watershed_saddles``), on
    the ids' device.  ``rows``: the basin table's row count when the caller knows it; ``cap``: the capacity of the
    first hash table, a power of two (default: from the row count)."""
    _check(ids, height, "saddle_pairs")
    check_ids_offsets(basin_ids, offsets, ids, "saddle_pairs")
    if not _native.use_native(ids) or ids.numel() == 0:
        return reference.watershed_saddles(ids, basin_ids, offsets, height)
    check_batch(ids, "saddle_pairs")
    ids, basin_ids, offsets, height = ids.contiguous(), basin_ids.contiguous(), offsets.contiguous(), height.contiguous()
    N, D, H, W = ids.shape
    dev = ids.device
    T = int(offsets[-1]) if rows is None else int(rows)
    K_, st = _native.kernels(), _native.stream(ids)
    # full: a slot for every forward neighbour of every voxel (<= 2^32) -- probed to its end it holds any pair list
    full = min(MAX_CAP, max(MIN_CAP, _next_pow2(13 * ids.numel())))
    if cap is not None and (cap < 2 or cap & (cap - 1)):
        raise ValueError(f"saddle_pairs: cap must be a power of two >= 2, not {cap!r}")
    cap = min(full, max(MIN_CAP, _next_pow2(4 * T)) if cap is None else cap)
    while True:
        buf = torch.zeros(2 * cap + 1, dtype=torch.int64, device=dev)      # keys | counts | lost, one fill
        keys, counts, lost = buf[:cap], buf[cap:2 * cap], buf[2 * cap:]
        K_.ws_saddle(ids.data_ptr(), basin_ids.data_ptr(), offsets.data_ptr(), height.data_ptr(), keys.data_ptr(),
                     counts.data_ptr(), lost.data_ptr(), N, D, H, W, T, cap, cap if cap >= full else PROBE, st,
                     [ids.numel(), basin_ids.numel(), offsets.numel(), height.numel(), cap, cap, 1])
        if int(lost) == 0:
            break
        if cap >= full:
            raise RuntimeError(f"saddle_pairs: {int(lost)} updates found no slot in a table of {cap} for "
                               f"{ids.numel()} voxels (corrupt ids or offsets?)")
        cap = min(full, 4 * cap)
    slot = torch.nonzero(keys).squeeze(1)
    key, order = torch.sort(keys[slot])          # (keys < 2^63: the int64 order is the uint64 order)
    return torch.stack([(key >> 32) - 1, (key & 0xFFFFFFFF) - 1, counts[slot][order]], 1)


def merge_steps(merge) -> int:
    """``m = 2 * merge`` of a merge height in voxels: a multiple of 0.5, ``>= 0``, in exact arithmetic."""
    if isinstance(merge, bool):
        raise ValueError(f"merge must be a number, not {merge!r}")
    try:
        m = 2 * Fraction(merge)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"merge must be a finite number, not {merge!r}") from None
    if m < 0 or m.denominator != 1:
        raise ValueError(f"merge must be a multiple of 0.5 voxels and >= 0, not {merge!r}")
    return int(m)


def joins(p: int, s: int, m: int) -> bool:
    """A basin of peak ``p`` joins over a pass of height ``s <= p`` (both squared distances) at ``m = 2 *
    merge``: ``2 sqrt(p) - 2 sqrt(s) <= m``, without a root -- with ``t = 4p - 4s - m^2`` that is ``t <= 4 m
    sqrt(s)``, so ``t <= 0 or t^2 <= 16 m^2 s``."""
    t = 4 * p - 4 * s - m * m
    return t <= 0 or t * t <= 16 * m * m * s


def merge_groups(pairs: torch.Tensor, table: torch.Tensor, m: int, peak: torch.Tensor):
    """Which basins are one instance -> ``(group, rep)``: ``group`` int64 ``[T]``, the 0-based new row of every
    basin row, and ``rep`` int64 ``[T']``, the basin row that stands for each new row, on the table's device.

    ``pairs`` as :func:`saddle_pairs` gives them, ``table`` the basin table ``[T, 13]``, ``peak`` int64 ``[T]``
    the height at each basin's root, ``m = 2 * merge``.  The edges are visited by ``(saddle descending, row_a,
    row_b)`` with a union-find; a group carries the largest peak of its members and is represented by the
    member of the largest ``(peak, lowest root)``; the groups ``A != B`` of an edge of saddle ``s`` merge when
    :func:`joins` ``(min(peak A, peak B), s, m)``.  Groups are numbered by their lowest basin row, which keeps
    them in the order of the samples.  Host work over ``P`` rows: nothing per-voxel is read."""
    T = table.shape[0]
    edges = pairs.cpu().tolist()
    pk = peak.cpu().tolist()
    root = table[:, 3].cpu().tolist()
    up = list(range(T))

    def find(a):
        while up[a] != a:
            up[a] = up[up[a]]
            a = up[a]
        return a

    best = list(range(T))                        # the representative of the group whose union-find root is the index
    for a, b, s in sorted(edges, key=lambda e: (-e[2], e[0], e[1])):
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        ka, kb = (pk[best[ra]], -root[best[ra]]), (pk[best[rb]], -root[best[rb]])
        if joins(min(ka[0], kb[0]), s, m):
            up[rb] = ra
            if kb > ka:
                best[ra] = best[rb]
    ends = [find(a) for a in range(T)]
    number, rep = {}, []
    for a, e in enumerate(ends):                 # ascending rows: a group is numbered when its lowest row comes by
        if e not in number:
            number[e] = len(rep)
            rep.append(best[e])
    dev = table.device
    return (torch.tensor([number[e] for e in ends], dtype=torch.int64, device=dev),
            torch.tensor(rep, dtype=torch.int64, device=dev))


def split_instances(ids: torch.Tensor, height: torch.Tensor, merge=1.0):
    """Every component of ``ids`` cut along the passes of ``height`` -> ``(ids', table', offsets',
    parent_component, peak2)``: ids' int32 ``[N, D, H, W]``, table' int64 ``[T', 13]`` and offsets' int64 ``[N +
    1]`` in the form of ``ccl.instance_table`` (the instances of a sample are numbered by the component they
    were cut from, then by their lowest basin, so ids 1..n that nothing cuts come back as they were; ``root`` is
    the representative basin's, the highest voxel of the instance, not the lowest; ``class`` is 1),
    ``parent_component``
    int64 ``[T']`` the id in ``ids`` each new row came from and ``peak2`` int64 ``[T']`` its largest height, all on
    the ids' device.  ``merge``: a multiple of 0.5 voxels ``>= 0``; 0 joins plateaus only, larger values join
    more, and on a constant height the input partition comes back."""
    _check(ids, height, "split_instances")
    m = merge_steps(merge)
    N, D, H, W = ids.shape
    V, dev = D * H * W, ids.device
    roots, flags = ascend(ids, height)
    basin_ids, table, offsets = ccl.instance_table((ids > 0).to(torch.uint8), roots, want_ids=True, flags=flags)
    T = table.shape[0]
    if T == 0:
        none = torch.zeros(0, dtype=torch.int64, device=dev)
        return basin_ids, table, offsets, none, none.clone()
    at = table[:, 0] * V + table[:, 3] - 1       # the flat index of every basin's root
    peak = height.reshape(-1)[at].clamp(min=0).to(torch.int64)
    pairs = saddle_pairs(ids, basin_ids, offsets, height, rows=T)
    group, rep = merge_groups(pairs, table, m, peak)
    T2 = rep.numel()
    # Renumber the groups by (sample, the component they were cut from, lowest basin row): the pieces of a
    # component follow one another in the component's place, and where nothing is cut ids 1..n come back as they
    # were.  Over T' rows; no per-voxel work.
    comp = ids.reshape(-1)[at[rep]].to(torch.int64)
    order = torch.argsort(table[rep, 0] << 31 | comp, stable=True)
    group = torch.empty_like(order).scatter_(0, order, torch.arange(T2, dtype=torch.int64, device=dev))[group]
    rep = rep[order]
    out = torch.zeros(T2, NCOL, dtype=torch.int64, device=dev)
    out[:, [0, 1, 3]] = table[rep][:, [0, 1, 3]]
    for c in (2, 10, 11, 12):
        out[:, c] = torch.zeros(T2, dtype=torch.int64, device=dev).index_add_(0, group, table[:, c])
    for c in (4, 5, 6):
        out[:, c] = torch.full((T2,), 1 << 31, dtype=torch.int64, device=dev).scatter_reduce(0, group, table[:, c], "amin")
    for c in (7, 8, 9):
        out[:, c] = torch.full((T2,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, group, table[:, c], "amax")
    offsets2 = torch.cat([offsets.new_zeros(1), torch.cumsum(torch.bincount(out[:, 0], minlength=N), 0)])
    # the relabel: one gather through lut, 1-based basin row -> new id (int32 throughout: T < 2^31)
    lut = torch.cat([group.new_zeros(1), group - offsets2[out[:, 0]][group] + 1]).to(torch.int32)
    row = torch.where(basin_ids > 0, basin_ids + offsets[:-1].to(torch.int32).view(N, 1, 1, 1), 0)
    return lut[row], out, offsets2, comp[order], peak[rep]
