"""Feature instances one by one, as the single-feature classifier wants them.

``isolate_instances`` turns one ``ids`` volume and a selection ``sel`` of its instances into one part per row of
``sel``: the instance alone in a solid stock block, at the classifier's resolution, as bits, bytes or bf16 (see
:func:`featurenet_amd.ops.reference.isolate_instances` for the exact definition).  Device tensors run
``isolate_parts`` (``isolate.hip``): a thread makes 8 to 32 voxels of one part and stores them once; rows of
the part whose source row misses the instance's box are constants and read nothing.  CPU tensors and empty
selections run the reference.  ``selection`` builds ``sel`` from an instance table on its device,
``material_window`` the stock of ``stock="bbox"``, and ``recognize_table`` runs a :class:`FeatureNet3D` over
the parts of a table's rows.
"""
from __future__ import annotations

import torch

from .. import _native
from . import reference

NCOL = reference.ISOLATE_NCOL
MAX_S = reference.ISOLATE_MAX_S


def isolate_instances(ids: torch.Tensor, sel: torch.Tensor, size: int, fmt: int = 1) -> torch.Tensor:
    """The parts of ``sel`` int32 ``[M, 14]`` cut from ``ids`` int32 ``[N, D, H, W]``
    (``reference.isolate_instances``) on the ids' device: ``fmt`` 0 uint8 ``[M, S^3 / 8]``, 1 uint8 ``[M, S,
    S, S]``, 2 bfloat16 ``[M, S, S, S, 1]``.  A row of ``sel`` whose sample or window lies outside the grid
    raises ``ValueError``; on the device that check reads one flag back."""
    S = reference.isolate_check(ids, sel, size, fmt)
    M = sel.shape[0]
    if not _native.use_native(ids) or M == 0 or ids.numel() == 0:
        return reference.isolate_instances(ids, sel, S, fmt)
    if bool(reference.isolate_bad_rows(sel, ids.shape).any()):
        raise ValueError(f"isolate_instances: a row of sel names a sample or a window outside the grid "
                         f"{tuple(ids.shape)}")
    ids, sel = ids.contiguous(), sel.contiguous()
    N, D, H, W = ids.shape
    V = S ** 3
    shape = {0: (M, V // 8), 1: (M, S, S, S), 2: (M, S, S, S, 1)}[fmt]
    out = torch.empty(shape, dtype=torch.bfloat16 if fmt == 2 else torch.uint8, device=ids.device)
    K_, st = _native.kernels(), _native.stream(ids)
    step = ((1 << 31) - 1) // V                  # parts of one launch: M * S^3 < 2^31
    for lo in range(0, M, step):
        s, o = sel[lo:lo + step], out[lo:lo + step]
        K_.isolate_parts(ids.data_ptr(), s.data_ptr(), o.data_ptr(), N, D, H, W, s.shape[0], S, fmt, st,
                         [ids.numel(), s.numel(), o.numel()])
    return out


def material_window(occ: torch.Tensor) -> torch.Tensor:
    """The bounding box of the material (``occ != 0``) of every sample of ``occ`` ``[N, D, H, W]`` -> int64
    ``[N, 6]`` ``(z0, y0, x0, Lz, Ly, Lx)`` on its device; a sample without material gets the whole grid."""
    if not isinstance(occ, torch.Tensor) or occ.dim() != 4:
        raise ValueError("material_window: occ must be an [N, D, H, W] tensor")
    N, dev = occ.shape[0], occ.device
    m = (occ != 0).to(torch.uint8)
    lo, ln = [], []
    for axis in (1, 2, 3):
        L = occ.shape[axis]
        if occ.numel() == 0:
            lo.append(torch.zeros(N, dtype=torch.int64, device=dev))
            ln.append(torch.full((N,), L, dtype=torch.int64, device=dev))
            continue
        line = m.amax(dim=tuple(a for a in (1, 2, 3) if a != axis)) != 0         # [N, L]: material in the slice
        idx = torch.arange(L, device=dev)
        first = torch.where(line, idx, L).amin(1)
        last = torch.where(line, idx, -1).amax(1)
        none = last < 0
        lo.append(torch.where(none, 0, first))
        ln.append(torch.where(none, L, last - first + 1))
    return torch.stack(lo + ln, 1)


def selection(table: torch.Tensor, offsets: torch.Tensor, rows: int | None = None, min_voxels: int = 1,
              window: torch.Tensor | None = None, shape=None):
    """``(sel, keep)`` for :func:`isolate_instances` from an instance table int64 ``[T, 13]`` and its
    ``offsets`` (``ops.ccl.instance_table``), on the table's device: ``sel`` int32 ``[M, 14]`` with the
    table's boxes, ``keep`` int64 ``[M]`` the table rows it was made from -- those of at least ``min_voxels``
    voxels, in order.  ``window``: int64 ``[N, 6]`` ``(z0, y0, x0, Lz, Ly, Lx)`` per sample
    (:func:`material_window`), or None for the whole grid, which then needs ``shape = (D, H, W)``.  ``rows``:
    ``T`` when the caller knows it.  Nothing is read back to the host unless ``min_voxels > 1`` drops rows
    (their number sizes ``sel``)."""
    if table.dim() != 2 or table.shape[1] != 13 or table.dtype != torch.int64:
        raise ValueError(f"selection: table must be int64 [T, 13], not {table.dtype} {tuple(table.shape)}")
    dev = table.device
    T = table.shape[0] if rows is None else int(rows)
    N = offsets.numel() - 1
    keep = torch.arange(T, dtype=torch.int64, device=dev)
    if min_voxels > 1:
        keep = keep[table[:T, 2] >= int(min_voxels)]
    row = table[keep]
    n = row[:, 0]
    if window is None:
        if shape is None or len(shape) != 3:
            raise ValueError("selection: window=None (the whole grid) needs shape = (D, H, W)")
        win = torch.tensor([0, 0, 0, *(int(s) for s in shape)], dtype=torch.int64, device=dev).expand(len(keep), 6)
    else:
        if window.dtype != torch.int64 or tuple(window.shape) != (N, 6):
            raise ValueError(f"selection: window must be int64 [{N}, 6], not {window.dtype} {tuple(window.shape)}")
        win = window.to(dev)[n]
    ident = keep - offsets.to(dev)[n] + 1
    sel = torch.cat([n[:, None], ident[:, None], row[:, 4:10], win], 1).to(torch.int32)
    return sel, keep


@torch.no_grad()
def recognize_table(classifier, ids: torch.Tensor, table: torch.Tensor, offsets: torch.Tensor,
                    rows: int | None = None, min_voxels: int = 1, window: torch.Tensor | None = None,
                    batch_size: int = 256, want_probs: bool = False):
    """The single-feature classifier's opinion on every row of an instance table -> ``(cls int64 [T], prob
    float32 [T], probs float32 [T, C] or None)`` on the ids' device.  Each instance of at least ``min_voxels``
    voxels is isolated in its ``window`` (None: the grid) at ``classifier.cfg.input_size`` -- bf16 parts
    straight from the kernel on the GPU, dense float on the CPU -- and the classifier runs in eval mode over
    ``batch_size`` parts at a time.  ``cls`` is the top-1 class (``reference.lowest_argmax``: ties go to the
    lowest class), ``prob`` its softmax probability; rows not selected hold ``-1`` and ``0``.  ``probs``
    (with ``want_probs``) holds every class's probability."""
    from ..models.featurenet3d import FeatureNet3D

    if not isinstance(classifier, FeatureNet3D):
        raise ValueError(f"recognize_table: the classifier must be a FeatureNet3D, not {type(classifier).__name__} "
                         "(a segmentation model labels voxels, see extract_features())")
    if batch_size < 1:
        raise ValueError(f"recognize_table: batch_size must be at least 1, not {batch_size!r}")
    dev = ids.device
    pdev = next(classifier.parameters()).device
    if pdev != dev:
        raise ValueError(f"recognize_table: the classifier ({pdev}) and ids ({dev}) must be on one device")
    S, C = int(classifier.cfg.input_size), int(classifier.cfg.num_classes)
    sel, keep = selection(table, offsets, rows, min_voxels, window, shape=tuple(ids.shape[1:]))
    T = table.shape[0] if rows is None else int(rows)
    cls = torch.full((T,), -1, dtype=torch.int64, device=dev)
    prob = torch.zeros(T, dtype=torch.float32, device=dev)
    probs = torch.zeros(T, C, dtype=torch.float32, device=dev) if want_probs else None
    was_training = classifier.training
    classifier.eval()
    try:
        for lo in range(0, sel.shape[0], batch_size):
            if dev.type == "cuda":
                x = isolate_instances(ids, sel[lo:lo + batch_size], S, 2)
            else:
                x = isolate_instances(ids, sel[lo:lo + batch_size], S, 1).float().unsqueeze(-1)
            p = torch.softmax(classifier(x).float(), -1)
            top = reference.lowest_argmax(p).to(torch.int64)
            at = keep[lo:lo + batch_size]
            cls[at] = top
            prob[at] = p.gather(1, top[:, None]).squeeze(1)
            if want_probs:
                probs[at] = p
    finally:
        classifier.train(was_training)
    return cls, prob, probs
