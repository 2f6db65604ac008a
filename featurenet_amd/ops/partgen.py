"""Multi-feature parts carved from parameter tables: occupancy, per-voxel labels and slots.

``carve`` takes ``params`` int32 ``[N, K, 16]`` (``reference.carve_parts`` has the row format and
the label rule; ``csrc/shared/partgen.h`` the 24 volumes) and returns the parts on the device
asked for.  Device tensors run ``partgen_carve`` (``partgen.hip``), CPU tensors
``_rt.carve_parts``: one header holds the predicates of both, everything is integer arithmetic,
and the two agree bit for bit with each other and with the torch oracle.

``sample`` draws tables (``_rt.sample_parts``): deterministic per ``(seed, part index)``.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native

ROW = 16
MAX_SIZE = 256
MAX_SLOTS = 32
NUM_CLASSES = 24


def check_size(size, what: str = "carve") -> int:
    if not isinstance(size, (int, np.integer)) or isinstance(size, bool) or size < 8 or size > MAX_SIZE or size % 8:
        raise ValueError(f"{what}: size must be a multiple of 8 in [8, {MAX_SIZE}], not {size!r}")
    return int(size)


def check_params(params: torch.Tensor, size: int, what: str = "carve") -> None:
    """Dtype, shape and value ranges of a parameter table: ``cls`` in -1..23, ``orient`` in 0..23
    and every geometry field of a used slot within +-8 * size (the bound under which no product
    of the predicates leaves int32)."""
    if not isinstance(params, torch.Tensor) or params.dtype != torch.int32 or params.dim() != 3 \
            or params.shape[2] != ROW:
        got = f"{params.dtype} {tuple(params.shape)}" if isinstance(params, torch.Tensor) else type(params).__name__
        raise ValueError(f"{what}: params must be an int32 [N, K, {ROW}] tensor, not {got}")
    if params.shape[1] > MAX_SLOTS:
        raise ValueError(f"{what}: at most {MAX_SLOTS} feature slots per part, not {params.shape[1]}")
    if params.numel() == 0:
        return
    cls, used = params[..., 0], params[..., 0] >= 0
    bad = torch.stack([((cls < -1) | (cls >= NUM_CLASSES)).any(),
                       (used & ((params[..., 1] < 0) | (params[..., 1] >= 24))).any(),
                       (used[..., None] & (params[..., 2:10].abs() > 8 * size)).any()]).tolist()
    if bad[0]:
        raise ValueError(f"{what}: cls must lie in -1..{NUM_CLASSES - 1}")
    if bad[1]:
        raise ValueError(f"{what}: orient must lie in 0..23")
    if bad[2]:
        raise ValueError(f"{what}: a geometry field exceeds 8 * size = {8 * size} quarter voxels")


def sample(n: int, size: int = 64, seed: int = 0, features=(1, 4), num_classes: int = NUM_CLASSES,
           separate: bool = True, gap: int = 1, threads: int = 0) -> torch.Tensor:
    """``n`` parameter tables -> int32 ``[n, features[1], 16]`` (CPU)."""
    size = check_size(size, "sample")
    lo, hi = (int(v) for v in features)
    if not 0 <= lo <= hi <= MAX_SLOTS:
        raise ValueError(f"sample: features must be (lo, hi) with 0 <= lo <= hi <= {MAX_SLOTS}, not {features!r}")
    tab = _native.runtime().sample_parts(int(n), size, int(seed), lo, hi, int(num_classes), bool(separate), int(gap),
                                         int(threads))
    return torch.from_numpy(tab)


def carve(params: torch.Tensor, size: int, device=None, packed: bool = False, want_slots: bool = False,
          threads: int = 0):
    """Parts of the tables ``params`` -> ``(voxels, labels)`` or ``(voxels, labels, slots)`` on
    ``device`` (default: where ``params`` is).  ``voxels`` is the occupancy, uint8 ``[N, S, S, S]``,
    or with ``packed`` its bits, uint8 ``[N, S^3 / 8]`` (bit i of byte j = voxel 8j + i);
    ``labels`` and ``slots`` are uint8 ``[N, S, S, S]``."""
    size = check_size(size)
    if isinstance(params, torch.Tensor) and device is not None:
        params = params.to(device)
    check_params(params, size)
    params = params.contiguous()
    N, K, _ = params.shape
    dev = params.device
    if not _native.use_native(params):
        if params.is_cuda:                       # (the debugging fall-back of _native.use_native)
            from . import reference

            occ, labels, slots = reference.carve_parts(params, size)
        else:
            occ, labels, slots = (torch.from_numpy(a) for a in
                                  _native.runtime().carve_parts(params.numpy(), size, int(threads)))
        vox = occ
        if packed:
            weights = 1 << torch.arange(8, dtype=torch.int32, device=dev)
            vox = (occ.reshape(N, -1, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8)
        return (vox, labels, slots) if want_slots else (vox, labels)
    V = size ** 3
    vox = torch.empty((N, V // 8) if packed else (N, size, size, size), dtype=torch.uint8, device=dev)
    labels = torch.empty((N, size, size, size), dtype=torch.uint8, device=dev)
    slots = torch.empty_like(labels) if want_slots else None
    _native.kernels().partgen_carve(params.data_ptr(), 0 if packed else vox.data_ptr(), vox.data_ptr() if packed else 0,
                                    labels.data_ptr(), _native.ptr(slots), N, K, size, _native.stream(params),
                                    [params.numel(), 0 if packed else vox.numel(), vox.numel() if packed else 0,
                                     labels.numel(), slots.numel() if want_slots else 0])
    return (vox, labels, slots) if want_slots else (vox, labels)
