"""Triangle meshes to voxel grids: occupancy from a batch of meshes on the integer lattice.

``voxelize`` takes ``tris`` int32 ``[T, 9]`` and ``offsets`` int32 ``[N + 1]``
(``reference.voxelize_tris`` has the lattice and the rule; ``csrc/shared/voxelize.h`` the integer
forms) and returns the occupancy and the leak counts on the device asked for.  Device tensors run
``voxelize_tris`` (``voxelize.hip``), CPU tensors ``_rt.voxelize_tris``: one header holds the
cover test and the crossing of both, everything is integer arithmetic, and the two agree bit for
bit with each other and with the torch oracle.

``quantize`` maps model units to the lattice.  It always runs on the host in float64 numpy, so
the lattice coordinates -- and with them every voxel -- do not depend on the device.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native
from .partgen import check_size

UNITS = 16                 # lattice units per voxel
MAX_COORD = 8192           # largest |coordinate|: edge functions stay in int32


def check_tris(tris, offsets, what: str = "voxelize") -> None:
    """Dtype and shape of ``tris`` and ``offsets``, the coordinate range, and the offsets: from 0
    to ``T`` without a decrease."""
    if not isinstance(tris, torch.Tensor) or tris.dtype != torch.int32 or tris.dim() != 2 or tris.shape[1] != 9:
        got = f"{tris.dtype} {tuple(tris.shape)}" if isinstance(tris, torch.Tensor) else type(tris).__name__
        raise ValueError(f"{what}: tris must be an int32 [T, 9] tensor, not {got}")
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int32 or offsets.dim() != 1 \
            or offsets.numel() < 1:
        got = f"{offsets.dtype} {tuple(offsets.shape)}" if isinstance(offsets, torch.Tensor) else type(offsets).__name__
        raise ValueError(f"{what}: offsets must be an int32 [N + 1] tensor, not {got}")
    off = offsets.tolist()
    if off[0] != 0 or off[-1] != tris.shape[0]:
        raise ValueError(f"{what}: offsets must run from 0 to T = {tris.shape[0]}, not from {off[0]} to {off[-1]}")
    if any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"{what}: offsets must not decrease")
    if tris.numel() and int(tris.abs().max()) > MAX_COORD:
        raise ValueError(f"{what}: a coordinate exceeds {MAX_COORD} lattice units ({UNITS} per voxel)")


def quantize(vertices, size: int, fit="bbox", margin: float = 0):
    """Model units -> the lattice: ``(int32 array of the shape of vertices, origin float64 [3],
    voxel_size)`` with ``lattice = rint((vertices - origin) * 16 / voxel_size)``, so voxel
    ``(x, y, z)`` is the cube of edge ``voxel_size`` at ``origin + voxel_size * (x, y, z)``.

    ``fit="bbox"``: the longest side of the vertices' bounding box spans exactly ``[16 m, 16 (S -
    m)]`` with ``m = margin`` voxels, and the shorter axes are centred to a lattice unit.
    ``fit=(origin, voxel_size)`` uses that transform; coordinates outside the lattice raise."""
    size = check_size(size, "quantize")
    v = np.asarray(vertices, dtype=np.float64)
    if v.shape[-1:] != (3,):
        raise ValueError(f"quantize: vertices must be [..., 3], not {v.shape}")
    if not np.isfinite(v).all():
        raise ValueError("quantize: a vertex is not finite")
    if isinstance(fit, str):
        if fit != "bbox":
            raise ValueError(f"quantize: fit must be 'bbox' or (origin, voxel_size), not {fit!r}")
        if not 0 <= margin < size / 2:
            raise ValueError(f"quantize: margin must lie in [0, size / 2), not {margin!r}")
        if v.size == 0:
            return np.zeros(v.shape, np.int32), np.zeros(3), 1.0
        lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
        longest = float((hi - lo).max())
        if longest <= 0:
            raise ValueError("quantize: the mesh has no extent")
        voxel_size = longest / (size - 2 * margin)
        span = np.rint((hi - lo) * (UNITS / voxel_size))             # lattice units per axis
        start = np.where(hi - lo == longest, np.rint(UNITS * margin), np.floor((UNITS * size - span) / 2))
        origin = lo - start * (voxel_size / UNITS)
    else:
        origin, voxel_size = fit
        origin, voxel_size = np.asarray(origin, dtype=np.float64).reshape(3), float(voxel_size)
        if not voxel_size > 0 or not np.isfinite(origin).all():
            raise ValueError(f"quantize: fit needs a finite origin and a positive voxel size, not {fit!r}")
    q = np.rint((v - origin) * (UNITS / voxel_size))
    if v.size and np.abs(q).max() > MAX_COORD:
        raise ValueError(f"quantize: a vertex lies {np.abs(q).max() / UNITS:.1f} voxels from the origin; the lattice "
                         f"ends at {MAX_COORD // UNITS}")
    return q.astype(np.int32), origin, voxel_size


def voxelize(tris: torch.Tensor, offsets: torch.Tensor, size: int, device=None, packed: bool = False,
             threads: int = 0):
    """Meshes ``tris`` / ``offsets`` -> ``(voxels, leaks)`` on ``device`` (default: where ``tris``
    is).  ``voxels`` is the occupancy, uint8 ``[N, S, S, S]``, or with ``packed`` its bits, uint8
    ``[N, S^3 / 8]`` (bit i of byte j = voxel 8j + i); ``leaks`` int64 ``[N]`` counts the columns
    that a mesh leaves open (0: watertight)."""
    size = check_size(size, "voxelize")
    check_tris(tris, offsets)
    if device is not None:
        tris, offsets = tris.to(device), offsets.to(device)
    tris, offsets = tris.contiguous(), offsets.contiguous()
    N, T, dev = offsets.numel() - 1, tris.shape[0], tris.device
    if not _native.use_native(tris):
        if tris.is_cuda:                         # (the debugging fall-back of _native.use_native)
            from . import reference

            occ, leaks = reference.voxelize_tris(tris, offsets, size)
        else:
            occ, leaks = (torch.from_numpy(a) for a in
                          _native.runtime().voxelize_tris(tris.numpy(), offsets.numpy(), size, int(threads)))
        vox = occ
        if packed:
            weights = 1 << torch.arange(8, dtype=torch.int32, device=dev)
            vox = (occ.reshape(N, size ** 3 // 8, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8)
        return vox, leaks
    K_ = _native.kernels()
    zs = K_.voxelize_planes(size)
    slabs = -(-size // zs)
    vox = torch.empty((N, size ** 3 // 8) if packed else (N, size, size, size), dtype=torch.uint8, device=dev)
    part = torch.empty((N, slabs), dtype=torch.int32, device=dev)
    K_.voxelize_tris(tris.data_ptr(), offsets.data_ptr(), 0 if packed else vox.data_ptr(),
                     vox.data_ptr() if packed else 0, part.data_ptr(), N, T, size, zs, _native.stream(tris),
                     [tris.numel(), offsets.numel(), 0 if packed else vox.numel(), vox.numel() if packed else 0,
                      part.numel()])
    return vox, part.sum(1, dtype=torch.int64)
