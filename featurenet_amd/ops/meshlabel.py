"""Mesh labels: which value of a voxel volume lies against each triangle of the mesh it came from.

``mesh_votes`` takes ``tris`` int32 ``[T, 9]`` and ``offsets`` int32 ``[N + 1]`` on the lattice of
``ops.voxelize`` and ``vol`` ``[N, S, S, S]`` (int32 instance ids or uint8 labels, 0 = nothing) and
returns int32 ``[T, 3]``: ``winner, votes, covered`` per triangle (``reference.mesh_votes`` has the
rule; ``csrc/shared/voxelize.h`` the integer forms).  Device tensors run ``mesh_votes``
(``meshlabel.hip``), CPU tensors ``_rt.mesh_votes``: one header under both, integers only, bit for
bit the torch oracle.

The kernel has two forms, chosen per triangle by the number of column centres in the triangle's
box: the thread form (one lane per triangle, the tally in registers) up to ``THREAD_COLS`` columns,
the wave form (the wave strides the box, the tally in LDS) above.  ``form`` forces one of them.
"""
from __future__ import annotations

import torch

from .. import _native
from .partgen import check_size
from .voxelize import check_tris

# Boxes of at most this many columns take the thread form.  bench/mesh_label.py finds the thread form
# faster at every box size it can hold, so this is the kernel's cap, mesh_votes_thread_cols() = 8; a
# cap of 16 was measured too and lost on small boxes (profiles/mesh_label.md).
THREAD_COLS = 8
FORMS = (None, "thread", "wave")


def check_volume(vol, n: int, what: str = "mesh_votes") -> int:
    """Dtype and shape of ``vol`` for ``n`` meshes -> ``S``, within the voxelizer's limits."""
    if not isinstance(vol, torch.Tensor) or vol.dtype not in (torch.int32, torch.uint8) or vol.dim() != 4 \
            or len(set(vol.shape[1:])) != 1:
        got = f"{vol.dtype} {tuple(vol.shape)}" if isinstance(vol, torch.Tensor) else type(vol).__name__
        raise ValueError(f"{what}: vol must be an int32 or uint8 [N, S, S, S] tensor, not {got}")
    if vol.shape[0] != n:
        raise ValueError(f"{what}: {n} meshes need {n} volumes, not {vol.shape[0]}")
    return check_size(int(vol.shape[1]), what)


def mesh_votes(tris: torch.Tensor, offsets: torch.Tensor, vol: torch.Tensor, device=None, form: str | None = None,
               threads: int = 0) -> torch.Tensor:
    """Meshes ``tris`` / ``offsets`` against ``vol`` -> int32 ``[T, 3]`` = ``winner, votes,
    covered`` on ``device`` (default: where ``tris`` is).  ``form``: ``None`` (each triangle takes
    the form its box size asks for), ``"thread"`` (every box the thread form can hold, 8 columns,
    stays with its lane) or ``"wave"`` (every triangle is taken by the wave); the rows never
    depend on it."""
    check_tris(tris, offsets, "mesh_votes")
    size = check_volume(vol, offsets.numel() - 1)
    if form not in FORMS:
        raise ValueError(f"mesh_votes: form must be one of {FORMS}, not {form!r}")
    dev = torch.device(device) if device is not None else tris.device
    tris, offsets, vol = tris.to(dev).contiguous(), offsets.to(dev).contiguous(), vol.to(dev).contiguous()
    N, T = offsets.numel() - 1, tris.shape[0]
    if not _native.use_native(tris):
        if tris.is_cuda:                         # (the debugging fall-back of _native.use_native)
            from . import reference

            return reference.mesh_votes(tris, offsets, vol, size)
        return torch.from_numpy(_native.runtime().mesh_votes(tris.numpy(), offsets.numpy(), vol.numpy(), int(threads)))
    K_ = _native.kernels()
    thr = {None: THREAD_COLS, "thread": K_.mesh_votes_thread_cols(), "wave": -1}[form]
    votes = torch.empty((T, 3), dtype=torch.int32, device=dev)
    wide = torch.empty(T + 1, dtype=torch.int32, device=dev)           # the wave form's triangles: count, list
    K_.mesh_votes(tris.data_ptr(), offsets.data_ptr(), vol.data_ptr(), votes.data_ptr(), wide.data_ptr(), N, T, size,
                  vol.element_size(), thr, _native.stream(tris),
                  [tris.numel(), offsets.numel(), vol.numel(), votes.numel(), wide.numel()])
    return votes
