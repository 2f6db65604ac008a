"""Argument checks shared by the volume ops (``ccl``, ``overlap``, ``access``, ``edt``, ``reach``).  ``what`` is the
public function's name: every message starts with it."""
import torch


def got(t) -> str:
    return f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__


def check_volume(t, what: str, name: str, dtype: torch.dtype = torch.uint8) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 4:
        kind = "a uint8" if dtype == torch.uint8 else "an int32"
        raise ValueError(f"{what}: {name} must be {kind} [N, D, H, W] tensor, not {got(t)}")


def check_ids_offsets(ids, offsets, occ: torch.Tensor, what: str) -> None:
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.shape != occ.shape:
        raise ValueError(f"{what}: ids must be int32 {tuple(occ.shape)}, not {got(ids)}")
    N = occ.shape[0]
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or tuple(offsets.shape) != (N + 1,):
        raise ValueError(f"{what}: offsets must be int64 [{N + 1}], not {got(offsets)}")
    if ids.device != occ.device or offsets.device != occ.device:
        raise ValueError(f"{what}: ids ({ids.device}), offsets ({offsets.device}) and occ ({occ.device}) must be on "
                         "one device")


def check_batch(t: torch.Tensor, what: str) -> None:
    if t.numel() >= 1 << 31:                     # (the kernels index the batch's voxels in int32)
        raise ValueError(f"{what}: a batch must have fewer than 2^31 voxels; split it by samples")
