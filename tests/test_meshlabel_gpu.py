"""The mesh-label kernel (``meshlabel.hip``) and what is built on it (``ops.meshlabel``,
``fn.label_mesh``) on the GPU.

Every comparison is ``torch.equal`` against the torch oracle (``reference.mesh_votes``, computed
on the CPU, once per process in ``_meshlabel_cases.expected``), for int32 and uint8 volumes, with
each form forced, with the default dispatch and with thresholds in between.  The kernel is called
at binding level, its output a view into a larger buffer filled with ``FILL``: the ``GUARD`` bytes
on both sides must come back untouched.  The large triangles hold more distinct values than the
wave form's table: they pass only through its exact multi-pass path.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
import _meshlabel_cases as lc  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.ops import meshlabel  # noqa: E402
from featurenet_amd.utils.voxelmesh import voxels_to_mesh  # noqa: E402

DEV = "cuda"
GUARD, FILL = 64, 0xA5


def launch(tris: torch.Tensor, off: torch.Tensor, vol: torch.Tensor, size: int, thr: int) -> torch.Tensor:
    """One ``mesh_votes`` call at binding level -> int32 ``[T, 3]`` on the device; checks the guard bytes."""
    N, T = off.numel() - 1, tris.shape[0]
    t, o, v = tris.to(DEV).contiguous(), off.to(DEV).contiguous(), vol.to(DEV).contiguous()
    buf = torch.full((12 * T + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + 12 * T]
    scratch = torch.full((4 * (T + 1) + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    wide = scratch[GUARD:GUARD + 4 * (T + 1)]
    _native.kernels().mesh_votes(t.data_ptr(), o.data_ptr(), v.data_ptr(), out.data_ptr(), wide.data_ptr(), N, T, size,
                                 v.element_size(), thr, _native.stream(t), [t.numel(), o.numel(), v.numel(), 3 * T, T + 1])
    for b, n in ((buf, 12 * T), (scratch, 4 * (T + 1))):
        assert bool((b[:GUARD] == FILL).all()) and bool((b[GUARD + n:] == FILL).all()), "guard bytes"
    return out.view(torch.int32).view(T, 3)


@pytest.mark.parametrize("dtype", ["int32", "uint8"])
@pytest.mark.parametrize("name", lc.NAMES)
def test_kernel_equals_the_oracle(name, dtype):
    _, size, tris, off, vol = next(c for c in lc.suite() if c[0] == name)
    v = lc.volume(vol, dtype)
    want = lc.expected(name, dtype)
    cap = _native.kernels().mesh_votes_thread_cols()
    assert 0 <= meshlabel.THREAD_COLS <= cap
    first = {}
    for thr in (-1, 0, 1, 4, cap // 2, cap):                       # the wave form for all ... the thread form where it can
        got = launch(tris, off, v, size, thr)
        bad = int((got.cpu() != want).any(1).sum())
        assert torch.equal(got.cpu(), want), (name, dtype, thr, bad)
        first[thr] = got
    assert torch.equal(launch(tris, off, v, size, -1), first[-1]) and torch.equal(launch(tris, off, v, size, cap), first[cap])
    for form in (None, "thread", "wave"):
        got = meshlabel.mesh_votes(tris, off, v, device=DEV, form=form)
        assert got.device.type == "cuda" and got.dtype == torch.int32 and torch.equal(got.cpu(), want), (name, form)


def test_large_triangles_overflow_the_table():
    """The premise of the exact path's cases: more distinct values than any table of the kernel's size."""
    for name in ("large", "large_axis"):
        _, size, tris, off, vol = next(c for c in lc.suite() if c[0] == name)
        assert int(lc.expected(name, "int32")[:, 2].max()) >= 120 and vol.unique().numel() == size ** 3


def test_binding_checks():
    _, size, tris, off, vol = next(c for c in lc.suite() if c[0] == "volumes8")
    K_ = _native.kernels()
    t, o, v = tris.to(DEV), off.to(DEV), vol.to(DEV)
    out = torch.empty((len(t), 3), dtype=torch.int32, device=DEV)
    N, T = o.numel() - 1, len(t)
    wide = torch.empty(T + 1, dtype=torch.int32, device=DEV)
    ext = [t.numel(), o.numel(), v.numel(), out.numel(), wide.numel()]

    def call(size=size, elem=4, thr=K_.mesh_votes_thread_cols(), ext=ext, T=T, N=N):
        K_.mesh_votes(t.data_ptr(), o.data_ptr(), v.data_ptr(), out.data_ptr(), wide.data_ptr(), N, T, size, elem, thr,
                      _native.stream(t), ext)

    call()
    for bad in (dict(size=12), dict(size=4), dict(elem=2), dict(thr=K_.mesh_votes_thread_cols() + 1), dict(thr=-2), dict(size=16), dict(T=T + 1),
                dict(N=N + 1), dict(ext=ext[:4]), dict(ext=ext[:3] + [ext[3] - 1, ext[4]]), dict(ext=ext[:4] + [T])):
        with pytest.raises(RuntimeError, match="mesh_votes"):
            call(**bad)
    with pytest.raises(ValueError, match="mesh_votes"):
        meshlabel.mesh_votes(tris, off, vol.long(), device=DEV)
    with pytest.raises(ValueError, match="form"):
        meshlabel.mesh_votes(tris, off, vol, device=DEV, form="both")


def test_label_mesh_is_the_same_on_both_devices():
    occ = np.ones((16, 16, 16), np.uint8)
    occ[10:, 3:9, 2:13] = 0
    occ[:, 11:14, 4:7] = 0
    mesh = voxels_to_mesh(occ) * 0.25 + np.float32([3.0, -2.0, 1.0])
    ids, _ = fn.label_components(1 - occ[None], device=DEV)
    gpu, grows = fn.label_mesh(mesh, ids[0], device=DEV, return_votes=True)
    cpu, crows = fn.label_mesh(mesh, ids[0], device="cpu", return_votes=True)
    assert np.array_equal(gpu, cpu) and np.array_equal(grows, crows) and set(np.unique(gpu)) == {0, 1, 2}
    assert np.array_equal(fn.label_mesh(mesh, ids[0]), cpu)              # the default device is the GPU
