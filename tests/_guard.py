"""Guard bands around everything a launch allocates (shared by the GPU oracle tests).

Every launch runs inside ``Guard``, which makes each device tensor the entry point allocates --
outputs, statistics slabs, partial-sum scratch, packed weights -- the middle of a flat buffer,
its ends holding a known pattern and its middle NaN (``empty``) or zero (``zeros``); after the
launch the bands of every such buffer still alive must be unchanged, and an output slot nobody
wrote is a NaN that fails the comparison.  ``launch`` also asserts that what the entry point
returned lives in such a buffer.  A buffer whose last reference is gone by then is skipped;
``KeepGuard`` / ``launch_kept`` hold every buffer until the check, for entry points whose scratch
(partial-sum slabs, workspaces) is dropped before they return.
"""
import math
import weakref

import torch

import _conv_oracle as O

_LIVE: list = []                                 # weak references to (flat buffer, payload elements)


def _pattern(dtype, device):
    return (torch.arange(O.BAND, device=device) % 119 + 1).to(dtype)


class Guard:
    def __enter__(self):
        self._empty, self._zeros = torch.empty, torch.zeros
        torch.empty, torch.zeros = self._alloc(False), self._alloc(True)
        return self

    def __exit__(self, et, ev, tb):
        torch.empty, torch.zeros = self._empty, self._zeros
        if et is None:
            check_bands()

    def _alloc(self, zero):
        real = self._zeros if zero else self._empty

        def alloc(*size, dtype=None, device=None, **kw):
            if kw or device is None or torch.device(device).type != "cuda":
                return real(*size, dtype=dtype, device=device, **kw)
            shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
            dtype = dtype or torch.get_default_dtype()
            n = math.prod(shape)
            flat = self._empty(n + 2 * O.BAND, dtype=dtype, device=device)
            flat[: O.BAND] = _pattern(dtype, device)
            flat[O.BAND + n:] = _pattern(dtype, device)
            mid = flat[O.BAND: O.BAND + n]
            mid.fill_(0 if zero or not dtype.is_floating_point else float("nan"))
            _LIVE.append((weakref.ref(flat), n))
            return mid.view(shape)

        return alloc


def check_bands():
    """After a launch: no band of any guarded buffer that is still in use has changed."""
    torch.cuda.synchronize()
    keep = []
    for ref, n in _LIVE:
        flat = ref()
        if flat is None:
            continue
        keep.append((ref, n))
        pat = _pattern(flat.dtype, flat.device)
        assert torch.equal(flat[: O.BAND], pat), f"a launch wrote in front of a {flat.dtype} buffer of {n}"
        assert torch.equal(flat[O.BAND + n:], pat), f"a launch wrote behind a {flat.dtype} buffer of {n}"
    _LIVE[:] = keep


def assert_guarded(out):
    """Every device tensor an entry point returned lives in a guarded buffer (an allocation that
    went past ``Guard`` -- ``empty_like``, ``new_empty``, C++ -- would have no bands to check)."""
    live = {f.untyped_storage().data_ptr() for f in (ref() for ref, _ in _LIVE) if f is not None}
    for t in (out if isinstance(out, (tuple, list)) else (out,)):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            assert t.untyped_storage().data_ptr() in live, f"an output of {tuple(t.shape)} was allocated outside the guard"


def launch(fn):
    """One entry-point call inside the guard bands."""
    with Guard():
        out = fn()
        assert_guarded(out)
    return out


class KeepGuard(Guard):
    """A ``Guard`` that also holds every tensor it hands out until it exits, so that scratch an
    entry point drops before it returns (partial-sum slabs, workspaces) still has its bands
    checked: ``check_bands`` skips a buffer whose last reference is gone."""

    def __enter__(self):
        self._held = []
        return super().__enter__()

    def __exit__(self, et, ev, tb):
        try:
            return super().__exit__(et, ev, tb)
        finally:
            self._held.clear()

    def _alloc(self, zero):
        inner = super()._alloc(zero)

        def alloc(*size, **kw):
            t = inner(*size, **kw)
            self._held.append(t)
            return t

        return alloc


def launch_kept(fn):
    """``launch`` under ``KeepGuard``: the bands of everything the call allocated are checked."""
    with KeepGuard():
        out = fn()
        assert_guarded(out)
    return out
