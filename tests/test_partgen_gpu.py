"""The part-carving kernel (``partgen.hip``) and what is built on it (``ops.partgen``,
``fn.generate_parts``, the ``voxel-seg`` dataset) on the GPU.

Every comparison is ``torch.equal`` against the torch oracle (``reference.carve_parts``, computed
on the CPU), each kernel result taken twice.  The kernel is called at binding level, with every
output a view into a larger buffer filled with ``FILL``: the ``GUARD`` bytes on both sides must
come back untouched.  Shapes are built round ``partgen_chunk()`` = 2,048 voxels per workgroup:
8^3 puts four parts into one workgroup, 16^3 two workgroups into a part, 24^3 = 6.75 chunks makes
workgroups straddle parts, and the last workgroup of an odd batch is half empty.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _partgen_cases import S, border_features, expected_components, single_features, single_features_tight, table, unused  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.ops import partgen, reference  # noqa: E402
from featurenet_amd.training.data import load_dataset, voxel_seg_dataset  # noqa: E402

DEV = "cuda"
GUARD, FILL = 64, 0xA5
OUTPUTS = ("occ", "packed", "labels", "slots")


def test_chunk():
    assert _native.kernels().partgen_chunk() == 2048         # the shapes of this file are built round it
    assert 24 ** 3 % 2048 != 0 and 8 ** 3 * 4 == 2048


def launch(params: torch.Tensor, size: int, want=OUTPUTS, stream=None):
    """One ``partgen_carve`` call -> {name: uint8 tensor on the device}; outputs not in ``want`` get
    a null pointer.  Checks the guard bytes round every output."""
    N, K, _ = params.shape
    V = size ** 3
    p = params.to(DEV).contiguous()
    numel = {"occ": N * V, "packed": N * V // 8, "labels": N * V, "slots": N * V}
    bufs = {name: torch.full((numel[name] + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV) for name in want}
    views = {name: b[GUARD:GUARD + numel[name]] for name, b in bufs.items()}
    ptr = [views[name].data_ptr() if name in want else 0 for name in OUTPUTS]
    ext = [p.numel()] + [numel[name] if name in want else 0 for name in OUTPUTS]
    st = stream.cuda_stream if stream is not None else _native.stream(p)
    _native.kernels().partgen_carve(p.data_ptr(), *ptr, N, K, size, st, ext)
    if stream is not None:
        ev = torch.cuda.Event()
        ev.record(stream)
        torch.cuda.current_stream().wait_event(ev)
    for name, b in bufs.items():
        assert bool((b[:GUARD] == FILL).all()) and bool((b[GUARD + numel[name]:] == FILL).all()), f"{name}: guard bytes"
    return views


def pack(occ: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(np.packbits(occ.numpy().reshape(-1), bitorder="little"))


def check(params: torch.Tensor, size: int, oracle=None, nulls: bool = False):
    occ, labels, slots = oracle if oracle is not None else reference.carve_parts(params, size)
    want = {"occ": occ.reshape(-1), "packed": pack(occ), "labels": labels.reshape(-1), "slots": slots.reshape(-1)}
    got, again = launch(params, size), launch(params, size)
    torch.cuda.synchronize()
    for name in OUTPUTS:
        assert torch.equal(got[name].cpu(), want[name]), (name, int((got[name].cpu() != want[name]).sum()))
        assert torch.equal(got[name], again[name]), (name, "second run differs")
    if nulls:
        for name in OUTPUTS:                         # each pointer null in turn, and each output alone
            rest = tuple(o for o in OUTPUTS if o != name)
            for some in (rest, (name,)):
                part = launch(params, size, want=some)
                for o in some:
                    assert torch.equal(part[o].cpu(), want[o]), (some, o)


def test_every_class_in_every_orientation():
    params, want = single_features()
    check(params, S, want, nulls=True)
    tight, _ = single_features_tight()               # exact boxes: the skips change nothing
    check(tight, S, want)


@pytest.mark.parametrize("separate", [True, False], ids=["separate", "overlapping"])
@pytest.mark.parametrize("N", [1, 3, 5])
@pytest.mark.parametrize("size", [8, 24, 64])
def test_sampler_tables(size, N, separate):
    params = partgen.sample(N, size, 11 * size + N, (1, 6), separate=separate)
    assert params.shape == (N, 6, 16)
    check(params, size)


@pytest.mark.parametrize("size,N,K", [(40, 2, 4), (256, 1, 2)], ids=["40", "largest"])
def test_other_sizes(size, N, K):
    """A size that is no power of two and the largest one (the kernel divides by multiplying)."""
    check(partgen.sample(N, size, 6, (K, K), separate=False), size)


@pytest.mark.parametrize("size", [8, 16, 24])
def test_empty_tables(size):
    for N in (1, 5):
        for params in (torch.zeros(N, 0, 16, dtype=torch.int32), table([[unused()] * 6] * N)):
            out = launch(params, size)
            assert bool((out["occ"] == 1).all()) and bool((out["packed"] == 0xFF).all())
            assert not out["labels"].any() and not out["slots"].any()
    assert launch(torch.zeros(0, 4, 16, dtype=torch.int32), size)["occ"].numel() == 0


def test_full_tables_and_the_lowest_slot():
    """K = 32 overlapping features per part at 8^3 (four parts per workgroup, five parts: the last
    workgroup holds one) and at 24^3."""
    for size, N in ((8, 5), (24, 2)):
        params = partgen.sample(N, size, 3, (32, 32), separate=False)
        assert bool((params[..., 0] >= 0).all())
        check(params, size)
        swapped = params.flip(1).contiguous()
        check(swapped, size)


def test_border_features():
    params, want = border_features()
    check(params, S, want, nulls=True)


def test_side_stream():
    params = partgen.sample(3, 24, 1, (2, 6), separate=False)
    occ, labels, slots = reference.carve_parts(params, 24)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = launch(params, 24, stream=side)            # (launch makes the current stream wait for it)
    assert torch.equal(got["labels"].cpu(), labels.reshape(-1)) and torch.equal(got["occ"].cpu(), occ.reshape(-1))
    with torch.cuda.stream(side):
        vox, lab, slo = partgen.carve(params, 24, device=DEV, want_slots=True)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(lab.cpu(), labels) and torch.equal(vox.cpu(), occ) and torch.equal(slo.cpu(), slots)


def test_unsupported_arguments_are_refused():
    K_ = _native.kernels()
    params = partgen.sample(1, 16, 0, (1, 4)).to(DEV)
    out = torch.zeros(16 ** 3 + 8, dtype=torch.uint8, device=DEV)
    st = _native.stream(params)
    ext = [params.numel(), 16 ** 3, 0, 0, 0]
    for size, K in ((12, 4), (4, 4), (264, 4), (16, 33), (16, -1)):
        with pytest.raises(RuntimeError, match="unsupported configuration|geometry needs"):
            K_.partgen_carve(params.data_ptr(), out.data_ptr(), 0, 0, 0, 1, K, size, st, [])
    with pytest.raises(RuntimeError, match="unsupported configuration"):     # a misaligned byte volume
        K_.partgen_carve(params.data_ptr(), out.data_ptr() + 4, 0, 0, 0, 1, 4, 16, st, ext)
    with pytest.raises(RuntimeError, match="occ has 4095 elements"):
        K_.partgen_carve(params.data_ptr(), out.data_ptr(), 0, 0, 0, 1, 4, 16, st, [params.numel(), 4095, 0, 0, 0])
    with pytest.raises(RuntimeError, match="params has 63 elements"):
        K_.partgen_carve(params.data_ptr(), out.data_ptr(), 0, 0, 0, 1, 4, 16, st, [63, 4096, 0, 0, 0])
    with pytest.raises(RuntimeError, match="packed has 511 elements"):
        K_.partgen_carve(params.data_ptr(), 0, out.data_ptr(), 0, 0, 1, 4, 16, st, [64, 0, 511, 0, 0])
    torch.cuda.synchronize()
    assert not out.any()
    with pytest.raises(ValueError, match="cls"):
        partgen.carve(table([[[24] + [0] * 15]]), 16, device=DEV)
    with pytest.raises(ValueError, match="multiple of 8"):
        partgen.carve(params, 20)


# ---------------------------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------------------------
class _Recorder:
    """Forwards to the real ``_C`` and records the entry points called."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


def test_generate_parts_is_the_same_on_both_devices(monkeypatch):
    rec = _Recorder(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    for kw in (dict(size=64, features=(1, 4)), dict(size=24, features=(2, 6), separate=False)):
        gpu = fn.generate_parts(5, seed=8, device=DEV, return_slots=True, **kw)
        assert rec.calls == ["partgen_carve"], rec.calls
        rec.calls.clear()
        cpu = fn.generate_parts(5, seed=8, device="cpu", return_slots=True, **kw)
        assert rec.calls == []
        assert gpu[2] == cpu[2] and len(gpu[2]) == 5
        for g, c in zip((gpu[0], gpu[1], gpu[3]), (cpu[0], cpu[1], cpu[3])):
            assert g.dtype == np.uint8 and g.shape == (5,) + (kw["size"],) * 3 and np.array_equal(g, c)
    bits, labels = partgen.carve(partgen.sample(3, 24, 2), 24, device=DEV, packed=True)
    vox, labels2 = partgen.carve(partgen.sample(3, 24, 2), 24, device="cpu", packed=True)
    assert bits.is_cuda and bits.shape == (3, 24 ** 3 // 8) and torch.equal(bits.cpu(), vox)
    assert torch.equal(labels.cpu(), labels2)


def test_voxel_seg_dataset_lives_on_the_device():
    ds = load_dataset("voxel-seg", synthetic_sizes=(60, 20), seed=4)
    assert ds.name == "voxel-seg" and ds.num_classes == 25 and ds.input_shape == (64, 64, 64, 1)
    for x, y, n in ((ds.x_train, ds.y_train, 6), (ds.x_test, ds.y_test, 2)):
        assert x.is_cuda and y.is_cuda and x.dtype == torch.uint8 and y.dtype == torch.uint8
        assert x.shape == (n, 64, 64, 64, 1) and y.shape == (n, 64, 64, 64)
    assert torch.equal(ds.y_test.cpu(), reference.carve_parts(ds.meta["params_test"], 64)[1])
    assert torch.equal(ds.x_test[..., 0] == 0, ds.y_test != 0)
    assert load_dataset("voxel-seg", synthetic_sizes=(60, 20), seed=4) is ds


def test_instances_of_the_labels_are_the_features():
    params = partgen.sample(8, 64, 21, (2, 4))
    _, labels = partgen.carve(params, 64, device=DEV)
    ids, inst = fn.label_components(labels, device=DEV)
    assert [len(i) for i in inst] == expected_components(params).tolist()
    for n in range(8):
        want = sorted(c + 1 for c in params[n, :, 0].tolist() if c >= 0 for _ in range(2 if c == 16 else 1))
        assert sorted(i.cls for i in inst[n]) == want
    assert int(ids.max()) == int(expected_components(params).max())


def test_training_on_generated_parts():
    ds = voxel_seg_dataset(64, 16, size=16, features=(1, 3), seed=1)
    assert ds.x_train.is_cuda
    res = fn.train("segmentation", data=ds, epochs=3, batch_size=16, verbose=0)
    losses = res.history["loss"]
    assert len(losses) == 3 and all(np.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    score = fn.evaluate_features(res.model, ds.x_test, ds.y_test, batch_size=8, device=DEV)
    assert len(score.matches) == 16 and int(score.tp.sum() + score.fn.sum()) > 0
