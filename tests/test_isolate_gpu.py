"""The instance-isolation kernel (``isolate.hip``) and the paths built on it (``ops.isolate``, ``fn.isolate_features``,
``fn.recognize``, the ``classifier`` option of ``fn.extract_features``) on the GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``ops.reference.isolate_instances``, which
``test_isolate_cpu.py`` holds against a per-voxel loop).  The kernel is called through the raw binding on buffers
pre-filled with a sentinel and with a guard region behind them, twice with two sentinels: an output equal to the
oracle under both was written in full."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _ccl_cases import PATTERNS, volume  # noqa: E402
from _isolate_cases import SHAPES, generator_parts, grid_window, inner_window, random_ids  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3D, FeatureNet3DConfig, FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import isolate, reference  # noqa: E402

DEV = "cuda"
GUARD = 256
ELEM = {0: torch.uint8, 1: torch.uint8, 2: torch.bfloat16}


def out_bytes(M: int, S: int, fmt: int) -> int:
    return M * S ** 3 // 8 if fmt == 0 else M * S ** 3 * (2 if fmt == 2 else 1)


def run_binding(ids: torch.Tensor, sel: torch.Tensor, S: int, fmt: int, sentinel: int = 0xA5) -> torch.Tensor:
    """``isolate_parts`` on a buffer pre-filled with ``sentinel`` with a guard region behind the live part ->
    the live part as the format's tensor; asserts that the guard was not touched."""
    N, D, H, W = ids.shape
    M = sel.shape[0]
    nb = out_bytes(M, S, fmt)
    buf = torch.full((nb + GUARD,), sentinel, dtype=torch.uint8, device=DEV)
    _native.kernels().isolate_parts(ids.data_ptr(), sel.data_ptr(), buf.data_ptr(), N, D, H, W, M, S, fmt,
                                    _native.stream(ids), [ids.numel(), sel.numel(), nb // (2 if fmt == 2 else 1)])
    torch.cuda.synchronize()
    assert bool((buf[nb:] == sentinel).all()), "the guard region was written"
    out = buf[:nb].view(ELEM[fmt])
    return out.view({0: (M, S ** 3 // 8), 1: (M, S, S, S), 2: (M, S, S, S, 1)}[fmt])


def check(ids_c: torch.Tensor, sel_c: torch.Tensor, S: int, what) -> None:
    """All three formats of the kernel against the oracle of the same call."""
    want = {1: reference.isolate_instances(ids_c, sel_c, S, 1)}
    weights = 1 << torch.arange(8, dtype=torch.int32)
    want[0] = (want[1].reshape(len(sel_c), S ** 3 // 8, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8)
    want[2] = want[1].to(torch.bfloat16).unsqueeze(-1)
    ids, sel = ids_c.to(DEV), sel_c.to(DEV)
    for fmt in (0, 1, 2):
        for sentinel in (0xA5, 0x5A):
            got = run_binding(ids, sel, S, fmt, sentinel)
            assert torch.equal(got.cpu(), want[fmt]), (what, fmt, sentinel, int((got.cpu() != want[fmt]).sum()))
        op = isolate.isolate_instances(ids, sel, S, fmt)             # the op layer takes the same kernel
        assert op.is_cuda and op.dtype == want[fmt].dtype and torch.equal(op.cpu(), want[fmt]), (what, fmt, "op")


def make_sel(ids: torch.Tensor, window, boxes: str, per_sample: int = 2) -> torch.Tensor:
    """Rows for up to ``per_sample`` of the ids that occur in each sample, with their true boxes (``true``), the
    whole grid and beyond (``wide``) or the true box cut in half along x (``half``), one row per sample for an
    id that no voxel carries, and the first two rows again."""
    N, D, H, W = ids.shape
    rows = []
    for n in range(N):
        vol = ids[n].numpy()
        present = [int(v) for v in np.unique(vol) if v > 0]
        for i in present[:per_sample]:
            z, y, x = np.nonzero(vol == i)
            box = [z.min(), y.min(), x.min(), z.max(), y.max(), x.max()]
            if boxes == "wide":
                box = [-3, 0, 0, 255, 300, W - 1]
            elif boxes == "half":
                box[5] = (box[2] + box[5]) // 2
            rows.append([n, i, *(int(b) for b in box), *window])
        rows.append([n, (present[-1] if present else 0) + 1, 0, 0, 0, D - 1, H - 1, W - 1, *window])
    return torch.tensor(rows + rows[:2], dtype=torch.int32).reshape(-1, 14)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"{s}-to-{z}" for s, z, _ in SHAPES])
def test_kernel_against_the_oracle(si, N):
    shape, S, _ = SHAPES[si]
    big = max(shape[0] * shape[1] * shape[2], S ** 3) > 1 << 15      # (fewer sources: the oracle is the slow side)
    sources = [(p, volume(p, N, *shape).to(torch.int32)) for p in (("blobs", "noise4", "solid", "wrap") if big else PATTERNS)]
    rnd = random_ids(N, *shape).clone()
    if N > 1:
        rnd[1] = 0                                           # one sample without any instance
    sources.append(("random", rnd))
    for name, ids in sources:
        for boxes in ("true", "wide", "half"):
            if big and boxes != "true" and name not in ("blobs", "random"):
                continue
            sel = make_sel(ids, grid_window(shape), boxes)
            check(ids, sel, S, (name, shape, S, N, boxes))
    none = torch.zeros(0, 14, dtype=torch.int32)
    check(sources[0][1], none, S, ("M = 0", shape, S, N))


@pytest.mark.parametrize("shape,S", [((16, 16, 16), 8), ((5, 12, 9), 8), ((20, 24, 28), 16), ((3, 5, 130), 72)])
def test_a_window_strictly_inside_the_grid(shape, S):
    ids = random_ids(2, *shape)
    win = inner_window(shape)
    for boxes in ("true", "half"):
        check(ids, make_sel(ids, win, boxes), S, ("inner window", shape, S, boxes))


def test_identity_windows_with_an_offset():
    """A window of S voxels on every axis maps voxel to voxel wherever it lies: with ``wx0 % 4 == 0`` through the
    16-byte loads, else (and with an ids pointer off the 16-byte grid) through the gathers."""
    shape, S = (20, 24, 28), 16
    ids = random_ids(2, *shape)
    for w0 in ((4, 8, 4), (1, 3, 5), (4, 8, 12), (0, 0, 0)):
        sel = make_sel(ids, [*w0, S, S, S], "true")
        check(ids, sel, S, ("identity at", w0))
        part = reference.isolate_instances(ids, sel[:1], S, 1)[0]
        n, i = sel[0, 0], sel[0, 1]
        assert torch.equal(part, (ids[n, w0[0]:w0[0] + S, w0[1]:w0[1] + S, w0[2]:w0[2] + S] != i).to(torch.uint8))
    cube = random_ids(2, 16, 16, 16)
    sel = make_sel(cube, grid_window((16, 16, 16)), "true")
    want = reference.isolate_instances(cube, sel, S, 1)
    buf = torch.zeros(cube.numel() + 1, dtype=torch.int32, device=DEV)
    buf[1:] = cube.reshape(-1).to(DEV)
    off = buf[1:].view(cube.shape)
    assert off.data_ptr() % 16 == 4
    assert torch.equal(run_binding(off, sel.to(DEV), S, 1).cpu(), want)


def test_rows_outside_the_grid_give_empty_parts_and_the_op_refuses_them():
    shape, S = (8, 8, 8), 8
    ids = random_ids(2, *shape)
    good = [0, 1, 0, 0, 0, 7, 7, 7, 0, 0, 0, 8, 8, 8]
    rows = [good]
    for col, bad in ((0, 2), (0, -1), (8, 1), (9, -1), (13, 9), (11, 0), (12, -3), (10, 2 ** 31 - 1), (13, 2 ** 31 - 1),
                     (8, -2 ** 31)):
        r = list(good)
        r[col] = bad
        rows.append(r)
    rows.append(good)
    sel = torch.tensor(rows, dtype=torch.int32)
    want = reference.isolate_instances(ids, sel[:1], S, 1)[0]
    for fmt in (0, 1, 2):
        got = run_binding(ids.to(DEV), sel.to(DEV), S, fmt).cpu()
        dense = got if fmt else ((got[..., None] >> torch.arange(8, dtype=torch.uint8)) & 1)
        dense = dense.reshape(len(rows), S, S, S).to(torch.uint8)
        assert torch.equal(dense[0], want) and torch.equal(dense[-1], want) and not bool(dense[1:-1].any()), fmt
    for r in rows[1:-1]:
        with pytest.raises(ValueError, match="outside the grid"):
            isolate.isolate_instances(ids.to(DEV), torch.tensor([good, r], dtype=torch.int32, device=DEV), S, 1)


def test_unsupported_arguments_are_refused():
    ids = torch.zeros(1, 8, 8, 8, dtype=torch.int32, device=DEV)
    sel = torch.tensor([[0, 1, 0, 0, 0, 7, 7, 7, 0, 0, 0, 8, 8, 8]], dtype=torch.int32, device=DEV)
    out = torch.zeros(8 ** 3 + 16, dtype=torch.uint8, device=DEV)
    K, st = _native.kernels(), _native.stream(ids)
    p = dict(ids=ids.data_ptr(), sel=sel.data_ptr(), out=out.data_ptr(), N=1, D=8, H=8, W=8, M=1, size=8, fmt=1, st=st,
             ext=[512, 14, 512])
    K.isolate_parts(**p)
    for bad in (dict(size=12, ext=[]), dict(size=0, ext=[]), dict(size=264, ext=[]), dict(fmt=3), dict(fmt=-1),
                dict(ids=0), dict(sel=0), dict(out=0), dict(out=out.data_ptr() + 4), dict(M=-1, ext=[]),
                dict(M=1 << 22, ext=[]), dict(D=0, ext=[]), dict(W=257, ext=[]), dict(N=0, ext=[])):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.isolate_parts(**{**p, **bad})
    with pytest.raises(RuntimeError, match="out has"):
        K.isolate_parts(**{**p, "M": 2, "ext": [512, 28, 512]})
    with pytest.raises(RuntimeError, match="sel has"):
        K.isolate_parts(**{**p, "M": 2, "ext": [512, 14, 1024]})
    with pytest.raises(RuntimeError, match="ids has"):
        K.isolate_parts(**{**p, "N": 2})
    with pytest.raises(ValueError, match="one device"):
        isolate.isolate_instances(ids, sel.cpu(), 8, 1)
    torch.cuda.synchronize()


def test_op_equals_the_cpu_path_on_generated_parts():
    S = 64
    slots, sel, want = generator_parts(S, n=4)
    assert len(sel) > 4
    for fmt in (0, 1, 2):
        cpu = isolate.isolate_instances(slots, sel, S, fmt)
        gpu = isolate.isolate_instances(slots.to(DEV), sel.to(DEV), S, fmt)
        assert gpu.is_cuda and torch.equal(gpu.cpu(), cpu), fmt
    assert torch.equal(isolate.isolate_instances(slots.to(DEV), sel.to(DEV), S, 1).cpu(), want)
    half = isolate.isolate_instances(slots.to(DEV), sel.to(DEV), 32, 1).cpu()      # 2 : 1, the nearest centre
    assert torch.equal(half, want[:, 1::2, 1::2, 1::2])
    win = isolate.material_window((slots == 0).to(torch.uint8).to(DEV))
    assert win.is_cuda and torch.equal(win.cpu(), isolate.material_window((slots == 0).to(torch.uint8)))


# ---------------------------------------------------------------------------------------------
# end to end on the device
# ---------------------------------------------------------------------------------------------
def classifier(cfg: FeatureNet3DConfig, seed: int = 0) -> FeatureNet3D:
    torch.manual_seed(seed)
    return FeatureNet3D(cfg).to(DEV).eval()


@pytest.mark.parametrize("cfg", [FeatureNet3DConfig.tiny(), FeatureNet3DConfig()], ids=["tiny-16", "default-64"])
def test_recognize_equals_isolate_plus_classify(cfg):
    S = cfg.input_size
    clf = classifier(cfg)
    vox, labels, _ = fn.generate_parts(2, size=S, seed=3, device=DEV)
    for bs in (256, 3):
        feats, ids, lab = fn.recognize(clf, vox, device=DEV, return_ids=True, return_labels=True, batch_size=bs)
        recs = [f for fs in feats for f in fs]
        assert len(recs) > 2 and not clf.training
        bits, index = fn.isolate_features(ids, packed=True, device=DEV)
        assert bits.shape == (len(recs), S ** 3 // 8)
        assert index.tolist() == [[n, f.id] for n, fs in enumerate(feats) for f in fs]
        want, p = fn.classify(clf, bits, batch_size=bs, packed_size=S)
        assert [f.recognized for f in recs] == want.tolist()
        assert [f.recognized_prob for f in recs] == [float(p[i, c]) for i, c in enumerate(want)]
        assert all(f.cls == f.recognized + 1 and f.agrees for f in recs)
        mapped = np.zeros_like(lab)
        for n, fs in enumerate(feats):
            for f in fs:
                mapped[n][ids[n] == f.id] = f.cls
        assert np.array_equal(lab, mapped) and np.array_equal(lab != 0, vox == 0)
    # separate=True parts: the components of the removed volume are those of the labels, on either device
    cpu_ids, cpu_feats = fn.label_components(labels, device="cpu")
    assert np.array_equal(cpu_ids, ids)
    assert [[(f.id, f.voxels, f.bbox) for f in fs] for fs in cpu_feats] == [[(f.id, f.voxels, f.bbox) for f in fs] for fs in feats]
    dense, _ = fn.isolate_features(ids, device=DEV)
    assert np.array_equal(dense, fn.isolate_features(ids, device="cpu")[0])
    assert np.array_equal(np.packbits(dense.reshape(len(dense), -1), axis=1, bitorder="little"), bits)
    _, truth = fn.label_components(labels, device=DEV, classifier=clf, batch_size=3)
    assert [[(t.id, t.recognized, t.recognized_prob) for t in ts] for ts in truth] == \
        [[(f.id, f.recognized, f.recognized_prob) for f in fs] for fs in feats]


def test_extract_features_with_a_classifier_keeps_every_other_field():
    S = 32
    torch.manual_seed(0)
    seg = FeatureNet3DSeg(S, num_classes=5).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                    # (BN folds that are not the identity: several classes)
        for c in list(seg.enc) + [seg.dec]:
            c.running_mean.copy_(torch.randn(c.cout, generator=g) * 0.1)
            c.running_var.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.gamma.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.beta.copy_(torch.randn(c.cout, generator=g) * 0.1)
        seg.head.bias.copy_(torch.randn(5, generator=g) * 0.1)
    seg = seg.to(DEV)
    clf = classifier(FeatureNet3DConfig.tiny())
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, S, S, S, generator=g) < 0.4).to(torch.uint8).numpy()
    kw = dict(batch_size=2, device=DEV, min_voxels=4, access=True, contacts=True)
    plain, _ = fn.extract_features(seg, x, **kw)
    both, ids = fn.extract_features(seg, x, return_ids=True, classifier=clf, **kw)
    recs = [f for fs in both for f in fs]
    assert len(recs) > 0 and all(f.recognized in (0, 1) and 0.5 <= f.recognized_prob <= 1 for f in recs)
    assert all(p.recognized is None for fs in plain for p in fs)
    for fs, ps in zip(both, plain):
        assert [{**f.__dict__, "recognized": None, "recognized_prob": None} for f in fs] == [p.__dict__ for p in ps]
    # the classifier sees each component resampled 32 -> 16, in the batches of its sample's model batch
    for lo in (0, 2):
        cut, index = fn.isolate_features(ids[lo:lo + 2], features=both[lo:lo + 2], size=16, device=DEV)
        want, p = fn.classify(clf, cut)
        got = [f for fs in both[lo:lo + 2] for f in fs]
        assert [f.recognized for f in got] == want.tolist()
        assert [f.recognized_prob for f in got] == [float(p[i, c]) for i, c in enumerate(want)]
