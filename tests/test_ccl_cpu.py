"""Connected components and the instance table on the CPU path: the oracle (``ops.reference``)
against ``scipy.ndimage.label`` and closed-form patterns, the record type, ``fn.label_components``,
``fn.extract_features``, the CLI, and the Python <-> ``_C`` plumbing of ``ops.ccl``.  Everything is
an exact integer comparison."""
import json
import re

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from _ccl_cases import closed_form_table, serpentine_mask
from featurenet_amd import _native
from featurenet_amd.models.featurenet3d import FeatureNet3D, FeatureNet3DConfig, FeatureNet3DSeg
from featurenet_amd.ops import ccl, reference
from featurenet_amd.utils.seginstances import FeatureInstance

S, NC = 16, 5


def cc(v, background=0, connectivity=6):
    lab = torch.as_tensor(np.asarray(v, dtype=np.uint8))
    roots = ccl.connected_components(lab, background, connectivity)
    return lab, roots, ccl.instance_table(lab, roots)


# --- the oracle against SciPy ----------------------------------------------------------------------
def scipy_roots(lab: np.ndarray, background, connectivity: int) -> np.ndarray:
    """Label class by class, then map SciPy's labels to 1 + the index of their first voxel."""
    ndimage = pytest.importorskip("scipy.ndimage")
    st = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    out = np.zeros(lab.shape, np.int32)
    for n in range(lab.shape[0]):
        flat_out = out[n].reshape(-1)
        for c in np.unique(lab[n]):
            if background is not None and c == background:
                continue
            comp, k = ndimage.label(lab[n] == c, structure=st)
            flat = comp.reshape(-1)
            first = np.zeros(k + 1, np.int64)
            first[flat[::-1]] = np.arange(flat.size)[::-1]           # (the last write is the first voxel)
            flat_out[flat > 0] = first[flat[flat > 0]] + 1
            # ids in ascending root order are SciPy's own numbering
            assert np.array_equal(np.argsort(first[1:]), np.arange(k))
    return out


@pytest.mark.parametrize("background", [0, None], ids=["bg0", "nobg"])
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (2, 20, 9, 33), (1, 16, 16, 16)], ids=str)
def test_oracle_against_scipy(shape, connectivity, background):
    pytest.importorskip("scipy")
    g = torch.Generator().manual_seed(sum(shape) + connectivity)
    for classes in (2, 4):
        lab = torch.randint(0, classes, shape, generator=g, dtype=torch.uint8)
        roots = reference.connected_components(lab, background, connectivity)
        assert roots.dtype == torch.int32 and roots.shape == lab.shape
        assert np.array_equal(roots.numpy(), scipy_roots(lab.numpy(), background, connectivity))


# --- closed-form patterns ---------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_empty_volume_has_no_rows(connectivity):
    lab, roots, (ids, table, offsets) = cc(np.zeros((2, 4, 5, 6)), 0, connectivity)
    assert not roots.any() and not ids.any()
    assert table.shape == (0, 13) and table.dtype == torch.int64 and offsets.tolist() == [0, 0, 0]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_solid_volume_is_one_row(connectivity):
    D, H, W = 4, 5, 6
    n = D * H * W
    lab, roots, (ids, table, offsets) = cc(np.full((1, D, H, W), 9), 0, connectivity)
    assert torch.all(roots == 1) and torch.all(ids == 1) and offsets.tolist() == [0, 1]
    want = [0, 9, n, 1, 0, 0, 0, D - 1, H - 1, W - 1,
            D * (D - 1) // 2 * H * W, H * (H - 1) // 2 * D * W, W * (W - 1) // 2 * D * H]
    assert table.tolist() == [want]


def test_checkerboard():
    D, H, W = 4, 5, 6
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    v = (1 + (z + y + x) % 2)[None]
    lab, roots, (ids, table, offsets) = cc(v, 0, 6)                 # every voxel on its own
    assert torch.equal(roots.reshape(-1), torch.arange(1, D * H * W + 1, dtype=torch.int32))
    assert torch.equal(ids, roots) and table.shape[0] == D * H * W and torch.all(table[:, 2] == 1)
    lab, roots, (ids, table, offsets) = cc(v, 0, 26)                # the two colours
    assert table.shape[0] == 2 and table[:, 1].tolist() == [1, 2] and table[:, 3].tolist() == [1, 2]
    assert table[:, 2].tolist() == [D * H * W // 2] * 2
    assert torch.equal(roots, torch.as_tensor(v.astype(np.int32))) and torch.equal(ids, roots)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_serpentine_is_one_component_rooted_at_its_first_voxel(connectivity):
    D, H, W = 5, 9, 7
    m = serpentine_mask(D, H, W)
    assert m[0, 0, 0] and 0.25 < m.mean() < 0.5
    lab, roots, (ids, table, offsets) = cc(m[None], 0, connectivity)
    assert np.array_equal(roots[0].numpy(), m.astype(np.int32)) and np.array_equal(ids[0].numpy(), m.astype(np.int32))
    assert np.array_equal(table.numpy(), closed_form_table(m, 0, 1)[None])


@pytest.mark.parametrize("connectivity", [6, 26])
def test_components_do_not_cross_samples_or_wrap(connectivity):
    D, H, W = 3, 4, 5
    v = np.zeros((2, D, H, W), np.uint8)
    v[0, D - 1] = 3                                                 # facing end planes of two samples
    v[1, 0] = 3
    lab, roots, (ids, table, offsets) = cc(v, 0, connectivity)
    assert offsets.tolist() == [0, 1, 2] and table[:, 0].tolist() == [0, 1]
    assert table[:, 3].tolist() == [(D - 1) * H * W + 1, 1] and table[:, 2].tolist() == [H * W, H * W]
    v = np.zeros((1, D, H, W), np.uint8)
    v[0, 0, 0, W - 1] = v[0, 0, 1, 0] = 2                           # end of a row, start of the next
    v[0, 0, H - 1, W - 1] = v[0, 1, 0, 0] = 4                       # end of a plane, start of the next
    lab, roots, (ids, table, offsets) = cc(v, 0, connectivity)
    assert table[:, 1].tolist() == [2, 2, 4, 4] and table[:, 2].tolist() == [1, 1, 1, 1]
    assert table[:, 3].tolist() == [W, W + 1, H * W, H * W + 1]


def test_class_255_and_no_background():
    v = np.zeros((1, 2, 3, 4), np.uint8)
    v[0, 1, 1:, 2:] = 255
    lab, roots, (ids, table, offsets) = cc(v, None, 6)
    assert table[:, 1].tolist() == [0, 255] and table[:, 2].tolist() == [20, 4]
    assert int((roots == 0).sum()) == 0
    lab, roots, (ids, table, offsets) = cc(v, 255, 6)               # 255 as the background
    assert table[:, 1].tolist() == [0] and int((roots == 0).sum()) == 4


def test_table_columns_ordering_and_offsets():
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, 3, (3, 5, 6, 7), generator=g, dtype=torch.uint8)
    lab[1] = 0                                                      # a sample without instances
    roots = ccl.connected_components(lab, 0, 6)
    ids, table, offsets = ccl.instance_table(lab, roots)
    none, table2, offsets2 = ccl.instance_table(lab, roots, want_ids=False)
    assert none is None and torch.equal(table, table2) and torch.equal(offsets, offsets2)
    assert offsets.dtype == torch.int64 and offsets[0] == 0 and offsets[1] == offsets[2] and offsets[-1] == len(table)
    key = table[:, 0] * lab[0].numel() + table[:, 3]
    assert torch.all(key[1:] > key[:-1])                            # sorted by (sample, root), no duplicates
    assert int(table[:, 2].sum()) == int((lab != 0).sum())
    lab_n, ids_n = lab.numpy(), ids.numpy()
    for k, row in enumerate(table.tolist()):                        # every row from its voxels
        n = row[0]
        mask = ids_n[n] == k - int(offsets[n]) + 1
        assert row == closed_form_table(mask, n, int(lab_n[n][mask][0])).tolist()
        assert len(np.unique(lab_n[n][mask])) == 1
    with pytest.raises(ValueError):
        ccl.instance_table(lab, roots.to(torch.int64))


def test_records_min_voxels_and_to_dict():
    v = np.zeros((2, 3, 4, 5), np.uint8)
    v[0, 0, 0, :3] = 1
    v[0, 2, 3, 4] = 2
    v[1, 1, 1:3, 1:4] = 4
    lab, roots, (ids, table, offsets) = cc(v)
    feats = FeatureInstance.from_table(table, offsets)
    assert [len(f) for f in feats] == [2, 1]
    a, b = feats[0]
    assert a == FeatureInstance(id=1, cls=1, voxels=3, bbox=(0, 0, 0, 0, 0, 2), centroid=(0.0, 0.0, 1.0))
    assert b.id == 2 and b.cls == 2 and b.bbox == (2, 3, 4, 2, 3, 4) and b.centroid == (2.0, 3.0, 4.0)
    c = feats[1][0]
    assert c.voxels == 6 and c.bbox == (1, 1, 1, 1, 2, 3) and c.centroid == (1.0, 1.5, 2.0)
    big = FeatureInstance.from_table(table.numpy(), offsets.numpy(), min_voxels=3)
    assert [[f.id for f in fs] for fs in big] == [[1], [1]]         # the survivors keep their ids
    d = c.to_dict()
    assert d == {"id": 1, "class": 4, "voxels": 6, "bbox": [1, 1, 1, 1, 2, 3], "centroid": [1.0, 1.5, 2.0]}
    assert json.loads(json.dumps(d)) == d


# --- public API on the CPU path ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg():
    torch.manual_seed(0)
    m = FeatureNet3DSeg(S, num_classes=NC).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for c in list(m.enc) + [m.dec]:
            c.running_mean.copy_(torch.randn(c.cout, generator=g) * 0.1)
            c.running_var.copy_(torch.rand(c.cout, generator=g) + 0.5)
        m.head.bias.copy_(torch.randn(NC, generator=g) * 0.1)
    x = torch.rand(3, S, S, S, generator=g) < 0.4
    return m, x


def test_label_components():
    g = torch.Generator().manual_seed(5)
    lab = torch.randint(0, 3, (2, 6, 7, 8), generator=g)
    ids, feats = fn.label_components(lab.numpy().astype(np.int32), connectivity=26, device="cpu")
    roots = reference.connected_components(lab.to(torch.uint8), 0, 26)
    want_ids, table, offsets = reference.instance_table(lab.to(torch.uint8), roots)
    assert ids.dtype == np.int32 and np.array_equal(ids, want_ids.numpy())
    assert feats == FeatureInstance.from_table(table, offsets)
    ids2, feats2 = fn.label_components(lab.to(torch.uint8), background=None, device="cpu")
    assert (ids2 > 0).all() and sum(f.voxels for fs in feats2 for f in fs) == lab.numel()


def test_extract_features_end_to_end(seg, tmp_path):
    m, x = seg
    labels, _ = fn.segment(m, x.numpy().astype(np.uint8), device="cpu")
    assert len(np.unique(labels)) > 1
    want_ids, want = fn.label_components(labels, device="cpu")
    feats, ids = fn.extract_features(m, x.numpy().astype(np.uint8), batch_size=2, device="cpu", return_ids=True)
    assert feats == want and ids.dtype == np.int32 and np.array_equal(ids, want_ids)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    packed = np.packbits(x.numpy().reshape(len(x), -1), axis=1, bitorder="little")
    feats2, none = fn.extract_features(str(path), packed, device="cpu", packed_size=S, min_voxels=4)
    assert none is None
    assert feats2 == [[f for f in fs if f.voxels >= 4] for fs in want]
    table, offsets, no_ids = m.instances(x[:1].float(), background=None, connectivity=26)
    assert no_ids is None and int(table[:, 2].sum()) == S ** 3 and offsets.tolist() == [0, len(table)]


def test_cli_features(seg, tmp_path, capsys):
    from featurenet_amd.cli import main

    m, x = seg
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": NC})
    np.save(tmp_path / "x.npy", x.numpy().astype(np.uint8))
    out, idf = tmp_path / "features.json", tmp_path / "ids.npy"
    assert main(["features", str(path), str(tmp_path / "x.npy"), "--json", str(out), "--ids", str(idf),
                 "--connectivity", "26", "--min-voxels", "2"]) == 0
    doc = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert doc == json.loads(out.read_text()) and len(doc["samples"]) == len(x)
    ids = np.load(idf)
    assert ids.shape == (len(x), S, S, S) and ids.dtype == np.int32
    for n, recs in enumerate(doc["samples"]):
        for r in recs:
            assert r["voxels"] >= 2 and r["voxels"] == int((ids[n] == r["id"]).sum())
    if not torch.cuda.is_available():                    # (the checkpoint loads onto the GPU when there is one)
        feats, _ = fn.extract_features(m, x.numpy().astype(np.uint8), device="cpu", connectivity=26, min_voxels=2)
        assert doc["samples"] == [[f.to_dict() for f in fs] for fs in feats]


def test_error_cases(seg):
    m, x = seg
    clf = FeatureNet3D(FeatureNet3DConfig.tiny())
    with pytest.raises(ValueError, match="FeatureNet3DSeg"):
        fn.extract_features(clf, np.zeros((1, 16, 16, 16), np.float32))
    lab = torch.zeros(1, 4, 4, 4, dtype=torch.uint8)
    for call in (lambda: ccl.connected_components(lab, 0, 18), lambda: reference.connected_components(lab, 0, 18),
                 lambda: fn.label_components(lab, connectivity=18, device="cpu"),
                 lambda: fn.extract_features(m, x, connectivity=18, device="cpu"),
                 lambda: m.instances(x.float(), connectivity=18)):
        with pytest.raises(ValueError, match="connectivity"):
            call()
    with pytest.raises(ValueError):
        ccl.connected_components(lab.float())
    with pytest.raises(ValueError, match="integers"):
        fn.label_components(np.zeros((1, 4, 4, 4), np.float32), device="cpu")
    with pytest.raises(ValueError, match="0..255"):
        fn.label_components(np.full((1, 4, 4, 4), 256), device="cpu")
    assert "extract_features" in fn.__all__ and "label_components" in fn.__all__
    assert callable(fn.extract_features) and callable(fn.label_components)


# --- Python <-> _C plumbing (the technique of tests/test_native_abi.py) -----------------------------
def _arity(fn_) -> tuple[int, int]:
    sig = fn_.__doc__.split("\n")[0]
    inner = sig[sig.index("(") + 1:sig.rindex(") ->")]
    depth, parts, cur = 0, [], ""
    for ch in inner:
        depth += ch in "[(" and 1 or 0
        depth -= ch in "])" and 1 or 0
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur)
    return sum("=" not in p for p in parts), len(parts)


class _FakeK:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        lo, hi = _arity(getattr(self.real, name))

        def f(*args):
            assert lo <= len(args) <= hi, f"{name}: called with {len(args)} args, binding takes {lo}..{hi}"
            self.calls.append((name, args))
        return f


def test_ccl_calls_match_bindings(monkeypatch):
    if not _native.kernels_available():
        pytest.skip("_C not built")
    assert len(_native.kernels().ccl_tile()) == 3
    fk = _FakeK(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: fk)
    monkeypatch.setattr(_native, "stream", lambda t=None: 0)
    monkeypatch.setattr(_native, "use_native", lambda t: True)
    lab = torch.zeros(2, 3, 4, 5, dtype=torch.uint8)
    roots, flags = ccl.connected_components(lab, None, 26, return_flags=True)
    assert roots.dtype == torch.int32 and roots.shape == lab.shape and flags.shape == lab.shape
    zeros = torch.zeros_like(roots)
    ids, table, offsets = ccl.instance_table(lab, zeros, want_ids=False, flags=zeros)
    assert ids is None and table.shape == (0, 13) and offsets.tolist() == [0, 0, 0]
    assert [n for n, _ in fk.calls] == ["ccl_local", "ccl_merge", "ccl_flatten", "ccl_stats"]
    a = fk.calls[0][1]                                    # labels roots N D H W background connectivity st ext
    assert a[0] == lab.data_ptr() and a[1] == roots.data_ptr() and a[2:8] == (2, 3, 4, 5, -1, 26)
    assert a[-1] == [120, 120]
    assert fk.calls[1][1][:8] == a[:8]
    f = fk.calls[2][1]                                    # roots flags N D H W st ext
    assert f[0] == roots.data_ptr() and f[1] == flags.data_ptr() and f[2:6] == (2, 3, 4, 5) and f[-1] == [120, 120]
    s = fk.calls[3][1]                                    # labels roots rank ids table N D H W T st ext
    assert s[3] == 0 and s[5:10] == (2, 3, 4, 5, 0) and s[-1] == [120, 120, 120, 0, 0]
    ccl.connected_components(lab, 7, 6)
    assert fk.calls[4][1][6:8] == (7, 6)


def test_ccl_extent_checks():
    """bind.cpp checks the operand extents before any HIP call."""
    if not _native.kernels_available():
        pytest.skip("_C not built")
    K = _native.kernels()
    n = 2 * 3 * 4 * 5
    with pytest.raises(RuntimeError, match="roots has"):
        K.ccl_local(16, 16, 2, 3, 4, 5, 0, 6, 0, [n, n - 1])
    with pytest.raises(RuntimeError, match="labels has"):
        K.ccl_local(16, 16, 2, 3, 4, 5, 0, 6, 0, [n - 1, n])
    with pytest.raises(RuntimeError, match="roots has"):
        K.ccl_merge(16, 16, 2, 3, 4, 5, 0, 26, 0, [n, n - 1])
    with pytest.raises(RuntimeError, match="flags has"):
        K.ccl_flatten(16, 16, 2, 3, 4, 5, 0, [n, n - 1])
    for i, name in ((0, "labels"), (1, "roots"), (2, "rank"), (3, "ids"), (4, "table")):
        ext = [n, n, n, n, 7 * 13]
        ext[i] -= 1
        with pytest.raises(RuntimeError, match=f"{name} has"):
            K.ccl_stats(16, 16, 16, 16, 16, 2, 3, 4, 5, 7, 0, ext)
    # arguments the kernels do not take are refused before any launch
    for bad in (dict(connectivity=18), dict(background=256), dict(D=0)):
        a = dict(N=2, D=3, H=4, W=5, background=0, connectivity=6)
        a.update(bad)
        with pytest.raises(RuntimeError, match=re.compile("unsupported configuration|elements")):
            K.ccl_local(16, 16, a["N"], a["D"], a["H"], a["W"], a["background"], a["connectivity"], 0, [n, n])
