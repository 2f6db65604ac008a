"""The feature-contact kernel (``contact.hip``) and the paths built on it
(``FeatureNet3DSeg.instances(want_contacts=True)``, ``fn.extract_features(contacts=True)``,
``fn.label_components(contacts=True)``) on the GPU.

Every comparison is ``torch.equal`` against the CPU oracle (``ops.reference.contact_table``, which
``test_contact_cpu.py`` holds against a per-voxel loop).  The shapes put a row under one wave, on exactly one
wave, one lane over, and on two 64-wide pieces plus a remainder; the largest one also spans two workgroups'
chunks of the flat voxel range, the first ending mid-row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featurenet_amd as fn  # noqa: E402
from _access_cases import occupancy, singles  # noqa: E402
from _ccl_cases import PATTERNS  # noqa: E402
from _contact_cases import check_identities, expected_contacts  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import contact, reference  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 1, 1), (1, 1, 64), (3, 5, 7), (4, 6, 64), (5, 3, 65), (9, 7, 130)]
SENTINEL = -0x0123456789ABCDEF


def run_binding(ids: torch.Tensor, offsets: torch.Tensor, occ: torch.Tensor, T: int, cap: int, probe: int):
    """``contact_stats`` on buffers pre-filled with a sentinel, the live parts zeroed as the kernel wants them,
    with a guard row behind ``contact`` and behind the pair table -> (contact, keys, counts, lost); asserts
    that nothing past the ends was touched."""
    N, D, H, W = ids.shape
    K, st = _native.kernels(), _native.stream(ids)
    con = torch.full((T + 1, 19), SENTINEL, dtype=torch.int64, device=DEV)
    tab = torch.full((2 * cap + 1 + 19,), SENTINEL, dtype=torch.int64, device=DEV)    # keys | counts | lost | guard
    con[:T] = 0
    tab[:2 * cap + 1] = 0
    keys, counts, lost = tab[:cap], tab[cap:2 * cap], tab[2 * cap:2 * cap + 1]
    K.contact_stats(ids.data_ptr(), occ.data_ptr(), offsets.data_ptr(), con.data_ptr(), keys.data_ptr(),
                    counts.data_ptr(), lost.data_ptr(), N, D, H, W, T, cap, probe, st,
                    [ids.numel(), occ.numel(), N + 1, T * 19, cap, cap, 1])
    torch.cuda.synchronize()
    assert bool((con[T] == SENTINEL).all()) and bool((tab[2 * cap + 1:] == SENTINEL).all())
    return con[:T], keys, counts, lost


def decode(keys: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """The occupied slots of the pair table as sorted ``adj`` rows (in torch, apart from the op layer)."""
    slot = torch.nonzero(keys).squeeze(1)
    key, order = torch.sort(keys[slot])
    return torch.stack([(key >> 33) - 1, ((key >> 3) & ((1 << 30) - 1)) - 1, key & 7, counts[slot][order]], 1)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("si", range(6), ids=["one-voxel", "one-row", "under-a-wave", "one-wave", "wave+1",
                                              "two-pieces+rest"])
def test_kernel_against_the_oracle(si, N, pattern):
    D, H, W = SHAPES[si]
    for kind in ("complement", "random"):
        ids_c, table, offsets_c, occ_c, want, want_adj = expected_contacts(pattern, N, D, H, W, kind)
        ids, offsets, occ = ids_c.to(DEV), offsets_c.to(DEV), occ_c.to(DEV)
        T, what = len(table), (pattern, N, (D, H, W), kind)
        cap = 1 << max(10, (6 * ids.numel() - 1).bit_length())       # a slot for every face: nothing can be lost
        con, keys, counts, lost = run_binding(ids, offsets, occ, T, cap, cap)
        adj = decode(keys, counts)
        assert int(lost) == 0 and con.dtype == adj.dtype == torch.int64, what
        assert torch.equal(con.cpu(), want), (what, int((con.cpu() != want).sum()))
        assert torch.equal(adj.cpu(), want_adj), (what, adj.shape, want_adj.shape)
        assert not bool(counts[keys == 0].any()), what
        con2, keys2, counts2, _ = run_binding(ids, offsets, occ, T, cap, cap)
        assert torch.equal(con2, con) and torch.equal(decode(keys2, counts2), adj), (what, "second run differs")
        got, got_adj = contact.contact_table(ids, offsets, occ)          # the op layer takes the same kernel
        assert got.is_cuda and torch.equal(got, con) and torch.equal(got_adj, adj), what
        again, adj_again = contact.contact_table(ids, offsets, occ, rows=T)
        assert torch.equal(again, con) and torch.equal(adj_again, adj), what
        if kind == "complement":
            check_identities(con, adj, table.to(DEV), what)


def test_the_pair_table_grows_when_updates_are_lost():
    """``checker`` makes every voxel its own instance: about three pair rows per instance, far more than the
    first table of ``2 T`` slots takes within its probe bound.  The bounded probe drops the updates it cannot
    place and counts them; the op layer sees the count and runs again with a larger table."""
    D, H, W = SHAPES[5]
    ids_c, table, offsets_c, occ_c, want, want_adj = expected_contacts("checker", 1, D, H, W)
    T = len(table)
    assert T == D * H * W and len(want_adj) > 2 * T > 1024
    ids, offsets, occ = ids_c.to(DEV), offsets_c.to(DEV), occ_c.to(DEV)
    con, keys, counts, lost = run_binding(ids, offsets, occ, T, 1024, 256)
    assert int(lost) > 0 and int(lost) + int(counts.sum()) == int(want_adj[:, 3].sum())
    assert torch.equal(con.cpu(), want)                              # the per-row counters do not go through the table
    part = decode(keys, counts).cpu()
    assert 0 < len(part) <= 1024
    oracle = {tuple(r[:3]): r[3] for r in want_adj.tolist()}
    assert all(tuple(r[:3]) in oracle and 0 < r[3] <= oracle[tuple(r[:3])] for r in part.tolist())
    got, got_adj = contact.contact_table(ids, offsets, occ)
    assert torch.equal(got.cpu(), want) and torch.equal(got_adj.cpu(), want_adj)


@pytest.mark.parametrize("N", [1, 2])
def test_single_voxel_instances_overflow_the_lds_table(N):
    """More instances in one workgroup's chunk than its LDS table has slots: the counter updates that find
    their slot held by another row go to global memory directly, the pair updates past the LDS stage too."""
    D, H, W = SHAPES[5]
    chunk, slots = _native.kernels().contact_chunk()
    assert chunk > slots and D * H * W > chunk and chunk % W != 0
    ids_c, offsets_c = singles(N, D, H, W)
    occ_c = occupancy(N, D, H, W, density=0.1, seed=1)
    want, want_adj = reference.contact_table(ids_c, offsets_c, occ_c)
    T = N * D * H * W
    assert bool((want[:, 18] == 1).all()) and bool((want[:, :18].sum(1) == 6).all())
    got, got_adj = contact.contact_table(ids_c.to(DEV), offsets_c.to(DEV), occ_c.to(DEV), rows=T)
    assert torch.equal(got.cpu(), want) and torch.equal(got_adj.cpu(), want_adj)


def test_rows_outside_the_table_count_nowhere():
    """ids that point past the table (offsets that do not belong to them) are dropped, not used as addresses; a
    neighbour with such an id is still another instance, but emits no pair."""
    D, H, W = SHAPES[4]
    ids_c, _ = singles(1, D, H, W)
    occ_c = occupancy(1, D, H, W)
    T = 100
    for off, carried in (([0, T], T), ([-50, T - 50], T - 50), ([1000, T], 0)):
        off_c = torch.tensor(off)
        want, want_adj = reference.contact_table(ids_c, off_c, occ_c)
        con, keys, counts, lost = run_binding(ids_c.to(DEV), off_c.to(DEV), occ_c.to(DEV), off[1], 4096, 4096)
        assert int(lost) == 0 and torch.equal(con.cpu(), want), off
        assert torch.equal(decode(keys, counts).cpu(), want_adj), off
        assert int(want[:, 18].sum()) == carried, off
    big = ids_c.clone()
    big.view(-1)[::3] = 2 ** 31 - 1                                  # ids beyond the sample's range, and negative ones
    big.view(-1)[1::7] = -5
    want, want_adj = reference.contact_table(big, torch.tensor([0, T]), occ_c)
    con, keys, counts, lost = run_binding(big.to(DEV), torch.tensor([0, T], device=DEV), occ_c.to(DEV), T, 4096, 4096)
    assert int(lost) == 0 and torch.equal(con.cpu(), want) and torch.equal(decode(keys, counts).cpu(), want_adj)


def test_unsupported_arguments_are_refused():
    ids = torch.zeros(1, 4, 4, 4, dtype=torch.int32, device=DEV)
    occ = torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device=DEV)
    off = torch.zeros(2, dtype=torch.int64, device=DEV)
    buf = torch.zeros(4 * 19 + 2 * 1024 + 1, dtype=torch.int64, device=DEV)
    K, st = _native.kernels(), _native.stream(ids)
    p = dict(ids=ids.data_ptr(), occ=occ.data_ptr(), offsets=off.data_ptr(), contact=buf.data_ptr(),
             keys=buf[76:].data_ptr(), counts=buf[76 + 1024:].data_ptr(), lost=buf[76 + 2048:].data_ptr(), N=1, D=4, H=4,
             W=4, T=4, cap=1024, probe=256, st=st, ext=[64, 64, 2, 76, 1024, 1024, 1])
    for bad in (dict(T=-1, ext=[]), dict(T=65, ext=[]), dict(ids=0), dict(occ=0), dict(offsets=0), dict(contact=0),
                dict(keys=0), dict(counts=0), dict(lost=0), dict(H=0, ext=[]), dict(cap=1000), dict(probe=0)):
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            K.contact_stats(**{**p, **bad})
    with pytest.raises(RuntimeError, match="contact has"):
        K.contact_stats(**{**p, "T": 5})
    with pytest.raises(ValueError, match="one device"):
        contact.contact_table(ids, off, occ.cpu())
    with pytest.raises(ValueError, match="int32"):
        contact.contact_table(ids.long(), off, occ)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
S = 32


def make_model(nc: int, seed: int = 0) -> FeatureNet3DSeg:
    """A CPU fp32 model whose BN folds are not the identity."""
    torch.manual_seed(seed)
    m = FeatureNet3DSeg(S, num_classes=nc).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for c in list(m.enc) + [m.dec]:
            c.running_mean.copy_(torch.randn(c.cout, generator=g) * 0.1)
            c.running_var.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.gamma.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.beta.copy_(torch.randn(c.cout, generator=g) * 0.1)
        m.head.bias.copy_(torch.randn(nc, generator=g) * 0.1)
    return m


def voxels(n: int, seed: int = 3) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, S, S, S, generator=g) < 0.4


def test_instances_with_contacts_equal_the_oracle_on_the_predicted_labels(monkeypatch):
    m = make_model(5)
    mg = FeatureNet3DSeg(S, num_classes=5)
    mg.load_state_dict(m.state_dict())
    mg = mg.to(DEV).eval()
    xc = voxels(2)
    x = xc.to(DEV).to(torch.bfloat16)
    labels = mg.predict(x)
    assert len(labels.unique()) > 1
    copies = []
    real_cpu, real_to = torch.Tensor.cpu, torch.Tensor.to

    def spy_cpu(t, *a, **k):
        copies.append((t.dtype, tuple(t.shape)))
        return real_cpu(t, *a, **k)

    def spy_to(t, *a, **k):
        out = real_to(t, *a, **k)
        if t.is_cuda and not out.is_cuda:
            copies.append((t.dtype, tuple(t.shape)))
        return out

    monkeypatch.setattr(torch.Tensor, "cpu", spy_cpu)
    monkeypatch.setattr(torch.Tensor, "to", spy_to)
    table, offsets, none, con, adj = mg.instances(x, want_contacts=True)
    full = mg.instances(x, want_ids=True, want_access=True, want_dims=True, want_reach=(4, 2), want_contacts=True)
    torch.cuda.synchronize()
    monkeypatch.undo()
    # no per-voxel tensor (occupancy, labels, ids ...) crossed to the host inside instances()
    assert not [c for c in copies if int(np.prod(c[1])) >= S ** 3], copies
    assert none is None and len(full) == 8 and con.is_cuda and adj.is_cuda
    assert torch.equal(full[0], table) and torch.equal(full[6], con) and torch.equal(full[7], adj)
    cpu_labels = labels.cpu()
    want_ids, want_table, want_offsets = reference.instance_table(cpu_labels,
                                                                  reference.connected_components(cpu_labels, 0, 6))
    want, want_adj = reference.contact_table(want_ids, want_offsets, xc.to(torch.uint8))
    assert torch.equal(table.cpu(), want_table) and torch.equal(full[2].cpu(), want_ids)
    assert torch.equal(con.cpu(), want) and torch.equal(adj.cpu(), want_adj) and len(want_adj) > 0
    check_identities(con, adj, table, "model")


def test_extract_features_with_contacts_end_to_end(tmp_path):
    n = 4
    m = make_model(5)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 5})
    xb = voxels(n)
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    feats, none = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S, access=True,
                                      dimensions=True, tool=3, contacts=True)
    labels, _ = fn.segment(str(path), packed, batch_size=3, device=DEV, packed_size=S)
    _, want = fn.label_components(labels, device="cpu", occupancy=xb.numpy(), dimensions=True, tool=3, contacts=True)
    assert none is None and len(feats) == n and feats == want
    _, on_gpu = fn.label_components(labels, device=DEV, occupancy=xb.numpy(), dimensions=True, tool=3, contacts=True)
    assert on_gpu == want and any(f.neighbors for fs in want for f in fs)
    only, _ = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S, contacts=True)
    assert all(f.access is None and f.clearance2 is None and f.reachable is None for fs in only for f in fs)
    key = lambda f: (f.id, f.voxels, f.wall_area, f.open_area, f.shared_area, f.neighbors)      # noqa: E731
    assert [[key(f) for f in fs] for fs in only] == [[key(f) for f in fs] for fs in want]
    _, alone = fn.label_components(labels, device=DEV, occupancy=xb.numpy(), contacts=True)
    assert [[key(f) for f in fs] for fs in alone] == [[key(f) for f in fs] for fs in want]
    plain, _ = fn.extract_features(str(path), packed, batch_size=3, device=DEV, packed_size=S)
    assert all(f.wall_area is None and f.neighbors is None for fs in plain for f in fs)


def test_intersecting_generated_parts():
    vox, labels, parts = fn.generate_parts(96, size=32, seed=3, device=DEV, separate=False)
    ids, feats = fn.label_components(labels, device=DEV, occupancy=vox, contacts=True)
    recs = [f for fs in feats for f in fs]
    assert len(recs) == 253 and sum(len(f.neighbors) for f in recs) == 2 * 109
    assert tuple(sum(f.shared_area[k] for f in recs) for k in range(6)) == (993, 993, 1121, 1121, 860, 860)
    assert tuple(sum(f.wall_area[k] for f in recs) for k in range(6)) == (19883, 21958, 27210, 27464, 16665, 16049)
    assert tuple(sum(f.open_area[k] for f in recs) for k in range(6)) == (10901, 8826, 10823, 10569, 7488, 8104)
