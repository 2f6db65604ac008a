"""The overlap-table oracle (``reference.overlap_table``), the matching and the feature-level score
(``utils.featscore``) and ``fn.match_features`` on the CPU.

The oracle is checked against a loop over voxels; the score against hand-built cases whose answers
have a closed form."""
import json
import math

import numpy as np
import pytest
import torch

import featurenet_amd as fn
from _ccl_cases import volume
from featurenet_amd.ops import overlap, reference
from featurenet_amd.utils.featscore import FeatureScore, match_pairs


def tables(lab: torch.Tensor, connectivity: int = 6, background=0):
    roots = reference.connected_components(lab, background, connectivity)
    return reference.instance_table(lab, roots, True)


def brute_force(ids_a, off_a, ids_b, off_b) -> torch.Tensor:
    """Every voxel visited in a Python loop, the pairs counted in a dict."""
    N = ids_a.shape[0]
    a, b = ids_a.reshape(N, -1).tolist(), ids_b.reshape(N, -1).tolist()
    oa, ob = off_a.tolist(), off_b.tolist()
    seen = {}
    for n in range(N):
        for ia, ib in zip(a[n], b[n]):
            if ia > 0 and ib > 0:
                k = (oa[n] + ia - 1, ob[n] + ib - 1)
                seen[k] = seen.get(k, 0) + 1
    return torch.tensor([[ra, rb, c] for (ra, rb), c in sorted(seen.items())], dtype=torch.int64).reshape(-1, 3)


@pytest.mark.parametrize("pa,pb", [("noise4", "blobs"), ("noise2", "noise4"), ("checker", "blobs"), ("solid", "noise4"),
                                   ("samples", "solid"), ("wrap", "solid")])
def test_oracle_against_a_loop_over_voxels(pa, pb):
    N, D, H, W = 2, 3, 4, 5
    ids_a, table_a, off_a = tables(volume(pa, N, D, H, W), 6)
    ids_b, table_b, off_b = tables(volume(pb, N, D, H, W), 26)
    got = reference.overlap_table(ids_a, off_a, ids_b, off_b)
    want = brute_force(ids_a, off_a, ids_b, off_b)
    assert got.dtype == torch.int64 and torch.equal(got, want), (pa, pb)
    assert len(got) > 0 and int(got[:, 2].sum()) == int(((ids_a > 0) & (ids_b > 0)).sum())
    assert torch.equal(overlap.overlap_table(ids_a, off_a, ids_b, off_b), want)       # the op's CPU path


def test_oracle_keeps_the_samples_apart():
    """Two samples whose per-sample ids coincide: id 1 of sample 0 and id 1 of sample 1 are two rows."""
    lab = torch.zeros(2, 2, 3, 4, dtype=torch.uint8)
    lab[0, 0, 0, :2] = 3
    lab[1, 1, 2, :3] = 3
    ids, table, off = tables(lab)
    assert ids.max() == 1 and off.tolist() == [0, 1, 2]
    pairs = reference.overlap_table(ids, off, ids, off)
    assert pairs.tolist() == [[0, 0, 2], [1, 1, 3]]
    assert torch.equal(pairs, brute_force(ids, off, ids, off))


def test_oracle_empty_side_and_identical_volumes():
    N, D, H, W = 2, 3, 4, 5
    ids_b, table_b, off_b = tables(volume("blobs", N, D, H, W), 26)
    ids_e, table_e, off_e = tables(volume("empty", N, D, H, W))
    for args in ((ids_e, off_e, ids_b, off_b), (ids_b, off_b, ids_e, off_e)):
        pairs = reference.overlap_table(*args)
        assert pairs.shape == (0, 3) and pairs.dtype == torch.int64
    diag = reference.overlap_table(ids_b, off_b, ids_b, off_b)
    T = len(table_b)
    assert T > 2 and torch.equal(diag, torch.stack([torch.arange(T), torch.arange(T), table_b[:, 2]], 1))
    none = overlap.overlap_table(ids_b[:0], off_b[:1], ids_b[:0], off_b[:1])
    assert none.shape == (0, 3) and none.dtype == torch.int64


def test_op_refuses_mismatched_inputs():
    ids, table, off = tables(volume("blobs", 2, 3, 4, 5))
    with pytest.raises(ValueError, match="int32"):
        overlap.overlap_table(ids.long(), off, ids, off)
    with pytest.raises(ValueError, match="ids_b must be"):
        overlap.overlap_table(ids, off, ids[:, :2], off)
    with pytest.raises(ValueError, match="offsets"):
        overlap.overlap_table(ids, off[:2], ids, off)
    with pytest.raises(ValueError, match="offsets"):
        overlap.overlap_table(ids, off, ids, off.int())


# ---------------------------------------------------------------------------------------------
# matching and the score, on hand-built label volumes [1, 1, 1, W] (every instance a run along x)
# ---------------------------------------------------------------------------------------------
def row(*runs, W=24, N=1) -> torch.Tensor:
    """uint8 [N, 1, 1, W] with ``(start, stop, cls)`` runs in every sample."""
    lab = torch.zeros(N, 1, 1, W, dtype=torch.uint8)
    for a, b, c in runs:
        lab[..., a:b] = c
    return lab


def score(pred: torch.Tensor, true: torch.Tensor, **kw) -> FeatureScore:
    ids_p, table_p, off_p = tables(pred)
    ids_t, table_t, off_t = tables(true)
    pairs = reference.overlap_table(ids_p, off_p, ids_t, off_t)
    return FeatureScore.from_tables(table_p, off_p, table_t, off_t, pairs, **kw)


def test_perfect_prediction():
    lab = row((0, 4, 1), (6, 9, 2), (10, 12, 2), (14, 20, 3))
    s = score(lab, lab)
    assert s.tp.tolist() == [0, 1, 2, 1] and s.fp.tolist() == [0] * 4 and s.fn.tolist() == [0] * 4
    assert s.tp.dtype == np.int64 and s.pq.dtype == np.float64
    for name in ("precision", "recall", "f1", "sq", "rq", "pq"):
        v = getattr(s, name)
        assert math.isnan(v[0]) and v[1:].tolist() == [1.0, 1.0, 1.0], name     # class 0 forms no instance
    assert s.mpq == 1.0 and s.msq == 1.0 and s.mrq == 1.0
    assert s.matches == [[(1, 1, 1, 1.0), (2, 2, 2, 1.0), (3, 3, 2, 1.0), (4, 4, 3, 1.0)]]
    d = json.loads(json.dumps(s.to_dict()))
    assert d["pq"] == [None, 1.0, 1.0, 1.0] and d["mpq"] == 1.0 and d["matches"][0][1] == [2, 2, 2, 1.0]


def test_one_slot_predicted_as_two_halves():
    true = row((0, 10, 2))
    s = score(row((0, 5, 2), (5, 10, 3)), true)         # the halves got two classes: two instances of IoU 0.5
    assert s.tp.tolist() == [0, 0, 0, 0] and s.fp.tolist() == [0, 0, 1, 1] and s.fn.tolist() == [0, 0, 1, 0]
    s = score(row((0, 4, 2), (5, 10, 2)), true)         # 4 + 5 voxels and a gap: IoU 0.4 and 0.5, no match
    assert int(s.tp.sum()) == 0 and s.fp.tolist() == [0, 0, 2] and s.fn.tolist() == [0, 0, 1]
    assert s.pq[2] == 0.0 and math.isnan(s.sq[2]) and s.rq[2] == 0.0 and s.mpq == 0.0 and math.isnan(s.msq)
    assert s.matches == [[]]
    s = score(row((0, 7, 2), (8, 10, 2)), true)         # 7 + 2 voxels: IoU 0.7 matches, the other is spurious
    assert s.tp.tolist() == [0, 0, 1] and s.fp.tolist() == [0, 0, 1] and s.fn.tolist() == [0, 0, 0]
    assert s.sq[2] == 0.7 and s.rq[2] == 1 / 1.5 and s.pq[2] == 0.7 / 1.5
    assert s.precision[2] == 0.5 and s.recall[2] == 1.0 and s.f1[2] == 2 / 3
    assert s.matches == [[(1, 1, 2, 0.7)]]


def test_iou_of_exactly_one_half_is_no_match():
    true, pred = row((0, 10, 1)), row((0, 5, 1))        # inter 5, union 10
    ids_p, table_p, off_p = tables(pred)
    ids_t, table_t, off_t = tables(true)
    pairs = reference.overlap_table(ids_p, off_p, ids_t, off_t)
    assert pairs.tolist() == [[0, 0, 5]] and 2 * 5 == 5 + 10 - 5
    matched, iou, _, _ = match_pairs(table_p, table_t, pairs)
    assert matched.shape == (0, 2) and iou.shape == (0,)
    s = score(pred, true)
    assert s.tp[1] == 0 and s.fp[1] == 1 and s.fn[1] == 1
    s = score(row((0, 6, 1)), true)                     # inter 6, union 10
    assert s.tp[1] == 1 and s.sq[1] == 0.6 and score(row((0, 6, 1)), true, iou_threshold=0.6).tp[1] == 0


def test_class_mismatch_with_full_overlap():
    s = score(row((2, 9, 3)), row((2, 9, 4)))
    assert s.tp.tolist() == [0] * 5 and s.fp.tolist() == [0, 0, 0, 1, 0] and s.fn.tolist() == [0, 0, 0, 0, 1]
    assert s.mpq == 0.0 and s.matches == [[]]


def test_min_voxels_removes_small_instances_on_both_sides():
    true = row((0, 10, 1), (12, 14, 1), (16, 19, 2))
    pred = row((0, 10, 1), (12, 14, 1), (16, 19, 2), (21, 22, 2))
    s = score(pred, true)
    assert s.tp.tolist() == [0, 2, 1] and s.fp.tolist() == [0, 0, 1] and s.fn.tolist() == [0, 0, 0]
    s = score(pred, true, min_voxels=3)                 # the 2-voxel pair and the 1-voxel extra count nowhere
    assert s.tp.tolist() == [0, 1, 1] and s.fp.tolist() == [0, 0, 0] and s.fn.tolist() == [0, 0, 0]
    assert s.matches == [[(1, 1, 1, 1.0), (3, 3, 2, 1.0)]]          # ids as in the ids volumes
    # a 4-voxel true instance whose 3-voxel partner (IoU 0.75) is removed stays unmatched
    s = score(row((0, 3, 1)), row((0, 4, 1)), min_voxels=4)
    assert s.tp[1] == 0 and s.fp[1] == 0 and s.fn[1] == 1
    assert score(row((0, 3, 1)), row((0, 4, 1))).tp[1] == 1


def test_merge_over_batches_equals_one_call():
    rng = np.random.default_rng(5)
    true = torch.from_numpy(np.kron(rng.integers(0, 4, (5, 2, 3, 4)), np.ones((1, 2, 2, 3), np.int64)).astype(np.uint8))
    pred = true.clone()
    flip = torch.from_numpy(rng.random(true.shape) < 0.12)
    pred[flip] = torch.from_numpy(rng.integers(0, 5, true.shape).astype(np.uint8))[flip]
    whole = score(pred, true)
    assert 0 < int(whole.tp.sum()) and 0 < int(whole.fp.sum()) and len(whole.matches) == 5
    parts = [score(pred[a:b], true[a:b]) for a, b in ((0, 2), (2, 3), (3, 5))]
    merged = FeatureScore.merge(parts)
    assert merged.to_dict() == whole.to_dict()
    assert (parts[0] + parts[1] + parts[2]).to_dict() == whole.to_dict()
    assert merged.matches == whole.matches and np.array_equal(merged.tp, whole.tp)
    assert 0.0 < whole.mpq < 1.0 and all(0.5 < m[3] <= 1.0 for ms in whole.matches for m in ms)


def test_thresholds_below_one_half_and_from_one_are_refused():
    lab = row((0, 4, 1))
    for thr in (0.49, 1.0):
        with pytest.raises(ValueError, match="unique"):
            score(lab, lab, iou_threshold=thr)
    with pytest.raises(ValueError, match="unique"):
        fn.match_features(lab.numpy(), lab.numpy(), iou_threshold=0.49, device="cpu")


def test_a_corrupt_table_is_refused():
    """Two predicted rows claiming most of one true instance cannot both be right."""
    ids_t, table_t, off_t = tables(row((0, 10, 1)))
    table_p = table_t.repeat(2, 1)
    pairs = torch.tensor([[0, 0, 9], [1, 0, 9]])
    with pytest.raises(ValueError, match="two partners"):
        match_pairs(table_p, table_t, pairs)
    with pytest.raises(ValueError, match="corrupt"):
        match_pairs(table_t, table_t, torch.tensor([[0, 0, 11]]))
    with pytest.raises(ValueError, match="rows"):
        match_pairs(table_t, table_t, torch.tensor([[0, 1, 3]]))


def test_match_features_end_to_end_on_the_cpu():
    assert "evaluate_features" in fn.__all__ and "match_features" in fn.__all__
    N, D, H, W = 2, 6, 7, 9
    true = volume("blobs", N, D, H, W)
    pred = true.clone()
    pred[0, :3] = 0                                     # cuts sample 0's instances, removes some
    s = fn.match_features(pred.numpy().astype(np.int64), true.numpy(), connectivity=26, device="cpu")
    assert s.to_dict() == score_26(pred, true).to_dict()
    assert int(s.fp.sum()) + int(s.fn.sum()) > 0 and int(s.tp.sum()) > 0
    same = fn.match_features(true, true, device="cpu")
    ids, feats = fn.label_components(true, device="cpu")
    assert int(same.tp.sum()) == sum(len(f) for f in feats) and same.mpq == 1.0
    assert [[(m[0], m[1]) for m in ms] for ms in same.matches] == [[(f.id, f.id) for f in fs] for fs in feats]
    with pytest.raises(ValueError, match="true labels"):
        fn.match_features(true, true[:1], device="cpu")
    with pytest.raises(ValueError, match="integers"):
        fn.match_features(true.float(), true, device="cpu")
    with pytest.raises(ValueError, match="connectivity"):
        fn.match_features(true, true, connectivity=18, device="cpu")


def score_26(pred, true) -> FeatureScore:
    ids_p, table_p, off_p = tables(pred, 26)
    ids_t, table_t, off_t = tables(true, 26)
    return FeatureScore.from_tables(table_p, off_p, table_t, off_t, reference.overlap_table(ids_p, off_p, ids_t, off_t))


def test_cli_parses_score_features():
    from featurenet_amd.cli import build_parser, cmd_score_features

    a = build_parser().parse_args(["score-features", "seg.fnk", "voxels.npy", "truth.npy", "--json", "out.json", "--iou",
                                   "0.6", "--min-voxels", "5", "--connectivity", "26"])
    assert a.fn is cmd_score_features and (a.model, a.input, a.truth) == ("seg.fnk", "voxels.npy", "truth.npy")
    assert (a.json, a.iou, a.min_voxels, a.connectivity) == ("out.json", 0.6, 5, 26)
