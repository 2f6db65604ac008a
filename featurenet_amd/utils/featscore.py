"""Feature-level quality: predicted instances matched to true ones, and what follows.

Inputs are the two instance tables (``ops.ccl.instance_table``: one row per connected component)
and their overlap table (``ops.overlap.overlap_table``: the shared voxels of every pair that
touches).  A predicted and a true instance of one class match when their IoU = inter / (|a| + |b| -
inter) exceeds the threshold.  Above 0.5 more than half of each lies in the other, so an instance
has at most one partner: no assignment solver, and no dependence on any order.  Everything is
float64 computed on the host from exact integer counts; a quantity whose denominator is 0 is NaN.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .segmetrics import _json, _ratio


def _host(t, dtype=np.int64) -> np.ndarray:
    return np.asarray(t.cpu() if hasattr(t, "cpu") else t, dtype=dtype)


def match_pairs(table_a, table_b, pairs, iou_threshold: float = 0.5, min_voxels: int = 1):
    """Match the instances of ``table_a`` (predicted) to those of ``table_b`` (true) ->
    ``(matched, iou, keep_a, keep_b)``.

    ``table_*`` int64 ``[T, 13]``, ``pairs`` int64 ``[P, 3]`` rows ``(row_a, row_b, voxels)``.
    ``matched`` int64 ``[M, 2]`` holds the ``(row_a, row_b)`` of the matches in ascending order,
    ``iou`` float64 ``[M]`` their IoU; ``keep_*`` bool ``[T]`` marks the instances of at least
    ``min_voxels`` voxels.  The others are removed before matching -- they count nowhere, and an
    instance only they would have matched stays unmatched."""
    thr = float(iou_threshold)
    if not 0.5 <= thr < 1.0:
        raise ValueError(f"match_pairs: iou_threshold must lie in [0.5, 1), not {iou_threshold!r}: below 0.5 an "
                         "instance can exceed it with two partners, so a match is no longer unique (that needs an "
                         "assignment solver), and no IoU exceeds 1")
    ta, tb = _host(table_a).reshape(-1, 13), _host(table_b).reshape(-1, 13)
    pr = _host(pairs).reshape(-1, 3)
    keep_a, keep_b = ta[:, 2] >= int(min_voxels), tb[:, 2] >= int(min_voxels)
    ra, rb, inter = pr[:, 0], pr[:, 1], pr[:, 2]
    if len(pr) and (ra.min() < 0 or ra.max() >= len(ta) or rb.min() < 0 or rb.max() >= len(tb)):
        raise ValueError("match_pairs: the overlap table names rows the instance tables do not have")
    va, vb = ta[ra, 2], tb[rb, 2]
    if bool(((inter < 1) | (inter > np.minimum(va, vb)) | (ta[ra, 0] != tb[rb, 0])).any()):
        raise ValueError("match_pairs: corrupt overlap table (a pair shares more voxels than an instance has, none, "
                         "or joins two samples)")
    iou = inter.astype(np.float64) / (va + vb - inter).astype(np.float64)
    hit = (ta[ra, 1] == tb[rb, 1]) & (iou > thr) & keep_a[ra] & keep_b[rb]
    ma, mb = ra[hit], rb[hit]
    if len(np.unique(ma)) != len(ma) or len(np.unique(mb)) != len(mb):
        raise ValueError("match_pairs: an instance has two partners above IoU 0.5 (corrupt instance or overlap table)")
    order = np.lexsort((mb, ma))
    return np.stack([ma[order], mb[order]], 1), iou[hit][order], keep_a, keep_b


@dataclass
class FeatureScore:
    """Per class (arrays of one length, index = class): ``tp`` matched pairs, ``fp`` unmatched
    predicted instances, ``fn`` unmatched true instances, and the ratios.  ``m*``: means over the
    classes that occur on either side (``tp + fp + fn > 0``); ``msq`` over those with a match."""
    tp: np.ndarray           # int64
    fp: np.ndarray
    fn: np.ndarray
    precision: np.ndarray    # tp / (tp + fp)
    recall: np.ndarray       # tp / (tp + fn)
    f1: np.ndarray           # 2 tp / (2 tp + fp + fn)
    sq: np.ndarray           # segmentation quality: mean IoU of the matched pairs
    rq: np.ndarray           # recognition quality: tp / (tp + fp / 2 + fn / 2)
    pq: np.ndarray           # panoptic quality: sum of the matched IoUs / (tp + fp / 2 + fn / 2) = sq * rq
    mpq: float
    msq: float
    mrq: float
    matches: list            # per sample: [(pred_id, true_id, cls, iou)], ids as in the ``ids`` volumes

    @classmethod
    def from_counts(cls, tp, fp, fn, matches) -> "FeatureScore":
        """From per-class counts and the per-sample match lists (the IoU sums are taken from the
        lists, in their order, so that merging batches gives what one call would)."""
        tp, fp, fn = (np.asarray(v, np.int64) for v in (tp, fp, fn))
        C = len(tp)
        flat = [m for ms in matches for m in ms]
        iou_sum = np.bincount(np.array([m[2] for m in flat], np.int64), np.array([m[3] for m in flat], np.float64),
                              minlength=C)[:C] if flat else np.zeros(C, np.float64)
        tpf = tp.astype(np.float64)
        den = tpf + 0.5 * fp + 0.5 * fn
        sq, rq, pq = _ratio(iou_sum, tpf), _ratio(tpf, den), _ratio(iou_sum, den)
        seen = den > 0

        def mean(v, where):
            return float(v[where].mean()) if where.any() else float("nan")

        return cls(tp=tp, fp=fp, fn=fn, precision=_ratio(tpf, (tp + fp).astype(np.float64)),
                   recall=_ratio(tpf, (tp + fn).astype(np.float64)),
                   f1=_ratio(2.0 * tpf, (2 * tp + fp + fn).astype(np.float64)), sq=sq, rq=rq, pq=pq,
                   mpq=mean(pq, seen), msq=mean(sq, tp > 0), mrq=mean(rq, seen),
                   matches=[list(ms) for ms in matches])

    @classmethod
    def from_tables(cls, table_a, off_a, table_b, off_b, pairs, iou_threshold: float = 0.5,
                    min_voxels: int = 1) -> "FeatureScore":
        """Score the predicted instances ``table_a`` / ``off_a`` against the true ones ``table_b``
        / ``off_b`` given their overlap table ``pairs`` (tensors or arrays).  The per-class arrays
        reach up to the largest class that occurs."""
        ta, tb = _host(table_a).reshape(-1, 13), _host(table_b).reshape(-1, 13)
        oa, ob = _host(off_a), _host(off_b)
        if len(oa) != len(ob) or len(oa) < 1 or oa[-1] != len(ta) or ob[-1] != len(tb):
            raise ValueError("FeatureScore: the offsets do not describe these instance tables")
        matched, iou, keep_a, keep_b = match_pairs(ta, tb, pairs, iou_threshold, min_voxels)
        C = max([0] + [int(t[:, 1].max()) + 1 for t in (ta, tb) if len(t)])
        mcls = ta[matched[:, 0], 1]
        tp = np.bincount(mcls, minlength=C)
        fp = np.bincount(ta[keep_a, 1], minlength=C) - tp
        fn = np.bincount(tb[keep_b, 1], minlength=C) - tp
        matches = [[] for _ in range(len(oa) - 1)]
        for (ra, rb), c, q in zip(matched.tolist(), mcls.tolist(), iou.tolist()):
            n = int(ta[ra, 0])
            matches[n].append((ra - int(oa[n]) + 1, rb - int(ob[n]) + 1, c, q))
        return cls.from_counts(tp, fp, fn, matches)

    @classmethod
    def merge(cls, scores) -> "FeatureScore":
        """The score of the batches' samples taken together, in the order given."""
        scores = list(scores)
        C = max([len(s.tp) for s in scores], default=0)

        def total(name):
            out = np.zeros(C, np.int64)
            for s in scores:
                out[:len(s.tp)] += getattr(s, name)
            return out

        return cls.from_counts(total("tp"), total("fp"), total("fn"), [ms for s in scores for ms in s.matches])

    def __add__(self, other: "FeatureScore") -> "FeatureScore":
        return FeatureScore.merge([self, other])

    def to_dict(self) -> dict:
        """JSON-safe summary (NaN as null)."""
        d = {k: _json(getattr(self, k)) for k in ("mpq", "msq", "mrq", "pq", "sq", "rq", "precision", "recall", "f1",
                                                   "tp", "fp", "fn")}
        d["matches"] = [[[int(a), int(b), int(c), float(q)] for a, b, c, q in ms] for ms in self.matches]
        return d
