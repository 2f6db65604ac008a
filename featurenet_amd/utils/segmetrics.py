"""Segmentation quality from a confusion matrix: per-class IoU / precision / recall / dice, mIoU.

Everything is float64 computed on the host from exact integer counts (rows = truth, columns =
prediction); a quantity whose denominator is 0 is NaN.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np


def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    out = np.full(den.shape, np.nan, np.float64)
    np.divide(num, den, out=out, where=den > 0)
    return out


def _json(v):
    if isinstance(v, np.ndarray):
        return [_json(e) for e in v.tolist()]
    if isinstance(v, float):
        return None if math.isnan(v) else v
    return v


@dataclass
class SegScore:
    """``confusion`` int64 ``[C, C]`` (``confusion[t, p]`` = voxels of class ``t`` labelled ``p``)
    and what follows from it."""
    confusion: np.ndarray
    voxels: int
    accuracy: float          # trace / sum
    support: np.ndarray      # voxels of each true class (row sums)
    predicted: np.ndarray    # voxels given each label (column sums)
    iou: np.ndarray          # tp / (support + predicted - tp)
    precision: np.ndarray    # tp / predicted
    recall: np.ndarray       # tp / support
    dice: np.ndarray         # 2 tp / (support + predicted)
    miou: float              # mean IoU over the classes that occur in truth or prediction

    @classmethod
    def from_confusion(cls, confusion) -> "SegScore":
        cm = np.asarray(confusion)
        if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or cm.dtype.kind not in "iu":
            raise ValueError("SegScore: confusion must be a square integer matrix")
        cm = cm.astype(np.int64)
        tp = np.diag(cm).astype(np.float64)
        support = cm.sum(1)
        predicted = cm.sum(0)
        total = int(cm.sum())
        union = support + predicted - np.diag(cm)
        iou = _ratio(tp, union.astype(np.float64))
        seen = union > 0
        return cls(confusion=cm, voxels=total,
                   accuracy=float(tp.sum() / total) if total else float("nan"),
                   support=support, predicted=predicted, iou=iou,
                   precision=_ratio(tp, predicted.astype(np.float64)),
                   recall=_ratio(tp, support.astype(np.float64)),
                   dice=_ratio(2.0 * tp, (support + predicted).astype(np.float64)),
                   miou=float(iou[seen].mean()) if seen.any() else float("nan"))

    def to_dict(self) -> dict:
        """JSON-safe summary (NaN as null)."""
        return {k: _json(getattr(self, k)) for k in ("voxels", "accuracy", "miou", "iou", "precision", "recall",
                                                      "dice", "support", "predicted", "confusion")}
