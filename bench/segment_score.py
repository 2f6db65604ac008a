#!/usr/bin/env python3
"""Scoring a segmentation model on the device: ``model.score(x, y)`` (the head counts (truth,
label) pairs in its own kernel and writes nothing per voxel) against ``model.predict(x)`` plus an
on-device ``torch.bincount(truth * C + labels)`` -- the best way to the confusion matrix a user had
before ``score``.

    python bench/segment_score.py --size 64 --classes 25 --batch 32 --iters 30

Random-init weights in eval mode, synthetic binary voxels, uniform random truth, bf16.  Both paths
are warmed up, checked to give the same matrix, then timed alternately in one process with device
events; prints the median and spread of each and whether ``score`` wins by more than the spread
(p10-p90) of the ``predict`` + ``bincount`` path.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--classes", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20, help="timed iterations of each path (alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("segment_score: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1:
        ap.error("--iters and --warmup must be >= 1")
    from featurenet_amd.models.featurenet3d import FeatureNet3DSeg

    torch.manual_seed(0)
    dev = torch.device("cuda")
    C = a.classes
    m = FeatureNet3DSeg(a.size, num_classes=C).to(dev).eval()
    x = (torch.rand(a.batch, a.size, a.size, a.size, 1, device=dev) < 0.3).to(torch.bfloat16)
    y = torch.randint(0, C, (a.batch, a.size, a.size, a.size), device=dev).to(torch.uint8)
    acc = torch.zeros(C * C + 1, dtype=torch.int64, device=dev)

    def score():
        return m.score(x, y, acc=acc.zero_())[0]

    def predict_bincount():
        labels = m.predict(x)
        return torch.bincount(y.reshape(-1).long() * C + labels.reshape(-1).long(), minlength=C * C)

    for _ in range(a.warmup):
        cs, cb = score(), predict_bincount()
    torch.cuda.synchronize()
    same = bool(torch.equal(cs[:C * C], cb)) and int(cs[C * C]) == 0
    times = {"score": [], "predict_bincount": []}
    for _ in range(a.iters):
        for name, f in (("predict_bincount", predict_bincount), ("score", score)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    res = {}
    for name, t in times.items():
        t = sorted(t)
        res[name] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3),
                     "p10_ms": round(t[len(t) // 10], 3), "p90_ms": round(t[(9 * len(t)) // 10 if len(t) > 1 else 0], 3),
                     "voxels_per_s": round(a.batch * a.size ** 3 / (statistics.median(t) * 1e-3))}
    gain = res["predict_bincount"]["median_ms"] - res["score"]["median_ms"]
    spread = res["predict_bincount"]["p90_ms"] - res["predict_bincount"]["p10_ms"]
    print(json.dumps({"metric": f"segmentation scoring, {a.size}^3 x {C} classes, batch {a.batch}, bf16",
                      "iters": a.iters, "same_matrix": same, "score": res["score"],
                      "predict_bincount": res["predict_bincount"],
                      "speedup_score_over_predict_bincount": round(res["predict_bincount"]["median_ms"] /
                                                                   res["score"]["median_ms"], 3),
                      "gain_ms": round(gain, 3), "predict_bincount_p10_p90_spread_ms": round(spread, 3),
                      "score_wins_beyond_spread": bool(gain > spread)}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
