#!/usr/bin/env python3
"""Per-voxel segmentation inference: ``model.predict(x)`` (sub-pixel decoder + fused head /
arg-max kernel, labels only) against ``model(x).argmax(-1)`` (27-tap decoder on the upsampled
tensor, bf16 logits to memory, torch arg-max) -- the path a user had before ``predict``.

    python bench/segment_infer.py --size 64 --classes 25 --batch 32 --iters 20

Random-init weights in eval mode, synthetic binary voxels, bf16.  Both paths are warmed up, then
timed alternately in one process with device events; prints the median and spread of each, their
ratio, the share of voxels on which the two label maps agree, and the bytes each head moves per
voxel (from shapes).  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def head_bytes_per_voxel(k: int, classes: int) -> dict:
    """HBM bytes per voxel of the 1x1 head alone (bf16 activations): the fused kernel reads the
    decoder output and writes one label byte; the unfused head writes the logits, which the
    arg-max then reads back (and writes an int64 index)."""
    return {"fused": {"read": 2 * k, "written": 1},
            "unfused": {"read": 2 * k + 2 * classes, "written": 2 * classes + 8}}


def decoder_flops_per_voxel(c: int, k: int) -> dict:
    return {"subpixel_8_taps": 2 * 8 * c * k, "full_res_27_taps": 2 * 27 * c * k}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--classes", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20, help="timed iterations of each path (alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("segment_infer: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1:
        ap.error("--iters and --warmup must be >= 1")
    from featurenet_amd.models.featurenet3d import FeatureNet3DSeg
    from featurenet_amd.ops import subpixel

    torch.manual_seed(0)
    dev = torch.device("cuda")
    m = FeatureNet3DSeg(a.size, num_classes=a.classes).to(dev).eval()
    x = (torch.rand(a.batch, a.size, a.size, a.size, 1, device=dev) < 0.3).to(torch.bfloat16)

    def fused():
        return m.predict(x)

    @torch.no_grad()
    def unfused():
        return m(x).argmax(-1)

    with torch.no_grad():
        z = x
        for c in m.enc:
            z = c(z)
        subpixel_path = bool(subpixel.infer_ok(z, m.dec.cout, z.shape[-1]))
        del z
    for _ in range(a.warmup):
        lf, lu = fused(), unfused()
    torch.cuda.synchronize()
    agree = float((lf.long() == lu).float().mean())
    del lf, lu
    times = {"fused": [], "unfused": []}
    for _ in range(a.iters):
        for name, f in (("fused", fused), ("unfused", unfused)):
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
    print(json.dumps({"metric": f"segmentation inference, {a.size}^3 x {a.classes} classes, batch {a.batch}, bf16",
                      "iters": a.iters, "subpixel_decoder": subpixel_path, "predict": res["fused"],
                      "forward_argmax": res["unfused"],
                      "speedup_predict_over_forward_argmax": round(res["unfused"]["median_ms"] /
                                                                   res["fused"]["median_ms"], 3),
                      "label_agreement": round(agree, 5),
                      "head_bytes_per_voxel": head_bytes_per_voxel(m.dec.cout, a.classes),
                      "decoder_flops_per_voxel": decoder_flops_per_voxel(m.dec.cin, m.dec.cout)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
