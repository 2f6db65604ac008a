#!/usr/bin/env python3
"""From voxels to the list of features on the device: ``model.instances(x)`` (labels -> connected
components -> instance table, ``ops.ccl``) against the route a user had before it: ``model.predict``,
the labels copied to the host, ``scipy.ndimage.label`` once per class and sample.

    python bench/feature_instances.py --size 64 --classes 25 --batch 32 --iters 20

Times, in one process, alternating, with device events (a host clock round the host route, which
ends on the host): (a) ``predict`` alone, (b) ``instances``, (c) the host route; and (d) the two
ops alone (``connected_components`` + ``instance_table`` with ids) on three synthetic label volumes
of the same shape: one solid class (one component per sample: the worst case for the table's
atomics), block-upsampled random blobs, per-voxel noise (the most components).  ``--ops-only``
runs (d) alone -- the form to put under a kernel trace for per-kernel times.  Random-init weights
in eval mode, synthetic binary voxels, bf16.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(t: list) -> dict:
    t = sorted(t)
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3),
            "p10_ms": round(t[len(t) // 10], 3), "p90_ms": round(t[(9 * len(t)) // 10 if len(t) > 1 else 0], 3)}


def device_time(f) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--classes", type=int, default=25)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20, help="timed iterations of each device path (alternating)")
    ap.add_argument("--host-iters", type=int, default=2, help="timed iterations of the host route")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--connectivity", type=int, default=6, choices=(6, 26))
    ap.add_argument("--ops-only", action="store_true", help="only the two ops on the synthetic volumes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("feature_instances: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1:
        ap.error("--iters and --warmup must be >= 1")
    from featurenet_amd.models.featurenet3d import FeatureNet3DSeg
    from featurenet_amd.ops import ccl

    torch.manual_seed(0)
    dev = torch.device("cuda")
    C, S, N = a.classes, a.size, a.batch
    out = {"metric": f"feature instances, {S}^3 x {C} classes, batch {N}, connectivity {a.connectivity}",
           "iters": a.iters}

    # (d) the ops alone
    rng = np.random.default_rng(0)
    b = 8
    coarse = rng.integers(0, C, (N, -(-S // b), -(-S // b), -(-S // b)))
    vols = {"solid": np.full((N, S, S, S), 1),
            "blobs": np.kron(coarse, np.ones((1, b, b, b), np.int64))[:, :S, :S, :S],
            "noise": rng.integers(0, C, (N, S, S, S))}
    ops = {}
    for name, v in vols.items():
        lab = torch.from_numpy(np.ascontiguousarray(v).astype(np.uint8)).to(dev)

        def labelling():
            return ccl.connected_components(lab, 0, a.connectivity, return_flags=True)

        def both():
            roots, flags = labelling()
            return ccl.instance_table(lab, roots, want_ids=True, flags=flags)

        for _ in range(a.warmup):
            ids, table, offsets = both()
        torch.cuda.synchronize()
        t_both = [device_time(both) for _ in range(a.iters)]
        t_lab = [device_time(labelling) for _ in range(a.iters)]
        ops[name] = {"components": int(table.shape[0]), "voxels_in_components": int(table[:, 2].sum()),
                     "both_ops": summary(t_both), "connected_components": summary(t_lab)}
    out["ops_alone"] = ops
    if a.ops_only:
        print(json.dumps(out))
        return 0

    m = FeatureNet3DSeg(S, num_classes=C).to(dev).eval()
    x = (torch.rand(N, S, S, S, 1, device=dev) < 0.3).to(torch.bfloat16)

    def predict():
        return m.predict(x)

    def instances():
        return m.instances(x, background=0, connectivity=a.connectivity)

    def host_route():
        from scipy import ndimage

        st = ndimage.generate_binary_structure(3, 1 if a.connectivity == 6 else 3)
        labels = m.predict(x).cpu().numpy()
        rows = 0
        for n in range(N):
            for c in np.unique(labels[n]):
                if c != 0:
                    rows += ndimage.label(labels[n] == c, structure=st)[1]
        return rows

    for _ in range(a.warmup):
        predict()
        table, offsets, _ = instances()
    torch.cuda.synchronize()
    same = host_route() == int(table.shape[0])
    times = {"predict": [], "instances": []}
    for _ in range(a.iters):
        for name, f in (("predict", predict), ("instances", instances)):
            times[name].append(device_time(f))
    host = []
    for _ in range(a.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route()
        host.append((time.perf_counter() - t0) * 1e3)
    res = {k: summary(v) for k, v in times.items()}
    res["host_route"] = summary(host) if host else None
    out.update(res)
    out["components"] = int(table.shape[0])
    out["same_component_count_as_scipy"] = bool(same)
    dev_extra = res["instances"]["median_ms"] - res["predict"]["median_ms"]
    out["instances_minus_predict_ms"] = round(dev_extra, 3)
    if host:
        out["host_route_minus_predict_ms"] = round(res["host_route"]["median_ms"] - res["predict"]["median_ms"], 3)
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
