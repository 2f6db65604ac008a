#!/usr/bin/env python3
"""Multi-feature parts carved on the device (``ops.partgen``, ``partgen.hip``) against a copy of
the same bytes, the host path and the torch oracle.

    python bench/part_generate.py --size 64 --batch 128 --slots 4 --iters 20

In one process, alternating, with device events over ``--reps`` launches each: (k) the
``partgen_carve`` launch writing occupancy, labels and slots (3 bytes per voxel) and (p) writing
bit-packed occupancy and labels (1.125 bytes per voxel, what a training set keeps); (c) a device
``copy_`` of as many bytes as (k) writes -- the yardstick: a kernel bound by its stores takes a
copy's time less the copy's reads.  Then once each: ``_rt.carve_parts`` on ``--threads`` host
threads (host clock) and ``reference.carve_parts`` on the device (device events, after one
warm-up).  All four must give the same volumes.  Also prints the sampler's feature-count histogram
over ``--hist-parts`` parts with 2..4 features.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(t: list) -> dict:
    t = sorted(t)
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}


def device_time(f, reps: int = 1) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--slots", type=int, default=4, help="feature slots per part (1..slots features)")
    ap.add_argument("--iters", type=int, default=20, help="timed windows of each device path (alternating)")
    ap.add_argument("--reps", type=int, default=200, help="launches per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="host threads of _rt.carve_parts")
    ap.add_argument("--hist-parts", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("part_generate: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1:
        ap.error("--iters, --reps and --warmup must be >= 1")
    from featurenet_amd import _native
    from featurenet_amd.ops import partgen, reference

    dev = torch.device("cuda")
    S, N, K = a.size, a.batch, a.slots
    V = S ** 3
    table = partgen.sample(N, S, 0, (1, K), threads=a.threads)
    params = table.to(dev)
    K_, st = _native.kernels(), _native.stream(params)
    occ, labels, slots = (torch.empty(N, S, S, S, dtype=torch.uint8, device=dev) for _ in range(3))
    bits = torch.empty(N, V // 8, dtype=torch.uint8, device=dev)
    src, dst = (torch.zeros(3 * N * V, dtype=torch.uint8, device=dev) for _ in range(2))
    ext = [params.numel(), N * V, N * V // 8, N * V, N * V]

    def all_three():
        K_.partgen_carve(params.data_ptr(), occ.data_ptr(), 0, labels.data_ptr(), slots.data_ptr(), N, K, S, st, ext)

    def packed():
        K_.partgen_carve(params.data_ptr(), 0, bits.data_ptr(), labels.data_ptr(), 0, N, K, S, st, ext)

    def copy():
        dst.copy_(src)

    paths = {"carve_occ_labels_slots": all_three, "carve_packed_labels": packed, "copy_same_bytes": copy}
    for _ in range(a.warmup):
        for f in paths.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.iters):
        for k, f in paths.items():
            times[k].append(device_time(f, a.reps))
    out = {"metric": f"part generation, {N} parts of {S}^3, {K} slots", "iters": a.iters, "reps": a.reps}
    out.update({k: summary(v) for k, v in times.items()})
    ms = out["carve_occ_labels_slots"]["median_ms"]
    out["parts_per_s"] = round(N / ms * 1e3, 1)
    out["carve_written_GBps"] = round(3 * N * V / ms / 1e6, 1)
    out["packed_parts_per_s"] = round(N / out["carve_packed_labels"]["median_ms"] * 1e3, 1)
    out["copy_written_GBps"] = round(3 * N * V / out["copy_same_bytes"]["median_ms"] / 1e6, 1)
    out["carve_over_copy"] = round(ms / out["copy_same_bytes"]["median_ms"], 3)

    t0 = time.perf_counter()
    host = _native.runtime().carve_parts(table.numpy(), S, a.threads)
    out["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["host_threads"] = a.threads
    out["host_parts_per_s"] = round(N / out["host_ms"] * 1e3, 1)
    reference.carve_parts(params[:2], S)
    torch.cuda.synchronize()
    want = []
    out["oracle_ms"] = round(device_time(lambda: want.append(reference.carve_parts(params, S))), 2)
    out["oracle_parts_per_s"] = round(N / out["oracle_ms"] * 1e3, 1)
    torch.cuda.synchronize()
    ok = all(torch.equal(g, w) and torch.equal(g.cpu(), torch.from_numpy(h))
             for g, w, h in zip((occ, labels, slots), want[0], host))
    weights = 1 << torch.arange(8, dtype=torch.int32, device=dev)
    ok &= torch.equal(bits, (occ.reshape(N, -1, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8))
    out["paths_agree"] = bool(ok)
    out["removed_share"] = round(float((labels != 0).float().mean()), 4)

    counts = (partgen.sample(a.hist_parts, 64, 0, (2, 4), threads=a.threads)[..., 0] >= 0).sum(1)
    out["sampler_feature_counts_2_4"] = torch.bincount(counts, minlength=5).tolist()
    out["sampler_short_share"] = round(float((counts < 2).float().mean()), 4)
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
