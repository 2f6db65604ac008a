#!/usr/bin/env python3
"""Triangle meshes voxelized on the device (``ops.voxelize``, ``voxelize.hip``) against a copy of
the bytes it writes and against the host path.

    python bench/mesh_voxelize.py --size 64 --batch 128 --iters 10

Three workloads at ``--size``^3, ``--batch`` meshes each: (a) ``parts``, the boundary meshes of
generated parts (tens of thousands of triangles that each cover one column); (b) ``spheres``,
icospheres of 20,480 triangles under random rotations; (c) ``boxes``, 12 triangles that each
cover a whole face.  Then one icosphere at ``--big``^3.  For each, in one process, alternating,
with device events over ``--reps`` launches: (k) the ``voxelize_tris`` launch writing occupancy
and leak counts, (p) the same writing bit-packed occupancy, (c) a device ``copy_`` of as many bytes
as (k) writes -- the floor of a kernel bound by its stores.  Then once: ``_rt.voxelize_tris`` on
``--threads`` host threads (host clock).  The paths must give the same volumes.  Needs a GPU:
there is no CPU fallback.
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
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}


def device_time(f, reps: int = 1) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def rotations(n: int, seed: int) -> np.ndarray:
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    return q * np.sign(np.linalg.det(q))[:, None, None]


def workloads(S: int, N: int, big: int, threads: int) -> dict:
    """name -> (size, list of int32 [T_i, 9] lattice meshes)."""
    from featurenet_amd.ops import partgen
    from featurenet_amd.utils.voxelmesh import icosphere, voxels_to_mesh

    vox, _ = partgen.carve(partgen.sample(N, S, 0, (1, 4), threads=threads), S, threads=threads)
    parts = [np.rint(voxels_to_mesh(v) * 16).astype(np.int32).reshape(-1, 9) for v in vox.numpy()]
    v, f = icosphere(5)                                    # 20,480 triangles
    g = np.random.default_rng(1)
    spheres = []
    for rot in rotations(N, 2):
        r, c = 16 * S * g.uniform(0.3, 0.45), 16 * S * g.uniform(0.48, 0.52, 3)
        spheres.append(np.rint((v @ rot.T) * r + c).astype(np.int32)[f].reshape(-1, 9))
    boxes = []
    corner = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    for _ in range(N):
        lo, hi = g.integers(0, 16 * S // 4, 3), g.integers(16 * S * 3 // 4, 16 * S + 1, 3)
        boxes.append(np.where(corner == 0, lo, hi).astype(np.int32)[faces].reshape(-1, 9))
    one = np.rint((v @ rotations(1, 3)[0].T) * (16 * big * 0.43) + 16 * big * 0.5).astype(np.int32)[f].reshape(-1, 9)
    return {"parts": (S, parts), "spheres": (S, spheres), "boxes": (S, boxes), f"sphere_{big}": (big, [one])}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--big", type=int, default=256, help="grid of the single large mesh")
    ap.add_argument("--iters", type=int, default=10, help="timed windows of each device path (alternating)")
    ap.add_argument("--reps", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16, help="host threads of _rt.voxelize_tris")
    ap.add_argument("--planes", type=int, default=0,
                    help="z-planes per workgroup at --size (0: voxelize_planes); changes the time, never the bits")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("mesh_voxelize: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1:
        ap.error("--iters, --reps and --warmup must be >= 1")
    from featurenet_amd import _native

    dev = torch.device("cuda")
    K_, rt = _native.kernels(), _native.runtime()
    out = {"metric": f"mesh voxelization, {a.batch} meshes at {a.size}^3 and one at {a.big}^3", "iters": a.iters,
           "reps": a.reps, "host_threads": a.threads}
    ok = True
    for name, (S, meshes) in workloads(a.size, a.batch, a.big, a.threads).items():
        N, V = len(meshes), S ** 3
        tris_h = torch.from_numpy(np.concatenate(meshes))
        off_h = torch.from_numpy(np.concatenate([[0], np.cumsum([len(m) for m in meshes])]).astype(np.int32))
        tris, off = tris_h.to(dev), off_h.to(dev)
        T, st = tris.shape[0], _native.stream(tris)
        zs = a.planes if a.planes and S == a.size else K_.voxelize_planes(S)
        slabs = -(-S // zs)
        occ = torch.empty(N, S, S, S, dtype=torch.uint8, device=dev)
        bits = torch.empty(N, V // 8, dtype=torch.uint8, device=dev)
        part = torch.empty(N, slabs, dtype=torch.int32, device=dev)
        src, dst = (torch.zeros(N * V, dtype=torch.uint8, device=dev) for _ in range(2))
        ext = [tris.numel(), off.numel(), N * V, N * V // 8, N * slabs]

        def dense():
            K_.voxelize_tris(tris.data_ptr(), off.data_ptr(), occ.data_ptr(), 0, part.data_ptr(), N, T, S, zs, st, ext)

        def packed():
            K_.voxelize_tris(tris.data_ptr(), off.data_ptr(), 0, bits.data_ptr(), part.data_ptr(), N, T, S, zs, st, ext)

        def copy():
            dst.copy_(src)

        paths = {"voxelize_occ": dense, "voxelize_packed": packed, "copy_same_bytes": copy}
        for _ in range(a.warmup):
            for f in paths.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.iters):
            for k, f in paths.items():
                times[k].append(device_time(f, a.reps))
        res = {"size": S, "meshes": N, "triangles": T, "planes_per_workgroup": zs, "workgroups": N * slabs}
        res.update({k: summary(v) for k, v in times.items()})
        ms = res["voxelize_occ"]["median_ms"]
        res["meshes_per_s"] = round(N / ms * 1e3, 1)
        res["Mtris_per_s"] = round(T / ms / 1e3, 1)
        res["over_copy"] = round(ms / res["copy_same_bytes"]["median_ms"], 2)
        t0 = time.perf_counter()
        host_occ, host_leaks = rt.voxelize_tris(tris_h.numpy(), off_h.numpy(), S, a.threads)
        res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res["host_over_kernel"] = round(res["host_ms"] / ms, 2)
        same = torch.equal(occ.cpu(), torch.from_numpy(host_occ)) and \
            torch.equal(part.sum(1, dtype=torch.int64).cpu(), torch.from_numpy(host_leaks)) and \
            torch.equal(bits.cpu(), torch.from_numpy(np.packbits(host_occ.reshape(N, -1), axis=1, bitorder="little")))
        res["paths_agree"] = bool(same)
        res["filled_share"] = round(float(host_occ.mean()), 4)
        res["leaks"] = int(host_leaks.sum())
        ok &= same
        out[name] = res
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
