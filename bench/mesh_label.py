#!/usr/bin/env python3
"""Feature instances painted back onto the mesh on the device (``ops.meshlabel``,
``meshlabel.hip``): both forms of the kernel against the torch oracle on the same device and
against the host path, and the crossover between the forms.

    python bench/mesh_label.py --size 64 --batch 32 --iters 10

Workloads at ``--size``^3, ``--batch`` meshes each, the volume holding the generated part's feature
slots on its removed voxels (int32): (a) ``parts``, the boundary meshes of generated parts (every
triangle's box holds one column or none); (b) ``spheres``, icospheres of 20,480 triangles under
random rotations (boxes of a few columns); (c) ``boxes``, 12 triangles that each span a whole face
of a coarse box (thousands of columns); (d) ``mixed``, (a) with the box of (c) appended to each
mesh.  For each, in one process, alternating, with device events over ``--reps`` launches: the
``mesh_votes`` launch with the wave form forced, with the thread form forced (every box it can
hold) and with the default threshold; then once ``reference.mesh_votes`` on the device
(``--oracle-meshes`` meshes of the batch, scaled up) and ``_rt.mesh_votes`` on ``--threads`` host
threads (host clock).  All paths must give the same rows.

``crossover``: ``--batch`` icospheres (20,480 triangles, or coarser where the grid is too small for
the finer one) scaled so that a triangle's box holds about 1, 2, 4, 8, 16 and 32 columns, each timed with every
threshold the thread form allows and with the wave form alone; the threshold
``ops.meshlabel.THREAD_COLS`` is read off this table.  Needs a GPU: no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.mesh_voxelize import device_time, rotations, summary  # noqa: E402


def box_mesh(lo, hi) -> np.ndarray:
    corner = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    return np.where(corner == 0, lo, hi).astype(np.int32)[faces].reshape(-1, 9)


def workloads(S: int, N: int, threads: int):
    """-> ``(vol int32 [N, S, S, S], {name: list of int32 [T_i, 9] lattice meshes})``."""
    from featurenet_amd.ops import partgen
    from featurenet_amd.utils.voxelmesh import icosphere, voxels_to_mesh

    vox, _, slots = partgen.carve(partgen.sample(N, S, 0, (1, 4), threads=threads), S, threads=threads, want_slots=True)
    vol = (slots.to(torch.int32) * (vox == 0)).contiguous()
    parts = [np.rint(voxels_to_mesh(v) * 16).astype(np.int32).reshape(-1, 9) for v in vox.numpy()]
    v, f = icosphere(5)                                    # 20,480 triangles
    g = np.random.default_rng(1)
    spheres = []
    for rot in rotations(N, 2):
        r, c = 16 * S * g.uniform(0.3, 0.45), 16 * S * g.uniform(0.48, 0.52, 3)
        spheres.append(np.rint((v @ rot.T) * r + c).astype(np.int32)[f].reshape(-1, 9))
    boxes = [box_mesh(g.integers(0, 16 * S // 4, 3), g.integers(16 * S * 3 // 4, 16 * S + 1, 3)) for _ in range(N)]
    mixed = [np.concatenate([p, b]) for p, b in zip(parts, boxes)]
    return vol, {"parts": parts, "spheres": spheres, "boxes": boxes, "mixed": mixed}


def batch(meshes):
    tris = torch.from_numpy(np.concatenate(meshes))
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(m) for m in meshes])]).astype(np.int32))
    return tris, off


def box_columns(tris: np.ndarray) -> np.ndarray:
    """Columns in each triangle's box on the plane of its dominant axis (not clipped to the grid)."""
    t = tris.reshape(-1, 3, 3).astype(np.int64)
    m = np.abs(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])).argmax(1)
    n = np.ones(len(t), np.int64)
    for k in (1, 2):
        c = np.take_along_axis(t, ((m + k) % 3)[:, None, None].repeat(3, 1), axis=2)[:, :, 0]
        n *= np.maximum(0, ((c.max(1) - 8) >> 4) - ((c.min(1) - 8 + 15) >> 4) + 1)
    return n


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10, help="timed windows of each device path (alternating)")
    ap.add_argument("--reps", type=int, default=20, help="launches per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16, help="host threads of _rt.mesh_votes")
    ap.add_argument("--oracle-meshes", type=int, default=2, help="meshes of each batch the torch oracle is timed on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("mesh_label: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1 or not 1 <= a.oracle_meshes <= a.batch:
        ap.error("--iters, --reps and --warmup must be >= 1, --oracle-meshes in 1..--batch")
    from featurenet_amd import _native
    from featurenet_amd.ops import meshlabel, reference
    from featurenet_amd.utils.voxelmesh import icosphere

    dev = torch.device("cuda")
    K_, rt = _native.kernels(), _native.runtime()
    cap, S, N = K_.mesh_votes_thread_cols(), a.size, a.batch
    out = {"metric": f"mesh labels, {N} meshes at {S}^3", "iters": a.iters, "reps": a.reps, "host_threads": a.threads,
           "default_thread_cols": meshlabel.THREAD_COLS}
    vol_h, loads = workloads(S, N, a.threads)
    vol = vol_h.to(dev)
    ok = True

    def timed(tris, off, thresholds):
        """median ms of the launch with each threshold, alternating -> ({thr: summary}, {thr: rows})."""
        T, st = tris.shape[0], _native.stream(tris)
        rows = {thr: torch.empty(T, 3, dtype=torch.int32, device=dev) for thr in thresholds}
        wide = torch.empty(T + 1, dtype=torch.int32, device=dev)
        ext = [tris.numel(), off.numel(), vol.numel(), 3 * T, T + 1]
        calls = {thr: (lambda thr=thr: K_.mesh_votes(tris.data_ptr(), off.data_ptr(), vol.data_ptr(), rows[thr].data_ptr(),
                                                     wide.data_ptr(), N, T, S, 4, thr, st, ext)) for thr in thresholds}
        for _ in range(a.warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        times = {thr: [] for thr in thresholds}
        for _ in range(a.iters):
            for thr, f in calls.items():
                times[thr].append(device_time(f, a.reps))
        return {thr: summary(v) for thr, v in times.items()}, rows

    for name, meshes in loads.items():
        tris_h, off_h = batch(meshes)
        tris, off = tris_h.to(dev), off_h.to(dev)
        cols = box_columns(tris_h.numpy())
        forms = {"wave": -1, "thread": cap, "default": meshlabel.THREAD_COLS}
        times, rows = timed(tris, off, sorted(set(forms.values())))
        res = {"triangles": int(tris.shape[0]), "box_columns_mean": round(float(cols.mean()), 2),
               "box_columns_max": int(cols.max()), "over_thread_cap": int((cols > cap).sum())}
        res.update({form: times[thr] for form, thr in forms.items()})
        ms = res["default"]["median_ms"]
        res["Mtris_per_s"] = round(tris.shape[0] / ms / 1e3, 2)
        # the oracle on the device, on the first meshes of the batch, scaled to the whole batch
        k = a.oracle_meshes
        sub_t, sub_o, sub_v = tris[:int(off_h[k])], off[:k + 1], vol[:k]
        want = reference.mesh_votes(sub_t, sub_o, sub_v, S)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reference.mesh_votes(sub_t, sub_o, sub_v, S)
        torch.cuda.synchronize()
        share = int(off_h[k]) / max(1, tris.shape[0])
        res["oracle_ms_scaled"] = round((time.perf_counter() - t0) * 1e3 / max(share, 1e-9), 1)
        res["oracle_over_kernel"] = round(res["oracle_ms_scaled"] / ms, 1)
        t0 = time.perf_counter()
        host = torch.from_numpy(rt.mesh_votes(tris_h.numpy(), off_h.numpy(), vol_h.numpy(), a.threads))
        res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res["host_over_kernel"] = round(res["host_ms"] / ms, 2)
        same = all(torch.equal(r.cpu(), host) for r in rows.values()) and torch.equal(want.cpu(), host[:int(off_h[k])])
        res["paths_agree"] = bool(same)
        res["labelled_share"] = round(float((host[:, 0] != 0).float().mean()), 4)
        res["centroid_share"] = round(float((host[:, 2] == 0).float().mean()), 4)
        ok &= same
        out[name] = res

    # the crossover: spheres whose triangles' boxes hold about `target` columns
    spheres = {sub: icosphere(sub) for sub in (5, 4, 3, 2)}
    edges = {sub: float(np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()) for sub, (v, f) in spheres.items()}
    cross = {}
    for target in (1, 2, 4, 8, 16, 32):
        # box side ~ one edge, in voxels; the finest sphere that still fits the grid at that edge
        sub = next((s for s in spheres if max(1.0, np.sqrt(target)) / edges[s] <= 0.49 * S), 2)
        (v, f), radius = spheres[sub], min(0.49 * S, max(1.0, np.sqrt(target)) / edges[sub])
        meshes = [np.rint((v @ rot.T) * (16 * radius) + 8 * S).astype(np.int32)[f].reshape(-1, 9)
                  for rot in rotations(N, 5 + target)]
        tris_h, off_h = batch(meshes)
        tris, off = tris_h.to(dev), off_h.to(dev)
        cols = box_columns(tris_h.numpy())
        times, rows = timed(tris, off, [-1] + list(range(cap + 1)))
        same = all(torch.equal(r, rows[-1]) for r in rows.values())
        ok &= same
        cross[f"about_{target}"] = {"triangles": int(tris.shape[0]), "radius_voxels": round(radius, 2), "box_columns_mean": round(float(cols.mean()), 2),
                                    "share_at_most": {str(t): round(float((cols <= t).mean()), 3) for t in (1, 2, 4, 8, 16)},
                                    "median_ms": {("wave" if t < 0 else str(t)): s["median_ms"] for t, s in times.items()},
                                    "rows_agree": bool(same)}
    out["crossover"] = cross
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
