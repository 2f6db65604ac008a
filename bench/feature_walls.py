#!/usr/bin/env python3
"""Walls between feature instances on the device (``ops.nearest``, ``nearest.hip``): the two transform
launches and the stats launch, each timed on its own, against three yardsticks measured in the same
process -- a device copy of the bytes the three launches move (4 B read and 2 x 16 B written per
voxel, plus the 16 B the second pass and the stats pass read again: 52 B per voxel, copied as 26 B),
the ``edt`` kernels on the same occupancy (``ids > 0``: one int32 instead of two keys per voxel), and
``reference.nearest_labels`` + ``reference.wall_table`` on device tensors (the plain-torch
formulation: one distance transform per label).

    python bench/feature_walls.py --iters 20 --md profiles/feature_walls.md

Volumes: 32 x 64^3 (``--shapes BATCHxSIZE ...``, each axis at most 128), twice: the instance ids of
generated parts (``fn.generate_parts``), and the same volumes with every instance given id 1 -- the
worst case, because with a single label rank 1 stays missing and no column scan stops early.  Every
launch is warmed up and timed with device events as ``--reps`` launches back to back, per launch; the
kernels' results are compared with the torch formulation's (``torch.equal``) before anything is
timed.  ``--md`` writes the tables and the compiler's resource report of the kernels (VGPRs, SGPRs,
LDS, scratch; needs ``hipcc``) as Markdown.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("nn_xy_kernel", "nn_z_kernel", "wall_init_kernel", "wall_stats_kernel")


def summary(t: list) -> dict:
    t = sorted(t)
    return {"median_us": round(statistics.median(t), 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2)}


def device_time_us(f, reps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def resource_usage() -> list:
    """[(kernel, VGPRs, SGPRs, scratch B/lane, static LDS B/workgroup, occupancy)] of the nearest kernels,
    from hipcc's -Rpass-analysis=kernel-resource-usage; [] without hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        return []
    src = os.path.join(ROOT, "featurenet_amd", "csrc", "kernels", "nearest.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    rows, cur = [], {}
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
        cur[m.group(1)] = m.group(2)
        if m.group(1).startswith("LDS"):
            k = next((w for w in KERNELS if w in cur["name"]), None)
            if k:
                rows.append((k, cur["VGPRs"], cur["TotalSGPRs"], cur["ScratchSize [bytes/lane]"],
                             cur["LDS Size [bytes/block]"], cur["Occupancy [waves/SIMD]"]))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32x64"], metavar="BATCHxSIZE")
    ap.add_argument("--iters", type=int, default=20, help="timed samples of each launch (alternating)")
    ap.add_argument("--reps", type=int, default=10, help="launches back to back per sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit2", type=int, default=4, help="the thin limit of the stats launch (a wall of 1 voxel)")
    ap.add_argument("--md", default="", metavar="OUT.md", help="also write the results as Markdown")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("feature_walls: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1:
        ap.error("--iters, --reps and --warmup must be >= 1")
    import featurenet_amd as fn
    from featurenet_amd import _native
    from featurenet_amd.ops import ccl, nearest, reference

    dev = torch.device("cuda")
    K = _native.kernels()
    res, ok = {}, True
    for shape in a.shapes:
        N, S = (int(v) for v in shape.split("x"))
        _, labels, _ = fn.generate_parts(N, size=S, seed=0, device="cuda")
        lab = torch.from_numpy(labels).to(dev)
        roots, flags = ccl.connected_components(lab, 0, 6, return_flags=True)
        part_ids, table, offsets = ccl.instance_table(lab, roots, want_ids=True, flags=flags)
        one_ids = (part_ids > 0).to(torch.int32)
        one_offsets = torch.arange(N + 1, dtype=torch.int64, device=dev)
        for case, ids, off, T in (("generated parts", part_ids, offsets, int(table.shape[0])),
                                  ("single instance", one_ids, one_offsets, N)):
            st = _native.stream(ids)
            V = ids.numel()
            occ = (ids > 0).to(torch.uint8)
            t = torch.empty((N, 2, S, S, S), dtype=torch.int64, device=dev)
            nn = torch.empty_like(t)
            raw = torch.empty(T, 3, dtype=torch.int64, device=dev)
            moved, spare = (torch.empty(26 * V, dtype=torch.uint8, device=dev) for _ in range(2))
            e_t = torch.empty(ids.shape, dtype=torch.int32, device=dev)
            e_d2 = torch.empty_like(e_t)

            def xy():
                K.nn_transform(ids.data_ptr(), t.data_ptr(), nn.data_ptr(), N, S, S, S, 1, st, [V, 2 * V, 2 * V])

            def z():
                K.nn_transform(ids.data_ptr(), t.data_ptr(), nn.data_ptr(), N, S, S, S, 2, st, [V, 2 * V, 2 * V])

            def stats():
                K.wall_stats(ids.data_ptr(), off.data_ptr(), nn.data_ptr(), raw.data_ptr(), N, S, S, S, T, a.limit2,
                             st, [V, N + 1, 2 * V, T * 3])

            def copy():
                spare.copy_(moved)

            def edt_xy():
                K.edt_transform(occ.data_ptr(), e_t.data_ptr(), e_d2.data_ptr(), N, S, S, S, False, 1, st, [V, V, V])

            def edt_z():
                K.edt_transform(occ.data_ptr(), e_t.data_ptr(), e_d2.data_ptr(), N, S, S, S, False, 2, st, [V, V, V])

            def torch_formulation():
                w = reference.nearest_labels(ids)
                return w, reference.wall_table(ids, off, w, a.limit2)

            xy(), z(), stats(), edt_xy(), edt_z()
            want_nn, want_wall = torch_formulation()
            wall, _ = nearest.wall_table(ids, off, a.limit2, rows=T)
            same = bool(torch.equal(nn, want_nn)) and bool(torch.equal(wall, want_wall)) and \
                bool(torch.equal(raw[:, 2], want_wall[:, 4])) and bool(torch.equal((nn[:, 0] >> 32).int(), e_d2))
            ok = ok and same
            timed = {"nn_xy": (xy, a.reps), "nn_z": (z, a.reps), "wall_stats": (stats, a.reps), "copy": (copy, a.reps),
                     "edt_xy": (edt_xy, a.reps), "edt_z": (edt_z, a.reps), "torch_formulation": (torch_formulation, 1)}
            for f, _ in timed.values():
                for _ in range(a.warmup):
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in timed}
            for i in range(a.iters):
                for k, (f, reps) in timed.items():
                    if k != "torch_formulation" or i < 3:          # (seconds per run: three samples)
                        times[k].append(device_time_us(f, reps))
            r = {k: summary(v) for k, v in times.items()}
            three = r["nn_xy"]["median_us"] + r["nn_z"]["median_us"] + r["wall_stats"]["median_us"]
            two_edt = r["edt_xy"]["median_us"] + r["edt_z"]["median_us"]
            r.update(instances=T, voxels_in_instances=int((ids > 0).sum()), equals_torch_formulation=same,
                     three_launches_us=round(three, 2), three_over_copy=round(three / r["copy"]["median_us"], 2),
                     transform_over_edt=round((r["nn_xy"]["median_us"] + r["nn_z"]["median_us"]) / two_edt, 2),
                     torch_over_kernels=round(r["torch_formulation"]["median_us"] / three, 1))
            res[f"{N} x {S}^3, {case}"] = r
    out = {"metric": "feature walls", "iters": a.iters, "reps": a.reps, "limit2": a.limit2, "volumes": res}
    print(json.dumps(out))
    if a.md:
        names = list(res)
        lines = [f"## Timing (device events, {a.reps} launches back to back, {a.iters} samples; "
                 "median (min - max), microseconds per launch)", "",
                 "| | " + " | ".join(names) + " |", "|---|" + "---|" * len(names),
                 "| instances | " + " | ".join(f"{res[n]['instances']:,}" for n in names) + " |",
                 "| voxels in instances | " + " | ".join(f"{res[n]['voxels_in_instances']:,}" for n in names) + " |"]
        for k, label in (("nn_xy", "`nn_xy_kernel`"), ("nn_z", "`nn_z_kernel`"),
                         ("wall_stats", "`wall_init_kernel` + `wall_stats_kernel`"),
                         ("copy", "yardstick: device copy of 26 B per voxel (52 B moved)"),
                         ("edt_xy", "yardstick: `edt_xy_kernel` on `ids > 0`"),
                         ("edt_z", "yardstick: `edt_z_kernel` on `ids > 0`"),
                         ("torch_formulation", "yardstick: `reference.nearest_labels` + `wall_table` on the device")):
            lines.append(f"| {label} | " + " | ".join(
                f"{res[n][k]['median_us']:,.1f} ({res[n][k]['min_us']:,.1f} - {res[n][k]['max_us']:,.1f})"
                for n in names) + " |")
        lines.append("| three launches | " + " | ".join(f"{res[n]['three_launches_us']:,.1f}" for n in names) + " |")
        lines.append("| **three launches / copy** | " +
                     " | ".join(f"**{res[n]['three_over_copy']:.2f}**" for n in names) + " |")
        lines.append("| **two transform launches / two `edt` launches** | " +
                     " | ".join(f"**{res[n]['transform_over_edt']:.2f}**" for n in names) + " |")
        lines.append("| **torch formulation / three launches** | " +
                     " | ".join(f"**{res[n]['torch_over_kernels']:,.0f}x**" for n in names) + " |")
        lines.append("| equals the torch formulation (and `edt`'s d2 in rank 0) | " +
                     " | ".join(str(res[n]["equals_torch_formulation"]).lower() for n in names) + " |")
        rows = resource_usage()
        lines += ["", "## Resource usage (gfx950, `-O3 -Rpass-analysis=kernel-resource-usage`)", "",
                  "The compiler's figures, not a run.  The LDS column is the static part: `nn_xy_kernel` adds "
                  "H x 1024 B and `nn_z_kernel` D x 1024 B at launch.", "",
                  "| kernel | VGPRs | SGPRs | scratch B/lane | LDS B/workgroup | occupancy waves/SIMD |",
                  "|---|---|---|---|---|---|"]
        lines += [f"| `{r[0]}` | " + " | ".join(r[1:]) + " |" for r in rows] or \
            ["| (no hipcc on this machine) | | | | | |"]
        notes = ""                                  # (hand-written findings below the figures survive a re-run)
        if os.path.exists(a.md):
            old = open(a.md).read()
            notes = old[old.index("\n## Notes"):] if "\n## Notes" in old else ""
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Walls between feature instances (`nearest.hip`)\n\n`python bench/feature_walls.py "
                    f"--shapes {' '.join(a.shapes)} --iters {a.iters} --reps {a.reps} --md OUT.md` on 1 x MI355X wrote "
                    "the two sections below.\n\n" + "\n".join(lines) + "\n" + notes)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
