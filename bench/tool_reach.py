#!/usr/bin/env python3
"""Tool reach of feature instances on the device (``ops.reach``, ``reach.hip``): the scan launch and
the stats launch, each timed on its own, against two yardsticks measured in the same process -- a
device copy of the bytes the launch moves (the scan reads 4 B and writes 24 B per voxel; the stats
pass reads 32 B per voxel) and the torch formulation on the same device tensors
(``reference.reach_scan``: six ``cummin``; ``reference.reach_table``: ``scatter_reduce`` and
``bincount``).  The steps between the two launches (the seeds, a torch reduction, and their distance
transform, the ``edt`` kernels) are timed too, for the whole of ``reach_table``.

    python bench/tool_reach.py --iters 20 --md profiles/tool_reach.md

Volumes: generated parts (``fn.generate_parts``: the occupancy and the true labels), 32 x 64^3 and
4 x 128^3 (``--shapes BATCHxSIZE ...``); the tool has ``--tool`` voxels diameter (default 3).  Every
launch is warmed up and timed with device events as ``--reps`` launches back to back, per launch;
the kernels' results are compared with the torch formulation's (``torch.equal``) before anything is
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

KERNELS = ("reach_scan_kernel", "reach_init_kernel", "reach_stats_kernel")


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
    """[(kernel, VGPRs, SGPRs, scratch B/lane, static LDS B/workgroup, occupancy)] of the reach kernels,
    from hipcc's -Rpass-analysis=kernel-resource-usage; [] without hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        return []
    src = os.path.join(ROOT, "featurenet_amd", "csrc", "kernels", "reach.hip")
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
    ap.add_argument("--shapes", nargs="+", default=["32x64", "4x128"], metavar="BATCHxSIZE")
    ap.add_argument("--tool", type=float, default=3.0, help="tool diameter in voxels")
    ap.add_argument("--iters", type=int, default=20, help="timed samples of each launch (alternating)")
    ap.add_argument("--reps", type=int, default=10, help="launches back to back per sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default="", metavar="OUT.md", help="also write the results as Markdown")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("tool_reach: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1:
        ap.error("--iters, --reps and --warmup must be >= 1")
    import featurenet_amd as fn
    from featurenet_amd import _native
    from featurenet_amd.ops import ccl, edt, reach, reference
    from featurenet_amd.utils.seginstances import tool_thresholds

    need2, cut2 = tool_thresholds(a.tool)
    dev = torch.device("cuda")
    K = _native.kernels()
    res, ok = {}, True
    for shape in a.shapes:
        N, S = (int(v) for v in shape.split("x"))
        vox, labels, _ = fn.generate_parts(N, size=S, seed=0, device="cuda")
        occ, lab = torch.from_numpy(vox).to(dev), torch.from_numpy(labels).to(dev)
        st = _native.stream(occ)
        roots, flags = ccl.connected_components(lab, 0, 6, return_flags=True)
        ids, table, offsets = ccl.instance_table(lab, roots, want_ids=True, flags=flags)
        T, V = int(table.shape[0]), occ.numel()
        d2 = edt.distance_sq(occ)
        r6 = torch.empty(N, 6, S, S, S, dtype=torch.int32, device=dev)
        spare6 = torch.empty_like(r6)
        raw = torch.empty(T, 15, dtype=torch.int64, device=dev)
        src4, spare4 = torch.zeros(4 * V, dtype=torch.int32, device=dev), torch.empty(4 * V, dtype=torch.int32, device=dev)
        d2x6 = d2[:, None].expand(N, 6, S, S, S)

        def scan():
            K.reach_scan(d2.data_ptr(), r6.data_ptr(), N, S, S, S, st, [V, 6 * V])

        scan()
        seeds = reference.reach_seeds(r6, need2)
        dc2 = edt.distance_sq(seeds)

        def stats():
            K.reach_stats(ids.data_ptr(), offsets.data_ptr(), r6.data_ptr(), dc2.data_ptr(), raw.data_ptr(), N, S, S, S,
                          T, need2, cut2, st, [V, N + 1, 6 * V, V, T * 15])

        def between():
            return edt.distance_sq(reference.reach_seeds(r6, need2))

        def copy_scan():                             # 4 B read (six times, five of them from cache), 24 B written
            spare6.copy_(d2x6)

        def copy_stats():                            # 16 B read and 16 B written: the 32 B the stats pass reads
            spare4.copy_(src4)

        def torch_scan():
            return reference.reach_scan(d2)

        def torch_table():
            return reference.reach_table(ids, offsets, r6, dc2, need2, cut2)

        def whole():
            return reach.reach_table(ids, offsets, occ, need2, cut2, rows=T, d2=d2)[0]

        stats()
        same = bool(torch.equal(r6, torch_scan())) and bool(torch.equal(raw, torch_table())) and \
            bool(torch.equal(whole(), raw)) and bool(torch.equal(raw[:, 14], table[:, 2]))
        ok = ok and same
        timed = {"reach_scan": (scan, a.reps), "reach_stats": (stats, a.reps), "between": (between, a.reps),
                 "whole": (whole, a.reps), "copy_scan": (copy_scan, a.reps), "copy_stats": (copy_stats, a.reps),
                 "torch_scan": (torch_scan, 1), "torch_table": (torch_table, 1)}
        for f, _ in timed.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in timed}
        for _ in range(a.iters):
            for k, (f, reps) in timed.items():
                times[k].append(device_time_us(f, reps))
        r = {k: summary(v) for k, v in times.items()}
        two = r["reach_scan"]["median_us"] + r["reach_stats"]["median_us"]
        both = r["torch_scan"]["median_us"] + r["torch_table"]["median_us"]
        r.update(instances=T, voxels_in_instances=int(table[:, 2].sum()), equals_torch_formulation=same,
                 two_launches_us=round(two, 2), torch_us=round(both, 2), torch_over_kernels=round(both / two, 1),
                 scan_over_copy=round(r["reach_scan"]["median_us"] / r["copy_scan"]["median_us"], 2),
                 stats_over_copy=round(r["reach_stats"]["median_us"] / r["copy_stats"]["median_us"], 2),
                 scan_gb_s=round(28 * V / r["reach_scan"]["median_us"] / 1e3, 1),
                 stats_gb_s=round(32 * V / r["reach_stats"]["median_us"] / 1e3, 1))
        res[f"{N} x {S}^3"] = r
    out = {"metric": "tool reach", "tool": [need2, cut2], "iters": a.iters, "reps": a.reps, "volumes": res}
    print(json.dumps(out))
    if a.md:
        names = list(res)
        lines = [f"## Timing (generated parts, tool need2 = {need2}, cut2 = {cut2}; device events, {a.reps} launches "
                 f"back to back, {a.iters} samples; median (min - max), microseconds per launch)", "",
                 "| | " + " | ".join(names) + " |", "|---|" + "---|" * len(names),
                 "| instances | " + " | ".join(f"{res[n]['instances']:,}" for n in names) + " |"]
        for k, label in (("reach_scan", "`reach_scan_kernel`"),
                         ("copy_scan", "yardstick: device copy, 4 B read and 24 B written per voxel"),
                         ("torch_scan", "yardstick: `reference.reach_scan` (six `cummin`) on the device"),
                         ("reach_stats", "`reach_init_kernel` + `reach_stats_kernel`"),
                         ("copy_stats", "yardstick: device copy, 16 B read and 16 B written per voxel"),
                         ("torch_table", "yardstick: `reference.reach_table` (`scatter_reduce`, `bincount`) on the "
                                         "device"),
                         ("between", "between the two: seeds (torch `any`) + `edt_xy_kernel` + `edt_z_kernel`"),
                         ("whole", "`ops.reach.reach_table` given `d2`, host time included")):
            lines.append(f"| {label} | " + " | ".join(
                f"{res[n][k]['median_us']:,.1f} ({res[n][k]['min_us']:,.1f} - {res[n][k]['max_us']:,.1f})"
                for n in names) + " |")
        lines.append("| scan + stats | " + " | ".join(f"{res[n]['two_launches_us']:,.1f}" for n in names) + " |")
        lines.append("| torch formulation of the two | " + " | ".join(f"{res[n]['torch_us']:,.1f}" for n in names) + " |")
        lines.append("| **torch formulation / (scan + stats)** | " +
                     " | ".join(f"**{res[n]['torch_over_kernels']:.1f}x**" for n in names) + " |")
        lines.append("| **scan / its copy** | " + " | ".join(f"**{res[n]['scan_over_copy']:.2f}**" for n in names) + " |")
        lines.append("| **stats / its copy** | " + " | ".join(f"**{res[n]['stats_over_copy']:.2f}**" for n in names) + " |")
        lines.append("| scan, GB/s of the 28 B per voxel | " + " | ".join(f"{res[n]['scan_gb_s']:,.0f}" for n in names) + " |")
        lines.append("| stats, GB/s of the 32 B per voxel | " + " | ".join(f"{res[n]['stats_gb_s']:,.0f}" for n in names) + " |")
        lines.append("| equals the torch formulation | " +
                     " | ".join(str(res[n]["equals_torch_formulation"]).lower() for n in names) + " |")
        rows = resource_usage()
        lines += ["", "## Resource usage (gfx950, `-O3 -Rpass-analysis=kernel-resource-usage`)", "",
                  "The compiler's figures, not a run.", "",
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
            f.write("# Tool reach of feature instances (`reach.hip`)\n\n`python bench/tool_reach.py "
                    f"--shapes {' '.join(a.shapes)} --tool {a.tool:g} --iters {a.iters} --reps {a.reps} --md OUT.md` on "
                    "1 x MI355X wrote the two sections below.\n\n" + "\n".join(lines) + "\n" + notes)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
