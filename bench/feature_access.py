#!/usr/bin/env python3
"""Access directions of feature instances on the device (``ops.access``, ``access.hip``): the
extents launch and the stats launch against two yardsticks measured in the same process --
``reference.access_table`` on device tensors (the plain-torch formulation: ``amin`` / ``amax`` over
index grids, then one ``bincount`` per column) and the ``ccl_stats`` launch on the same volume (the
kernel whose structure ``access_stats`` follows; it reads 9 B and writes 4 B per voxel).

    python bench/feature_access.py --size 64 --batch 32 --iters 20 --md profiles/feature_access.md

Volumes, ``batch`` x ``size``^3 each: generated parts (``fn.generate_parts``: the occupancy and the
true labels), solid (all material, one instance per sample), empty (no material, one instance per
sample), noise (half the voxels material, per-voxel random classes).  Every launch is warmed up and
timed with device events as ``--reps`` launches back to back, per launch; the result of the kernels
is compared with the torch formulation's before anything is timed.  ``--md`` writes the table, the
two ratios and the compiler's resource report of the kernels (VGPRs, SGPRs, LDS, scratch; needs
``hipcc``) as Markdown.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    """[(kernel, VGPRs, SGPRs, scratch B/lane, LDS B/workgroup, occupancy)] of the access kernels and
    of ccl_stats_kernel, from hipcc's -Rpass-analysis=kernel-resource-usage; [] without hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        return []
    rows = []
    src = os.path.join(ROOT, "featurenet_amd", "csrc", "kernels")
    for name, want in (("access.hip", ("access_extents_kernel", "access_init_kernel", "access_stats_kernel")),
                       ("ccl.hip", ("ccl_stats_kernel",))):
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", os.path.join(src, name), "-o",
                            os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        cur = {}
        for line in p.stderr.splitlines():
            m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|"
                          r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                cur = {"name": m.group(2)}
            cur[m.group(1)] = m.group(2)
            if m.group(1).startswith("LDS"):
                k = next((w for w in want if w in cur["name"]), None)
                if k:
                    rows.append((k, cur["VGPRs"], cur["TotalSGPRs"], cur["ScratchSize [bytes/lane]"],
                                 cur["LDS Size [bytes/block]"], cur["Occupancy [waves/SIMD]"]))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--classes", type=int, default=25, help="classes of the noise volume")
    ap.add_argument("--iters", type=int, default=20, help="timed samples of each launch (alternating)")
    ap.add_argument("--reps", type=int, default=10, help="launches back to back per sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default="", metavar="OUT.md", help="also write the results as Markdown")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("feature_access: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1:
        ap.error("--iters, --reps and --warmup must be >= 1")
    import featurenet_amd as fn
    from featurenet_amd import _native
    from featurenet_amd.ops import access, ccl, reference

    dev = torch.device("cuda")
    S, N = a.size, a.batch
    rng = np.random.default_rng(0)
    vox, labels, _ = fn.generate_parts(N, size=S, seed=0, device="cuda")
    full = np.ones((N, S, S, S), np.uint8)
    vols = {"parts": (vox, labels), "solid": (full, full), "empty": (0 * full, full),
            "noise": ((rng.random((N, S, S, S)) < 0.5).astype(np.uint8),
                      rng.integers(0, a.classes, (N, S, S, S)).astype(np.uint8))}
    K = _native.kernels()
    res, ok = {}, True
    for name, (o, l) in vols.items():
        occ, lab = torch.from_numpy(o).to(dev), torch.from_numpy(l).to(dev)
        st = _native.stream(occ)
        roots, flags = ccl.connected_components(lab, 0, 6, return_flags=True)
        rank = torch.cumsum(flags.reshape(-1), 0, dtype=torch.int32)
        ids, table, offsets = ccl.instance_table(lab, roots, want_ids=True, flags=flags)
        T = int(table.shape[0])
        ex, ey, ez = access.column_extents(occ)
        acc = torch.empty(T, 8, dtype=torch.int64, device=dev)
        ids2, table2 = torch.empty_like(ids), torch.empty_like(table)
        V = occ.numel()

        def extents():
            K.access_extents(occ.data_ptr(), ex.data_ptr(), ey.data_ptr(), ez.data_ptr(), N, S, S, S, st,
                             [V, ex.numel(), ey.numel(), ez.numel()])

        def stats():
            K.access_stats(ids.data_ptr(), offsets.data_ptr(), ex.data_ptr(), ey.data_ptr(), ez.data_ptr(), 0,
                           acc.data_ptr(), N, S, S, S, T, st, [V, N + 1, ex.numel(), ey.numel(), ez.numel(), 0, T * 8])

        def ccl_stats():
            K.ccl_stats(lab.data_ptr(), roots.data_ptr(), rank.data_ptr(), ids2.data_ptr(), table2.data_ptr(), N, S, S,
                        S, T, st, [V, V, V, V, T * 13])

        def torch_formulation():
            return reference.access_table(ids, offsets, occ)

        stats()
        want, _ = torch_formulation()
        same = bool(torch.equal(acc, want)) and bool(torch.equal(acc[:, 7], table[:, 2]))
        ok = ok and same
        timed = {"access_extents": (extents, a.reps), "access_stats": (stats, a.reps), "ccl_stats": (ccl_stats, a.reps),
                 "torch_formulation": (torch_formulation, 1)}
        for f, _ in timed.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in timed}
        for _ in range(a.iters):
            for k, (f, reps) in timed.items():
                times[k].append(device_time_us(f, reps))
        r = {k: summary(v) for k, v in times.items()}
        both = r["access_extents"]["median_us"] + r["access_stats"]["median_us"]
        r.update(instances=T, voxels_in_instances=int(table[:, 2].sum()), equals_torch_formulation=same,
                 stats_over_ccl_stats=round(r["access_stats"]["median_us"] / r["ccl_stats"]["median_us"], 3),
                 torch_over_kernels=round(r["torch_formulation"]["median_us"] / both, 1))
        res[name] = r
    out = {"metric": f"feature access, {N} x {S}^3", "iters": a.iters, "reps": a.reps, "volumes": res}
    print(json.dumps(out))
    if a.md:
        names = list(res)
        lines = [f"## Timing ({N} x {S}^3 voxels per launch, device events, {a.reps} launches back to back, "
                 f"{a.iters} samples; median (min - max), microseconds per launch)", "",
                 "| | " + " | ".join(names) + " |", "|---|" + "---|" * len(names),
                 "| instances | " + " | ".join(f"{res[n]['instances']:,}" for n in names) + " |"]
        for k, label in (("access_extents", "`access_extents_kernel`"),
                         ("access_stats", "`access_init_kernel` + `access_stats_kernel`"),
                         ("ccl_stats", "yardstick: `ccl_table_init_kernel` + `ccl_stats_kernel`"),
                         ("torch_formulation", "yardstick: `reference.access_table` on the device")):
            lines.append(f"| {label} | " + " | ".join(
                f"{res[n][k]['median_us']:,.1f} ({res[n][k]['min_us']:,.1f} - {res[n][k]['max_us']:,.1f})"
                for n in names) + " |")
        lines.append("| **stats launch / `ccl_stats` launch** | " +
                     " | ".join(f"**{res[n]['stats_over_ccl_stats']:.2f}**" for n in names) + " |")
        lines.append("| **torch formulation / (extents + stats)** | " +
                     " | ".join(f"**{res[n]['torch_over_kernels']:.0f}x**" for n in names) + " |")
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
            f.write("# Access directions of feature instances (`access.hip`)\n\n`python bench/feature_access.py "
                    f"--size {S} --batch {N} --iters {a.iters} --reps {a.reps} --md OUT.md` on 1 x MI355X wrote the "
                    "two sections below.\n\n" + "\n".join(lines) + "\n" + notes)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
