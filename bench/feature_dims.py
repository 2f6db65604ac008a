#!/usr/bin/env python3
"""Dimensions of feature instances on the device (``ops.edt``, ``edt.hip``): the two transform
launches and the stats launch, each timed on its own, against three yardsticks measured in the
same process -- ``reference.distance_sq`` + ``reference.dimension_table`` on device tensors (the
plain-torch min-plus formulation), ``scipy.ndimage.distance_transform_edt`` + ``ndimage.maximum``
per instance on the host (when scipy is installed), and a device copy of the ``d2`` volume (4 B
read and 4 B written per voxel: the memory floor of one pass over it).

    python bench/feature_dims.py --iters 20 --md profiles/feature_dims.md

Volumes: generated parts (``fn.generate_parts``: the occupancy and the true labels), 32 x 64^3 and
4 x 128^3 (``--shapes BATCHxSIZE ...``).  Every launch is warmed up and timed with device events as
``--reps`` launches back to back, per launch; the kernels' results are compared with the torch
formulation's (``torch.equal``) before anything is timed.  ``--md`` writes the tables and the
compiler's resource report of the kernels (VGPRs, SGPRs, LDS, scratch; needs ``hipcc``) as
Markdown.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("edt_xy_kernel", "edt_z_kernel", "edt_init_kernel", "edt_stats_kernel")


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
    """[(kernel, VGPRs, SGPRs, scratch B/lane, static LDS B/workgroup, occupancy)] of the edt kernels,
    from hipcc's -Rpass-analysis=kernel-resource-usage; [] without hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        return []
    src = os.path.join(ROOT, "featurenet_amd", "csrc", "kernels", "edt.hip")
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


def host_scipy(occ: np.ndarray, ids: np.ndarray):
    """(seconds, largest d2 per instance) of scipy's transform and a per-instance maximum; None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t0 = time.perf_counter()
    r2 = []
    for o, i in zip(occ, ids):
        d = ndimage.distance_transform_edt(o == 0) if o.any() else np.full(o.shape, np.inf)
        n = int(i.max())
        r2.append(np.rint(np.asarray(ndimage.maximum(d, i, np.arange(1, n + 1))) ** 2) if n else np.zeros(0))
    return time.perf_counter() - t0, np.concatenate(r2)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32x64", "4x128"], metavar="BATCHxSIZE")
    ap.add_argument("--iters", type=int, default=20, help="timed samples of each launch (alternating)")
    ap.add_argument("--reps", type=int, default=10, help="launches back to back per sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default="", metavar="OUT.md", help="also write the results as Markdown")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("feature_dims: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1:
        ap.error("--iters, --reps and --warmup must be >= 1")
    import featurenet_amd as fn
    from featurenet_amd import _native
    from featurenet_amd.ops import ccl, edt, reference

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
        t = torch.empty(occ.shape, dtype=torch.int32, device=dev)
        d2, spare = torch.empty_like(t), torch.empty_like(t)
        raw = torch.empty(T, 3, dtype=torch.int64, device=dev)

        def xy():
            K.edt_transform(occ.data_ptr(), t.data_ptr(), d2.data_ptr(), N, S, S, S, False, 1, st, [V, V, V])

        def z():
            K.edt_transform(occ.data_ptr(), t.data_ptr(), d2.data_ptr(), N, S, S, S, False, 2, st, [V, V, V])

        def stats():
            K.edt_stats(ids.data_ptr(), offsets.data_ptr(), d2.data_ptr(), raw.data_ptr(), N, S, S, S, T, st,
                        [V, N + 1, V, T * 3])

        def copy():
            spare.copy_(d2)

        def torch_formulation():
            w = reference.distance_sq(occ)
            return w, reference.dimension_table(ids, offsets, w)

        xy(), z(), stats()
        want_d2, want_dim = torch_formulation()
        dim, _ = edt.dimension_table(ids, offsets, occ, rows=T)
        same = bool(torch.equal(d2, want_d2)) and bool(torch.equal(dim, want_dim)) and \
            bool(torch.equal(dim[:, 3], table[:, 2])) and bool(torch.equal(raw[:, 2], table[:, 2]))
        host = host_scipy(vox, ids.cpu().numpy())
        if host is not None:
            same = same and np.array_equal(host[1], want_dim[:, 0].cpu().numpy())
        ok = ok and same
        timed = {"edt_xy": (xy, a.reps), "edt_z": (z, a.reps), "edt_stats": (stats, a.reps), "copy": (copy, a.reps),
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
        three = r["edt_xy"]["median_us"] + r["edt_z"]["median_us"] + r["edt_stats"]["median_us"]
        r.update(instances=T, voxels_in_instances=int(table[:, 2].sum()), equals_torch_formulation=same,
                 three_launches_us=round(three, 2), three_over_copy=round(three / r["copy"]["median_us"], 2),
                 torch_over_kernels=round(r["torch_formulation"]["median_us"] / three, 1),
                 host_scipy_us=None if host is None else round(host[0] * 1e6, 1),
                 scipy_over_kernels=None if host is None else round(host[0] * 1e6 / three, 1))
        res[f"{N} x {S}^3"] = r
    out = {"metric": "feature dimensions", "iters": a.iters, "reps": a.reps, "volumes": res}
    print(json.dumps(out))
    if a.md:
        names = list(res)
        lines = [f"## Timing (generated parts, device events, {a.reps} launches back to back, {a.iters} samples; "
                 "median (min - max), microseconds per launch)", "",
                 "| | " + " | ".join(names) + " |", "|---|" + "---|" * len(names),
                 "| instances | " + " | ".join(f"{res[n]['instances']:,}" for n in names) + " |"]
        for k, label in (("edt_xy", "`edt_xy_kernel`"), ("edt_z", "`edt_z_kernel`"),
                         ("edt_stats", "`edt_init_kernel` + `edt_stats_kernel`"),
                         ("copy", "yardstick: device copy of the `d2` volume"),
                         ("torch_formulation", "yardstick: `reference.distance_sq` + `dimension_table` on the device")):
            lines.append(f"| {label} | " + " | ".join(
                f"{res[n][k]['median_us']:,.1f} ({res[n][k]['min_us']:,.1f} - {res[n][k]['max_us']:,.1f})"
                for n in names) + " |")
        lines.append("| yardstick: scipy `distance_transform_edt` + `ndimage.maximum` on the host (one run) | " +
                     " | ".join("n/a" if res[n]["host_scipy_us"] is None else f"{res[n]['host_scipy_us']:,.0f}"
                                for n in names) + " |")
        lines.append("| three launches | " + " | ".join(f"{res[n]['three_launches_us']:,.1f}" for n in names) + " |")
        lines.append("| **three launches / copy** | " +
                     " | ".join(f"**{res[n]['three_over_copy']:.2f}**" for n in names) + " |")
        lines.append("| **torch formulation / three launches** | " +
                     " | ".join(f"**{res[n]['torch_over_kernels']:.0f}x**" for n in names) + " |")
        lines.append("| **host scipy / three launches** | " +
                     " | ".join("n/a" if res[n]["scipy_over_kernels"] is None else
                                f"**{res[n]['scipy_over_kernels']:,.0f}x**" for n in names) + " |")
        lines.append("| equals the torch formulation (and scipy's r2) | " +
                     " | ".join(str(res[n]["equals_torch_formulation"]).lower() for n in names) + " |")
        rows = resource_usage()
        lines += ["", "## Resource usage (gfx950, `-O3 -Rpass-analysis=kernel-resource-usage`)", "",
                  "The compiler's figures, not a run.  The LDS column is the static part: `edt_xy_kernel` adds "
                  "H x 128 B and `edt_z_kernel` D x 256 B at launch.", "",
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
            f.write("# Dimensions of feature instances (`edt.hip`)\n\n`python bench/feature_dims.py "
                    f"--shapes {' '.join(a.shapes)} --iters {a.iters} --reps {a.reps} --md OUT.md` on 1 x MI355X wrote "
                    "the two sections below.\n\n" + "\n".join(lines) + "\n" + notes)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
