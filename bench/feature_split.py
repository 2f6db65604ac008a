#!/usr/bin/env python3
"""The watershed split of touching features on the device (``ops.watershed``, ``watershed.hip``): its three
launches against two yardsticks measured in the same process -- a device copy that moves the bytes each launch
must move (12 B per voxel for all three: ``ws_ascend`` reads ids and height and writes parent, ``ws_resolve``
reads parent and writes roots and flags, ``ws_saddle`` reads ids, basin ids and height; the copy reads and writes
6 B per voxel) and the plain-torch formulation on device tensors (``reference.watershed_ascend``: 26 shifted views
and pointer doubling; ``reference.watershed_saddles``: 13 shifted views, ``torch.unique``, a scatter maximum).

    python bench/feature_split.py --size 64 --batch 32 --iters 20 --md profiles/feature_split.md

The volume: ``batch`` intersecting generated parts of ``size``^3 (``fn.generate_parts(separate=False)``), the
6-connected components of their removed volume over the squared distance to the material.  ``ws_ascend`` is timed
in both forms, the LDS tile and the plain 27 reads from global memory (``ops.watershed.STAGED`` names the one the
op runs); the pair table has the capacity the op settles on and its fill is timed apart, as is the whole of
``split_instances`` (the launches, ``ccl_stats``, the host's merge of the pair list and the relabelling; host time
included).  Every launch is warmed up and timed with
device events as ``--reps`` launches back to back, per launch; the kernels' results are compared with the torch
formulation's before anything is timed.  ``--md`` writes the table, the counts and the compiler's resource report
of the kernels (VGPRs, SGPRs, LDS, scratch; needs ``hipcc``) as Markdown.  Needs a GPU: there is no CPU fallback.
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

KERNELS = ("ws_ascend_kernel", "ws_ascend_plain_kernel", "ws_resolve_kernel", "ws_saddle_kernel")


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
    """[(kernel, VGPRs, SGPRs, scratch B/lane, LDS B/workgroup, occupancy)] of the watershed kernels, from hipcc's
    -Rpass-analysis=kernel-resource-usage; [] without hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        return []
    src = os.path.join(ROOT, "featurenet_amd", "csrc", "kernels", "watershed.hip")
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
            k = next((w for w in KERNELS if w + "P" in cur["name"] or cur["name"].endswith(w)), None)
            if k:
                rows.append((k, cur["VGPRs"], cur["TotalSGPRs"], cur["ScratchSize [bytes/lane]"],
                             cur["LDS Size [bytes/block]"], cur["Occupancy [waves/SIMD]"]))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--merge", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=20, help="timed samples of each launch (alternating)")
    ap.add_argument("--reps", type=int, default=10, help="launches back to back per sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default="", metavar="OUT.md", help="also write the results as Markdown")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("feature_split: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1:
        ap.error("--iters, --reps and --warmup must be >= 1")
    import featurenet_amd as fn
    from featurenet_amd import _native
    from featurenet_amd.ops import ccl, edt, reference, watershed

    dev = torch.device("cuda")
    S, N = a.size, a.batch
    vox, _, _ = fn.generate_parts(N, size=S, seed=0, device="cuda", separate=False)
    occ = torch.from_numpy(np.ascontiguousarray(vox)).to(dev)
    removed = (occ == 0).to(torch.uint8)
    roots0, flags0 = ccl.connected_components(removed, 0, 6, return_flags=True)
    ids, table0, _ = ccl.instance_table(removed, roots0, want_ids=True, flags=flags0)
    height = edt.distance_sq(occ)
    V = ids.numel()
    K, st = _native.kernels(), _native.stream(ids)
    parent, roots, flags = (torch.empty_like(ids) for _ in range(3))
    ext = [V, V, V]

    def ascend(staged):
        K.ws_ascend(ids.data_ptr(), height.data_ptr(), parent.data_ptr(), N, S, S, S, staged, st, ext)

    def resolve():
        K.ws_resolve(parent.data_ptr(), roots.data_ptr(), flags.data_ptr(), N, S, S, S, st, ext)

    want_parent = reference.watershed_parents(ids, height)
    want_roots = reference.watershed_ascend(ids, height)
    same = True
    for staged in (0, 1):
        parent.fill_(-1)
        ascend(staged)
        same = same and bool(torch.equal(parent, want_parent))
    resolve()
    same = same and bool(torch.equal(roots, want_roots))
    labels = (ids > 0).to(torch.uint8)
    bids, table, offsets = ccl.instance_table(labels, roots, want_ids=True, flags=flags)
    T = int(table.shape[0])
    want_pairs = reference.watershed_saddles(ids, bids, offsets, height)
    pairs = watershed.saddle_pairs(ids, bids, offsets, height, rows=T)
    same = same and bool(torch.equal(pairs, want_pairs))
    new, table2, _, _, _ = watershed.split_instances(ids, height, a.merge)
    # the capacity the op settles on: the first of its sizes that loses nothing
    cap = max(watershed.MIN_CAP, watershed._next_pow2(4 * T))
    while True:
        buf = torch.zeros(2 * cap + 1, dtype=torch.int64, device=dev)
        keys, counts, lost = buf[:cap], buf[cap:2 * cap], buf[2 * cap:]

        def saddle():
            K.ws_saddle(ids.data_ptr(), bids.data_ptr(), offsets.data_ptr(), height.data_ptr(), keys.data_ptr(),
                        counts.data_ptr(), lost.data_ptr(), N, S, S, S, T, cap, watershed.PROBE, st,
                        [V, V, N + 1, V, cap, cap, 1])

        saddle()
        if int(lost) == 0:
            break
        cap *= 4
    src, dst = torch.empty(6 * V, dtype=torch.uint8, device=dev), torch.empty(6 * V, dtype=torch.uint8, device=dev)
    src.zero_()
    rank = torch.cumsum(flags.reshape(-1), 0, dtype=torch.int32)
    tab = torch.empty(T, 13, dtype=torch.int64, device=dev)

    def stats():
        K.ccl_stats(labels.data_ptr(), roots.data_ptr(), rank.data_ptr(), bids.data_ptr(), tab.data_ptr(), N, S, S, S, T,
                    st, [V, V, V, V, T * 13])

    timed = {"ws_ascend": (lambda: ascend(1), a.reps), "ws_ascend_plain": (lambda: ascend(0), a.reps),
             "ws_resolve": (resolve, a.reps), "ws_saddle": (saddle, a.reps), "fill": (buf.zero_, a.reps),
             "ccl_stats": (stats, a.reps), "copy": (lambda: dst.copy_(src), a.reps),
             "torch_ascend": (lambda: reference.watershed_ascend(ids, height), 1),
             "torch_saddles": (lambda: reference.watershed_saddles(ids, bids, offsets, height), 1)}
    for f, _ in timed.values():
        for _ in range(a.warmup):
            f()
    ascend(1)                                    # (resolve reads what the op's form wrote: the same parents either way)
    torch.cuda.synchronize()
    times = {k: [] for k in timed}
    times["whole"] = []
    for _ in range(a.iters):
        for k, (f, reps) in timed.items():
            if k == "ws_saddle":
                buf.zero_()
            times[k].append(device_time_us(f, reps))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        watershed.split_instances(ids, height, a.merge)
        torch.cuda.synchronize()
        times["whole"].append((time.perf_counter() - t0) * 1e6)
    r = {k: summary(v) for k, v in times.items()}
    med = {k: v["median_us"] for k, v in r.items()}
    r.update(voxels=V, voxels_in_components=int(table0[:, 2].sum()), components=int(table0.shape[0]), basins=T,
             pairs=int(pairs.shape[0]), table_slots=cap, instances=int(table2.shape[0]), merge=a.merge,
             equals_torch_formulation=same,
             ascend_over_copy=round(med["ws_ascend"] / med["copy"], 2),
             plain_over_ascend=round(med["ws_ascend_plain"] / med["ws_ascend"], 2),
             resolve_over_copy=round(med["ws_resolve"] / med["copy"], 2),
             saddle_over_copy=round(med["ws_saddle"] / med["copy"], 2),
             torch_ascend_over_kernels=round(med["torch_ascend"] / (med["ws_ascend"] + med["ws_resolve"]), 1),
             torch_saddles_over_kernel=round(med["torch_saddles"] / med["ws_saddle"], 1))
    out = {"metric": f"feature split, {N} x {S}^3", "iters": a.iters, "reps": a.reps, "parts": r}
    print(json.dumps(out))
    if a.md:
        lines = ["## Counts", "", "| | |", "|---|---|"]
        for k, label in (("voxels", "voxels"), ("voxels_in_components", "voxels in components"),
                         ("components", "components (6-connected, before the split)"), ("basins", "basins"),
                         ("pairs", "rows of `pairs` (touching basins)"), ("table_slots", "pair-table slots"),
                         ("instances", f"instances at `merge={a.merge:g}`")):
            lines.append(f"| {label} | {r[k]:,} |")
        lines += ["", f"## Timing ({N} x {S}^3 voxels per launch, device events, {a.reps} launches back to back, "
                  f"{a.iters} samples; median (min - max), microseconds per launch)", "", "| | |", "|---|---|"]
        for k, label in (("ws_ascend", "`ws_ascend_kernel` (LDS tile + halo)"),
                         ("ws_ascend_plain", "`ws_ascend_plain_kernel` (27 reads of each array)"),
                         ("ws_resolve", "`ws_resolve_kernel`"), ("ws_saddle", "`ws_saddle_kernel`"),
                         ("fill", "zero-fill of the pair table"),
                         ("ccl_stats", "`ccl_table_init_kernel` + `ccl_stats_kernel` over the basins"),
                         ("copy", "yardstick: device copy that moves 12 B per voxel (6 B read, 6 B written)"),
                         ("torch_ascend", "yardstick: `reference.watershed_ascend` on the device"),
                         ("torch_saddles", "yardstick: `reference.watershed_saddles` on the device"),
                         ("whole", "`ops.watershed.split_instances`, host time included")):
            lines.append(f"| {label} | {r[k]['median_us']:,.1f} ({r[k]['min_us']:,.1f} - {r[k]['max_us']:,.1f}) |")
        for k, label, unit in (("ascend_over_copy", "`ws_ascend` / copy", ""),
                               ("plain_over_ascend", "plain `ws_ascend` / tile-staged `ws_ascend`", ""),
                               ("resolve_over_copy", "`ws_resolve` / copy", ""),
                               ("saddle_over_copy", "`ws_saddle` / copy", ""),
                               ("torch_ascend_over_kernels", "torch ascent / (`ws_ascend` + `ws_resolve`)", "x"),
                               ("torch_saddles_over_kernel", "torch saddles / `ws_saddle`", "x")):
            lines.append(f"| **{label}** | **{r[k]:.2f}{unit}** |")
        lines.append(f"| equals the torch formulation | {str(same).lower()} |")
        rows = resource_usage()
        lines += ["", "## Resource usage (gfx950, `-O3 -Rpass-analysis=kernel-resource-usage`)", "",
                  "The compiler's figures, not a run.", "",
                  "| kernel | VGPRs | SGPRs | scratch B/lane | LDS B/workgroup | occupancy waves/SIMD |",
                  "|---|---|---|---|---|---|"]
        lines += [f"| `{r_[0]}` | " + " | ".join(r_[1:]) + " |" for r_ in rows] or \
            ["| (no hipcc on this machine) | | | | | |"]
        notes = ""                                  # (hand-written findings below the figures survive a re-run)
        if os.path.exists(a.md):
            old = open(a.md).read()
            notes = old[old.index("\n## Notes"):] if "\n## Notes" in old else ""
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Watershed split of touching features (`watershed.hip`)\n\n`python bench/feature_split.py "
                    f"--size {S} --batch {N} --iters {a.iters} --reps {a.reps} --md OUT.md` on 1 x MI355X wrote the "
                    "three sections below.\n\n" + "\n".join(lines) + "\n" + notes)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
