#!/usr/bin/env python3
"""Contacts of feature instances on the device (``ops.contact``, ``contact.hip``): the ``contact_stats``
launch against three yardsticks measured in the same process -- a device copy of the 5 B per voxel the
kernel must read (ids int32 + occ uint8), the ``access_stats`` launch on the same volume (the instance
pass whose structure it follows; that one reads its voxel and three small extent tables, this one its
voxel and six neighbours) and ``reference.contact_table`` on device tensors (the plain-torch formulation:
shifted views, ``bincount``, ``torch.unique``).

    python bench/feature_contacts.py --size 64 --batch 32 --iters 20 --md profiles/feature_contacts.md

Volumes, ``batch`` x ``size``^3 each: solid (one instance per sample, no material: every face interior
or open), block-upsampled random blobs (every voxel labelled: shared faces between 8^3 blocks), and
intersecting generated parts (``fn.generate_parts(separate=False)``: the occupancy and the true labels).
The pair table has the capacity the op settles on; its fill is timed apart, as is the whole of
``contact_table`` (fills, launch, the read of ``lost``, compaction, sort and decode; host time included).
Every launch is warmed up and timed with device events as ``--reps`` launches back to back, per launch;
the result of the kernel is compared with the torch formulation's before anything is timed.  ``--md``
writes the table, the ratios and the compiler's resource report of the kernel (VGPRs, SGPRs, LDS,
scratch; needs ``hipcc``) as Markdown.  Needs a GPU: there is no CPU fallback.
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
    """[(kernel, VGPRs, SGPRs, scratch B/lane, LDS B/workgroup, occupancy)] of contact_stats_kernel,
    access_stats_kernel and overlap_pairs_kernel, from hipcc's -Rpass-analysis=kernel-resource-usage; []
    without hipcc."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        return []
    rows = []
    src = os.path.join(ROOT, "featurenet_amd", "csrc", "kernels")
    for name, want in (("contact.hip", ("contact_stats_kernel",)), ("access.hip", ("access_stats_kernel",)),
                       ("overlap.hip", ("overlap_pairs_kernel",))):
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
    ap.add_argument("--classes", type=int, default=25, help="classes of the blobs volume")
    ap.add_argument("--iters", type=int, default=20, help="timed samples of each launch (alternating)")
    ap.add_argument("--reps", type=int, default=10, help="launches back to back per sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default="", metavar="OUT.md", help="also write the results as Markdown")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("feature_contacts: no GPU visible (this benchmark has no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1:
        ap.error("--iters, --reps and --warmup must be >= 1")
    import featurenet_amd as fn
    from featurenet_amd import _native
    from featurenet_amd.ops import access, ccl, contact, reference

    dev = torch.device("cuda")
    S, N = a.size, a.batch
    rng = np.random.default_rng(0)
    vox, labels, _ = fn.generate_parts(N, size=S, seed=0, device="cuda", separate=False)
    b = 8
    coarse = rng.integers(1, a.classes, (N, -(-S // b), -(-S // b), -(-S // b)))
    blobs = np.kron(coarse, np.ones((1, b, b, b), np.int64))[:, :S, :S, :S].astype(np.uint8)
    full = np.ones((N, S, S, S), np.uint8)
    vols = {"solid": (0 * full, full), "blobs": (0 * full, blobs), "parts": (vox, labels)}
    K = _native.kernels()
    res, ok = {}, True
    for name, (o, l) in vols.items():
        occ, lab = torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(np.ascontiguousarray(l)).to(dev)
        st = _native.stream(occ)
        roots, flags = ccl.connected_components(lab, 0, 6, return_flags=True)
        ids, table, offsets = ccl.instance_table(lab, roots, want_ids=True, flags=flags)
        T = int(table.shape[0])
        V = occ.numel()
        want, want_adj = reference.contact_table(ids, offsets, occ)
        got, got_adj = contact.contact_table(ids, offsets, occ, rows=T)
        same = bool(torch.equal(got, want)) and bool(torch.equal(got_adj, want_adj)) \
            and bool(torch.equal(got[:, 18], table[:, 2]))
        ok = ok and same
        # the capacity the op settles on: the first of its sizes that loses nothing
        cap = max(contact.MIN_CAP, contact._next_pow2(2 * T))
        while True:
            buf = torch.zeros(T * 19 + 2 * cap + 1, dtype=torch.int64, device=dev)
            con, keys, counts, lost = buf[:T * 19], buf[T * 19:T * 19 + cap], buf[T * 19 + cap:-1], buf[-1:]

            def stats():
                K.contact_stats(ids.data_ptr(), occ.data_ptr(), offsets.data_ptr(), con.data_ptr(), keys.data_ptr(),
                                counts.data_ptr(), lost.data_ptr(), N, S, S, S, T, cap, contact.PROBE, st,
                                [V, V, N + 1, T * 19, cap, cap, 1])

            stats()
            if int(lost) == 0:
                break
            cap *= 4
        ex, ey, ez = access.column_extents(occ)
        acc = torch.empty(T, 8, dtype=torch.int64, device=dev)
        ids2, occ2 = torch.empty_like(ids), torch.empty_like(occ)

        def fill():
            buf.zero_()

        def access_stats():
            K.access_stats(ids.data_ptr(), offsets.data_ptr(), ex.data_ptr(), ey.data_ptr(), ez.data_ptr(), 0,
                           acc.data_ptr(), N, S, S, S, T, st, [V, N + 1, ex.numel(), ey.numel(), ez.numel(), 0, T * 8])

        def copy():
            ids2.copy_(ids)
            occ2.copy_(occ)

        def torch_formulation():
            return reference.contact_table(ids, offsets, occ)

        def whole():
            return contact.contact_table(ids, offsets, occ, rows=T)

        # (the kernel adds into its tables: timing it on tables that already hold every key is the steady state
        # of its atomics -- the compare-and-swap finds its key where the first launch found an empty slot)
        timed = {"contact_stats": (stats, a.reps), "fill": (fill, a.reps), "access_stats": (access_stats, a.reps),
                 "copy": (copy, a.reps), "torch_formulation": (torch_formulation, 1)}
        for f, _ in timed.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in timed}
        times["whole"] = []
        for _ in range(a.iters):
            for k, (f, reps) in timed.items():
                if k == "contact_stats":
                    fill()
                times[k].append(device_time_us(f, reps))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            whole()
            torch.cuda.synchronize()
            times["whole"].append((time.perf_counter() - t0) * 1e6)
        r = {k: summary(v) for k, v in times.items()}
        r.update(instances=T, pairs=int(got_adj.shape[0]), shared_faces=int(got_adj[:, 3].sum()), table_slots=cap,
                 voxels_in_instances=int(table[:, 2].sum()), equals_torch_formulation=same,
                 stats_over_copy=round(r["contact_stats"]["median_us"] / r["copy"]["median_us"], 2),
                 stats_over_access_stats=round(r["contact_stats"]["median_us"] / r["access_stats"]["median_us"], 2),
                 torch_over_stats=round(r["torch_formulation"]["median_us"] / r["contact_stats"]["median_us"], 1),
                 torch_over_whole=round(r["torch_formulation"]["median_us"] / r["whole"]["median_us"], 1))
        res[name] = r
    out = {"metric": f"feature contacts, {N} x {S}^3", "iters": a.iters, "reps": a.reps, "volumes": res}
    print(json.dumps(out))
    if a.md:
        names = list(res)
        lines = [f"## Timing ({N} x {S}^3 voxels per launch, device events, {a.reps} launches back to back, "
                 f"{a.iters} samples; median (min - max), microseconds per launch)", "",
                 "| | " + " | ".join(names) + " |", "|---|" + "---|" * len(names)]
        for k, label in (("instances", "instances"), ("pairs", "rows of `adj`"), ("shared_faces", "shared faces"),
                         ("table_slots", "pair-table slots")):
            lines.append(f"| {label} | " + " | ".join(f"{res[n][k]:,}" for n in names) + " |")
        for k, label in (("contact_stats", "`contact_stats_kernel`"),
                         ("fill", "zero-fill of `contact` and the pair table"),
                         ("copy", "yardstick: device copy of ids (4 B) and occ (1 B) per voxel"),
                         ("access_stats", "yardstick: `access_init_kernel` + `access_stats_kernel`"),
                         ("torch_formulation", "yardstick: `reference.contact_table` on the device"),
                         ("whole", "`ops.contact.contact_table`, host time included")):
            lines.append(f"| {label} | " + " | ".join(
                f"{res[n][k]['median_us']:,.1f} ({res[n][k]['min_us']:,.1f} - {res[n][k]['max_us']:,.1f})"
                for n in names) + " |")
        for k, label, unit in (("stats_over_copy", "kernel / copy", ""),
                               ("stats_over_access_stats", "kernel / `access_stats` launch", ""),
                               ("torch_over_stats", "torch formulation / kernel", "x"),
                               ("torch_over_whole", "torch formulation / `contact_table`", "x")):
            lines.append(f"| **{label}** | " + " | ".join(f"**{res[n][k]:.2f}{unit}**" for n in names) + " |")
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
            f.write("# Contacts of feature instances (`contact.hip`)\n\n`python bench/feature_contacts.py "
                    f"--size {S} --batch {N} --iters {a.iters} --reps {a.reps} --md OUT.md` on 1 x MI355X wrote the "
                    "two sections below.\n\n" + "\n".join(lines) + "\n" + notes)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
