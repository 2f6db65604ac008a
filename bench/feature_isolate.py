#!/usr/bin/env python3
"""Instance isolation on the device (``ops.isolate``, ``isolate.hip``): the ``isolate_parts`` launch in its
three output formats against two yardsticks measured in the same process -- a device fill of the same output
bytes (the kernel reads almost nothing, so the fill is its floor) and ``reference.isolate_instances`` on device
tensors (the plain-torch formulation: index vectors and a gather) -- and ``fn.recognize`` end to end.

    python bench/feature_isolate.py --iters 20 --md profiles/feature_isolate.md

Parts: the first 32 instances of generated parts (``fn.generate_parts``) at 64^3, cut at 64 (the identity map),
and at 128^3, cut at 64 (resampled 2 : 1).  Every launch is warmed up and timed with device events as ``--reps``
launches back to back, per launch; the kernel's results are compared with the torch formulation's
(``torch.equal``) before anything is timed.  ``fn.recognize`` is timed on the host clock around a device
synchronisation, with a default ``FeatureNet3D`` at random weights (its speed does not depend on them).
``--md`` writes the tables as Markdown.  The timed launches need a GPU: there is no CPU fallback.

``--accuracy`` adds reported numbers, no gate: a classifier trained with ``fn.train`` on single-feature parts of
the same generator (so isolated features are in distribution), ``fn.match_features`` F1 / PQ of
``fn.recognize(..., return_labels=True)`` on held-out multi-feature parts, and next to it ``fn.evaluate_features``
of a segmentation model trained on multi-feature parts, on the same held-out parts.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS = ((0, "bits"), (1, "uint8"), (2, "bf16"))


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


def micro(score) -> dict:
    """F1 over all classes' counts and the mean panoptic quality of a ``FeatureScore``."""
    tp, fp, fn_ = int(score.tp.sum()), int(score.fp.sum()), int(score.fn.sum())
    return {"tp": tp, "fp": fp, "fn": fn_, "f1": round(2 * tp / max(1, 2 * tp + fp + fn_), 4),
            "mpq": round(score.mpq, 4), "msq": round(score.msq, 4)}


def accuracy(a) -> dict:
    """Train the classifier on single-feature parts of the part generator (each part's class is the class its
    table gives to slot 0), then score ``fn.recognize`` on held-out multi-feature parts with
    ``fn.match_features`` -- and, with ``--seg-epochs``, a segmentation model trained on multi-feature parts
    of the same generator with ``fn.evaluate_features`` on the same held-out parts."""
    import featurenet_amd as fn
    from featurenet_amd.models.featurenet3d import FeatureNet3DConfig
    from featurenet_amd.ops import partgen
    from featurenet_amd.training.data import Dataset, voxel_seg_dataset

    S, dev = a.acc_size, a.device
    sets = []
    for n, seed in ((a.acc_train, 11), (max(64, a.acc_train // 16), 12)):
        tab = partgen.sample(n, S, seed, (1, 1))
        vox, _ = partgen.carve(tab, S, device=dev)
        sets += [vox.unsqueeze(-1), tab[:, 0, 0].to(torch.int64).to(vox.device)]
    ds = Dataset("parts-1", *sets, partgen.NUM_CLASSES, (S, S, S, 1), synthetic=True)
    t0 = time.perf_counter()
    clf = fn.train(FeatureNet3DConfig(input_size=S), data=ds, epochs=a.acc_epochs, batch_size=a.acc_batch, device=dev,
                   verbose=0)
    out = {"size": S, "classifier": {"train_parts": a.acc_train, "epochs": a.acc_epochs,
                                     "single_feature_accuracy": round(clf.accuracy, 4),
                                     "last_epoch": {k: round(float(v[-1]), 4) for k, v in clf.history.items()
                                                    if isinstance(v, list) and v and isinstance(v[-1], (int, float))},
                                     "train_s": round(time.perf_counter() - t0, 1)}}
    held = voxel_seg_dataset(a.seg_train, a.acc_test, size=S, features=(1, 4), seed=21, device=dev)
    x, y = held.x_test, held.y_test
    _, _, labels = fn.recognize(clf.model, x[..., 0], device=dev, return_labels=True, min_voxels=a.acc_min_voxels)
    out["held_out_parts"] = int(x.shape[0])
    out["recognize"] = micro(fn.match_features(labels, y, min_voxels=a.acc_min_voxels, device=dev))
    out["segmentation"] = None
    if a.seg_epochs > 0:
        t0 = time.perf_counter()
        seg = fn.train("segmentation", data=held, epochs=a.seg_epochs, batch_size=a.seg_batch, device=dev, verbose=0)
        out["segmentation"] = {**micro(fn.evaluate_features(seg.model, x, y, min_voxels=a.acc_min_voxels)),
                               "train_parts": a.seg_train, "epochs": a.seg_epochs,
                               "train_s": round(time.perf_counter() - t0, 1)}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", action="store_true", help="also train a classifier (and a segmentation model) and "
                                                            "score fn.recognize on held-out multi-feature parts")
    ap.add_argument("--no-timing", action="store_true", help="with --accuracy: skip the timed launches")
    ap.add_argument("--device", default="cuda", help="of the --accuracy run")
    ap.add_argument("--acc-size", type=int, default=64)
    ap.add_argument("--acc-train", type=int, default=4096, help="single-feature parts the classifier trains on")
    ap.add_argument("--acc-test", type=int, default=256, help="held-out multi-feature parts")
    ap.add_argument("--acc-epochs", type=int, default=8)
    ap.add_argument("--acc-batch", type=int, default=64)
    ap.add_argument("--acc-min-voxels", type=int, default=1)
    ap.add_argument("--seg-train", type=int, default=600, help="multi-feature parts the segmentation model trains on")
    ap.add_argument("--seg-epochs", type=int, default=8, help="0: no segmentation model")
    ap.add_argument("--seg-batch", type=int, default=16)
    ap.add_argument("--parts", type=int, default=32, help="instances cut per launch")
    ap.add_argument("--grids", type=int, nargs="+", default=[64, 128], help="source grids (cut at --size)")
    ap.add_argument("--size", type=int, default=64, help="the classifier's grid")
    ap.add_argument("--iters", type=int, default=20, help="timed samples of each launch (alternating)")
    ap.add_argument("--reps", type=int, default=10, help="launches back to back per sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--recognize", type=int, default=16, metavar="N", help="parts of the end-to-end run (0: skip it)")
    ap.add_argument("--md", default="", metavar="OUT.md", help="also write the results as Markdown")
    a = ap.parse_args()
    if a.no_timing and not a.accuracy:
        ap.error("--no-timing leaves nothing to do without --accuracy")
    if not a.no_timing and not torch.cuda.is_available():
        print("feature_isolate: no GPU visible (the timed launches have no CPU fallback)", file=sys.stderr)
        return 2
    if a.iters < 1 or a.warmup < 1 or a.reps < 1 or a.parts < 1:
        ap.error("--parts, --iters, --reps and --warmup must be >= 1")
    import featurenet_amd as fn
    from featurenet_amd import _native
    from featurenet_amd.models.featurenet3d import FeatureNet3D
    from featurenet_amd.ops import ccl, isolate, reference

    dev = torch.device("cuda")
    K = _native.kernels()
    S, M = a.size, a.parts
    res, ok = {}, True
    for G in ([] if a.no_timing else a.grids):
        _, labels, _ = fn.generate_parts(M, size=G, seed=0, device="cuda")       # >= one feature per part
        lab = torch.from_numpy(labels).to(dev)
        roots, flags = ccl.connected_components(lab, 0, 6, return_flags=True)
        ids, table, offsets = ccl.instance_table(lab, roots, want_ids=True, flags=flags)
        sel, _ = isolate.selection(table, offsets, shape=(G, G, G))
        sel = sel[:M].contiguous()
        st = _native.stream(ids)
        r = {"feature_voxels": int(table[:M, 2].sum()), "samples_read": int(sel[:, 0].max()) + 1}
        want = reference.isolate_instances(ids, sel, S, 1)
        for fmt, name in FORMATS:
            out = isolate.isolate_instances(ids, sel, S, fmt)
            same = bool(torch.equal(out, reference.isolate_instances(ids, sel, S, fmt)))
            ok = ok and same
            flat = out.view(-1).view(torch.uint8) if fmt != 2 else out.view(-1).view(torch.int16)
            spare = torch.empty_like(flat)

            def kernel():
                K.isolate_parts(ids.data_ptr(), sel.data_ptr(), out.data_ptr(), M, G, G, G, M, S, fmt, st,
                                [ids.numel(), sel.numel(), out.numel()])

            def fill():
                spare.fill_(1)

            def torch_formulation():
                return reference.isolate_instances(ids, sel, S, fmt)

            timed = {"kernel": (kernel, a.reps), "fill": (fill, a.reps), "torch": (torch_formulation, 1)}
            for f, _ in timed.values():
                for _ in range(a.warmup):
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in timed}
            for i in range(a.iters):
                for k, (f, reps) in timed.items():
                    if k != "torch" or i < 5:
                        times[k].append(device_time_us(f, reps))
            t = {k: summary(v) for k, v in times.items()}
            nbytes = flat.numel() * flat.element_size()
            r[name] = {**t, "bytes": nbytes, "equals_torch_formulation": same,
                       "kernel_over_fill": round(t["kernel"]["median_us"] / t["fill"]["median_us"], 2),
                       "torch_over_kernel": round(t["torch"]["median_us"] / t["kernel"]["median_us"], 1),
                       "write_GBps": round(nbytes / t["kernel"]["median_us"] / 1e3, 1)}
        assert want.shape[0] == M
        res[f"{M} parts, {G}^3 -> {S}^3"] = r
    e2e = None
    if a.recognize > 0 and not a.no_timing:
        clf = FeatureNet3D().to(dev).eval()
        vox, _, _ = fn.generate_parts(a.recognize, size=S, seed=1, device="cuda")
        runs = []
        for i in range(3 + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            feats, _, _ = fn.recognize(clf, vox, device=dev)
            torch.cuda.synchronize()
            if i >= 3:
                runs.append((time.perf_counter() - t0) * 1e3)
        e2e = {"parts": a.recognize, "features": sum(len(fs) for fs in feats),
               "median_ms": round(statistics.median(runs), 2), "min_ms": round(min(runs), 2),
               "max_ms": round(max(runs), 2)}
    acc = accuracy(a) if a.accuracy else None
    out = {"metric": "feature isolate", "iters": a.iters, "reps": a.reps, "cases": res, "recognize": e2e,
           "accuracy": acc or "unmeasured"}
    print(json.dumps(out))
    if a.md:
        lines = [f"## Timing (device events, {a.reps} launches back to back, {a.iters} samples; median (min - max), "
                 "microseconds per launch)", ""]
        for case, r in res.items():
            lines += [f"### {case} ({r['feature_voxels']:,} feature voxels, ids of {r['samples_read']} samples)", "",
                      "| | " + " | ".join(n for _, n in FORMATS) + " |", "|---|" + "---|" * len(FORMATS),
                      "| output bytes | " + " | ".join(f"{r[n]['bytes']:,}" for _, n in FORMATS) + " |"]
            for k, label in (("kernel", "`isolate_kernel`"), ("fill", "yardstick: device fill of the same bytes"),
                             ("torch", "yardstick: `reference.isolate_instances` on the device")):
                lines.append(f"| {label} | " + " | ".join(
                    f"{r[n][k]['median_us']:,.1f} ({r[n][k]['min_us']:,.1f} - {r[n][k]['max_us']:,.1f})"
                    for _, n in FORMATS) + " |")
            lines.append("| **kernel / fill** | " + " | ".join(f"**{r[n]['kernel_over_fill']:.2f}**" for _, n in FORMATS) + " |")
            lines.append("| **torch formulation / kernel** | " +
                         " | ".join(f"**{r[n]['torch_over_kernel']:,.0f}x**" for _, n in FORMATS) + " |")
            lines.append("| kernel's store rate, GB/s | " + " | ".join(f"{r[n]['write_GBps']:,.0f}" for _, n in FORMATS) + " |")
            lines.append("| equals the torch formulation | " +
                         " | ".join(str(r[n]["equals_torch_formulation"]).lower() for _, n in FORMATS) + " |")
            lines.append("")
        lines += ["## `fn.recognize` end to end (host clock around a device synchronisation, 5 runs after 3)", ""]
        if e2e is None:
            lines.append("Not run.")
        else:
            lines.append(f"{e2e['parts']} generated parts at {S}^3 with {e2e['features']} features, default "
                         f"`FeatureNet3D` at random weights: {e2e['median_ms']:.1f} ms ({e2e['min_ms']:.1f} - "
                         f"{e2e['max_ms']:.1f}), occupancy in host memory to records in host memory.")
        lines += ["", "## Accuracy (reported, not a gate)", ""]
        if acc is None:
            lines.append("Unmeasured: run with `--accuracy` (train the classifier on single-feature parts, score "
                         "`fn.recognize` with `fn.match_features` next to a segmentation model's "
                         "`fn.evaluate_features`).")
        else:
            c = acc["classifier"]
            lines += [f"Classifier: `FeatureNet3D` at {acc['size']}^3, {c['train_parts']:,} single-feature parts of "
                      f"`generate_parts(features=(1, 1))`, {c['epochs']} epochs ({c['train_s']} s); accuracy on its own "
                      f"held-out single-feature parts {c['single_feature_accuracy']:.4f}.  Scored on "
                      f"{acc['held_out_parts']} held-out parts with 1 to 4 features (IoU > 0.5, same class):", "",
                      "| | TP | FP | FN | F1 | mean PQ | mean SQ |", "|---|---|---|---|---|---|---|"]
            rows = [("`fn.recognize` + `fn.match_features`", acc["recognize"])]
            if acc["segmentation"]:
                s = acc["segmentation"]
                rows.append((f"segmentation model ({s['train_parts']} parts, {s['epochs']} epochs, {s['train_s']} s) + "
                             "`fn.evaluate_features`", s))
            lines += [f"| {k} | {v['tp']} | {v['fp']} | {v['fn']} | {v['f1']:.4f} | {v['mpq']:.4f} | {v['msq']:.4f} |"
                      for k, v in rows]
            if not acc["segmentation"]:
                lines.append("\nThe segmentation model: unmeasured (`--seg-epochs 0`).")
        notes = ""                                  # (hand-written findings below the figures survive a re-run)
        if os.path.exists(a.md):
            old = open(a.md).read()
            notes = old[old.index("\n## Notes"):] if "\n## Notes" in old else ""
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("# Instance isolation (`isolate.hip`)\n\n`python bench/feature_isolate.py "
                    f"--iters {a.iters} --reps {a.reps} --md OUT.md` on 1 x MI355X wrote the sections below.\n\n" +
                    "\n".join(lines) + "\n" + notes)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
