"""Command line: ``python -m featurenet_amd <command> ...``.

========== =================================================================
command    reference equivalent
========== =================================================================
run        ``run.py`` (-n BxCxN -t -b -f -a -i -p -d -m -g -r -s -e -y -l)
pledge     ``pledge_evolution.py`` (-n -d -b -i -o -p -t)
products   ``full.py`` / ``full_mnist.py`` / ``full_cifar.py`` (-i -d -t)
retrain    ``pledge_trainer.py`` (-p -j -i -e -t -b -d)
ga         ``evolution.py`` (-i -o)
resume     ``utils/retrainer.py`` (continue training a checkpoint)
serve      ``ui/back/main.py`` (REST task service, port 9999)
train      ``TensorflowGenerator(...)`` one architecture (template / product /
           featurenet3d) -> checkpoint
classify   load a checkpoint and predict (npy / binvox folder)
segment    per-voxel labels of a segmentation checkpoint -> .npy
score      confusion matrix / per-class IoU / mIoU of a segmentation checkpoint against true labels
features   the feature instances (connected components of the labels) of a segmentation checkpoint -> JSON
recognize  the features of multi-feature parts by a single-feature classifier checkpoint alone -> JSON
split      touching features of an instance-id volume told apart by a watershed on the distance to the material
score-features
           predicted features matched to the true ones: per-class TP / FP / FN, F1 and panoptic quality
generate-parts
           procedural multi-feature parts with per-voxel labels (and their feature lists) -> .npz
extend     ``PledgeEvolution.end2end`` (FM template -> B x C)
sample     ``run_pledge`` (native diverse product sampler)
template   write the built-in 1-block search-space FM
========== =================================================================
"""
from __future__ import annotations

import argparse
import json
import os
import sys

from .config import SearchConfig


def _scheduler(devices: str, timeout: float, workers_per_device: int = 0):
    """Trial scheduler over ``devices``; ``workers_per_device`` 0 = auto: 4 worker processes per GPU
    (the candidates' small kernels from 4 processes keep one MI355X busy: 12.5K -> 19.7K candidates
    per hour against 7.8K for one worker, profiles/r5_nas.md), one trial at a time on the CPU."""
    from .search.trial import TrialScheduler

    devs = [d for d in devices.split(",") if d] if devices else None
    if workers_per_device <= 0:
        probe = TrialScheduler(devices=devs, mode="inline")
        workers_per_device = 1 if probe.devices == ["cpu"] else 4
    return TrialScheduler(devices=devs, timeout_s=timeout or None, workers_per_device=workers_per_device)


def _template(base: str, fm_path: str) -> str:
    if fm_path:
        return fm_path
    from .fm.space import default_template

    return str(default_template(os.path.join(base, "main_1block_nas.xml")))


# ---------------------------------------------------------------------- run
def cmd_run(a) -> int:
    from .fm.sampler import run_pledge
    from .search.evolution import run_evolution
    from .search.mutation import MutationStrategies, SelectionStrategies
    from .search.pledge_evolution import end2end
    from .search.trial import TrialConfig

    cfg = SearchConfig.load(a.config) if a.config else SearchConfig()
    for k in ("nb", "training_epochs", "base_path", "fm_path", "pledge_duration", "products_file", "dataset",
              "mutation_strategy", "selection_strategy", "mutation_rate", "survival_rate", "evolution_epochs",
              "model", "devices", "seed", "workers_per_device"):
        v = getattr(a, k, None)
        if v is not None:
            setattr(cfg, k, v)
    if a.breed is not None:
        cfg.breed = a.breed not in ("0", "false", "False", "")
    nb = cfg.nb_tuple
    # the trial worker pool starts now: its start-up overlaps the product sampling below
    sched = _scheduler(cfg.devices, cfg.trial_timeout_s, cfg.workers_per_device).start()
    ms = MutationStrategies.ALL if cfg.mutation_strategy == "all" else MutationStrategies.CHOICE
    ss = {"pareto": SelectionStrategies.PARETO, "elitist": SelectionStrategies.ELITIST,
          "hybrid": SelectionStrategies.HYBRID}[cfg.selection_strategy]
    products = cfg.products_file
    if len(nb) == 3 and not products:
        blocks, cells, n = nb
        os.makedirs(cfg.base_path, exist_ok=True)
        products = f"{cfg.base_path}/products_{int(cfg.pledge_duration)}s_{blocks}_{cells}_{n}.pdt"
        if not os.path.isfile(products):
            fm = end2end(cfg.base_path, nb, _template(cfg.base_path, cfg.fm_path))
            run_pledge(fm, n, products, duration=cfg.pledge_duration, seed=cfg.seed)
    trial = TrialConfig(dataset=cfg.dataset, epochs=cfg.training_epochs, batch_size=cfg.batch_size,
                        fill_defaults=True, seed=cfg.seed, synthetic_sizes=tuple(cfg.synthetic_sizes))
    res = run_evolution(cfg.base_path, last_pdts_path=products, nb_base_products=nb[-1], dataset=cfg.dataset,
                        training_epochs=cfg.training_epochs, mutation_rate=cfg.mutation_rate,
                        survival_rate=cfg.survival_rate, breed=cfg.breed, evolution_epochs=cfg.evolution_epochs,
                        model=cfg.model, attacks=tuple(cfg.attacks), mutation_strategy=ms, selection_strategy=ss,
                        max_nb_cells=cfg.max_nb_cells, max_nb_blocks=cfg.max_nb_blocks,
                        scheduler=sched, trial=trial, seed=cfg.seed)
    sched.close()
    print(json.dumps({"session": res.session_path, "generations": res.generations, "history": res.history}))
    return 0


def cmd_pledge(a) -> int:
    from .search import pledge_evolution as pe
    from .search.trial import TrialConfig

    nb = tuple(int(v) for v in a.nb.split("x"))
    template = _template(a.base, a.input)
    fm = pe.end2end(a.base, nb, template) if len(nb) == 3 else template
    res = pe.run(a.base, fm, a.output, a.products, nb_base_products=nb[-1], dataset=a.dataset,
                 training_epochs=a.training_epochs, evolution_epochs=a.evolution_epochs,
                 scheduler=_scheduler(a.devices, 0), trial=TrialConfig(fill_defaults=True),
                 pledge_duration_s=a.dtime)
    print(json.dumps({"session": res.session_path, "population": len(res.population)}))
    return 0


def cmd_products(a) -> int:
    from .search.batch import train_product_set
    from .search.trial import TrialConfig

    res = train_product_set(a.input, datasets=a.datasets.split(","), epochs=a.training_epochs,
                            min_index=a.min_index, max_index=a.max_index, output_folder=a.output,
                            scheduler=_scheduler(a.devices, 0), cfg=TrialConfig(fill_defaults=True))
    print(json.dumps({ds: [s.accuracy for s in specs] for ds, specs in res}))
    return 0


def cmd_retrain(a) -> int:
    from .search.batch import train_from_json, train_from_product

    idx = a.index.split("-") if a.index else None
    if a.json:
        out = train_from_json(a.pledge, a.json, idx, a.export, a.training_epochs, a.batch_size, a.dataset,
                              scheduler=_scheduler(a.devices, 0))
        print(json.dumps([v.accuracy for v in out]))
    else:
        v = train_from_product(a.pledge, int(idx[0]) if idx else 0, a.export, a.training_epochs, a.batch_size,
                               a.dataset, scheduler=_scheduler(a.devices, 0))
        print(json.dumps({"accuracy": v.accuracy}))
    return 0


def cmd_ga(a) -> int:
    from .search import legacy_ga

    pop = legacy_ga.run(a.input, a.output, generations=a.generations, scheduler=_scheduler(a.devices, 0))
    print(json.dumps([v.accuracy for v in pop]))
    return 0


def cmd_resume(a) -> int:
    from .search.batch import retrain_checkpoint

    acc, _ = retrain_checkpoint(a.model, a.epochs, a.dataset, not a.no_augment, a.batch_size, a.save or a.model)
    print(json.dumps({"accuracy": acc}))
    return 0


def cmd_serve(a) -> int:
    from .service.server import serve

    serve(a.host, a.port, a.db, a.base, a.devices or None, max_workers=a.max_workers,
          cors_origins=[o for o in a.cors.split(",") if o] or None)
    return 0


def cmd_train(a) -> int:
    from . import api
    from .fm.products import ProductSet

    arch = a.arch
    if a.pdt:
        arch, _ = ProductSet(a.pdt).format_product(a.index)
    res = api.train(arch, data=a.data, epochs=a.epochs, batch_size=a.batch_size, lr=a.lr, save_path=a.save,
                    fill_defaults=True, scheduler=a.lr_schedule, augment=a.augment,
                    robustness=a.robustness.split(",") if a.robustness else None)
    print(json.dumps({"accuracy": res.accuracy, "loss": res.loss, "path": res.path}))
    return 0


def cmd_classify(a) -> int:
    import numpy as np

    from . import api

    if os.path.isdir(a.input):
        from .training.data import binvox_folder

        x, _, _ = binvox_folder(a.input)
        x = np.asarray(x, np.float32)[..., None]
    else:
        x = np.load(a.input, allow_pickle=False)
    calib = None
    if a.fp8_calib is not None:          # (the first N inputs calibrate the fp8 activation scales)
        calib = x[:a.fp8_calib]
    labels, probs = api.classify(a.model, x, packed_size=a.packed_size, fp8_calib=calib)
    print(json.dumps({"labels": labels.tolist(), "confidence": probs.max(-1).round(4).tolist()}))
    return 0


def cmd_segment(a) -> int:
    import numpy as np

    from . import api

    if os.path.isdir(a.input):
        from .training.data import binvox_folder

        x, _, _ = binvox_folder(a.input)
        x = np.asarray(x, np.float32)[..., None]
    else:
        x = np.load(a.input, allow_pickle=False)
    model, _ = api.load(a.model)
    labels, conf = api.segment(model, x, packed_size=a.packed_size, return_confidence=bool(a.confidence))
    np.save(a.output, labels)
    if a.confidence:
        np.save(a.confidence, conf)
    counts = np.bincount(labels.reshape(-1), minlength=int(getattr(model, "num_classes", 1)))
    print(json.dumps({"shape": list(labels.shape), "counts": counts.tolist()}))
    return 0


def cmd_score(a) -> int:
    import numpy as np

    from . import api

    x = np.load(a.input, allow_pickle=False)
    y = np.load(a.truth, allow_pickle=False)
    score = api.evaluate_segmentation(a.model, x, y, packed_size=a.packed_size, ignore_index=a.ignore_index)
    summary = json.dumps(score.to_dict())
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_features(a) -> int:
    import numpy as np

    from . import api

    x = np.load(a.input, allow_pickle=False)
    feats, ids = api.extract_features(a.model, x, packed_size=a.packed_size,
                                      background=None if a.background < 0 else a.background,
                                      connectivity=a.connectivity, min_voxels=a.min_voxels, return_ids=bool(a.ids),
                                      access=a.access, dimensions=a.dimensions, tool=a.tool,
                                      contacts=a.contacts, walls=False if a.walls is None else a.walls,
                                      classifier=a.classifier or None)
    if a.ids:
        np.save(a.ids, ids)
    summary = json.dumps({"samples": [[f.to_dict(a.access_fraction) for f in fs] for fs in feats]})
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_recognize(a) -> int:
    import numpy as np

    from . import api

    x = np.load(a.input, allow_pickle=False)
    feats, ids, labels = api.recognize(a.model, x, stock=a.stock, connectivity=a.connectivity,
                                       min_voxels=a.min_voxels, return_ids=bool(a.ids), return_labels=bool(a.labels),
                                       device=a.device or None, access=a.access, dimensions=a.dimensions, tool=a.tool,
                                       contacts=a.contacts, walls=False if a.walls is None else a.walls, split=a.split)
    if a.ids:
        np.save(a.ids, ids)
    if a.labels:
        np.save(a.labels, labels)
    summary = json.dumps({"samples": [[f.to_dict() for f in fs] for fs in feats]})
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_split(a) -> int:
    import numpy as np

    from . import api

    ids = np.load(a.ids, allow_pickle=False)
    vox = np.load(a.voxels, allow_pickle=False)
    out, feats = api.split_features(ids, occupancy=vox, merge=a.merge, device=a.device or None)
    np.save(a.output, out)
    summary = json.dumps({"samples": [[f.to_dict() for f in fs] for fs in feats]})
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_distance(a) -> int:
    import numpy as np

    from . import api

    vol = np.load(a.input, allow_pickle=False)
    d2 = api.distance_transform(vol, border=a.border, device=a.device or None)
    np.save(a.output, d2)
    finite = d2[d2 < api.EDT_INF]
    summary = json.dumps({"shape": list(d2.shape), "seeds": int((d2 == 0).sum()),
                          "max_distance_sq": int(finite.max()) if finite.size else None,
                          "unreached_voxels": int((d2 >= api.EDT_INF).sum())})
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_nearest(a) -> int:
    import numpy as np

    from . import api

    ids = np.load(a.input, allow_pickle=False)
    d2, nearest = api.nearest_instances(ids, device=a.device or None)
    np.savez(a.output, d2=d2, nearest=nearest)
    other = np.moveaxis(d2, -4, 0)[1]
    on = other[(ids > 0) & (other < api.EDT_INF)]
    summary = json.dumps({"shape": list(d2.shape), "instance_voxels": int((ids > 0).sum()),
                          "min_gap_sq": int(on.min()) if on.size else None,
                          "voxels_without_other": int((other >= api.EDT_INF).sum())})
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_reach(a) -> int:
    import numpy as np

    from . import api
    from .utils.partfeatures import FACES

    vol = np.load(a.input, allow_pickle=False)
    r6 = api.tool_reach(vol, device=a.device or None)
    np.save(a.output, r6)
    faces = np.moveaxis(r6, -4, 0).reshape(6, -1)
    summary = json.dumps({"shape": list(r6.shape), "material": int(np.count_nonzero(vol)),
                          "open_voxels": {f: int((faces[k] >= 1).sum()) for k, f in enumerate(FACES)},
                          "max_entry_sq": {f: (int(faces[k].max()) if faces[k].size and faces[k].max() < api.EDT_INF
                                               else None) for k, f in enumerate(FACES)}})
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_score_features(a) -> int:
    import numpy as np

    from . import api

    x = np.load(a.input, allow_pickle=False)
    y = np.load(a.truth, allow_pickle=False)
    score = api.evaluate_features(a.model, x, y, packed_size=a.packed_size,
                                  background=None if a.background < 0 else a.background,
                                  connectivity=a.connectivity, iou_threshold=a.iou, min_voxels=a.min_voxels)
    summary = json.dumps(score.to_dict())
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_generate_parts(a) -> int:
    import numpy as np

    from . import api

    voxels, labels, parts = api.generate_parts(a.n, size=a.size, seed=a.seed, features=tuple(a.features),
                                               separate=not a.overlap, device=a.device or None)
    np.savez_compressed(a.output, voxels=voxels, labels=labels)
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps({"parts": [[p.to_dict() for p in ps] for ps in parts]}) + "\n")
    counts = np.bincount([len(ps) for ps in parts], minlength=a.features[1] + 1)
    print(json.dumps({"shape": list(labels.shape), "features_per_part": counts.tolist(),
                      "removed_voxels": int((labels != 0).sum())}))
    return 0


def cmd_voxelize(a) -> int:
    import numpy as np

    from . import _native, api

    fit = "bbox" if a.voxel_size is None else (a.origin, a.voxel_size)
    voxels, info = api.voxelize(list(a.meshes), size=a.size, fit=fit, margin=a.margin, device=a.device or None,
                                return_info=True)
    np.save(a.output, voxels)
    doc = {"shape": list(voxels.shape), "meshes": list(a.meshes), "filled_voxels": voxels.reshape(len(voxels), -1)
           .sum(1).tolist(), "leaks": info["leaks"].tolist(), "origin": info["origin"].tolist(),
           "voxel_size": info["voxel_size"].tolist()}
    if a.binvox:
        os.makedirs(a.binvox, exist_ok=True)
        for path, vox, origin, vs in zip(a.meshes, voxels, info["origin"], info["voxel_size"]):
            stem = os.path.splitext(os.path.basename(path))[0]
            _native.runtime().write_binvox(os.path.join(a.binvox, stem + ".binvox"), vox, list(origin), vs * a.size)
    summary = json.dumps(doc)
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_label_mesh(a) -> int:
    import numpy as np

    from . import api

    ids = np.load(a.ids, allow_pickle=False)
    if ids.ndim == 4:
        if not 0 <= a.index < len(ids):
            raise SystemExit(f"label-mesh: --index {a.index} outside 0..{len(ids) - 1}")
        ids = ids[a.index]
    if ids.ndim != 3:
        raise SystemExit(f"label-mesh: {a.ids} holds an array of shape {ids.shape}, not [S, S, S] or [N, S, S, S]")
    fit = "bbox" if a.voxel_size is None else (a.origin, a.voxel_size)
    if a.fit and a.fit != ["bbox"]:
        try:
            *origin, voxel_size = [float(v) for v in a.fit]
            assert len(origin) == 3
        except (ValueError, AssertionError):
            raise SystemExit(f"label-mesh: --fit is 'bbox' or OX OY OZ VOXEL_SIZE, not {' '.join(a.fit)!r}")
        fit = (origin, voxel_size)
    winners, rows = api.label_mesh(a.mesh, ids, fit=fit, margin=a.margin, device=a.device or None, return_votes=True)
    np.save(a.output, winners)
    values, counts = np.unique(winners, return_counts=True)
    doc = {"mesh": a.mesh, "triangles": int(len(winners)), "labelled": int((winners != 0).sum()),
           "centroid_votes": int((rows[:, 2] == 0).sum()),
           "faces": {str(int(v)): int(c) for v, c in zip(values, counts) if v != 0}}
    if a.obj:
        from .utils.voxelmesh import write_labelled_obj

        write_labelled_obj(a.obj, api._mesh_triangles(a.mesh), winners)
    summary = json.dumps(doc)
    if a.json:
        with open(a.json, "w") as f:
            f.write(summary + "\n")
    print(summary)
    return 0


def cmd_export_stl(a) -> int:
    import numpy as np

    from . import _native
    from .utils.voxelmesh import voxels_to_mesh

    x = np.load(a.input, allow_pickle=False)
    if x.ndim == 5 and x.shape[-1] == 1:
        x = x[..., 0]
    if x.ndim == 4:
        if not 0 <= a.index < len(x):
            raise SystemExit(f"export-stl: --index {a.index} outside 0..{len(x) - 1}")
        x = x[a.index]
    if x.ndim != 3:
        raise SystemExit(f"export-stl: {a.input} holds an array of shape {x.shape}, not [S, S, S] or [N, S, S, S]")
    solid = x == a.value if a.value is not None else x != 0
    tris = voxels_to_mesh(solid) * a.voxel_size + np.asarray(a.origin, np.float32)
    _native.runtime().write_stl(a.output, tris.astype(np.float32), not a.ascii)
    print(json.dumps({"triangles": int(len(tris)), "voxels": int(solid.sum()), "output": a.output}))
    return 0


def cmd_extend(a) -> int:
    from .fm.extend import generate_featuretree

    generate_featuretree(_template(os.path.dirname(a.output) or ".", a.input), a.output, a.cells, a.blocks,
                         block_features=a.block_features)
    print(a.output)
    return 0


def cmd_sample(a) -> int:
    from .fm.sampler import run_pledge

    run_pledge(a.fm, a.n, a.output, duration=a.duration, seed=a.seed)
    print(a.output)
    return 0


def cmd_template(a) -> int:
    from .fm.space import default_template

    print(default_template(a.output))
    return 0


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="featurenet_amd", description=__doc__.split("\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)

    r = sub.add_parser("run", help="feature-model NAS (reference run.py)")
    r.add_argument("--config", help="YAML/JSON SearchConfig")
    r.add_argument("-n", "--nb", help="BLOCKSxCELLSxPRODUCTS (10x5x100) or PRODUCTS")
    r.add_argument("-t", "--training_epoch", dest="training_epochs", type=int)
    r.add_argument("-b", "--bpath", dest="base_path")
    r.add_argument("-f", "--fpath", dest="fm_path")
    r.add_argument("-a", "--ppath", dest="ppath", help="ignored: sampling is native (no PLEDGE.jar)")
    r.add_argument("-i", "--dtime", dest="pledge_duration", type=float)
    r.add_argument("-p", "--pfile", dest="products_file")
    r.add_argument("-d", "--dataset")
    r.add_argument("-m", "--mutation_strategy", choices=["all", "random"])
    r.add_argument("-g", "--selection_strategy", choices=["pareto", "elitist", "hybrid"])
    r.add_argument("-r", "--mutation_rate", type=float)
    r.add_argument("-s", "--survival_rate", type=float)
    r.add_argument("-e", "--evolution_epoch", dest="evolution_epochs", type=int)
    r.add_argument("-y", "--breed")
    r.add_argument("-l", "--model")
    r.add_argument("--devices")
    r.add_argument("--workers-per-device", dest="workers_per_device", type=int,
                   help="trial worker processes per GPU (0 / unset = auto: 4 per GPU)")
    r.add_argument("--seed", type=int)
    r.set_defaults(fn=cmd_run)

    q = sub.add_parser("pledge", help="diversity-driven evolution (reference pledge_evolution.py)")
    q.add_argument("-n", "--nb", default="5x5x100")
    q.add_argument("-d", "--dataset", default="mnist")
    q.add_argument("-b", "--base", default="./products")
    q.add_argument("-i", "--input", default="", help="1-block FM template (default: built-in)")
    q.add_argument("-o", "--output", default="")
    q.add_argument("-p", "--products", default="", help="resume from a {N}products[_e{n}].json")
    q.add_argument("-t", "--training_epochs", type=int, default=2)
    q.add_argument("-e", "--evolution_epochs", type=int, default=50)
    q.add_argument("--dtime", type=float, default=30.0)
    q.add_argument("--devices", default="")
    q.set_defaults(fn=cmd_pledge)

    b = sub.add_parser("products", help="train every product of a .pdt (reference full.py)")
    b.add_argument("-i", "--input", required=True, help="product file (with or without .pdt)")
    b.add_argument("-d", "--datasets", default="cifar")
    b.add_argument("-t", "--training_epochs", type=int, default=12)
    b.add_argument("--min-index", type=int, default=0)
    b.add_argument("--max-index", type=int, default=0)
    b.add_argument("-o", "--output", default="./products/")
    b.add_argument("--devices", default="")
    b.set_defaults(fn=cmd_products)

    t = sub.add_parser("retrain", help="retrain products by index / vector list (reference pledge_trainer.py)")
    t.add_argument("-p", "--pledge", required=True)
    t.add_argument("-j", "--json", default="")
    t.add_argument("-i", "--index", default="")
    t.add_argument("-e", "--export", default="")
    t.add_argument("-t", "--training_epochs", type=int, default=300)
    t.add_argument("-b", "--batch_size", type=int, default=64)
    t.add_argument("-d", "--dataset", default="cifar")
    t.add_argument("--devices", default="")
    t.set_defaults(fn=cmd_retrain)

    g = sub.add_parser("ga", help="bit-vector GA (reference evolution.py)")
    g.add_argument("-i", "--input", required=True)
    g.add_argument("-o", "--output", required=True)
    g.add_argument("--generations", type=int, default=10)
    g.add_argument("--devices", default="")
    g.set_defaults(fn=cmd_ga)

    c = sub.add_parser("resume", help="continue training a checkpoint (reference utils/retrainer.py)")
    c.add_argument("model")
    c.add_argument("--epochs", type=int, default=100)
    c.add_argument("--dataset", default="cifar")
    c.add_argument("--batch-size", type=int, default=64)
    c.add_argument("--no-augment", action="store_true")
    c.add_argument("--save", default="")
    c.set_defaults(fn=cmd_resume)

    s = sub.add_parser("serve", help="REST task service (reference ui/back)")
    s.add_argument("--host", default="127.0.0.1", help="bind address (no authentication: keep it local)")
    s.add_argument("--port", type=int, default=9999)
    s.add_argument("--db", default="samples.db")
    s.add_argument("--base", default="products")
    s.add_argument("--devices", default="")
    s.add_argument("--max-workers", type=int, default=2, help="concurrently running task workers")
    s.add_argument("--cors", default="", help="comma list of origins allowed cross-origin (default none)")
    s.set_defaults(fn=cmd_serve)

    tr = sub.add_parser("train", help="train one architecture and save a checkpoint")
    tr.add_argument("arch", nargs="?", default="featurenet3d", help="featurenet3d | lenet5 | keras | ...")
    tr.add_argument("--pdt", default="", help="train product --index of this .pdt instead")
    tr.add_argument("--index", type=int, default=0)
    tr.add_argument("--data", default="voxel")
    tr.add_argument("--epochs", type=int, default=12)
    tr.add_argument("--batch-size", type=int, default=128)
    tr.add_argument("--lr", type=float, default=1e-3)
    tr.add_argument("--lr-schedule", action="store_true", help="reference plateau/step/early-stop callbacks")
    tr.add_argument("--augment", action="store_true")
    tr.add_argument("--robustness", default="", help="comma list: clever,pgd,cw,fgsm")
    tr.add_argument("--save", default="model.fnk")
    tr.set_defaults(fn=cmd_train)

    cl = sub.add_parser("classify", help="predict with a checkpoint")
    cl.add_argument("model")
    cl.add_argument("input", help=".npy array or a folder of .binvox files")
    cl.add_argument("--packed-size", type=int, default=None)
    cl.add_argument("--fp8-calib", type=int, default=None, metavar="N",
                    help="FeatureNet-3D on the GPU: run in fp8, activation scales calibrated on the first N inputs "
                         "(block / per-tensor scales or bf16, as the calibration check decides)")
    cl.set_defaults(fn=cmd_classify)

    sg = sub.add_parser("segment", help="per-voxel labels with a segmentation checkpoint")
    sg.add_argument("model")
    sg.add_argument("input", help=".npy array or a folder of .binvox files")
    sg.add_argument("-o", "--output", required=True, help="labels, uint8 [N, S, S, S] (.npy)")
    sg.add_argument("--confidence", default="", metavar="CONF.npy",
                    help="also write the top-1 softmax probability per voxel (float32 .npy)")
    sg.add_argument("--packed-size", type=int, default=None)
    sg.set_defaults(fn=cmd_segment)

    sc = sub.add_parser("score", help="confusion matrix, per-class IoU and mIoU of a segmentation checkpoint")
    sc.add_argument("model")
    sc.add_argument("input", help="voxels (.npy), as for segment")
    sc.add_argument("truth", help="true labels, integer [N, S, S, S] (.npy)")
    sc.add_argument("--ignore-index", type=int, default=None, metavar="K", help="label value of unlabelled voxels")
    sc.add_argument("--packed-size", type=int, default=None)
    sc.add_argument("--json", default="", metavar="OUT", help="also write the summary to this file")
    sc.set_defaults(fn=cmd_score)

    ft = sub.add_parser("features", help="feature instances (connected components of the labels) of a "
                                         "segmentation checkpoint")
    ft.add_argument("model")
    ft.add_argument("input", help="voxels (.npy), as for segment")
    ft.add_argument("--json", default="", metavar="OUT", help="also write the JSON document to this file")
    ft.add_argument("--ids", default="", metavar="IDS.npy", help="also write the instance-id volume (int32 .npy)")
    ft.add_argument("--background", type=int, default=0, metavar="B",
                    help="class that forms no instance (default 0; -1: every class does)")
    ft.add_argument("--connectivity", type=int, default=6, choices=(6, 26))
    ft.add_argument("--min-voxels", type=int, default=1, metavar="K", help="leave out smaller instances")
    ft.add_argument("--packed-size", type=int, default=None)
    ft.add_argument("--access", action="store_true",
                    help="add the access directions: voxels open toward each face (+z -z +x -x +y -y), open_faces, "
                         "through, enclosed")
    ft.add_argument("--access-fraction", type=float, default=1.0, metavar="F",
                    help="with --access: a face is open when at least this fraction of the voxels is (default 1.0)")
    ft.add_argument("--dimensions", action="store_true",
                    help="add the clear widths: clearance2 (largest squared distance to the material), clearance_at, "
                         "tool_diameter, wall_voxels")
    ft.add_argument("--tool", type=float, default=None, metavar="T",
                    help="add the reach of a ball-shaped tool of diameter T voxels: entry2 and reachable per face, "
                         "tool_faces (at --access-fraction), unreachable, machinable, residual")
    ft.add_argument("--contacts", action="store_true",
                    help="add what each feature borders: wall_area, open_area, shared_area and floor per face, surface, "
                         "neighbors (id, face, faces)")
    ft.add_argument("--walls", type=float, nargs="?", const=True, default=None, metavar="T",
                    help="add the gap to the nearest other feature of the part: gap2, gap_at, gap_to, min_wall; with T "
                         "also thin_voxels, the voxels with another feature behind a wall of at most T voxels")
    ft.add_argument("--classifier", default="", metavar="CLF.fnk",
                    help="add the single-feature classifier's opinion on every feature put alone into a solid stock "
                         "block: recognized, recognized_prob, agrees")
    ft.set_defaults(fn=cmd_features)

    rg = sub.add_parser("recognize", help="the features of multi-feature parts by a single-feature classifier "
                                          "checkpoint alone: removed volume -> components -> each one alone in a "
                                          "solid block -> class")
    rg.add_argument("model", help="FeatureNet-3D classifier checkpoint (.fnk)")
    rg.add_argument("input", help="[N, D, H, W] occupancy (.npy), non-zero = material")
    rg.add_argument("--json", default="", metavar="OUT", help="also write the JSON document to this file")
    rg.add_argument("--labels", default="", metavar="LABELS.npy",
                    help="also write the label volume (uint8 .npy): 1 + class on every voxel of a feature, else 0")
    rg.add_argument("--ids", default="", metavar="IDS.npy", help="also write the instance-id volume (int32 .npy)")
    rg.add_argument("--stock", default="grid", choices=("grid", "bbox"),
                    help="the stock the part was cut from: the whole grid, or the bounding box of the material")
    rg.add_argument("--connectivity", type=int, default=6, choices=(6, 26))
    rg.add_argument("--min-voxels", type=int, default=1, metavar="K", help="leave out smaller components")
    rg.add_argument("--device", default="", help="cuda / cpu (default: where the checkpoint loads)")
    rg.add_argument("--access", action="store_true", help="as for features")
    rg.add_argument("--dimensions", action="store_true", help="as for features")
    rg.add_argument("--tool", type=float, default=None, metavar="T", help="as for features")
    rg.add_argument("--contacts", action="store_true", help="as for features")
    rg.add_argument("--walls", type=float, nargs="?", const=True, default=None, metavar="T", help="as for features")
    rg.add_argument("--split", type=float, nargs="?", const=1.0, default=None, metavar="H",
                    help="cut touching features apart first (a watershed on the distance to the material); two "
                         "peaks stay one feature when the lower rises less than H voxels of clearance above the pass "
                         "between them (a multiple of 0.5, default 1); adds component and peak2")
    rg.set_defaults(fn=cmd_recognize)

    sp = sub.add_parser("split", help="touching features told apart: each component of an instance-id volume cut "
                                      "along the passes of the distance to the material -> int32 .npy and JSON")
    sp.add_argument("ids", help="[N, D, H, W] integer instance ids (.npy), > 0 = a component's voxel, each axis at "
                                "most 256")
    sp.add_argument("voxels", help="[N, D, H, W] occupancy (.npy), non-zero = material")
    sp.add_argument("-o", "--output", required=True, help="the new instance ids, int32, the input's shape (.npy)")
    sp.add_argument("--merge", type=float, default=1.0, metavar="H",
                    help="two peaks stay one feature when the lower rises less than H voxels of clearance above the "
                         "pass between them (a multiple of 0.5, default 1)")
    sp.add_argument("--device", default="", help="cuda / cpu (default: the GPU when there is one)")
    sp.add_argument("--json", default="", metavar="OUT", help="also write the JSON document to this file")
    sp.set_defaults(fn=cmd_split)

    nr = sub.add_parser("nearest", help="labelled distance transform: the nearest and the nearest other instance of "
                                        "every voxel with their squared distances -> .npz (d2, nearest)")
    nr.add_argument("input", help="[D, H, W] or [N, D, H, W] integer instance ids (.npy), > 0 = an instance's voxel, "
                                  "each axis at most 128")
    nr.add_argument("-o", "--output", required=True,
                    help="d2 and nearest, int32 [2, D, H, W] or [N, 2, D, H, W]: rank 0 the nearest instance, rank 1 "
                         "the nearest other one (.npz)")
    nr.add_argument("--device", default="", help="cuda / cpu (default: the GPU when there is one)")
    nr.add_argument("--json", default="", metavar="OUT", help="also write the summary to this file")
    nr.set_defaults(fn=cmd_nearest)

    rc = sub.add_parser("reach", help="directional clearance: the squared clearance of the largest ball that reaches "
                                      "each voxel in a straight line from each face -> int32 .npy")
    rc.add_argument("input", help="[D, H, W] or [N, D, H, W] integer or bool array (.npy), non-zero = material, each "
                                  "axis at most 256")
    rc.add_argument("-o", "--output", required=True,
                    help="r6, int32 [6, D, H, W] or [N, 6, D, H, W], faces +z -z +x -x +y -y (.npy)")
    rc.add_argument("--device", default="", help="cuda / cpu (default: the GPU when there is one)")
    rc.add_argument("--json", default="", metavar="OUT", help="also write the summary to this file")
    rc.set_defaults(fn=cmd_reach)

    dt = sub.add_parser("distance", help="exact squared Euclidean distance to the nearest non-zero voxel -> int32 .npy")
    dt.add_argument("input", help="[D, H, W] or [N, D, H, W] integer or bool array (.npy), each axis at most 256")
    dt.add_argument("-o", "--output", required=True, help="squared distances, int32, the input's shape (.npy)")
    dt.add_argument("--border", action="store_true", help="the positions just outside the grid count as non-zero too")
    dt.add_argument("--device", default="", help="cuda / cpu (default: the GPU when there is one)")
    dt.add_argument("--json", default="", metavar="OUT", help="also write the summary to this file")
    dt.set_defaults(fn=cmd_distance)

    sf = sub.add_parser("score-features", help="match the predicted feature instances of a segmentation checkpoint "
                                               "to the true ones: per-class TP / FP / FN, F1, panoptic quality")
    sf.add_argument("model")
    sf.add_argument("input", help="voxels (.npy), as for segment")
    sf.add_argument("truth", help="true labels, integer [N, S, S, S] (.npy)")
    sf.add_argument("--json", default="", metavar="OUT", help="also write the summary to this file")
    sf.add_argument("--iou", type=float, default=0.5, metavar="T",
                    help="a pair matches when its IoU exceeds T (0.5 <= T < 1)")
    sf.add_argument("--min-voxels", type=int, default=1, metavar="K", help="leave out smaller instances on both sides")
    sf.add_argument("--connectivity", type=int, default=6, choices=(6, 26))
    sf.add_argument("--background", type=int, default=0, metavar="B",
                    help="class that forms no instance (default 0; -1: every class does)")
    sf.add_argument("--packed-size", type=int, default=None)
    sf.set_defaults(fn=cmd_score_features)

    gp = sub.add_parser("generate-parts", help="procedural multi-feature parts with per-voxel labels -> .npz")
    gp.add_argument("-n", type=int, default=16, help="number of parts")
    gp.add_argument("--size", type=int, default=64, help="grid edge (a multiple of 8, at most 256)")
    gp.add_argument("--seed", type=int, default=0)
    gp.add_argument("--features", type=int, nargs=2, default=[1, 4], metavar=("LO", "HI"),
                    help="features per part")
    gp.add_argument("--overlap", action="store_true", help="let features overlap (the lowest slot owns shared voxels)")
    gp.add_argument("--device", default="", help="cuda / cpu (default: the GPU when there is one)")
    gp.add_argument("-o", "--output", required=True, help="voxels and labels, uint8 [N, S, S, S] each (.npz)")
    gp.add_argument("--json", default="", metavar="OUT", help="also write the per-part feature lists to this file")
    gp.set_defaults(fn=cmd_generate_parts)

    vx = sub.add_parser("voxelize", help="STL meshes -> occupancy .npy (the input of classify / segment / features)")
    vx.add_argument("meshes", nargs="+", help="binary or ASCII STL files")
    vx.add_argument("--size", type=int, default=64, help="grid edge (a multiple of 8, at most 256)")
    vx.add_argument("--margin", type=float, default=0, help="empty voxels at either end of the longest side")
    vx.add_argument("--origin", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                    help="with --voxel-size: the model-space corner of voxel (0, 0, 0)")
    vx.add_argument("--voxel-size", type=float, default=None,
                    help="edge of a voxel in model units (default: fit each mesh's bounding box to the grid)")
    vx.add_argument("--device", default="", help="cuda / cpu (default: the GPU when there is one)")
    vx.add_argument("-o", "--output", required=True, help="occupancy, uint8 [N, S, S, S] (.npy)")
    vx.add_argument("--json", default="", metavar="OUT", help="also write leaks and transforms to this file")
    vx.add_argument("--binvox", default="", metavar="DIR", help="also write one .binvox per mesh into this folder")
    vx.set_defaults(fn=cmd_voxelize)

    lm = sub.add_parser("label-mesh", help="instance ids or labels on the grid (.npy) -> the id against each triangle of the STL")
    lm.add_argument("mesh", help="the binary or ASCII STL file the volume was voxelized from")
    lm.add_argument("ids", help="[S, S, S] or [N, S, S, S] integer array (.npy): instance ids or labels, 0 = nothing")
    lm.add_argument("--index", type=int, default=0, help="which volume of an [N, S, S, S] array")
    lm.add_argument("--fit", nargs="+", default=[], metavar="FIT",
                    help="'bbox' (default) or OX OY OZ VOXEL_SIZE, the origin and voxel_size that voxelize --json reports")
    lm.add_argument("--margin", type=float, default=0, help="as given to voxelize")
    lm.add_argument("--origin", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                    help="with --voxel-size: the model-space corner of voxel (0, 0, 0)")
    lm.add_argument("--voxel-size", type=float, default=None,
                    help="edge of a voxel in model units (default: fit the mesh's bounding box to the grid, as voxelize does)")
    lm.add_argument("--device", default="", help="cuda / cpu (default: the GPU when there is one)")
    lm.add_argument("-o", "--output", required=True, help="winners, int32 [F] (.npy)")
    lm.add_argument("--json", default="", metavar="OUT", help="also write the summary to this file")
    lm.add_argument("--obj", default="", metavar="OUT",
                    help="also write the triangles as an OBJ with one group per feature (g feature_<id>, g unlabelled)")
    lm.set_defaults(fn=cmd_label_mesh)

    xs = sub.add_parser("export-stl", help="boundary of a voxel volume (.npy) -> STL")
    xs.add_argument("input", help="[S, S, S] or [N, S, S, S] array (.npy)")
    xs.add_argument("-o", "--output", required=True)
    xs.add_argument("--index", type=int, default=0, help="which volume of an [N, S, S, S] array")
    xs.add_argument("--value", type=int, default=None,
                    help="export the voxels equal to this value (a label or an instance id; default: every non-zero one)")
    xs.add_argument("--origin", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"))
    xs.add_argument("--voxel-size", type=float, default=1.0)
    xs.add_argument("--ascii", action="store_true")
    xs.set_defaults(fn=cmd_export_stl)

    e = sub.add_parser("extend", help="expand the 1-block template to B x C")
    e.add_argument("--input", default="")
    e.add_argument("--output", required=True)
    e.add_argument("--blocks", type=int, default=5)
    e.add_argument("--cells", type=int, default=5)
    e.add_argument("--block-features", action="store_true")
    e.set_defaults(fn=cmd_extend)

    sm = sub.add_parser("sample", help="sample diverse valid products (native PLEDGE)")
    sm.add_argument("fm")
    sm.add_argument("-n", type=int, default=100)
    sm.add_argument("-o", "--output", required=True)
    sm.add_argument("--duration", type=float, default=30.0)
    sm.add_argument("--seed", type=int, default=0)
    sm.set_defaults(fn=cmd_sample)

    tp = sub.add_parser("template", help="write the built-in search-space FM")
    tp.add_argument("output")
    tp.set_defaults(fn=cmd_template)
    return p


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
