"""Public Python API: ``train()``, ``classify()``, ``segment()``, ``extract_features()``,
``label_components()``, ``recognize()``, ``isolate_features()``, ``evaluate()``, ``evaluate_segmentation()``, ``evaluate_features()``,
``match_features()``, ``generate_parts()``, ``voxelize()``, ``distance_transform()``, ``load()``, ``save()``, ``build_model()`` and ``search()``.

Reference parity: the de-facto entry point of the reference is the
``TensorflowGenerator(product, epochs, dataset, ...)`` constructor
(``tensorflow_generator.py:97-136``), which parses a product / template,
builds, trains, evaluates and scores robustness in one go.  Here the same
pipeline is split into composable calls:

    >>> import featurenet_amd as fn
    >>> res = fn.train("featurenet3d", data="voxel", epochs=2)        # 64^3, 24 classes
    >>> labels, probs = fn.classify(res.path, voxels)
    >>> seg = fn.train("segmentation", data="voxel-seg", epochs=4)     # per-voxel labels, generated parts
    >>> res = fn.train("lenet5", data="mnist", epochs=12)              # NAS template
    >>> res = fn.train(product_tree, data="cifar", epochs=25)          # a PLEDGE product

``arch`` may be ``"featurenet3d"`` / a :class:`FeatureNet3DConfig`, an IR
:class:`ModelSpec`, a template name (``lenet5``, ``keras``, ...), or a product
tree (list of block dicts from :class:`~featurenet_amd.fm.products.ProductSet`).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import torch

from .ir.compile import CandidateNet, compile_model
from .ir.parse import parse_feature_model
from .ir.spec import ModelSpec
from .ir.templates import TEMPLATES
from .ops.reference import EDT_INF  # noqa: F401
from .models.featurenet3d import FeatureNet3D, FeatureNet3DConfig, FeatureNet3DSeg
from .training.callbacks import reference_callbacks
from .training.checkpoint import read_checkpoint, save_checkpoint
from .training.data import Dataset, load_dataset
from .training.trainer import Trainer


@dataclass
class TrainResult:
    model: torch.nn.Module
    trainer: Trainer
    history: dict
    accuracy: float
    loss: float
    path: str | None = None
    spec: ModelSpec | None = None
    meta: dict = field(default_factory=dict)


def _is_featurenet3d(arch) -> bool:
    return isinstance(arch, FeatureNet3DConfig) or (isinstance(arch, str) and arch.lower() in
                                                     ("featurenet3d", "featurenet-3d", "featurenet"))


def build_model(arch, input_shape: tuple, num_classes: int, compat: bool = True, fill_defaults: bool = False):
    """-> (module, meta) where meta describes how to rebuild it from a checkpoint."""
    if _is_featurenet3d(arch):
        cfg = arch if isinstance(arch, FeatureNet3DConfig) else FeatureNet3DConfig(
            input_size=int(input_shape[0]), in_channels=int(input_shape[-1]), num_classes=num_classes)
        return FeatureNet3D(cfg), {"model_kind": "featurenet3d", "config": cfg.to_dict()}
    if isinstance(arch, str) and arch.lower() in ("featurenet3d-seg", "segmentation"):
        m = FeatureNet3DSeg(input_size=int(input_shape[0]), in_channels=int(input_shape[-1]), num_classes=num_classes)
        return m, {"model_kind": "featurenet3d_seg", "input_size": int(input_shape[0]),
                   "in_channels": int(input_shape[-1]), "num_classes": num_classes}
    if isinstance(arch, ModelSpec):
        spec = arch
    elif isinstance(arch, str):
        if arch not in TEMPLATES:
            raise ValueError(f"unknown architecture / template {arch!r}")
        spec = parse_feature_model(arch, name=arch)
    else:
        spec = parse_feature_model(arch)
    net = compile_model(spec, tuple(input_shape), num_classes, compat=compat, fill_defaults=fill_defaults)
    spec.nb_params, spec.nb_layers, spec.nb_flops = net.nb_params, net.nb_layers, net.flops_per_sample
    return net, {"model_kind": "candidate", "spec": spec.to_dict(), "input_shape": list(input_shape),
                 "num_classes": num_classes, "compat": compat, "fill_defaults": fill_defaults}


def _resolve_data(data, batch_size) -> Dataset:
    if isinstance(data, Dataset):
        return data
    if isinstance(data, str):
        return load_dataset(data)
    if isinstance(data, (tuple, list)) and len(data) == 4:
        xtr, ytr, xte, yte = data
        ncls = int(max(np.max(ytr), np.max(yte)) + 1)
        return Dataset("custom", xtr, ytr, xte, yte, ncls, tuple(np.asarray(xtr).shape[1:]))
    raise ValueError("data must be a dataset name, a Dataset or (x_train, y_train, x_test, y_test)")


def train(arch="featurenet3d", data="voxel", epochs: int = 12, batch_size: int = 128, lr: float = 1e-3,
          optimizer: str = "adam", device=None, callbacks=None, augment: bool = False, scheduler: bool = False,
          save_path: str | None = None, compat: bool = True, fill_defaults: bool = False, verbose: int = 1,
          seed: int = 0, robustness: list | None = None, graph: bool = True, precise_bn: int = 32) -> TrainResult:
    """Build + train + evaluate one architecture (the reference ``TensorflowGenerator`` pipeline)."""
    torch.manual_seed(seed)
    ds = _resolve_data(data, batch_size)
    model, meta = build_model(arch, ds.input_shape, ds.num_classes, compat=compat, fill_defaults=fill_defaults)
    meta.update({"dataset": ds.name, "synthetic_data": ds.synthetic})
    trainer = Trainer(model, optimizer=optimizer, lr=lr, device=device, meta=meta, graph=graph, precise_bn=precise_bn)
    cbs = list(callbacks) if callbacks is not None else reference_callbacks(scheduler)
    packed = ds.input_shape[0] if ds.packed else None
    hist = trainer.fit(ds.x_train, ds.y_train, epochs=epochs, batch_size=batch_size,
                       validation_data=(ds.x_test, ds.y_test), callbacks=cbs, augment=augment,
                       packed_size=packed, verbose=verbose, seed=seed)
    loss, acc = trainer.evaluate(ds.x_test, ds.y_test, packed_size=packed)
    meta.update({"accuracy": acc, "test_loss": loss})
    trainer.meta.update(meta)
    spec = None
    if meta["model_kind"] == "candidate":
        spec = ModelSpec.from_dict(meta["spec"])
        spec.accuracy, spec.status, spec.history = acc, "trained", hist.history
    if robustness:
        from .robust.evaluate import eval_robustness

        scores = eval_robustness(model, ds, robustness, device=trainer.device)
        meta["robustness"] = scores
        if spec is not None:
            spec.robustness_score = scores.get("score", 0.0)
    path = None
    if save_path:
        path = str(trainer.save(save_path))
    return TrainResult(model, trainer, hist.history, acc, loss, path, spec, meta)


def save(model: torch.nn.Module, path: str | Path, meta: dict) -> Path:
    return save_checkpoint(path, model, meta)


def load(path: str | Path, device=None) -> tuple[torch.nn.Module, dict]:
    """Rebuild a model from a ``.fnk`` checkpoint (weights + architecture)."""
    meta, state, _ = read_checkpoint(path)
    kind = meta.get("model_kind")
    if kind == "featurenet3d":
        model = FeatureNet3D(FeatureNet3DConfig.from_dict(meta["config"]))
    elif kind == "featurenet3d_seg":
        model = FeatureNet3DSeg(meta["input_size"], meta["in_channels"], meta["num_classes"])
    elif kind == "candidate":
        spec = ModelSpec.from_dict(meta["spec"])
        model = compile_model(spec, tuple(meta["input_shape"]), int(meta["num_classes"]),
                              compat=meta.get("compat", True), fill_defaults=meta.get("fill_defaults", False))
    else:
        raise ValueError(f"{path}: unknown model kind {kind!r}")
    model.load_state_dict(state)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    return model.to(device).eval(), meta


@torch.no_grad()
def classify(model, x, batch_size: int = 256, device=None, packed_size: int | None = None, fp8_calib=None):
    """Predict classes for ``x`` -> (labels int64 [N], probabilities [N, C]).

    ``model`` may be a module or a checkpoint path.  For voxel models ``x`` is
    ``[N, S, S, S]`` / ``[N, S, S, S, 1]`` occupancy (any dtype) or bit-packed
    ``uint8 [N, S^3/8]`` with ``packed_size=S``.

    ``fp8_calib`` (FeatureNet-3D on the GPU): calibration voxels in the same format as ``x``; the
    model then runs in fp8 (OCP e4m3) with the numerics its calibration check chooses --
    block-scaled activations, per-tensor scales, or bf16 when neither agrees with the bf16 model
    on >= 99 % of the calibration set (``inference.fp8.quantize_model(fallback=True)``,
    profiles/r6_fp8_fallback.md).
    """
    if isinstance(model, (str, Path)):
        model, _ = load(model, device)
    dev = next(model.parameters()).device
    model.eval()
    from .training.data import unpack_voxels

    def prep(xb):
        xb = xb.to(dev)
        if packed_size is not None:
            xb = unpack_voxels(xb, packed_size)
        return xb.to(torch.bfloat16) if dev.type == "cuda" else xb.float()

    fwd = model
    if fp8_calib is not None:
        from .models.featurenet3d import FeatureNet3D

        if dev.type != "cuda" or not isinstance(model, FeatureNet3D):
            raise ValueError("fp8 inference (fp8_calib) takes a FeatureNet-3D model on the GPU")
        from .inference.fp8 import quantize_model

        ct = torch.as_tensor(np.asarray(fp8_calib)) if not isinstance(fp8_calib, torch.Tensor) else fp8_calib
        fwd = quantize_model(model, prep(ct), fallback=True)
    xt = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    probs = []
    for i in range(0, len(xt), batch_size):
        probs.append(torch.softmax(fwd(prep(xt[i:i + batch_size])).float(), -1).cpu())
    p = torch.cat(probs).numpy() if probs else np.zeros((0, 0), np.float32)
    return p.argmax(-1), p


@torch.no_grad()
def segment(model, x, batch_size: int = 32, device=None, packed_size: int | None = None,
            return_confidence: bool = False):
    """Per-voxel labels of a segmentation model -> (labels uint8 [N, S, S, S], confidence float32
    [N, S, S, S] or None).

    ``model`` is a :class:`FeatureNet3DSeg` or a checkpoint path of one; ``x`` as for
    :func:`classify`.  Runs ``FeatureNet3DSeg.predict``: the logits are never stored, and only the
    labels (one byte per voxel) and, with ``return_confidence``, the top-1 softmax probability
    cross to the host.  Ties go to the lowest class index.
    """
    if isinstance(model, (str, Path)):
        model, _ = load(model, device)
    if not isinstance(model, FeatureNet3DSeg):
        raise ValueError(f"segment() takes a FeatureNet3DSeg model, not {type(model).__name__} (see classify())")
    dev = next(model.parameters()).device
    model.eval()
    from .training.data import unpack_voxels

    xt = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    labels, confs = [], []
    for i in range(0, len(xt), batch_size):
        xb = xt[i:i + batch_size].to(dev)
        if packed_size is not None:
            xb = unpack_voxels(xb, packed_size)
        xb = xb.to(torch.bfloat16) if dev.type == "cuda" else xb.float()
        out = model.predict(xb, want_conf=return_confidence)
        lb, cf = out if return_confidence else (out, None)
        labels.append(lb.cpu())
        if cf is not None:
            confs.append(cf.float().cpu())
    S = model.input_size
    lab = torch.cat(labels).numpy() if labels else np.zeros((0, S, S, S), np.uint8)
    if not return_confidence:
        return lab, None
    return lab, (torch.cat(confs).numpy() if confs else np.zeros((0, S, S, S), np.float32))


@torch.no_grad()
def evaluate_segmentation(model, x, y, batch_size: int = 32, device=None, packed_size: int | None = None,
                          ignore_index: int | None = None):
    """Score a segmentation model against true per-voxel labels -> :class:`SegScore` (confusion
    matrix, accuracy, per-class IoU / precision / recall / dice, mIoU).

    ``model`` and ``x`` as for :func:`segment`; ``y`` is ``[N, S, S, S]`` of any integer dtype with
    values 0..255.  Voxels whose label equals ``ignore_index`` are left out.  Runs
    ``FeatureNet3DSeg.score``: on the GPU the head counts (truth, label) pairs in its own kernel,
    the matrix is summed over the batches on the device and crosses to the host once, at the end.
    """
    from .utils.segmetrics import SegScore

    if isinstance(model, (str, Path)):
        model, _ = load(model, device)
    if not isinstance(model, FeatureNet3DSeg):
        raise ValueError(f"evaluate_segmentation() takes a FeatureNet3DSeg model, not {type(model).__name__} "
                         "(see evaluate())")
    dev = next(model.parameters()).device
    model.eval()
    from .training.data import unpack_voxels

    xt = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    yt = torch.as_tensor(np.asarray(y)) if not isinstance(y, torch.Tensor) else y
    if yt.is_floating_point() or yt.dtype == torch.bool:
        raise ValueError(f"evaluate_segmentation(): labels must be integers, not {yt.dtype}")
    if len(yt) != len(xt):
        raise ValueError(f"evaluate_segmentation(): {len(xt)} samples but {len(yt)} label volumes")
    if yt.dtype != torch.uint8 and yt.numel() and not yt.is_cuda and (int(yt.min()) < 0 or int(yt.max()) > 255):
        raise ValueError("evaluate_segmentation(): label values must lie in 0..255")
    C = model.num_classes
    acc = torch.zeros(C * C + 1, dtype=torch.int64, device=dev)
    for i in range(0, len(xt), batch_size):
        xb = xt[i:i + batch_size].to(dev)
        if packed_size is not None:
            xb = unpack_voxels(xb, packed_size)
        xb = xb.to(torch.bfloat16) if dev.type == "cuda" else xb.float()
        acc, _ = model.score(xb, yt[i:i + batch_size].to(dev).to(torch.uint8), ignore_index=ignore_index, acc=acc)
    counts = acc.cpu().numpy()
    if counts[-1]:
        raise ValueError(f"evaluate_segmentation(): {int(counts[-1])} voxels carry a label >= {C} (the model's "
                         "class count); pass ignore_index to mask unlabelled voxels")
    return SegScore.from_confusion(counts[:-1].reshape(C, C))


@torch.no_grad()
def extract_features(model, x, batch_size: int = 32, device=None, packed_size: int | None = None,
                     background: int | None = 0, connectivity: int = 6, min_voxels: int = 1,
                     return_ids: bool = False, access: bool = False, dimensions: bool = False, tool=None,
                     contacts: bool = False, walls=False, classifier=None, meshes=None, fit="bbox",
                     margin: float = 0):
    """The machining features of each part -> (one list of :class:`FeatureInstance` per sample,
    ids int32 [N, S, S, S] or None).

    ``model`` and ``x`` as for :func:`segment`.  Runs ``FeatureNet3DSeg.instances``: the per-voxel
    labels are split into connected components of one class (``connectivity`` 6 = faces, 26 =
    faces, edges and corners; voxels of class ``background`` -- None: no such class -- belong to
    none) on the model's device, and only the instance table (13 integers per component) crosses
    to the host, plus, with ``return_ids``, the volume that numbers each sample's components from
    1 in raster order of their first voxel.  ``min_voxels`` drops smaller components from the lists
    only: the others keep their ``id``, and ``ids`` keeps every component.

    With ``access`` every record also says from which faces of the grid the feature is reached
    (``FeatureInstance.access``, ``open_faces()``, ``through``, ``enclosed``): a voxel is open
    toward ``+x`` when no material (``x != 0``) lies beyond it in its x column, and so on for the
    six faces ``+z, -z, +x, -x, +y, -y`` (``+z`` is the high-index end of z).  The counts are made
    on the model's device (``ops.access``); 8 more integers per component cross to the host.

    With ``dimensions`` every record also says how wide the feature is: ``clearance2`` is the
    largest squared Euclidean distance from one of its voxels to the nearest material voxel (``x
    != 0``; the faces of the grid are no wall, so a through hole is measured against its side),
    ``clearance_at`` the first voxel that attains it, ``wall_voxels`` the voxels with a material
    face neighbour; ``clearance`` and ``tool_diameter`` follow from these.  The distance transform
    runs on the model's device (``ops.edt``); 4 more integers per component cross to the host.

    With ``tool``, the diameter in voxels of a ball-shaped tool (the convention of
    ``tool_diameter``), every record also says what that tool does to the feature: ``entry2`` is,
    per face, the largest squared clearance of a straight path from outside that face to one of
    its voxels (``entry_diameter(face)``), ``reachable`` the voxels the tool's centre reaches
    from each face, ``unreachable`` those it reaches from none, ``machinable`` the voxels it removes
    from the centres it reaches (``residual``: the rest); ``tool_faces()`` names the faces it can
    come from.  Runs on the model's device (``ops.reach``); 15 more integers per component cross
    to the host.

    With ``contacts`` every record also says what the feature borders: ``wall_area``, ``open_area``
    and ``shared_area`` are, per side ``+z, -z, +x, -x, +y, -y``, the faces of its voxels that meet
    material (``x != 0``), free space or the outside of the grid, and another feature; ``neighbors``
    lists ``(id, face, faces)`` for every feature of the same part it touches and the side on which
    that one lies; ``surface``, ``floor(face)``, ``blind(face)`` and ``entered_through(face)`` follow
    from these.  Runs on the model's device (``ops.contact``); 19 more integers per component and 4
    per touching pair and side cross to the host.

    With ``walls`` -- True, or a wall thickness ``t`` in voxels -- every record also says how close
    the feature comes to another one of its part without touching it: ``gap2`` is the smallest
    squared distance from one of its voxels to a voxel of another feature, ``gap_at`` the first voxel
    that attains it, ``gap_to`` the id of the feature nearest to that voxel, and ``gap`` and
    ``min_wall`` (the wall left between the two, in voxels: ``max(0, gap - 1)``) follow from these;
    all are None for a feature alone in its part.  With a thickness, ``thin_voxels`` counts its voxels
    that have another feature behind a wall of at most ``t`` voxels.  The labelled distance
    transform runs on the model's device (``ops.nearest``); 5 more integers per component cross to
    the host.

    With ``classifier`` -- a :class:`FeatureNet3D` or a checkpoint path of one, with the grid's size as
    its input size -- every record also carries the single-feature classifier's second opinion:
    ``recognized`` is the class (0..C-1) it gives to the component put alone into a solid stock block
    (``ops.isolate``, the FeatureNet paper's recipe), ``recognized_prob`` that class's probability, and
    ``agrees`` says whether ``cls == recognized + 1``.  The parts are made and classified on the model's
    device; two numbers per component cross to the host.

    With ``meshes`` -- the meshes ``x`` was voxelized from, as for :func:`voxelize`, with the ``fit`` and
    ``margin`` used there -- every record also says which triangles of its part's mesh are its own:
    ``faces`` holds the indices of the triangles that :func:`label_mesh` gives to its ``id``.
    """
    from .utils.seginstances import FeatureInstance, tool_thresholds

    thresholds = None if tool is None else tool_thresholds(tool)
    limit2 = _wall_limit(walls)
    if isinstance(model, (str, Path)):
        model, _ = load(model, device)
    if classifier is not None:
        classifier, _ = _classifier(classifier, next(model.parameters()).device, "extract_features()")
    if not isinstance(model, FeatureNet3DSeg):
        raise ValueError(f"extract_features() takes a FeatureNet3DSeg model, not {type(model).__name__} "
                         "(see classify())")
    if connectivity not in (6, 26):
        raise ValueError(f"extract_features(): connectivity must be 6 or 26, not {connectivity!r}")
    dev = next(model.parameters()).device
    model.eval()
    from .training.data import unpack_voxels

    xt = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    feats, ids = [], []
    for i in range(0, len(xt), batch_size):
        xb = xt[i:i + batch_size].to(dev)
        if packed_size is not None:
            xb = unpack_voxels(xb, packed_size)
        xb = xb.to(torch.bfloat16) if dev.type == "cuda" else xb.float()
        table, offsets, idb, *more = model.instances(xb, background=background, connectivity=connectivity,
                                                     want_ids=return_ids or classifier is not None
                                                     or meshes is not None,
                                                     want_access=access, want_dims=dimensions,
                                                     want_reach=thresholds, want_contacts=contacts,
                                                     want_walls=limit2)
        wall = None
        if limit2 is not None:
            *more, wall = more
        pairs = None
        if contacts:
            *more, con, adj = more
            pairs = (con, adj)
        seen = None
        if classifier is not None:
            from .ops import isolate

            seen = isolate.recognize_table(classifier, idb, table, offsets, rows=table.shape[0],
                                           min_voxels=min_voxels)[:2]
        feats += FeatureInstance.from_table(table, offsets, min_voxels, access=more[0] if access else None,
                                            dims=more[1 if access else 0] if dimensions else None,
                                            shape=tuple(xb.shape[1:4]),
                                            reach=more[-1] if thresholds is not None else None, tool=thresholds,
                                            contacts=pairs, walls=wall, thin=walls is not True, recognized=seen)
        if return_ids or meshes is not None:
            ids.append(idb.cpu())
    if meshes is not None:
        S = model.input_size
        _assign_faces(feats, torch.cat(ids) if ids else torch.zeros((0, S, S, S), dtype=torch.int32), meshes, fit,
                      margin, dev, "extract_features()")
    if not return_ids:
        return feats, None
    S = model.input_size
    return feats, (torch.cat(ids).numpy() if ids else np.zeros((0, S, S, S), np.int32))


@torch.no_grad()
def label_components(labels, background: int | None = 0, connectivity: int = 6, device=None, occupancy=None,
                     dimensions: bool = False, tool=None, contacts: bool = False, walls=False, classifier=None,
                     min_voxels: int = 1, batch_size: int = 256, split=None):
    """Connected components of label volumes the caller already has (ground truth, say) ->
    (ids int32 [N, D, H, W], one list of :class:`FeatureInstance` per sample).

    ``labels`` is ``[N, D, H, W]`` of any integer dtype with values
    0..255; ``background`` and ``connectivity`` as for :func:`extract_features`.  ``device``
    defaults to the GPU when there is one (the ``ccl`` kernels), else the CPU reference path.
    ``occupancy``, an integer or bool array of the labels' shape (material: non-zero), adds the
    access counts to the records as :func:`extract_features` does with ``access``; ``dimensions``
    (which needs ``occupancy``) adds the clear widths as its ``dimensions`` does, ``tool`` (a
    diameter in voxels, which needs ``occupancy`` too) the reach of that tool as its ``tool`` does,
    ``contacts`` (which needs ``occupancy`` too) the wall, open and shared areas and the neighbours
    as its ``contacts`` does, ``walls`` (True or a wall thickness in voxels; it needs no
    ``occupancy``) the gap to the nearest other feature as its ``walls`` does, ``classifier`` (a
    :class:`FeatureNet3D` or a checkpoint path of one; it needs no ``occupancy``) the single-feature
    classifier's ``recognized`` / ``recognized_prob`` as its ``classifier`` does: the grid is resampled
    to the classifier's input size, ``batch_size`` parts run at a time, and components of fewer than
    ``min_voxels`` voxels are not classified -- they stay in the lists with ``recognized = None``.
    ``split`` (a merge height in voxels, a multiple of 0.5; it needs ``occupancy``) cuts every component
    along the passes of the distance to the material before anything else is computed, as
    :func:`split_features` does: the ids, the records and every table are those of the pieces, which keep
    their component's class and carry ``component`` and ``peak2``.  None leaves every result as it is.
    """
    from .ops import ccl
    from .utils.seginstances import FeatureInstance, tool_thresholds

    if split is not None and occupancy is None:
        raise ValueError("label_components(): split needs occupancy (the material the passes are measured against)")
    if dimensions and occupancy is None:
        raise ValueError("label_components(): dimensions=True needs occupancy (the material the widths are "
                         "measured against)")
    if tool is not None and occupancy is None:
        raise ValueError("label_components(): tool needs occupancy (the material the tool must clear)")
    if contacts and occupancy is None:
        raise ValueError("label_components(): contacts=True needs occupancy (the material that tells a wall from "
                         "an opening)")
    thresholds = None if tool is None else tool_thresholds(tool)
    limit2 = _wall_limit(walls)

    lt = torch.as_tensor(np.asarray(labels)) if not isinstance(labels, torch.Tensor) else labels
    if lt.is_floating_point() or lt.dtype == torch.bool:
        raise ValueError(f"label_components(): labels must be integers, not {lt.dtype}")
    if connectivity not in (6, 26):
        raise ValueError(f"label_components(): connectivity must be 6 or 26, not {connectivity!r}")
    if lt.dim() != 4:
        raise ValueError(f"label_components(): labels must be [N, D, H, W], not {tuple(lt.shape)}")
    if lt.dtype != torch.uint8 and lt.numel() and (int(lt.min()) < 0 or int(lt.max()) > 255):
        raise ValueError("label_components(): label values must lie in 0..255")
    if classifier is not None:
        classifier, device = _classifier(classifier, device, "label_components()")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    ot = None
    if occupancy is not None:
        ot = torch.as_tensor(np.asarray(occupancy)) if not isinstance(occupancy, torch.Tensor) else occupancy
        if ot.is_floating_point() or ot.is_complex():
            raise ValueError(f"label_components(): occupancy must be integers or bools, not {ot.dtype}")
        if ot.shape != lt.shape:
            raise ValueError(f"label_components(): occupancy is {tuple(ot.shape)} but labels {tuple(lt.shape)}")
    lt = lt.to(device).to(torch.uint8).contiguous()
    roots, flags = ccl.connected_components(lt, background, connectivity, return_flags=True)
    ids, table, offsets = ccl.instance_table(lt, roots, want_ids=True, flags=flags)
    occ = None if ot is None else (ot.to(device) != 0).to(torch.uint8)
    ids, table, offsets, cut, d2 = _split(ids, table, offsets, occ, split)
    more = _geometry_tables(ids, table, offsets, occ, occ is not None, dimensions, thresholds, contacts, limit2, d2=d2)
    seen = None
    if classifier is not None:
        from .ops import isolate

        seen = isolate.recognize_table(classifier, ids, table, offsets, rows=table.shape[0], min_voxels=min_voxels,
                                       batch_size=batch_size)[:2]
    return ids.cpu().numpy(), FeatureInstance.from_table(table, offsets, shape=tuple(lt.shape[1:]), tool=thresholds,
                                                         thin=walls is not True, recognized=seen, split=cut, **more)


def _split(ids, table, offsets, occ, split):
    """The ``split`` option of :func:`label_components` and :func:`recognize` -> ``(ids, table, offsets, (component,
    peak2) or None, d2 or None)``: with a merge height every component is cut by ``ops.watershed`` on ``d2 =
    distance_sq(occ)``, and a piece keeps its component's class; None passes everything through."""
    if split is None:
        return ids, table, offsets, None, None
    from .ops import edt, watershed

    d2 = edt.distance_sq(occ)
    ids2, table2, offsets2, comp, peak2 = watershed.split_instances(ids, d2, split)
    if len(table2):
        table2[:, 1] = table[offsets[table2[:, 0]] + comp - 1, 1]
    return ids2, table2, offsets2, (comp, peak2), d2


def _geometry_tables(ids, table, offsets, occ, access: bool, dimensions: bool, thresholds, contacts: bool, limit2,
                     d2=None):
    """The optional tables of an id volume as keyword arguments of ``FeatureInstance.from_table``
    (``access``, ``dims``, ``reach``, ``contacts``, ``walls``), each None where it is not asked for.
    Everything but ``walls`` needs the occupancy ``occ``.  ``d2``: ``edt.distance_sq(occ)`` where a split has
    computed it already."""
    from .ops import access as access_, contact, edt, nearest, reach

    acc = dim = rch = pairs = wall = None
    T = table.shape[0]
    if access:
        acc, _ = access_.access_table(ids, offsets, occ, rows=T)
    if dimensions:
        dim, d2 = edt.dimension_table(ids, offsets, occ, rows=T, want_d2=thresholds is not None or d2 is not None,
                                      d2=d2)
    if thresholds is not None:
        rch, _ = reach.reach_table(ids, offsets, occ, *thresholds, rows=T, d2=d2)
    if contacts:
        pairs = contact.contact_table(ids, offsets, occ, rows=T)
    if limit2 is not None:
        wall, _ = nearest.wall_table(ids, offsets, limit2, rows=T)
    return {"access": acc, "dims": dim, "reach": rch, "contacts": pairs, "walls": wall}


def _classifier(classifier, device, what: str):
    """The ``classifier`` option -> ``(a FeatureNet3D on the device, that device)``: a checkpoint path is
    loaded, ``device=None`` is where a module already lives."""
    if isinstance(classifier, (str, Path)):
        classifier, _ = load(classifier, device)
    if not isinstance(classifier, FeatureNet3D):
        raise ValueError(f"{what}: the classifier must be a FeatureNet3D, not {type(classifier).__name__} (a "
                         "segmentation model labels voxels: pass it as the model)")
    dev = next(classifier.parameters()).device if device is None else torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return classifier.to(dev), dev


def _cut_stock(occ: torch.Tensor, stock: str, what: str):
    """``window`` (None: the grid) of the ``stock`` option for an occupancy volume on its device."""
    from .ops import isolate

    if stock == "grid":
        return None
    if stock == "bbox":
        return isolate.material_window(occ)
    raise ValueError(f"{what}: stock must be 'grid' or 'bbox', not {stock!r}")


@torch.no_grad()
def isolate_features(ids, features=None, size: int | None = None, occupancy=None, stock: str = "grid",
                     packed: bool = False, min_voxels: int = 1, device=None):
    """Each feature of an ``ids`` volume alone in a solid stock block -> ``(parts, index)``: ``parts``
    uint8 ``[M, S, S, S]`` (1 = material; the input of :func:`classify`), or with ``packed`` its bits,
    uint8 ``[M, S^3 / 8]`` (``packed_size=S``), and ``index`` int64 ``[M, 2]``, the ``(sample, id)`` of
    every part.

    ``ids`` is ``[N, D, H, W]`` of an integer dtype, as :func:`extract_features` (``return_ids``),
    :func:`label_components` and :func:`recognize` give it: a voxel ``> 0`` belongs to the feature of
    that number in its sample.  ``features``: one list of :class:`FeatureInstance` per sample, the
    features to cut out (their ``id`` and ``bbox`` are used); None: every id that occurs.  Features
    of fewer than ``min_voxels`` voxels are left out.  The stock block is the whole grid
    (``stock="grid"``) or the bounding box of the material of ``occupancy`` (``"bbox"``; non-zero:
    material), scaled by its longest side to ``size`` voxels with the shorter sides centred; a
    voxel looks at the source voxel under its centre, so a feature thinner than ``longest side /
    size`` voxels can vanish.  ``size=None`` takes the grid's own size, which must then be a cube.
    What lies outside the stock is free space (0); inside it everything but the feature itself is
    material, other features too.  ``device`` defaults to the GPU when there is one (the
    ``isolate_parts`` kernel), else the CPU reference path; the result is the same.
    """
    from .ops import isolate

    it = torch.as_tensor(np.asarray(ids)) if not isinstance(ids, torch.Tensor) else ids
    if it.is_floating_point() or it.is_complex() or it.dtype == torch.bool:
        raise ValueError(f"isolate_features(): ids must be integers, not {it.dtype}")
    if it.dim() != 4:
        raise ValueError(f"isolate_features(): ids must be [N, D, H, W], not {tuple(it.shape)}")
    N, D, H, W = it.shape
    if size is None:
        if not D == H == W:
            raise ValueError(f"isolate_features(): size=None takes the grid's size, but {(D, H, W)} is no cube")
        size = D
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 8 or size > 256 or size % 8:
        raise ValueError(f"isolate_features(): size must be a multiple of 8 in [8, 256], not {size!r}")
    if stock not in ("grid", "bbox"):
        raise ValueError(f"isolate_features(): stock must be 'grid' or 'bbox', not {stock!r}")
    if stock == "bbox" and occupancy is None:
        raise ValueError("isolate_features(): stock='bbox' needs occupancy (the material whose box is the stock)")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    it = it.to(device).to(torch.int32).contiguous()
    window = None
    if stock == "bbox":
        ot = torch.as_tensor(np.asarray(occupancy)) if not isinstance(occupancy, torch.Tensor) else occupancy
        if ot.shape != it.shape:
            raise ValueError(f"isolate_features(): occupancy is {tuple(ot.shape)} but ids {tuple(it.shape)}")
        window = isolate.material_window(ot.to(device))
    if features is None:
        top = int(it.max()) if it.numel() else 0
        flat = it.clamp(min=0).reshape(N, -1).to(torch.int64) + (top + 1) * torch.arange(N, device=it.device)[:, None]
        counts = torch.bincount(flat.reshape(-1), minlength=N * (top + 1)).view(N, top + 1)
        counts[:, 0] = 0
        index = torch.nonzero(counts >= max(1, int(min_voxels)))
        box = torch.tensor([0, 0, 0, D - 1, H - 1, W - 1], dtype=torch.int64, device=it.device).expand(len(index), 6)
    else:
        if len(features) != N:
            raise ValueError(f"isolate_features(): {N} samples but {len(features)} feature lists")
        rows = [(n, f.id, *f.bbox) for n, fs in enumerate(features) for f in fs if f.voxels >= min_voxels]
        both = torch.tensor(rows, dtype=torch.int64, device=it.device).reshape(-1, 8)
        index, box = both[:, :2], both[:, 2:]
    win = torch.tensor([0, 0, 0, D, H, W], dtype=torch.int64, device=it.device).expand(len(index), 6) \
        if window is None else window[index[:, 0]]
    sel = torch.cat([index, box, win], 1).to(torch.int32)
    parts = isolate.isolate_instances(it, sel, int(size), 0 if packed else 1)
    return parts.cpu().numpy(), index.cpu().numpy()


@torch.no_grad()
def recognize(classifier, voxels, stock: str = "grid", connectivity: int = 6, min_voxels: int = 1,
              return_ids: bool = False, return_labels: bool = False, batch_size: int = 256, device=None,
              access: bool = False, dimensions: bool = False, tool=None, contacts: bool = False, walls=False,
              split=None, meshes=None, fit="bbox", margin: float = 0):
    """The features of each part by the single-feature classifier alone, the multi-feature recipe of
    the FeatureNet paper -> ``(features, ids or None, labels or None)``: one list of
    :class:`FeatureInstance` per sample, ids int32 ``[N, D, H, W]`` with ``return_ids`` and labels
    uint8 ``[N, D, H, W]`` with ``return_labels``.

    ``classifier`` is a :class:`FeatureNet3D` or a checkpoint path of one; ``voxels`` is ``[N, D, H,
    W]`` occupancy of an integer or bool dtype (non-zero: material), every axis at most 256.  The
    removed volume -- ``voxels == 0`` inside the stock, which is the grid (``stock="grid"``) or the
    bounding box of the material (``"bbox"``) -- is split into ``connectivity``-connected components
    (``ops.ccl``), each component is put back alone into a solid stock block at the classifier's input
    size and classified (``ops.isolate``), all on ``device`` (default: the GPU when there is one).
    A record has ``recognized`` and ``recognized_prob``, and ``cls = 1 + recognized``, the label rule
    of :func:`generate_parts`, so the records compare with those of a segmentation model; ``labels``
    holds that ``cls`` on every voxel of the component and 0 elsewhere, ready for
    :func:`match_features`.  Components of fewer than ``min_voxels`` voxels are left out of the lists
    and of ``labels``; ``ids`` keeps them.  Features that touch are one component; ``split`` (a merge
    height in voxels, a multiple of 0.5; the paper's watershed step) cuts each component along the passes
    of the distance to the material before it is isolated and classified, as :func:`split_features` does
    -- a hole in a pocket floor then becomes a record of its own, with ``component`` and ``peak2`` -- and
    None leaves touching features as one.  ``access``, ``dimensions``, ``tool``, ``contacts`` and
    ``walls`` as for :func:`extract_features`; with ``split`` they describe the pieces.  ``meshes`` (with
    ``fit`` and ``margin``), the meshes ``voxels`` was made from, fills every record's ``faces`` as there.
    """
    from .ops import ccl, isolate
    from .utils.seginstances import FeatureInstance, tool_thresholds

    thresholds = None if tool is None else tool_thresholds(tool)
    limit2 = _wall_limit(walls)
    if connectivity not in (6, 26):
        raise ValueError(f"recognize(): connectivity must be 6 or 26, not {connectivity!r}")
    vt = torch.as_tensor(np.asarray(voxels)) if not isinstance(voxels, torch.Tensor) else voxels
    if vt.is_floating_point() or vt.is_complex():
        raise ValueError(f"recognize(): voxels must be integers or bools, not {vt.dtype}")
    if vt.dim() != 4:
        raise ValueError(f"recognize(): voxels must be [N, D, H, W], not {tuple(vt.shape)}")
    classifier, device = _classifier(classifier, device, "recognize()")
    occ = (vt.to(device) != 0).to(torch.uint8).contiguous()
    window = _cut_stock(occ, stock, "recognize()")
    removed = occ == 0
    if window is not None:
        for axis in (1, 2, 3):
            idx = torch.arange(occ.shape[axis], device=occ.device).view([-1 if a == axis else 1 for a in range(4)])
            lo = window[:, axis - 1].view(-1, 1, 1, 1)
            removed = removed & (idx >= lo) & (idx < lo + window[:, axis + 2].view(-1, 1, 1, 1))
    removed = removed.to(torch.uint8)
    roots, flags = ccl.connected_components(removed, 0, connectivity, return_flags=True)
    ids, table, offsets = ccl.instance_table(removed, roots, want_ids=True, flags=flags)
    ids, table, offsets, cut, d2 = _split(ids, table, offsets, occ, split)
    T = table.shape[0]
    cls, prob, _ = isolate.recognize_table(classifier, ids, table, offsets, rows=T, min_voxels=min_voxels,
                                           window=window, batch_size=batch_size)
    table = table.clone()
    table[:, 1] = cls + 1
    more = _geometry_tables(ids, table, offsets, occ, access, dimensions, thresholds, contacts, limit2, d2=d2)
    feats = FeatureInstance.from_table(table, offsets, min_voxels, shape=tuple(occ.shape[1:]), tool=thresholds,
                                       thin=walls is not True, recognized=(cls, prob), split=cut, **more)
    if meshes is not None:
        _assign_faces(feats, ids, meshes, fit, margin, device, "recognize()")
    labels = None
    if return_labels:
        lut = torch.cat([table.new_zeros(1), table[:, 1]])                      # 0: no component
        row = torch.where(ids > 0, ids.to(torch.int64) + offsets[:-1].view(-1, 1, 1, 1), 0)
        labels = lut[row].to(torch.uint8).cpu().numpy()
    return feats, (ids.cpu().numpy() if return_ids else None), labels


@torch.no_grad()
def split_features(ids, occupancy=None, height=None, merge=1.0, device=None):
    """Touching features told apart by a watershed on the distance to the material -> ``(ids, features)``: ids
    int32 ``[N, D, H, W]`` and one list of :class:`FeatureInstance` per sample.

    ``ids`` is ``[N, D, H, W]`` of an integer dtype, as :func:`label_components`, :func:`extract_features`
    (``return_ids``) and :func:`recognize` give it: a voxel ``> 0`` belongs to the component of that number in
    its sample; every axis is at most 256.  Exactly one of ``occupancy`` (integers or bools of the ids' shape,
    non-zero: material; the height is then :func:`distance_transform` of it, squared distances) and ``height``
    (integers of the ids' shape, below 2^31; negative values count as 0) is given.  Inside each component every
    voxel climbs to its highest 26-neighbour until it reaches a peak; the voxels of one peak are a basin, two
    basins that touch are joined over their highest pass, and they become one feature when the lower of the two
    peaks rises less than ``merge`` voxels of clearance above that pass: ``sqrt(peak2) - sqrt(saddle2) <= merge /
    2``, decided in integers.  ``merge`` is a multiple of 0.5, ``>= 0``: 0 joins only what is equally high,
    larger values join more, and a height that is constant gives the components back.  The new ids number the
    features of a sample from 1; a record has ``cls = 1``, ``component`` (the id it was cut from) and ``peak2``.
    ``device`` defaults to the GPU when there is one (the ``watershed`` kernels), else the CPU reference path;
    the result is the same.
    """
    from .ops import edt, watershed
    from .utils.seginstances import FeatureInstance

    if (occupancy is None) == (height is None):
        raise ValueError("split_features(): give exactly one of occupancy and height")
    it = torch.as_tensor(np.asarray(ids)) if not isinstance(ids, torch.Tensor) else ids
    if it.is_floating_point() or it.is_complex() or it.dtype == torch.bool:
        raise ValueError(f"split_features(): ids must be integers, not {it.dtype}")
    if it.dim() != 4:
        raise ValueError(f"split_features(): ids must be [N, D, H, W], not {tuple(it.shape)}")
    if it.dtype != torch.int32 and it.numel() and int(it.max()) >= 1 << 31:
        raise ValueError("split_features(): ids must be below 2^31")
    watershed.merge_steps(merge)
    src = occupancy if height is None else height
    name = "occupancy" if height is None else "height"
    st = torch.as_tensor(np.asarray(src)) if not isinstance(src, torch.Tensor) else src
    if st.is_floating_point() or st.is_complex() or (height is not None and st.dtype == torch.bool):
        raise ValueError(f"split_features(): {name} must be integers{' or bools' if height is None else ''}, not "
                         f"{st.dtype}")
    if st.shape != it.shape:
        raise ValueError(f"split_features(): {name} is {tuple(st.shape)} but ids {tuple(it.shape)}")
    if height is not None and st.dtype != torch.int32 and st.numel() and int(st.max()) >= 1 << 31:
        raise ValueError("split_features(): height must be below 2^31")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    it = it.to(device).clamp(min=0).to(torch.int32).contiguous()
    if height is None:
        h = edt.distance_sq((st.to(device) != 0).to(torch.uint8))
    else:
        h = st.to(device).clamp(min=0).to(torch.int32).contiguous()
    out, table, offsets, comp, peak2 = watershed.split_instances(it, h, merge)
    return out.cpu().numpy(), FeatureInstance.from_table(table, offsets, split=(comp, peak2))


def _wall_limit(walls):
    """``limit2`` of the ``walls`` option: None when off, 0 for True (no thin count is reported),
    else ``wall_threshold`` of the thickness."""
    from .utils.seginstances import wall_threshold

    if walls is None or walls is False:
        return None
    return 0 if walls is True else wall_threshold(walls)


@torch.no_grad()
def nearest_instances(ids, device=None):
    """Labelled distance transform -> ``(d2, nearest)``, both int32 ``[N, 2, D, H, W]`` (or ``[2, D, H,
    W]`` for one ``[D, H, W]`` volume).  A voxel of ``ids`` (an integer array) with a value ``> 0``
    belongs to the instance of that number (up to ``2^31 - 1``); for every voxel ``nearest[:, 0]`` is
    the id of the nearest instance of its sample (the smallest among equally near ones) and ``d2[:,
    0]`` the squared distance to it, 0 and its own id on an instance's voxel; ``nearest[:, 1]`` and
    ``d2[:, 1]`` are the same for the nearest OTHER instance.  A missing one (no instance, or a single
    one, in the sample) is id 0 at :data:`EDT_INF`.  Each axis is at most 128 long.  ``device``
    defaults to the GPU when there is one (the ``nearest`` kernels), else the CPU reference path; the
    result is the same.
    """
    from .ops import nearest

    it = torch.as_tensor(np.asarray(ids)) if not isinstance(ids, torch.Tensor) else ids
    if it.is_floating_point() or it.is_complex() or it.dtype == torch.bool:
        raise ValueError(f"nearest_instances(): ids must be integers, not {it.dtype}")
    if it.dim() not in (3, 4):
        raise ValueError(f"nearest_instances(): ids must be [D, H, W] or [N, D, H, W], not {tuple(it.shape)}")
    if it.dtype != torch.int32 and it.numel() and int(it.max()) >= 1 << 31:
        raise ValueError("nearest_instances(): ids must be below 2^31")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    it = it.clamp(min=0).to(torch.int32).to(device)
    nn = nearest.nearest_labels(it if it.dim() == 4 else it[None])
    nn = (nn if it.dim() == 4 else nn[0]).cpu()
    return (nn >> 32).to(torch.int32).numpy(), (nn & 0xFFFFFFFF).to(torch.int32).numpy()


@torch.no_grad()
def tool_reach(voxels, device=None):
    """Directional clearance -> int32 ``[N, 6, D, H, W]`` (or ``[6, D, H, W]`` for one ``[D, H, W]``
    volume): for each face ``+z, -z, +x, -x, +y, -y`` of the grid (``+z`` the high-index end) the
    squared clearance of the largest ball whose centre can travel in a straight line from outside
    that face to the voxel -- the smallest :func:`distance_transform` value (``border=False``) on
    the way, the voxel included.  0 on material (non-zero ``voxels``), :data:`EDT_INF` in a sample
    without any.  Each axis is at most 256 long.  ``device`` defaults to the GPU when there is one
    (the ``edt`` and ``reach`` kernels), else the CPU reference path; the result is the same.
    """
    from .ops import edt, reach

    vt = torch.as_tensor(np.asarray(voxels)) if not isinstance(voxels, torch.Tensor) else voxels
    if vt.is_floating_point() or vt.is_complex():
        raise ValueError(f"tool_reach(): voxels must be integers or bools, not {vt.dtype}")
    if vt.dim() not in (3, 4):
        raise ValueError(f"tool_reach(): voxels must be [D, H, W] or [N, D, H, W], not {tuple(vt.shape)}")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    occ = (vt.to(device) != 0).to(torch.uint8)
    r6 = reach.reach_scan(edt.distance_sq(occ if vt.dim() == 4 else occ[None]))
    return (r6 if vt.dim() == 4 else r6[0]).cpu().numpy()


@torch.no_grad()
def distance_transform(volume, border: bool = False, device=None):
    """Exact squared Euclidean distance transform -> int32 ``[N, D, H, W]`` (or ``[D, H, W]`` for
    one ``[D, H, W]`` volume): the squared distance, in voxels, from every voxel to the nearest
    non-zero voxel of ``volume`` (an integer or bool array) of the same sample, 0 on those,
    :data:`EDT_INF` in a sample that has none.  With ``border`` the positions just outside the
    grid count as non-zero too.  Each axis is at most 256 long.  ``device`` defaults to the GPU
    when there is one (the ``edt`` kernels), else the CPU reference path; the result is the same.
    """
    from .ops import edt

    vt = torch.as_tensor(np.asarray(volume)) if not isinstance(volume, torch.Tensor) else volume
    if vt.is_floating_point() or vt.is_complex():
        raise ValueError(f"distance_transform(): volume must be integers or bools, not {vt.dtype}")
    if vt.dim() not in (3, 4):
        raise ValueError(f"distance_transform(): volume must be [D, H, W] or [N, D, H, W], not {tuple(vt.shape)}")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    seeds = (vt.to(device) != 0).to(torch.uint8)
    d2 = edt.distance_sq(seeds if vt.dim() == 4 else seeds[None], border=border)
    return (d2 if vt.dim() == 4 else d2[0]).cpu().numpy()


def _label_volumes(labels, what: str, name: str = "labels") -> torch.Tensor:
    lt = torch.as_tensor(np.asarray(labels)) if not isinstance(labels, torch.Tensor) else labels
    if lt.is_floating_point() or lt.dtype == torch.bool:
        raise ValueError(f"{what}: {name} must be integers, not {lt.dtype}")
    if lt.dim() != 4:
        raise ValueError(f"{what}: {name} must be [N, D, H, W], not {tuple(lt.shape)}")
    if lt.dtype != torch.uint8 and lt.numel() and not lt.is_cuda and (int(lt.min()) < 0 or int(lt.max()) > 255):
        raise ValueError(f"{what}: label values must lie in 0..255")
    return lt


@torch.no_grad()
def evaluate_features(model, x, y, batch_size: int = 32, device=None, packed_size: int | None = None,
                      background: int | None = 0, connectivity: int = 6, iou_threshold: float = 0.5,
                      min_voxels: int = 1):
    """Score a segmentation model feature by feature -> :class:`FeatureScore` (per class TP / FP /
    FN, precision, recall, F1, segmentation / recognition / panoptic quality, and the matches).

    ``model`` and ``x`` as for :func:`segment`, ``y`` as for :func:`evaluate_segmentation`;
    ``background`` and ``connectivity`` as for :func:`extract_features`.  Runs
    ``FeatureNet3DSeg.match``: the predicted labels and ``y`` are split into instances and the
    shared voxels of every pair are counted on the model's device; only the two instance tables
    and the overlap table cross to the host.  A predicted and a true instance of one class match
    when their IoU exceeds ``iou_threshold`` (0.5 <= threshold < 1: above one half a match is
    unique); instances of fewer than ``min_voxels`` voxels, on either side, count nowhere.  The
    per-class arrays reach up to the largest class that occurs, as :func:`match_features`' do.
    """
    from .utils.featscore import FeatureScore

    if isinstance(model, (str, Path)):
        model, _ = load(model, device)
    if not isinstance(model, FeatureNet3DSeg):
        raise ValueError(f"evaluate_features() takes a FeatureNet3DSeg model, not {type(model).__name__} "
                         "(see evaluate())")
    if connectivity not in (6, 26):
        raise ValueError(f"evaluate_features(): connectivity must be 6 or 26, not {connectivity!r}")
    dev = next(model.parameters()).device
    model.eval()
    from .training.data import unpack_voxels

    xt = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    yt = _label_volumes(y, "evaluate_features()")
    if len(yt) != len(xt):
        raise ValueError(f"evaluate_features(): {len(xt)} samples but {len(yt)} label volumes")
    scores = []
    for i in range(0, len(xt), batch_size):
        xb = xt[i:i + batch_size].to(dev)
        if packed_size is not None:
            xb = unpack_voxels(xb, packed_size)
        xb = xb.to(torch.bfloat16) if dev.type == "cuda" else xb.float()
        five = model.match(xb, yt[i:i + batch_size].to(dev).to(torch.uint8), background=background,
                           connectivity=connectivity)
        scores.append(FeatureScore.from_tables(*five, iou_threshold=iou_threshold, min_voxels=min_voxels))
    return FeatureScore.merge(scores)


@torch.no_grad()
def match_features(pred_labels, true_labels, background: int | None = 0, connectivity: int = 6,
                   iou_threshold: float = 0.5, min_voxels: int = 1, device=None):
    """:func:`evaluate_features` for label volumes the caller already has -> :class:`FeatureScore`.

    ``pred_labels`` and ``true_labels`` are ``[N, D, H, W]`` of one shape, any integer dtype with
    values 0..255.  ``device`` defaults to the GPU when there is one (the ``ccl`` and ``overlap``
    kernels), else the CPU reference path.
    """
    from .ops import overlap
    from .utils.featscore import FeatureScore

    pt = _label_volumes(pred_labels, "match_features()", "pred_labels")
    tt = _label_volumes(true_labels, "match_features()", "true_labels")
    if pt.shape != tt.shape:
        raise ValueError(f"match_features(): predicted labels are {tuple(pt.shape)} but true labels {tuple(tt.shape)}")
    if connectivity not in (6, 26):
        raise ValueError(f"match_features(): connectivity must be 6 or 26, not {connectivity!r}")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    five = overlap.instance_overlap(pt.to(device).to(torch.uint8), tt.to(device).to(torch.uint8), background,
                                    connectivity)
    return FeatureScore.from_tables(*five, iou_threshold=iou_threshold, min_voxels=min_voxels)


def generate_parts(n: int, size: int = 64, seed: int = 0, features=(1, 4), separate: bool = True, device=None,
                   return_slots: bool = False):
    """``n`` procedural machining parts with per-voxel truth -> ``(voxels, labels, parts)`` or
    ``(voxels, labels, parts, slots)``.

    A part is a solid ``size``^3 stock block with ``features = (lo, hi)`` subtractive features of
    the 24 classes, each entering from one of the six faces.  ``voxels`` uint8 ``[n, S, S, S]`` is
    the occupancy, ``labels`` uint8 ``[n, S, S, S]`` is 0 where nothing was removed and 1 + class
    where a feature of that class removed the voxel, ``parts`` holds one list of
    :class:`~featurenet_amd.utils.partfeatures.PartFeature` per part, and ``slots`` (uint8) names
    the removing feature as 1 + its ``slot``.  With ``separate`` the features' bounding boxes keep
    a voxel apart, so every feature is its own connected component of ``labels``; without it
    features may overlap and the one in the lowest slot owns the shared voxels.  Deterministic per
    ``(seed, part index)`` and the same on every device: ``device`` (default: the GPU when there
    is one) only chooses between the ``partgen_carve`` kernel and the host path.
    """
    from .ops import partgen
    from .utils.partfeatures import from_params

    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    tab = partgen.sample(n, size, seed, features, separate=separate)
    out = partgen.carve(tab, size, device=device, want_slots=return_slots)
    arrays = [t.cpu().numpy() for t in out]
    return (arrays[0], arrays[1], from_params(tab), *arrays[2:])


def _mesh_triangles(mesh) -> np.ndarray:
    """One mesh of :func:`voxelize` -> float64 ``[F, 3, 3]``."""
    if isinstance(mesh, (str, Path)):
        from . import _native

        return _native.runtime().read_stl(str(mesh)).astype(np.float64)
    if isinstance(mesh, tuple) and len(mesh) == 2:
        vertices, faces = np.asarray(mesh[0], dtype=np.float64), np.asarray(mesh[1])
        if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3 \
                or faces.dtype.kind not in "iu":
            raise ValueError(f"voxelize(): a (vertices, faces) pair is float [V, 3] and integer [F, 3], not "
                             f"{vertices.shape} and {faces.dtype} {faces.shape}")
        if faces.size and (faces.min() < 0 or faces.max() >= len(vertices)):
            raise ValueError(f"voxelize(): a face names a vertex outside 0..{len(vertices) - 1}")
        return vertices[faces]
    tris = np.asarray(mesh.cpu() if isinstance(mesh, torch.Tensor) else mesh, dtype=np.float64)
    if tris.ndim != 3 or tris.shape[1:] != (3, 3):
        raise ValueError(f"voxelize(): a mesh is an STL path, a (vertices, faces) pair or an [F, 3, 3] array, not an "
                         f"array of shape {tris.shape}")
    return tris


def _mesh_lattice(meshes, size: int, fit, margin):
    """The ``meshes`` of :func:`voxelize` on the lattice of a ``size``^3 grid -> ``(single, tris int32
    [T, 9], offsets int32 [N + 1], origins, voxel sizes)``; ``single``: one mesh was given, not a list."""
    from .ops import voxelize as vx

    single = isinstance(meshes, (str, Path, np.ndarray, torch.Tensor)) or \
        (isinstance(meshes, tuple) and len(meshes) == 2 and not isinstance(meshes[0], (str, Path, tuple)))
    if single and isinstance(meshes, (np.ndarray, torch.Tensor)) and meshes.ndim == 4:
        single, meshes = False, list(meshes)             # [N, F, 3, 3]: N meshes of F triangles
    lattice, origins, sizes = [], [], []
    for mesh in ([meshes] if single else list(meshes)):
        q, origin, voxel_size = vx.quantize(_mesh_triangles(mesh), size, fit, margin)
        lattice.append(q.reshape(-1, 9))
        origins.append(origin)
        sizes.append(voxel_size)
    counts = [len(q) for q in lattice]
    tris = torch.from_numpy(np.concatenate(lattice) if lattice else np.zeros((0, 9), np.int32))
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    return single, tris, offsets, origins, sizes


def voxelize(meshes, size: int = 64, fit="bbox", margin: float = 0, device=None, packed: bool = False,
             return_info: bool = False):
    """Triangle meshes -> occupancy uint8 ``[N, S, S, S]`` (1 = material, indexed ``[n, z, y, x]``),
    or with ``packed`` its bits, uint8 ``[N, S^3 / 8]``: the input of :func:`classify`,
    :func:`segment` and :func:`extract_features` from a CAD part's STL file.

    ``meshes`` is an STL path, a ``(vertices [V, 3], faces [F, 3])`` pair, an ``[F, 3, 3]`` array
    of triangles, or a list of those.  Each mesh is placed on the grid by ``fit``: ``"bbox"``
    scales it so that the longest side of its bounding box spans the grid less ``margin`` voxels
    at either end and centres the other axes; ``(origin, voxel_size)`` puts voxel ``(x, y, z)`` at
    ``origin + voxel_size * (x, y, z)``.  Vertices are snapped to a lattice of 1/16 voxel on the
    host; from there on everything is integer arithmetic -- a voxel is material when a ray along
    +x has crossed the surface an odd number of times before its centre, with a tie rule that
    keeps closed meshes closed -- so the result is the same on every device: ``device`` (default:
    the GPU when there is one) only chooses between the ``voxelize_tris`` kernel and the host path.

    ``return_info`` adds a dict: ``leaks`` int64 ``[N]``, the columns of each mesh whose ray leaves
    the grid inside the part (0 for a watertight mesh), and ``origin`` float64 ``[N, 3]`` and
    ``voxel_size`` float64 ``[N]``, the transforms used (what a binvox header holds).
    """
    from .ops import voxelize as vx

    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    _, tris, offsets, origins, sizes = _mesh_lattice(meshes, size, fit, margin)
    vox, leaks = vx.voxelize(tris, offsets, size, device=device, packed=packed)
    vox = vox.cpu().numpy()
    if not return_info:
        return vox
    return vox, {"leaks": leaks.cpu().numpy(), "origin": np.asarray(origins, np.float64).reshape(-1, 3),
                 "voxel_size": np.asarray(sizes, np.float64)}


def label_mesh(meshes, volume, fit="bbox", margin: float = 0, device=None, return_votes: bool = False):
    """Which value of a voxel volume lies against each triangle of the mesh the volume was made
    from -> one int32 ``[F_i]`` array of winners per mesh (the array itself for a single mesh): the
    way from instance ids or labels on the grid back to the faces of the CAD model.

    ``meshes`` as for :func:`voxelize`; ``volume`` is ``[N, S, S, S]`` or, for one mesh, ``[S, S,
    S]``: the ``ids`` of :func:`extract_features` / :func:`recognize` / :func:`label_components`
    (any integer dtype that fits int32) or uint8 labels of :func:`segment`, 0 = nothing.  The meshes
    are placed by the same ``quantize`` call as in :func:`voxelize`, so the same ``fit`` and
    ``margin`` -- or ``fit=(origin, voxel_size)`` from its ``return_info`` -- land the triangles on
    the voxels they made.  Each triangle is looked at along the dominant axis of its normal: in
    every voxel column whose centre it covers, the voxel just before the surface and the one just
    behind it vote with their value; a triangle too small to cover a column centre votes once at
    its centroid.  The value with the most votes wins, the lowest on a tie, 0 with none: winding
    and vertex order do not matter, and material (0 in an id volume) does not vote.  Integer
    arithmetic on the lattice, the same on every device: ``device`` (default: the GPU when there
    is one) chooses between the ``mesh_votes`` kernel and the host path.

    ``return_votes`` adds, per mesh, the int32 ``[F_i, 3]`` rows ``winner, votes, covered``
    (``covered``: the columns the triangle covers; 0: it voted at its centroid)."""
    from .ops import meshlabel

    vt = torch.as_tensor(np.asarray(volume)) if not isinstance(volume, torch.Tensor) else volume
    if vt.is_floating_point() or vt.is_complex() or vt.dtype == torch.bool:
        raise ValueError(f"label_mesh(): volume must be integers, not {vt.dtype}")
    if vt.dim() == 3:
        vt = vt.unsqueeze(0)
    if vt.dim() != 4 or len(set(vt.shape[1:])) != 1:
        raise ValueError(f"label_mesh(): volume must be [N, S, S, S] or [S, S, S], not {tuple(vt.shape)}")
    if vt.dtype not in (torch.uint8, torch.int32):
        if vt.numel() and (int(vt.min()) < -2 ** 31 or int(vt.max()) >= 2 ** 31):
            raise ValueError("label_mesh(): the values of volume must fit int32")
        vt = vt.to(torch.int32)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    single, tris, offsets, _, _ = _mesh_lattice(meshes, int(vt.shape[1]), fit, margin)
    if offsets.numel() - 1 != vt.shape[0]:
        raise ValueError(f"label_mesh(): {offsets.numel() - 1} meshes but {vt.shape[0]} volumes")
    rows = meshlabel.mesh_votes(tris, offsets, vt, device=device).cpu().numpy()
    rows = [rows[a:b] for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]
    winners = [np.ascontiguousarray(r[:, 0]) for r in rows]
    if single:
        return (winners[0], rows[0]) if return_votes else winners[0]
    return (winners, rows) if return_votes else winners


def _assign_faces(feats, ids, meshes, fit, margin, device, what: str) -> None:
    """The ``meshes=`` option of :func:`extract_features` and :func:`recognize`: ``FeatureInstance.faces``
    from :func:`label_mesh` of the meshes against ``ids`` (a tensor, every sample of the call)."""
    from .utils.seginstances import assign_faces

    winners = label_mesh(meshes, ids, fit=fit, margin=margin, device=device)
    if isinstance(winners, np.ndarray):
        winners = [winners]
    if len(winners) != len(feats):
        raise ValueError(f"{what}: {len(winners)} meshes but {len(feats)} samples")
    assign_faces(feats, winners)


def evaluate(model, x, y, batch_size: int = 256, packed_size: int | None = None) -> float:
    labels, _ = classify(model, x, batch_size, packed_size=packed_size)
    return float((labels == np.asarray(y)).mean())


def search(**kwargs):
    """Run the mutation-driven NAS (reference ``FullEvolution.run``); see
    :func:`featurenet_amd.search.evolution.run_evolution` for arguments."""
    from .search.evolution import run_evolution

    return run_evolution(**kwargs)
