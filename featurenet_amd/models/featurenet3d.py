"""FeatureNet-3D: the voxel machining-feature classifier (north-star workload).

Architecture (Zhang, Jaiswal & Rai, "FeatureNet: Machining feature
recognition based on 3D Convolution Neural Network", CAD 2018 -- recalled, not
present in the reference repository):

    64^3 x 1 occupancy grid
    Conv3d 32 @ 7^3, stride 2   -> 29^3   (BN + ReLU)
    Conv3d 32 @ 5^3             -> 25^3   (BN + ReLU)
    Conv3d 64 @ 4^3             -> 22^3   (BN + ReLU)
    Conv3d 64 @ 3^3             -> 20^3   (BN + ReLU + MaxPool3d 2^3 -> 10^3, fused)
    Dense 128 (ReLU)
    Dense 24 (softmax, fused into the loss)

All four convolutions run on the implicit-GEMM MFMA kernels; BN statistics
come out of the conv epilogue; conv4's BN+ReLU is applied inside the
MaxPool3d kernel.  The same class builds the tiny "16^3, 2-class" CPU
reference configuration and the per-voxel segmentation variant
(:class:`FeatureNet3DSeg`).
"""
from __future__ import annotations

from dataclasses import asdict, dataclass

import torch
from torch import nn

from .. import ops
from ..ops import bn as bn_ops
from ..ops import subpixel
from ..ops.elementwise import upsample2x
from .layers import Conv, Dense


@dataclass
class FeatureNet3DConfig:
    input_size: int = 64
    in_channels: int = 1
    num_classes: int = 24
    widths: tuple = (32, 32, 64, 64)
    kernels: tuple = (7, 5, 4, 3)
    strides: tuple = (2, 1, 1, 1)
    pool: int = 2
    fc: int = 128
    bn: bool = True
    init: str = "he"

    def to_dict(self) -> dict:
        d = asdict(self)
        return {k: list(v) if isinstance(v, tuple) else v for k, v in d.items()}

    @staticmethod
    def from_dict(d: dict) -> "FeatureNet3DConfig":
        d = dict(d)
        for k in ("widths", "kernels", "strides"):
            if k in d:
                d[k] = tuple(d[k])
        return FeatureNet3DConfig(**d)

    @staticmethod
    def tiny() -> "FeatureNet3DConfig":
        """16^3-voxel 2-class tiny 3D-CNN (BASELINE.json config 1, CPU plumbing)."""
        return FeatureNet3DConfig(input_size=16, num_classes=2, widths=(8, 8, 16, 16), kernels=(3, 3, 3, 3),
                                  strides=(1, 1, 1, 1), pool=2, fc=32)


def _feature_shape(cfg: FeatureNet3DConfig) -> tuple[int, int]:
    s = cfg.input_size
    for k, st in zip(cfg.kernels, cfg.strides):
        s = (s - k) // st + 1
    s = s // cfg.pool
    if s <= 0:
        raise ValueError(f"FeatureNet-3D config collapses the {cfg.input_size}^3 input to nothing")
    return s, cfg.widths[-1]


class FeatureNet3D(nn.Module):
    def __init__(self, cfg: FeatureNet3DConfig | None = None):
        super().__init__()
        self.cfg = cfg = cfg or FeatureNet3DConfig()
        convs = []
        cin = cfg.in_channels
        n = len(cfg.widths)
        for i, (w, k, s) in enumerate(zip(cfg.widths, cfg.kernels, cfg.strides)):
            last = i == n - 1
            convs.append(Conv(cin, w, (k, k, k), (s, s, s), "valid", bn=cfg.bn, act="relu",
                              pool=(cfg.pool,) * 3 if last and cfg.pool > 1 else None, init=cfg.init))
            cin = w
        self.convs = nn.ModuleList(convs)
        sp, c = _feature_shape(cfg)
        self.flat_features = sp ** 3 * c
        self.fc1 = Dense(self.flat_features, cfg.fc, act="relu", init=cfg.init)
        self.fc2 = Dense(cfg.fc, cfg.num_classes, act=None)

    def features(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4:  # [N, D, H, W] occupancy -> add channel axis
            x = x.unsqueeze(-1)
        for c in self.convs:
            x = c(x)
        return x

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [N, S, S, S, 1] (or [N, S, S, S]) -> fp32 logits [N, num_classes]."""
        # (no packs.pack_scope here: the three tile-stream packs in one launch measured neutral on
        # this step -- 4.633 vs 4.632 ms -- and the seg step slower, 19.05 vs 18.91 ms; NAS
        # candidates, with one 3-5 us pack per conv and direction, gain 2.5 %)
        f = self.features(x)
        f = f.reshape(f.shape[0], -1)
        h = self.fc1(f)
        return self.fc2(h, out_fp32=True)

    def train_flops_per_sample(self) -> int:
        """Analytic FLOPs of one training sample (fwd + dgrad + wgrad)."""
        cfg = self.cfg
        shape = (1, cfg.input_size, cfg.input_size, cfg.input_size, cfg.in_channels)
        fwd = 0
        bwd = 0
        for i, c in enumerate(self.convs):
            cs, ps = c.specs(shape)
            f = cs.flops()
            fwd += f
            bwd += f * (2 if i > 0 else 1)  # conv1 needs no dgrad (input has no grad)
            shape = ps.out_shape5 if ps is not None else cs.out_shape5
        fc = 2 * (self.flat_features * cfg.fc + cfg.fc * cfg.num_classes)
        return fwd + bwd + 3 * fc


class FeatureNet3DSeg(nn.Module):
    """Per-voxel multi-feature segmentation head (BASELINE.json config 4).

    Encoder = FeatureNet-3D convs with ``same`` padding (spatial size kept
    except for the stride-2 stem), decoder = nearest 2x upsample + 3^3 conv
    back to the input grid, 1x1x1 classifier producing per-voxel logits
    ``[N, S, S, S, num_classes]``.
    """

    def __init__(self, input_size: int = 64, in_channels: int = 1, num_classes: int = 25, widths=(32, 32, 64, 64)):
        super().__init__()
        self.input_size, self.num_classes = input_size, num_classes
        w0, w1, w2, w3 = widths
        self.enc = nn.ModuleList([
            Conv(in_channels, w0, (7, 7, 7), (2, 2, 2), "same", bn=True, act="relu", init="he"),
            Conv(w0, w1, (5, 5, 5), 1, "same", bn=True, act="relu", init="he"),
            Conv(w1, w2, (4, 4, 4), 1, "same", bn=True, act="relu", init="he"),
            Conv(w2, w3, (3, 3, 3), 1, "same", bn=True, act="relu", init="he"),
        ])
        self.dec = Conv(w3, w1, (3, 3, 3), 1, "same", bn=True, act="relu", init="he")
        self.head = Conv(w1, num_classes, (1, 1, 1), 1, "valid", bn=False, act=None, bias=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4:
            x = x.unsqueeze(-1)
        for c in self.enc:
            x = c(x)
        return self._decode(x)

    def _decode(self, x: torch.Tensor) -> torch.Tensor:
        d, h = self.dec, self.head
        if self.training and subpixel.gpu_ok(x, d.cout, x.shape[-1]) and \
                bn_ops.fused_pointwise_ok(x, d.cout, h.cout, d.act):
            # training on the GPU: upsample + decoder conv as 8 parity-class 2^3 convs (3.4x
            # fewer FLOPs, the 2x-upsampled tensor never exists), the BN + ReLU inside the 1x1
            # head's kernels, backward through the shifted space-to-depth dy (ops/subpixel.py)
            return subpixel.decoder_head(x, d.weight, d.gamma, d.beta, d.running_mean, d.running_var, h.weight,
                                         h.bias, d.bn_momentum, d.bn_eps, d.act)
        x = upsample2x(x)                  # nearest x2 upsample on the channels-last grid
        if self.training and bn_ops.fused_pointwise_ok(x, d.cout, h.cout, d.act):
            # training on the GPU: the decoder's BN + ReLU run inside the 1x1 head's pointwise
            # kernels (forward and weight gradient), so its 64^3 x 32 output is never written
            cs, _ = d.specs(tuple(x.shape))
            y, slab = ops.conv(x, d.weight, None, cs, None, want_stats=True)
            return bn_ops.batchnorm_act_pointwise(y, d.gamma, d.beta, d.running_mean, d.running_var, h.weight, h.bias,
                                                  d.bn_momentum, d.bn_eps, d.act, stats_slab=slab)
        return h(d(x))  # [N, S, S, S, classes]

    def _head_operands(self, x: torch.Tensor):
        """Eval-mode trunk shared by :meth:`predict` and :meth:`score` -> ``(y, w2, pro, native)``:
        the 1x1 head's input ``y [N, S, S, S, C]``, its weight as ``[classes, C]``, the input
        prologue ``(scale, shift, act)`` or None, and whether the native head kernels run.  On the
        GPU the decoder is the sub-pixel one (8 parity-class 2^3 convs, its folded BN + activation
        left to the head's prologue) where :func:`subpixel.infer_ok`, else the 27-tap layer; on
        the CPU the reference layer."""
        from .. import _native
        from ..ops.conv import pw_prologue_ok
        from ..ops.spec import act_code

        if x.dim() == 4:
            x = x.unsqueeze(-1)
        z = x
        for c in self.enc:
            z = c(z)
        d, h = self.dec, self.head
        w2 = h.weight.reshape(h.cout, d.cout)
        if not _native.use_native(z):
            return d(upsample2x(z)), w2, None, False
        if subpixel.infer_ok(z, d.cout, z.shape[-1]) and pw_prologue_ok(d.cout):
            y, _ = subpixel.upconv_forward(z.to(torch.bfloat16).contiguous(), d.weight)   # (BN slab: unused)
            scale = (d.gamma * torch.rsqrt(d.running_var + d.bn_eps)).float()
            shift = (d.beta - d.running_mean * scale).float()
            return y, w2, (scale.contiguous(), shift.contiguous(), act_code(d.act)), True
        return d(upsample2x(z)), w2, None, True

    @torch.no_grad()
    def predict(self, x: torch.Tensor, want_conf: bool = False):
        """Per-voxel labels ``uint8 [N, S, S, S]`` (and, with ``want_conf``, the top-1 softmax
        probability ``[N, S, S, S]``) of a model in eval mode, without the logits: on the GPU the
        1x1 head runs in the fused head + arg-max kernel (``ops.conv.pw_argmax``) -- behind the
        sub-pixel decoder (8 parity-class 2^3 convs, the folded BN + activation as the head's input
        prologue) where :func:`subpixel.infer_ok`, else behind the 27-tap decoder layer; on the
        CPU ``reference.head_argmax``.  Ties go to the lowest class index."""
        from ..ops import reference
        from ..ops.conv import pw_argmax

        if self.training:
            raise RuntimeError("FeatureNet3DSeg.predict is inference only: call model.eval() first")
        y, w2, pro, native = self._head_operands(x)
        if not native:
            labels, conf = reference.head_argmax(y, w2, self.head.bias)
        else:
            labels, conf = pw_argmax(y.reshape(-1, y.shape[-1]), w2, self.head.bias, pro=pro, want_conf=want_conf)
        labels = labels.reshape(y.shape[:-1])
        return (labels, conf.reshape(y.shape[:-1])) if want_conf else labels

    @torch.no_grad()
    def score(self, x: torch.Tensor, y: torch.Tensor, ignore_index: int | None = None,
              acc: torch.Tensor | None = None, want_labels: bool = False):
        """Confusion counts of :meth:`predict`'s labels against the true labels ``y [N, S, S, S]``
        (any integer dtype, values 0..255) of a model in eval mode -> ``(acc, labels or None)``:
        ``acc`` int64 ``[C*C + 1]`` on the model's device, ``acc[t*C + p]`` = voxels with truth
        ``t`` labelled ``p``, ``acc[C*C]`` = voxels whose truth is ``>= C``; voxels with
        ``y == ignore_index`` are counted nowhere.  ``acc`` is added to when given (sum over
        batches on the device, copy once).  Same decoder dispatch as :meth:`predict`; on the GPU
        the head counts in its own kernel (``ops.conv.pw_argmax_score``) and writes nothing per
        voxel unless ``want_labels``."""
        from ..ops import reference
        from ..ops.conv import pw_argmax_score

        if self.training:
            raise RuntimeError("FeatureNet3DSeg.score is inference only: call model.eval() first")
        if y.is_floating_point() or y.dtype == torch.bool:
            raise ValueError(f"score: labels must be an integer tensor, not {y.dtype}")
        yv, w2, pro, native = self._head_operands(x)
        if y.numel() != yv.numel() // yv.shape[-1]:
            raise ValueError(f"score: labels {tuple(y.shape)} do not match the output grid {tuple(yv.shape[:-1])}")
        if y.dtype != torch.uint8:
            if not y.is_cuda and y.numel() and (int(y.min()) < 0 or int(y.max()) > 255):
                raise ValueError("score: label values must lie in 0..255")
            y = y.to(yv.device).to(torch.uint8)
        y = y.to(yv.device)
        C = self.head.cout
        if not native:
            labels, _ = reference.head_argmax(yv, w2, self.head.bias)
            cm = reference.confusion(y, labels, C, ignore_index)
            acc = cm if acc is None else acc.add_(cm)
            labels = labels if want_labels else None
        else:
            acc, labels = pw_argmax_score(yv.reshape(-1, yv.shape[-1]), w2, self.head.bias, y, pro=pro,
                                          ignore_index=ignore_index, acc=acc, want_labels=want_labels)
        return acc, (labels.reshape(yv.shape[:-1]) if labels is not None else None)

    @torch.no_grad()
    def instances(self, x: torch.Tensor, background: int | None = 0, connectivity: int = 6,
                  want_ids: bool = False, want_access: bool = False, want_dims: bool = False,
                  want_reach: tuple | None = None, want_contacts: bool = False, want_walls: int | None = None):
        """The features in each sample: :meth:`predict`'s labels split into connected components
        -> ``(table, offsets, ids or None)`` on the model's device.  ``table`` int64 ``[T, 13]``
        has one row per component (``sample, class, voxels, root, z0, y0, x0, z1, y1, x1, sum_z,
        sum_y, sum_x``, sorted by sample and first voxel), sample ``n`` owns rows
        ``offsets[n]:offsets[n + 1]``, ``ids`` int32 ``[N, S, S, S]`` numbers each sample's
        components from 1 (``ops.ccl``).  Voxels of class ``background`` (None: no such class)
        belong to no component; ``connectivity`` is 6 or 26.  The labels never leave the device.

        With ``want_access`` -> ``(table, offsets, ids or None, acc)``: ``acc`` int64 ``[T, 8]``
        counts, row by row of ``table``, the component's voxels that are open toward the faces
        ``+z, -z, +x, -x, +y, -y`` of the grid (no material, ``x != 0``, lies beyond the voxel on
        that side), toward none, and all of them (``ops.access``).

        With ``want_dims`` ``dim`` int64 ``[T, 4]`` is appended (after ``acc`` when that is there):
        row by row of ``table`` the largest squared distance from one of the component's voxels
        to the material, the smallest index ``(z * S + y) * S + x`` of a voxel that attains it,
        the component's voxels with a material face neighbour, and all of them (``ops.edt``).

        With ``want_reach = (need2, cut2)``, a tool (``utils.seginstances.tool_thresholds``),
        ``reach`` int64 ``[T, 15]`` is appended (after ``acc`` and ``dim``): row by row of ``table``
        the largest squared clearance of a straight path from each face to one of the component's
        voxels, the voxels the tool's centre reaches from each face and from none, the voxels the
        tool clears, and all of them (``ops.reach``).  It shares the distance transform of
        ``want_dims``.

        With ``want_contacts`` ``contact`` int64 ``[T, 19]`` and ``adj`` int64 ``[P, 4]`` are appended
        (after ``acc``, ``dim`` and ``reach``): row by row of ``table`` the voxel faces toward each
        side that meet material (``x != 0``), free space or the outside of the grid, and another
        component, and the voxels; and one row ``(row_a, row_b, face, faces)`` per pair of components
        ``row_a < row_b`` and side of ``a`` on which they share faces (``ops.contact``).

        With ``want_walls = limit2`` (None: off) ``wall`` int64 ``[T, 5]`` is appended after
        everything else: row by row of ``table`` the smallest squared distance from one of the
        component's voxels to a voxel of another component of the sample, the smallest index of a
        voxel that attains it, the row of that other component (each ``-1`` where the sample has no
        other), the component's voxels that have another component within the squared distance
        ``limit2`` (``utils.seginstances.wall_threshold``), and all of them (``ops.nearest``).  It
        needs no occupancy."""
        from ..ops import access, ccl, contact, edt, nearest, reach

        if connectivity not in (6, 26):
            raise ValueError(f"instances: connectivity must be 6 or 26, not {connectivity!r}")
        labels = self.predict(x)
        roots, flags = ccl.connected_components(labels, background, connectivity, return_flags=True)
        more = want_access or want_dims or want_reach is not None or want_contacts
        walls = want_walls is not None
        ids, table, offsets = ccl.instance_table(labels, roots, want_ids=want_ids or more or walls, flags=flags)
        if not more and not walls:
            return table, offsets, ids
        out = [table, offsets, ids if want_ids else None]
        if more:
            occ = (x != 0).to(device=labels.device, dtype=torch.uint8)
            if occ.dim() == 5:                   # [N, S, S, S, C]: material in any channel
                occ = occ.amax(-1)
            occ = occ.reshape(labels.shape)
        if want_access:
            out.append(access.access_table(ids, offsets, occ, rows=table.shape[0])[0])
        d2 = None
        if want_dims:
            dim, d2 = edt.dimension_table(ids, offsets, occ, rows=table.shape[0], want_d2=want_reach is not None)
            out.append(dim)
        if want_reach is not None:
            need2, cut2 = want_reach
            out.append(reach.reach_table(ids, offsets, occ, need2, cut2, rows=table.shape[0], d2=d2)[0])
        if want_contacts:
            out.extend(contact.contact_table(ids, offsets, occ, rows=table.shape[0]))
        if walls:
            out.append(nearest.wall_table(ids, offsets, want_walls, rows=table.shape[0])[0])
        return tuple(out)

    def match(self, x: torch.Tensor, y: torch.Tensor, background: int | None = 0, connectivity: int = 6):
        """The predicted features against the true ones: the instances of :meth:`predict`'s labels,
        the instances of ``y`` (true labels, uint8 ``[N, S, S, S]`` on the model's device) and the
        overlap table of the two -> ``(table_pred, off_pred, table_true, off_true, pairs)`` on the
        model's device.  Tables and offsets as :meth:`instances` gives them; ``pairs`` int64 ``[P,
        3]`` has one row ``(row_pred, row_true, shared voxels)`` per pair of instances that touch
        (``ops.overlap``).  ``utils.featscore`` turns the five into matches and a score.  No
        per-voxel tensor leaves the device."""
        from ..ops import overlap

        if connectivity not in (6, 26):
            raise ValueError(f"match: connectivity must be 6 or 26, not {connectivity!r}")
        labels = self.predict(x)
        if not isinstance(y, torch.Tensor) or y.dtype != torch.uint8 or y.shape != labels.shape \
                or y.device != labels.device:
            got = f"{y.dtype} {tuple(y.shape)} on {y.device}" if isinstance(y, torch.Tensor) else type(y).__name__
            raise ValueError(f"match: y must be uint8 {tuple(labels.shape)} on {labels.device}, not {got}")
        return overlap.instance_overlap(labels, y, background, connectivity)

    def loss(self, x: torch.Tensor, labels: torch.Tensor, smoothing: float = 0.0, with_correct: bool = False):
        """Mean per-voxel softmax cross-entropy against ``labels`` [N, S, S, S] (+ the number of
        top-1 hits when ``with_correct``).  Training on the GPU's sub-pixel path computes the loss
        in the 1x1 head's epilogue (``subpixel.decoder_head_xent``: the logits are never stored);
        otherwise ``softmax_xent(self(x), labels)``."""
        from ..ops import softmax_xent

        if x.dim() == 4:
            x = x.unsqueeze(-1)
        d, h = self.dec, self.head
        if self.training:
            z = x
            for c in self.enc:
                z = c(z)
            if subpixel.gpu_ok(z, d.cout, z.shape[-1]) and bn_ops.fused_pointwise_ok(z, d.cout, h.cout, d.act) \
                    and subpixel.xent_ok(d.cout, h.cout):
                loss, hits = subpixel.decoder_head_xent(z, d.weight, d.gamma, d.beta, d.running_mean, d.running_var,
                                                        h.weight, h.bias, labels, d.bn_momentum, d.bn_eps, d.act,
                                                        smoothing, want_hits=with_correct)
                return (loss, hits) if with_correct else loss
            return softmax_xent(self._decode(z), labels, smoothing, with_correct)
        return softmax_xent(self(x), labels, smoothing, with_correct)
