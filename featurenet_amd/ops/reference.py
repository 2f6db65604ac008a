"""PyTorch reference implementations (the numerical oracle / CPU path).

Every native op in :mod:`featurenet_amd.ops` has a reference twin here with
the same channels-last calling convention.  CPU tensors run these directly
(BASELINE.json config 1: the CPU reference path); the kernel tests compare
the HIP kernels against them in fp32.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .spec import ConvSpec, PoolSpec


def to_ncdhw(x5: torch.Tensor) -> torch.Tensor:
    return x5.permute(0, 4, 1, 2, 3)


def to_ndhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 4, 1)


def activation(x: torch.Tensor, act) -> torch.Tensor:
    if act in (None, "none", "linear"):
        return x
    if act == "relu":
        return F.relu(x)
    if act == "tanh":
        return torch.tanh(x)
    if act == "sigmoid":
        return torch.sigmoid(x)
    if act == "softmax":
        return torch.softmax(x, dim=-1)
    raise ValueError(f"unknown activation {act!r}")


def conv(x5: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None, spec: ConvSpec, act=None) -> torch.Tensor:
    """x5 [N,D,H,W,C], w [K,KD,KH,KW,C] -> [N,OD,OH,OW,K]."""
    xin = to_ncdhw(x5)
    hd, hh, hw = spec.pads_hi
    if spec.pd or spec.ph or spec.pw or hd or hh or hw:
        xin = F.pad(xin, (spec.pw, hw, spec.ph, hh, spec.pd, hd))
    y = F.conv3d(xin, w.permute(0, 4, 1, 2, 3), b, stride=(spec.sd, spec.sh, spec.sw),
                 dilation=(spec.dd, spec.dh, spec.dw))
    y = y[:, :, : spec.OD, : spec.OH, : spec.OW]
    return activation(to_ndhwc(y), act)


def depthwise_conv(x5: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None, spec: ConvSpec, mult: int = 1,
                   act=None) -> torch.Tensor:
    """Depthwise: w [C*mult, KD, KH, KW, 1]."""
    xin = to_ncdhw(x5)
    hd, hh, hw = spec.pads_hi
    xin = F.pad(xin, (spec.pw, hw, spec.ph, hh, spec.pd, hd))
    y = F.conv3d(xin, w.permute(0, 4, 1, 2, 3), b, stride=(spec.sd, spec.sh, spec.sw),
                 dilation=(spec.dd, spec.dh, spec.dw), groups=spec.C)
    y = y[:, :, : spec.OD, : spec.OH, : spec.OW]
    return activation(to_ndhwc(y), act)


def batchnorm_act(y5: torch.Tensor, gamma, beta, running_mean, running_var, training: bool, momentum: float,
                  eps: float, act=None) -> torch.Tensor:
    C = y5.shape[-1]
    flat = y5.reshape(-1, C)
    z = F.batch_norm(flat, running_mean, running_var, gamma, beta, training, momentum, eps)
    return activation(z, act).reshape(y5.shape)


def pool(x5: torch.Tensor, spec: PoolSpec, kind: str = "max", count_pad: bool = False) -> torch.Tensor:
    xin = to_ncdhw(x5)
    k = (spec.KD, spec.KH, spec.KW)
    s = (spec.sd, spec.sh, spec.sw)
    hd = max((spec.OD - 1) * spec.sd + spec.KD - spec.D - spec.pd, 0)
    hh = max((spec.OH - 1) * spec.sh + spec.KH - spec.H - spec.ph, 0)
    hw = max((spec.OW - 1) * spec.sw + spec.KW - spec.W - spec.pw, 0)
    pads = (spec.pw, hw, spec.ph, hh, spec.pd, hd)
    if kind == "max":
        if any(pads):
            xin = F.pad(xin, pads, value=float("-inf"))
        y = F.max_pool3d(xin, k, s)
    else:
        if any(pads):
            ones = torch.ones_like(xin[:, :1])
            num = F.avg_pool3d(F.pad(xin, pads), k, s, divisor_override=1)
            if count_pad:
                den = torch.full_like(num[:, :1], float(spec.KD * spec.KH * spec.KW))
            else:
                den = F.avg_pool3d(F.pad(ones, pads), k, s, divisor_override=1)
            y = num / den
        else:
            y = F.avg_pool3d(xin, k, s)
    y = y[:, :, : spec.OD, : spec.OH, : spec.OW]
    return to_ndhwc(y)


def softmax_xent(logits: torch.Tensor, labels: torch.Tensor, smoothing: float = 0.0) -> torch.Tensor:
    lg = logits if logits.dtype == torch.float64 else logits.float()   # >= fp32 (fp64 kept for gradcheck)
    return F.cross_entropy(lg, labels, label_smoothing=smoothing)


def lowest_argmax(logits: torch.Tensor) -> torch.Tensor:
    """uint8 arg-max over the last axis, ties to the lowest index (``torch.argmax`` leaves the
    choice among equal maxima open)."""
    n = logits.shape[-1]
    idx = torch.arange(n, device=logits.device)
    top = logits == logits.max(-1, keepdim=True).values
    return torch.where(top, idx, n).min(-1).values.clamp_(max=n - 1).to(torch.uint8)   # (all-NaN row: n - 1)


def head_argmax(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None, pro=None):
    """Classifier head -> per-row labels: x [..., K], w [N, K], b [N] or None ->
    (uint8 labels [...], fp32 top-1 softmax probability [...]), in fp32.

    ``pro = (scale, shift, act)``: the head reads ``act(x * scale + shift)`` (act: a name or
    the kernels' code, none / relu).  Ties go to the lowest class index.  The oracle of the
    ``pw_argmax`` kernel and the CPU path of ``FeatureNet3DSeg.predict``."""
    z = x.float()
    if pro is not None:
        scale, shift, act = pro
        z = z * scale.float() + shift.float()
        if act in (1, "relu"):
            z = F.relu(z)
        elif act not in (0, None, "none", "linear"):
            raise ValueError(f"head_argmax: prologue activation {act!r}")
    logits = F.linear(z, w.float(), None if b is None else b.float())
    conf = torch.softmax(logits, -1).max(-1).values
    return lowest_argmax(logits), conf


def confusion(truth: torch.Tensor, pred: torch.Tensor, n_classes: int, ignore_index: int | None = None) -> torch.Tensor:
    """Confusion counts of ``pred`` against ``truth`` (integer tensors of one shape) -> int64
    ``[n*n + 1]``: slot ``t*n + p`` counts the elements with truth ``t < n`` and prediction ``p``
    (rows = truth, columns = prediction), the last slot those whose truth is ``>= n`` (out of
    range); elements whose truth equals ``ignore_index`` are counted nowhere.  Exact integers:
    the oracle of the scoring kernel (``pw_argmax_cm``) and the CPU path of
    ``FeatureNet3DSeg.score``."""
    n = int(n_classes)
    t = truth.reshape(-1).to(torch.int64)
    p = pred.reshape(-1).to(torch.int64)
    if ignore_index is not None:
        keep = t != int(ignore_index)
        t, p = t[keep], p[keep]
    key = torch.where(t >= n, torch.full_like(t, n * n), t * n + p)
    return torch.bincount(key, minlength=n * n + 1)


def _ccl_offsets(connectivity: int) -> list[tuple[int, int, int]]:
    if connectivity not in (6, 26):
        raise ValueError(f"connectivity must be 6 (faces) or 26 (faces, edges and corners), not {connectivity!r}")
    offs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
    return offs if connectivity == 26 else [o for o in offs if sum(map(abs, o)) == 1]


def connected_components(labels: torch.Tensor, background: int | None = 0, connectivity: int = 6) -> torch.Tensor:
    """Connected components of a label volume ``uint8 [N, D, H, W]`` -> ``roots`` int32 of the same
    shape: 1 + the smallest C-order linear index (within the sample) of any voxel of the component,
    0 for voxels of class ``background`` (None: every class forms components).  Two voxels of one
    class are linked when they are 6- or 26-neighbours; nothing links across samples or wraps
    round a row or plane.

    Neighbour-min propagation over shifted views to a fixed point (every voxel keeps taking the
    smallest value among itself and its linked neighbours, and then the value its own value's
    voxel holds, until a sweep changes nothing): no union-find, the oracle of the ``ccl_*``
    kernels and the CPU path of ``ops.ccl.connected_components``."""
    offs = _ccl_offsets(connectivity)
    if labels.dim() != 4 or labels.dtype != torch.uint8:
        raise ValueError(f"connected_components: labels must be uint8 [N, D, H, W], not {labels.dtype} "
                         f"{tuple(labels.shape)}")
    N, D, H, W = labels.shape
    V = D * H * W
    if V >= 1 << 31:
        raise ValueError("connected_components: a sample must have fewer than 2^31 voxels")
    fg = torch.ones_like(labels, dtype=torch.bool) if background is None else labels != int(background)
    cur = torch.where(fg, torch.arange(1, V + 1, device=labels.device).view(1, D, H, W), 0)
    links = []
    for dz, dy, dx in offs:
        def sl(n, d):                            # (destination, source) slices of one axis
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (zd, zs), (yd, ys), (xd, xs) = sl(D, dz), sl(H, dy), sl(W, dx)
        dst, src = (slice(None), zd, yd, xd), (slice(None), zs, ys, xs)
        ok = fg[dst] & (labels[dst] == labels[src])
        if ok.any():
            links.append((dst, src, ok))
    while N and V:
        before = cur.clone()
        for dst, src, ok in links:
            cur[dst] = torch.where(ok, torch.minimum(cur[dst], cur[src]), cur[dst])
        if torch.equal(cur, before):
            break
        flat = cur.view(N, V)                    # then the value of the voxel my value names
        cur = torch.where(flat > 0, flat.gather(1, (flat - 1).clamp_(min=0)), 0).view(N, D, H, W)
    return cur.to(torch.int32)


def instance_table(labels: torch.Tensor, roots: torch.Tensor, want_ids: bool = True):
    """Instance table of a labelled volume -> ``(ids or None, table, offsets)``.

    ``roots`` as :func:`connected_components` gives them.  ``ids`` int32 ``[N, D, H, W]`` numbers
    the components of each sample 1..n in ascending order of their root (0: background).
    ``table`` int64 ``[T, 13]``, rows sorted by (sample, root), columns ``sample, class, voxels,
    root, z0, y0, x0, z1, y1, x1`` (bounds inclusive), ``sum_z, sum_y, sum_x``; ``offsets`` int64
    ``[N + 1]``: sample ``n`` owns rows ``offsets[n]:offsets[n + 1]``.  Exact integers: the oracle
    of ``ccl_stats`` and the CPU path of ``ops.ccl.instance_table``."""
    N, D, H, W = labels.shape
    V = D * H * W
    dev = labels.device
    r = roots.reshape(N, V).to(torch.int64)
    flags = r == torch.arange(1, V + 1, device=dev)
    rank = torch.cumsum(flags.reshape(-1), 0).view(N, V)            # 1-based table row of each root
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), rank[:, -1]]) if V else \
        torch.zeros(N + 1, dtype=torch.int64, device=dev)
    T = int(offsets[-1])
    fg = r > 0
    row = torch.where(fg, rank.gather(1, (r - 1).clamp_(min=0)), 0)   # 1-based row of every voxel
    ids = None
    if want_ids:
        ids = torch.where(fg, row - offsets[:-1, None], 0).to(torch.int32).view(N, D, H, W)
    table = torch.zeros(T, 13, dtype=torch.int64, device=dev)
    if T:
        n, v = fg.nonzero(as_tuple=True)
        k = row[n, v] - 1
        z, y, x = v // (H * W), v // W % H, v % W
        table[:, 2] = torch.bincount(k, minlength=T)
        first = flags[n, v]                                         # the root voxels, in row order
        table[:, 0], table[:, 3] = n[first], v[first] + 1
        table[:, 1] = labels.reshape(N, V)[n, v][first].to(torch.int64)
        for c, q in enumerate((z, y, x)):
            table[:, 4 + c] = torch.full((T,), 1 << 31, dtype=torch.int64, device=dev).scatter_reduce(0, k, q, "amin")
            table[:, 7 + c] = torch.full((T,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, k, q, "amax")
            table[:, 10 + c] = torch.zeros(T, dtype=torch.int64, device=dev).index_add_(0, k, q)
    return ids, table, offsets


def overlap_table(ids_a: torch.Tensor, off_a: torch.Tensor, ids_b: torch.Tensor, off_b: torch.Tensor) -> torch.Tensor:
    """Overlap table of two instance-id volumes -> ``pairs`` int64 ``[P, 3]``.

    ``ids_a`` / ``ids_b`` int32 ``[N, D, H, W]`` and ``off_a`` / ``off_b`` int64 ``[N + 1]`` as
    :func:`instance_table` gives them for two label volumes of one shape.  One row ``(row_a, row_b,
    voxels)`` per pair of instances that share a voxel: their 0-based rows in the two instance
    tables and the number of shared voxels, sorted by ``(row_a, row_b)``.  Exact integers: the
    oracle of ``overlap_pairs`` and the CPU path of ``ops.overlap.overlap_table``."""
    N = ids_a.shape[0]
    a = ids_a.reshape(N, -1).to(torch.int64)
    b = ids_b.reshape(N, -1).to(torch.int64)
    both = (a > 0) & (b > 0)
    ra = a + off_a.to(torch.int64)[:-1, None] - 1
    rb = b + off_b.to(torch.int64)[:-1, None] - 1
    keys, counts = torch.unique((ra << 32 | rb)[both], return_counts=True)
    return torch.stack([keys >> 32, keys & 0xffffffff, counts], 1)


def column_extents(occ: torch.Tensor):
    """Column extents of an occupancy volume ``uint8 [N, D, H, W]`` (material: ``occ != 0``) ->
    ``(ex, ey, ez)`` int32 ``[N, D, H, 2]``, ``[N, D, W, 2]``, ``[N, H, W, 2]``: ``[..., 0]`` is the
    smallest index along x / y / z that holds material in the column (the axis length when it has
    none), ``[..., 1]`` the largest (-1 when none).  ``amin`` / ``amax`` over an index grid: the
    oracle of ``access_extents`` and the CPU path of ``ops.access.column_extents``."""
    if occ.dim() != 4 or occ.dtype != torch.uint8:
        raise ValueError(f"column_extents: occ must be uint8 [N, D, H, W], not {occ.dtype} {tuple(occ.shape)}")
    m = occ != 0
    out = []
    for axis in (3, 2, 1):
        L = occ.shape[axis]
        rest = [s for a, s in enumerate(occ.shape) if a != axis]
        if L == 0 or occ.numel() == 0:
            lo = torch.full(rest, L, dtype=torch.int64, device=occ.device)
            hi = torch.full(rest, -1, dtype=torch.int64, device=occ.device)
        else:
            idx = torch.arange(L, device=occ.device).view([L if a == axis else 1 for a in range(4)])
            lo = torch.where(m, idx, L).amin(axis)
            hi = torch.where(m, idx, -1).amax(axis)
        out.append(torch.stack([lo, hi], -1).to(torch.int32))
    return tuple(out)


def access_table(ids: torch.Tensor, offsets: torch.Tensor, occ: torch.Tensor, want_mask: bool = False):
    """Access table of an instance-id volume over an occupancy volume -> ``(acc, mask or None)``.

    ``ids`` int32 ``[N, D, H, W]`` and ``offsets`` int64 ``[N + 1]`` as :func:`instance_table`
    gives them, ``occ`` uint8 of the ids' shape.  A voxel ``(z, y, x)`` is open toward ``+x`` when
    no material lies strictly beyond it in its x column (``ex hi <= x``), toward ``-x`` when none
    lies strictly before it (``ex lo >= x``), likewise y and z; its own occupancy does not enter.
    ``mask`` uint8 ``[N, D, H, W]`` holds bit ``k`` where the voxel is open toward face ``k`` of
    ``+z, -z, +x, -x, +y, -y`` (0 where ``ids == 0``).  ``acc`` int64 ``[T, 8]``, ``T =
    offsets[-1]``: row ``offsets[n] + id - 1`` counts, of id ``id`` of sample ``n``, the voxels open
    toward each face (columns 0..5), toward none (6) and all of them (7).  Exact integers: the
    oracle of ``access_stats`` and the CPU path of ``ops.access.access_table``."""
    N, D, H, W = ids.shape
    dev = ids.device
    ex, ey, ez = column_extents(occ)
    z = torch.arange(D, device=dev).view(1, D, 1, 1)
    y = torch.arange(H, device=dev).view(1, 1, H, 1)
    x = torch.arange(W, device=dev).view(1, 1, 1, W)
    open_ = (ez[..., 1].unsqueeze(1) <= z, ez[..., 0].unsqueeze(1) >= z,
             ex[..., 1].unsqueeze(3) <= x, ex[..., 0].unsqueeze(3) >= x,
             ey[..., 1].unsqueeze(2) <= y, ey[..., 0].unsqueeze(2) >= y)
    T = int(offsets[-1])
    row = ids.to(torch.int64) + offsets.to(torch.int64)[:-1].view(N, 1, 1, 1) - 1
    fg = (ids > 0) & (row >= 0) & (row < T)
    mask = torch.zeros(ids.shape, dtype=torch.int64, device=dev)
    for k, b in enumerate(open_):
        mask |= b.expand(ids.shape).to(torch.int64) << k
    mask = torch.where(fg, mask, 0)
    rows, bits = row[fg], mask[fg]
    acc = torch.zeros(T, 8, dtype=torch.int64, device=dev)
    if T:
        for k in range(6):
            acc[:, k] = torch.bincount(rows[(bits >> k & 1) != 0], minlength=T)
        acc[:, 6] = torch.bincount(rows[bits == 0], minlength=T)
        acc[:, 7] = torch.bincount(rows, minlength=T)
    return acc, (mask.to(torch.uint8) if want_mask else None)


EDT_INF = 1 << 30          # distance_sq of a sample without a seed
EDT_MAX_S = 256            # longest axis distance_sq takes: every result fits 3 * 255^2


def distance_sq(seeds: torch.Tensor, border: bool = False) -> torch.Tensor:
    """Exact squared Euclidean distance transform of ``seeds`` uint8 ``[N, D, H, W]`` (a voxel is a
    seed when ``seeds != 0``) -> int32 ``[N, D, H, W]``: the smallest ``(z-z')^2 + (y-y')^2 +
    (x-x')^2`` over the seeds ``(z', y', x')`` of the same sample, 0 on a seed, ``EDT_INF`` in a
    sample without one.  With ``border`` every position just outside the grid (index -1 or the
    axis length, on any axis) is a seed too, so the result is also bounded by the smallest ``min(i
    + 1, L - i)^2`` over the axes.  Each axis is at most ``EDT_MAX_S``.

    Three separable min-plus passes (x, y, z), ``out[i] = min_j g[j] + (i - j)^2`` from ``g = 0`` on
    seeds and ``EDT_INF`` elsewhere, in int64: the oracle of ``edt_xy`` / ``edt_z`` and the CPU path
    of ``ops.edt.distance_sq``."""
    if seeds.dim() != 4 or seeds.dtype != torch.uint8:
        raise ValueError(f"distance_sq: seeds must be uint8 [N, D, H, W], not {seeds.dtype} {tuple(seeds.shape)}")
    if max(seeds.shape[1:]) > EDT_MAX_S:
        raise ValueError(f"distance_sq: each of D, H, W is at most {EDT_MAX_S}, not {tuple(seeds.shape[1:])}")
    inf = torch.tensor(EDT_INF, dtype=torch.int64, device=seeds.device)
    g = torch.where(seeds != 0, 0, inf)
    if g.numel() == 0:
        return g.to(torch.int32)
    for axis in (3, 2, 1):
        L = seeds.shape[axis]
        i = torch.arange(L, device=seeds.device).view([L if a == axis else 1 for a in range(4)])
        out = torch.minimum((i + 1) ** 2, (L - i) ** 2).expand(g.shape).clone() if border else g.clone()
        for j in range(L):
            out = torch.minimum(out, g.narrow(axis, j, 1) + (i - j) ** 2)
        g = out.clamp_(max=EDT_INF)
    return g.to(torch.int32)


def dimension_table(ids: torch.Tensor, offsets: torch.Tensor, d2: torch.Tensor) -> torch.Tensor:
    """Dimension table of an instance-id volume over a squared-distance volume -> int64 ``[T, 4]``.

    ``ids`` int32 ``[N, D, H, W]`` and ``offsets`` int64 ``[N + 1]`` as :func:`instance_table` gives
    them (``T = offsets[-1]``), ``d2`` int32 of the ids' shape (:func:`distance_sq`).  Row ``offsets[n]
    + id - 1`` holds, of id ``id`` of sample ``n``: ``r2``, the largest ``d2`` over its voxels; ``at``,
    the smallest linear index ``(z * H + y) * W + x`` within the sample of a voxel that attains it;
    ``wall``, its voxels with ``d2 == 1``; ``voxels``, all of them.  A row that no voxel carries
    holds ``(-1, -1, 0, 0)``; a voxel with id 0 or whose row lies outside the table counts nowhere.
    Exact integers: the oracle of ``edt_stats`` and the CPU path of ``ops.edt.dimension_table``."""
    N, D, H, W = ids.shape
    dev = ids.device
    T = int(offsets[-1])
    row = ids.to(torch.int64) + offsets.to(torch.int64)[:-1].view(N, 1, 1, 1) - 1
    fg = (ids > 0) & (row >= 0) & (row < T)
    dim = torch.zeros(T, 4, dtype=torch.int64, device=dev)
    if T:
        rows, d = row[fg], d2.to(torch.int64)[fg]
        lin = torch.arange(D * H * W, device=dev).view(1, D, H, W).expand(ids.shape)[fg]
        # the largest d2 and, among equals, the smallest index: one max over (d2, ~index)
        key = torch.full((T,), -1, dtype=torch.int64, device=dev).scatter_reduce(
            0, rows, d << 32 | (0xFFFFFFFF - lin), "amax")
        dim[:, 0] = torch.where(key >= 0, key >> 32, -1)
        dim[:, 1] = torch.where(key >= 0, 0xFFFFFFFF - (key & 0xFFFFFFFF), -1)
        dim[:, 2] = torch.bincount(rows[d == 1], minlength=T)
        dim[:, 3] = torch.bincount(rows, minlength=T)
    return dim


NN_MAX_S = 128             # longest axis nearest_labels takes (the kernels' column strip of key pairs fills the LDS)
NN_NONE = EDT_INF << 32    # the key of a missing rank
WALL_NCOL = 5              # gap2 at other thin voxels
_NN_CHUNK = 1 << 22        # voxels of the label volumes that nearest_labels holds at a time


def nearest_labels(ids: torch.Tensor) -> torch.Tensor:
    """Labelled distance transform of ``ids`` int32 ``[N, D, H, W]`` (a voxel is a seed of label
    ``ids`` when ``ids > 0``) -> ``nn`` int64 ``[N, 2, D, H, W]`` of keys ``d2 << 32 | label``.  With
    ``dist2_L(v)`` the smallest ``(z-z')^2 + (y-y')^2 + (x-x')^2`` over the seeds of label ``L`` in
    ``v``'s sample, rank 0 of ``v`` is the smallest key ``dist2_L(v) << 32 | L`` over the sample's
    labels -- the nearest label, among equally near ones the smallest -- and rank 1 the smallest key
    over the other labels; a missing rank (no seed / fewer than two labels in the sample) is
    ``NN_NONE = EDT_INF << 32``.  Each axis is at most ``NN_MAX_S``.

    Label by label, straight from the definition: one :func:`distance_sq` per label present -- or,
    for a label of fewer seeds than the transform has steps, the distances from every voxel to each
    of its seeds (predicted labels break into thousands of such specks) -- then the smallest key and
    the smallest key of another label over all of them, a chunk of labels or seeds at a time.  The
    oracle of ``nn_xy`` / ``nn_z`` (which keep two keys through three separable passes instead) and
    the CPU path of ``ops.nearest.nearest_labels``."""
    if ids.dim() != 4 or ids.dtype != torch.int32:
        raise ValueError(f"nearest_labels: ids must be int32 [N, D, H, W], not {ids.dtype} {tuple(ids.shape)}")
    if max(ids.shape[1:]) > NN_MAX_S:
        raise ValueError(f"nearest_labels: each of D, H, W is at most {NN_MAX_S}, not {tuple(ids.shape[1:])}")
    N, D, H, W = ids.shape
    V, dev = D * H * W, ids.device
    nn = torch.full((N, 2, V), NN_NONE, dtype=torch.int64, device=dev)
    if nn.numel() == 0:
        return nn.view(N, 2, D, H, W)

    def top2(best, keys):                        # the two best keys of distinct labels among best [2, V] and keys [K, V]
        keys = torch.cat([best, keys])
        a = keys.min(0).values
        return torch.stack([a, torch.where((keys & 0xFFFFFFFF) == (a & 0xFFFFFFFF), NN_NONE, keys).min(0).values])

    per = max(1, _NN_CHUNK // V)
    lin = torch.arange(V, device=dev)
    zyx = torch.stack([lin // (H * W), lin // W % H, lin % W])                # [3, V]
    for n in range(N):
        flat = ids[n].reshape(-1)
        seeds = torch.nonzero(flat > 0).view(-1)
        labels, which, counts = torch.unique(flat[seeds], return_inverse=True, return_counts=True)
        few = counts < D + H + W
        best = nn[n]
        at = seeds[few[which]]                   # the seeds of the labels of few seeds: all pairs (voxel, seed)
        for c in range(0, len(at), per):
            s = at[c:c + per]
            d2 = ((zyx[:, None, :] - zyx[:, s, None]) ** 2).sum(0)
            best = top2(best, d2 << 32 | flat[s].to(torch.int64)[:, None])
        many = labels[~few]
        for c in range(0, len(many), per):
            ls = many[c:c + per].view(-1, 1, 1, 1)
            d2 = distance_sq((ids[n][None] == ls).to(torch.uint8)).to(torch.int64)
            best = top2(best, (d2 << 32 | ls.to(torch.int64)).view(-1, V))
        nn[n] = best
    return nn.view(N, 2, D, H, W)


def wall_decode(raw: torch.Tensor, offsets: torch.Tensor, nn: torch.Tensor) -> torch.Tensor:
    """The wall table int64 ``[T, 5]`` from its raw form int64 ``[T, 3]`` (the smallest ``rank-1 d2 <<
    32 | index in the sample`` over the row's voxels, the thin voxels, the voxels), over ``T`` rows:
    the sample of a row is the one whose ``offsets`` hold it, and ``other`` is read from rank 1 of
    ``nn`` at ``at``."""
    T = raw.shape[0]
    N, V = nn.shape[0], nn[0, 0].numel()
    key, thin, vox = raw.unbind(1)
    d = key >> 32
    has = (vox > 0) & (d >= 0) & (d < EDT_INF)
    at = torch.where(has, key & 0xFFFFFFFF, 0).clamp_(max=V - 1)       # (an index of a voxel, whatever raw holds)
    n = (torch.bucketize(torch.arange(T, device=raw.device), offsets[1:].contiguous(), right=True)).clamp_(max=N - 1)
    label = nn[:, 1].reshape(-1)[n * V + at] & 0xFFFFFFFF
    minus = torch.full_like(key, -1)
    return torch.stack([torch.where(has, d, minus), torch.where(has, at, minus),
                        torch.where(has, offsets[:-1][n] + label - 1, minus), thin, vox], 1)


def wall_table(ids: torch.Tensor, offsets: torch.Tensor, nn: torch.Tensor, limit2: int = 0) -> torch.Tensor:
    """Wall table of an instance-id volume over its labelled transform -> int64 ``[T, 5]``.

    ``ids`` int32 ``[N, D, H, W]`` and ``offsets`` int64 ``[N + 1]`` as :func:`instance_table` gives
    them (``T = offsets[-1]``), ``nn`` int64 ``[N, 2, D, H, W]`` (:func:`nearest_labels` of ``ids``).
    Row ``offsets[n] + id - 1`` holds, of id ``id`` of sample ``n``: ``gap2``, the smallest rank-1
    distance over its voxels -- the squared distance between the centres of the nearest voxels of the
    instance and of any other instance of the sample; ``at``, the smallest linear index ``(z * H +
    y) * W + x`` within the sample of a voxel that attains it; ``other``, the table row ``offsets[n]
    + id' - 1`` of rank 1's id at that voxel; ``thin``, its voxels whose rank-1 distance is ``<=
    limit2``; ``voxels``, all of them.  ``gap2, at, other`` are ``-1`` where the sample has no other
    instance or no voxel carries the row; a voxel with id 0 or whose row lies outside the table counts
    nowhere.  Exact integers: the oracle of ``wall_stats`` and the CPU path of
    ``ops.nearest.wall_table``."""
    N, D, H, W = ids.shape
    dev = ids.device
    T = int(offsets[-1])
    row = ids.to(torch.int64) + offsets.to(torch.int64)[:-1].view(N, 1, 1, 1) - 1
    fg = (ids > 0) & (row >= 0) & (row < T)
    raw = torch.zeros(T, 3, dtype=torch.int64, device=dev)
    if T == 0 or ids.numel() == 0:
        return torch.cat([torch.full((T, 3), -1, dtype=torch.int64, device=dev), raw[:, 1:]], 1)
    rows, d = row[fg], (nn[:, 1] >> 32)[fg]
    lin = torch.arange(D * H * W, device=dev).view(1, D, H, W).expand(ids.shape)[fg]
    # the smallest d2 and, among equals, the smallest index: one min over (d2, index)
    raw[:, 0] = torch.full((T,), -1, dtype=torch.int64, device=dev).scatter_reduce(
        0, rows, d << 32 | lin, "amin", include_self=False)
    raw[:, 1] = torch.bincount(rows[d <= limit2], minlength=T)
    raw[:, 2] = torch.bincount(rows, minlength=T)
    return wall_decode(raw, offsets.to(torch.int64), nn)


REACH_NCOL = 15            # entry2 of the six faces, reached from each, from none, machinable, voxels


def reach_scan(vol: torch.Tensor) -> torch.Tensor:
    """Directional minima of ``vol`` int32 ``[N, D, H, W]`` -> ``r6`` int32 ``[N, 6, D, H, W]``:
    ``r6[n, k, v]`` is the smallest ``vol[n]`` over the voxels from ``v`` to face ``k`` of the grid
    (``+z, -z, +x, -x, +y, -y``; ``+z`` the high-index end) along that face's axis, ``v`` included.
    Over ``vol = distance_sq(occ)`` it is the squared clearance of the largest ball whose centre
    travels in a straight line from outside face ``k`` to ``v``.  Each axis is at most
    ``EDT_MAX_S``.  ``torch.cummin`` along the axis, on a flipped view for the ``+`` faces: the
    oracle of ``reach_scan`` (kernel) and the CPU path of ``ops.reach.reach_scan``."""
    if vol.dim() != 4 or vol.dtype != torch.int32:
        raise ValueError(f"reach_scan: vol must be int32 [N, D, H, W], not {vol.dtype} {tuple(vol.shape)}")
    if max(vol.shape[1:]) > EDT_MAX_S:
        raise ValueError(f"reach_scan: each of D, H, W is at most {EDT_MAX_S}, not {tuple(vol.shape[1:])}")
    if vol.numel() == 0:
        return vol.new_zeros((vol.shape[0], 6) + tuple(vol.shape[1:]))
    out = []
    for axis in (1, 3, 2):
        out.append(vol.flip(axis).cummin(axis).values.flip(axis))
        out.append(vol.cummin(axis).values)
    return torch.stack(out, 1)


def reach_seeds(r6: torch.Tensor, need2: int) -> torch.Tensor:
    """uint8 ``[N, D, H, W]``: 1 where a tool that needs the squared clearance ``need2`` reaches the
    voxel with its centre from at least one face (``r6[:, k] >= need2`` for some ``k``)."""
    return (r6 >= need2).any(1).to(torch.uint8)


def reach_table(ids: torch.Tensor, offsets: torch.Tensor, r6: torch.Tensor, dc2: torch.Tensor, need2: int,
                cut2: int) -> torch.Tensor:
    """Reach table of an instance-id volume for one tool -> int64 ``[T, 15]``.

    ``ids`` int32 ``[N, D, H, W]`` and ``offsets`` int64 ``[N + 1]`` as :func:`instance_table` gives
    them (``T = offsets[-1]``); ``r6`` = :func:`reach_scan` of ``distance_sq(occ)``; ``dc2`` =
    ``distance_sq(reach_seeds(r6, need2))``, the squared distance to the nearest centre the tool
    reaches.  The tool, a ball of diameter ``t``, enters as ``need2 = ceil(((t + 1) / 2)^2) >= 1``
    (a centre is admissible from face ``k`` iff ``r6[k] >= need2``) and ``cut2 = floor((t / 2)^2)
    >= 0`` (at a centre it removes the voxels within squared distance ``cut2``).  Row ``offsets[n]
    + id - 1`` holds, of id ``id`` of sample ``n``: the largest ``r6[k]`` over its voxels (columns
    0..5), its voxels with ``r6[k] >= need2`` (6..11), with no such ``k`` (12), with ``dc2 <=
    cut2`` (13: machinable) and all of them (14).  A row that no voxel carries holds -1 in columns
    0..5 and 0 elsewhere; a voxel with id 0 or whose row lies outside the table counts nowhere.
    Exact integers: the oracle of ``reach_stats`` and the CPU path of ``ops.reach.reach_table``."""
    if need2 < 1 or cut2 < 0:
        raise ValueError(f"reach_table: need2 >= 1 and cut2 >= 0, not {need2}, {cut2}")
    N = ids.shape[0]
    dev = ids.device
    T = int(offsets[-1])
    row = ids.to(torch.int64) + offsets.to(torch.int64)[:-1].view(N, 1, 1, 1) - 1
    fg = (ids > 0) & (row >= 0) & (row < T)
    out = torch.zeros(T, REACH_NCOL, dtype=torch.int64, device=dev)
    if T:
        rows = row[fg]
        none = torch.ones_like(rows, dtype=torch.bool)
        for k in range(6):
            e = r6[:, k].to(torch.int64)[fg]
            out[:, k] = torch.full((T,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, rows, e, "amax")
            out[:, 6 + k] = torch.bincount(rows[e >= need2], minlength=T)
            none &= e < need2
        out[:, 12] = torch.bincount(rows[none], minlength=T)
        out[:, 13] = torch.bincount(rows[dc2[fg] <= cut2], minlength=T)
        out[:, 14] = torch.bincount(rows, minlength=T)
    return out


CONTACT_NCOL = 19          # wall, open and shared faces toward the six sides, voxels
CONTACT_MAX_T = 1 << 30    # rows a pair key of the contact kernel holds (two rows and a face in 63 bits)


def contact_table(ids: torch.Tensor, offsets: torch.Tensor, occ: torch.Tensor):
    """Contact table of an instance-id volume over an occupancy volume -> ``(contact, adj)``.

    ``ids`` int32 ``[N, D, H, W]`` and ``offsets`` int64 ``[N + 1]`` as :func:`instance_table`
    gives them (``T = offsets[-1]``), ``occ`` uint8 of the ids' shape (material: ``occ != 0``).  For
    a voxel ``v`` with ``ids[v] > 0`` and a face ``k`` of ``+z, -z, +x, -x, +y, -y`` let ``u`` be its
    neighbour toward that face in the same sample.  The face of ``v`` is *interior* when ``u`` lies
    in the grid and carries the same id; a *wall* when ``u`` lies in the grid, carries no id
    (``ids[u] <= 0``) and is material; *open* when ``u`` lies outside the grid, or carries no id and
    is not material; *shared* when ``u`` lies in the grid and carries another id ``> 0``.  The
    voxel's own occupancy does not enter.

    ``contact`` int64 ``[T, 19]``: row ``offsets[n] + id - 1`` counts, of id ``id`` of sample ``n``,
    the wall faces toward each side (columns 0..5), the open faces (6..11), the shared faces
    (12..17) and the voxels (18); a voxel with id 0 or whose row lies outside the table counts
    nowhere, a row that no voxel carries is 0.  ``adj`` int64 ``[P, 4]``: one row ``(row_a, row_b, k,
    faces)`` per triple that occurs, 0-based table rows with ``row_a < row_b``, sorted by ``(row_a,
    row_b, k)``: ``faces`` faces of ``a`` have their neighbour toward side ``k`` in ``b`` (each
    shared face is told once, from its lower row; a neighbour whose row lies outside the table is
    *shared* in ``contact`` and has no row in ``adj``).  Shifted views, ``bincount`` and
    ``torch.unique``: the oracle of ``contact_stats`` and the CPU path of
    ``ops.contact.contact_table``."""
    N, D, H, W = ids.shape
    dev = ids.device
    T = int(offsets[-1])
    contact = torch.zeros(T, CONTACT_NCOL, dtype=torch.int64, device=dev)
    adj = torch.zeros(0, 4, dtype=torch.int64, device=dev)
    if T == 0 or ids.numel() == 0:
        return contact, adj
    if T >= CONTACT_MAX_T:
        raise ValueError(f"contact_table: the instance table must have fewer than 2^30 rows, not {T}")
    own = ids.to(torch.int64)
    base = offsets.to(torch.int64)[:-1].view(N, 1, 1, 1) - 1
    row = own + base                                                # 0-based
    live = (own > 0) & (row >= 0) & (row < T)
    material = occ != 0
    keys = []
    for k, (axis, toward) in enumerate(((1, 1), (1, -1), (3, 1), (3, -1), (2, 1), (2, -1))):
        L = ids.shape[axis]
        inside = torch.zeros(ids.shape, dtype=torch.bool, device=dev)
        other = torch.zeros_like(own)
        solid = torch.zeros_like(inside)
        if L > 1:                                # the voxels that have a neighbour on that side, and it
            here, there = (0, 1) if toward > 0 else (1, 0)
            inside.narrow(axis, here, L - 1).fill_(True)
            other.narrow(axis, here, L - 1).copy_(own.narrow(axis, there, L - 1))
            solid.narrow(axis, here, L - 1).copy_(material.narrow(axis, there, L - 1))
        named = inside & (other > 0)
        shared = named & (other != own)
        bare = inside & ~named
        for c, m in enumerate((bare & solid, ~inside | (bare & ~solid), shared)):
            contact[:, 6 * c + k] = torch.bincount(row[live & m], minlength=T)
        mate = other + base
        tell = live & shared & (mate < T) & (row < mate)
        keys.append((row[tell] << 33) | (mate[tell] << 3) | k)
    contact[:, 18] = torch.bincount(row[live], minlength=T)
    key, faces = torch.unique(torch.cat(keys), return_counts=True)
    if key.numel():
        adj = torch.stack([key >> 33, (key >> 3) & (CONTACT_MAX_T - 1), key & 7, faces], 1)
    return contact, adj


def _part_volume(cls: int, f: dict, X, Y, Z, top: int):
    """The volume of one feature class over canonical quarter-voxel coordinates ``X, Y, Z``
    (int64 ``[n, S, S, S]``); ``f`` maps the field names of a table row to ``[n, 1, 1, 1]``."""
    u, v, dz = X - f["cu"], Y - f["cv"], top - Z
    r, a, b, depth, w = f["r"], f["a"], f["b"], f["depth"], f["w"]

    def circle(p, q, rad):
        return p * p + q * q <= rad * rad

    def rect(p, q, ha, hb):
        return (p.abs() <= ha) & (q.abs() <= hb)

    def tri(p, q, rad):
        return (2 * q >= -rad) & (q <= rad) & (3 * p * p <= (rad - q) ** 2)

    def hexagon(p, q, rad):
        return (4 * q * q <= 3 * rad * rad) & (p.abs() <= rad) & (q * q <= 3 * (rad - p.abs()) ** 2)

    def slot_ends(p, q):
        return rect(p, q, a, r) | circle(p - a, q, r) | circle(p + a, q, r)

    blind = dz <= depth
    if cls == 0:
        return blind & circle(u, v, r) & ~circle(u, v, f["r2"])
    if cls in (1, 2):
        return blind & circle(u, v, r)
    if cls in (3, 9):
        return blind & tri(u, v, r)
    if cls in (4, 10):
        return blind & rect(u, v, a, b)
    if cls in (5, 11):
        return blind & slot_ends(u, v)
    if cls == 6:
        return blind & (5 * u.abs() <= 3 * (depth - dz))
    if cls == 7:
        return blind & (u.abs() <= a)
    if cls == 8:
        return blind & (u.abs() <= a) & (v <= b)
    if cls == 12:
        return blind & (X + Y <= r)
    if cls == 13:
        return blind & circle(X, Y, r)
    if cls == 14:
        return blind & (X <= a) & (Y <= b)
    if cls == 15:
        return blind & (X <= a)
    if cls == 16:
        return blind & ((X <= a) | (X >= top - a))
    if cls == 17:
        return blind & (2 * X * depth <= 4 * a * (depth - dz) + a * depth)
    if cls == 18:
        return X + dz < w
    if cls == 19:
        return (X < w) & (dz < w) & ((w - X) ** 2 + (w - dz) ** 2 > w * w)
    if cls == 20:
        return blind & (((u.abs() <= r) & (v <= 0)) | circle(u, v, r))
    if cls == 21:
        return (v <= b) & (((dz <= depth - r) & (u.abs() <= r)) | circle(u, dz - (depth - r), r))
    if cls in (22, 23):
        return blind & hexagon(u, v, r)
    raise ValueError(f"carve_parts: class {cls} outside -1..23")


PART_FIELDS = ("cls", "orient", "cu", "cv", "r", "r2", "a", "b", "depth", "w", "x0", "x1", "y0", "y1", "z0", "z1")


def carve_parts(params: torch.Tensor, size: int):
    """Multi-feature parts from their parameter tables -> ``(occupancy, labels, slots)``, each
    uint8 ``[N, S, S, S]`` on the table's device.

    ``params`` int32 ``[N, K, 16]``, a row being ``cls, orient, cu, cv, r, r2, a, b, depth, w`` and
    the feature's bounding box ``x0, x1, y0, y1, z0, z1`` (which this function does not read: a
    box is never smaller than its feature).  ``cls`` -1 is an unused slot.  ``orient = o + 6 fx +
    12 fy``: output voxel ``(X, Y, Z)`` is canonical voxel ``(x, y, z)`` mirrored in x (``fx``)
    and y (``fy``) and then turned so that the canonical top face z = S-1 becomes face ``o`` (+z,
    -z, +x, -x, +y, -y).  Geometry is in quarter voxels, voxel centres at multiples of 4.
    ``labels`` is 1 + the class of the lowest slot whose volume holds the voxel, ``slots`` 1 + that
    slot, both 0 where there is none, and ``occupancy`` is 1 exactly there.  Exact integers
    (int64 throughout): the oracle of ``partgen_carve`` and ``_rt.carve_parts``."""
    if params.dim() != 3 or params.shape[2] != 16 or params.dtype != torch.int32:
        raise ValueError(f"carve_parts: params must be int32 [N, K, 16], not {params.dtype} {tuple(params.shape)}")
    N, K, _ = params.shape
    S, dev = int(size), params.device
    e, top = S - 1, 4 * (S - 1)
    p = params.to(torch.int64)
    ax = torch.arange(S, device=dev, dtype=torch.int64)
    Zo, Yo, Xo = (t.expand(1, S, S, S) for t in torch.meshgrid(ax, ax, ax, indexing="ij"))
    labels = torch.zeros(N, S, S, S, dtype=torch.uint8, device=dev)
    slots = torch.zeros_like(labels)
    # canonical (x, y, z) of an output voxel for each access face, before the mirrors
    faces = [(Xo, Yo, Zo), (Xo, e - Yo, e - Zo), (e - Zo, Yo, Xo), (Zo, Yo, e - Xo), (Xo, e - Zo, Yo),
             (Xo, Zo, e - Yo)]
    for k in reversed(range(K)):                 # the lowest slot is painted last: it wins
        for cls in p[:, k, 0].unique().tolist():
            if cls == -1:
                continue
            for orient in p[p[:, k, 0] == cls, k, 1].unique().tolist():
                if not 0 <= orient < 24:
                    raise ValueError(f"carve_parts: orient {orient} outside 0..23")
                sel = ((p[:, k, 0] == cls) & (p[:, k, 1] == orient)).nonzero().squeeze(1)
                x, y, z = faces[orient % 6]
                if orient // 6 % 2:
                    x = e - x
                if orient // 12:
                    y = e - y
                f = {name: p[sel, k, i].view(-1, 1, 1, 1) for i, name in enumerate(PART_FIELDS)}
                vol = _part_volume(int(cls), f, 4 * x, 4 * y, 4 * z, top)
                labels[sel] = torch.where(vol, torch.full_like(labels[sel], cls + 1), labels[sel])
                slots[sel] = torch.where(vol, torch.full_like(slots[sel], k + 1), slots[sel])
    return (labels == 0).to(torch.uint8), labels, slots


def voxelize_tris(tris: torch.Tensor, offsets: torch.Tensor, size: int):
    """Triangle meshes to voxel grids -> ``(occupancy uint8 [N, S, S, S], leaks int64 [N])`` on the
    device of ``tris``.

    ``tris`` int32 ``[T, 9]`` (``ax ay az bx by bz cx cy cz``) on the lattice of 16 units per voxel
    (voxel ``k`` of an axis has its centre at ``16 k + 8``, every ``|coordinate| <= 8192``) and
    ``offsets`` int32 ``[N + 1]``: mesh ``n`` owns ``tris[offsets[n]:offsets[n + 1]]``.  A ray
    runs along +x through every column centre ``(py, pz)``.  A triangle whose ``(y, z)`` projection
    has area covers the columns whose centre has all three edge functions (taken with the
    projection turned counter-clockwise) positive, or zero on an edge that runs towards +y, or
    straight towards -z (the low-z and low-y edges of the projection); the ray crosses its plane at ``x_hit`` and toggles the first voxel
    ``k >= 0`` whose centre is not left of ``x_hit`` (``k = S``: beyond the grid).  A voxel is
    material when the toggles at or left of it are odd in number; ``leaks`` counts the columns
    whose toggles, those beyond the grid included, are odd -- 0 for a closed mesh.  Exact integers
    (int64 throughout): the oracle of ``voxelize_tris`` (kernel) and ``_rt.voxelize_tris``."""
    if tris.dim() != 2 or tris.shape[1] != 9 or tris.dtype != torch.int32:
        raise ValueError(f"voxelize_tris: tris must be int32 [T, 9], not {tris.dtype} {tuple(tris.shape)}")
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("voxelize_tris: offsets must be [N + 1]")
    S, dev = int(size), tris.device
    off = [int(v) for v in offsets.tolist()]
    N = len(off) - 1
    occ = torch.zeros(N, S, S, S, dtype=torch.uint8, device=dev)
    leaks = torch.zeros(N, dtype=torch.int64, device=dev)
    centre = 16 * torch.arange(S, device=dev, dtype=torch.int64) + 8
    pz, py = (c.reshape(1, -1) for c in torch.meshgrid(centre, centre, indexing="ij"))      # [1, S*S], column = z*S + y
    chunk = max(1, (1 << 21) // (S * S))
    for n in range(N):
        counts = torch.zeros(S * S * (S + 1), dtype=torch.int64, device=dev)
        for lo in range(off[n], off[n + 1], chunk):
            t = tris[lo:min(lo + chunk, off[n + 1])].to(torch.int64)
            a, b, c = t[:, 0:3], t[:, 3:6], t[:, 6:9]
            area2 = (b[:, 1] - a[:, 1]) * (c[:, 2] - a[:, 2]) - (b[:, 2] - a[:, 2]) * (c[:, 1] - a[:, 1])
            flip = (area2 < 0).unsqueeze(1)
            b, c = torch.where(flip, c, b), torch.where(flip, b, c)
            keep = area2 != 0
            a, b, c = a[keep], b[keep], c[keep]
            if not len(a):
                continue
            inside = torch.ones(len(a), S * S, dtype=torch.bool, device=dev)
            for p, q in ((a, b), (b, c), (c, a)):
                dy, dz = (q[:, 1] - p[:, 1]).unsqueeze(1), (q[:, 2] - p[:, 2]).unsqueeze(1)
                E = dy * (pz - p[:, 2:3]) - dz * (py - p[:, 1:2])
                inside &= (E > 0) | ((E == 0) & ((dy > 0) | ((dy == 0) & (dz < 0))))
            nrm = torch.linalg.cross(b - a, c - a)                          # nrm[:, 0] = |area2| > 0
            ti, col = inside.nonzero(as_tuple=True)
            nx = nrm[ti, 0]
            A = nrm[ti, 1] * (py[0, col] - a[ti, 1]) + nrm[ti, 2] * (pz[0, col] - a[ti, 2])
            k = -torch.div(-(a[ti, 0] * nx - A - 8 * nx), 16 * nx, rounding_mode="floor")      # ceil
            counts += torch.bincount(col * (S + 1) + k.clamp(0, S), minlength=counts.numel())
        odd = (counts.view(S, S, S + 1) % 2).cumsum(-1) % 2
        occ[n] = odd[..., :S].to(torch.uint8)
        leaks[n] = odd[..., S].sum()
    return occ, leaks


def mesh_votes(tris: torch.Tensor, offsets: torch.Tensor, vol: torch.Tensor, size: int) -> torch.Tensor:
    """Which value of ``vol`` lies against each triangle -> int32 ``[T, 3]`` = ``winner, votes,
    covered``, on the device of ``tris``.

    ``tris`` / ``offsets`` as in :func:`voxelize_tris`; ``vol`` ``[N, S, S, S]`` (indexed ``[n, z,
    y, x]``; int32 instance ids or uint8 labels, 0 = nothing).  Per triangle ``nrm = (b - a) x (c -
    a)``; zero: the row is ``(0, 0, 0)``.  ``m`` is the first of x, y, z with the largest ``|nrm|``,
    ``u = (m + 1) % 3``, ``v = (m + 2) % 3``, and every vertex becomes ``(p[m], p[u], p[v])``: the
    ``(x, y, z)`` of :func:`voxelize_tris`, whose cover test (tie rule included) says which columns
    ``(iu, iv)`` in ``[0, S)^2`` the triangle covers.  In a covered column ``k = ceil((x_hit - 8) /
    16)``, not clamped, and the voxels ``k - 1`` and ``k`` along ``m`` -- one on each side of the
    surface -- give their value one vote each if they lie in the grid and hold one.  ``covered``
    counts the covered columns; a triangle with none votes once at its centroid, column ``(floor(
    sum_u / 48), floor(sum_v / 48))`` (nothing if outside the grid), ``k = ceil((sum_m - 24) / 48)``.
    ``winner`` is the value with the most votes, the lowest on a tie.  Exact integers (int64
    throughout): the oracle of ``mesh_votes`` (kernel) and ``_rt.mesh_votes``."""
    if tris.dim() != 2 or tris.shape[1] != 9 or tris.dtype != torch.int32:
        raise ValueError(f"mesh_votes: tris must be int32 [T, 9], not {tris.dtype} {tuple(tris.shape)}")
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("mesh_votes: offsets must be [N + 1]")
    S, dev = int(size), tris.device
    off = [int(x) for x in offsets.tolist()]
    N, T = len(off) - 1, tris.shape[0]
    if vol.dtype not in (torch.int32, torch.uint8) or tuple(vol.shape) != (N, S, S, S):
        raise ValueError(f"mesh_votes: vol must be int32 or uint8 [{N}, {S}, {S}, {S}], not {vol.dtype} "
                         f"{tuple(vol.shape)}")
    out = torch.zeros(T, 3, dtype=torch.int64, device=dev)
    centre = 16 * torch.arange(S, device=dev, dtype=torch.int64) + 8
    pv, pu = (c.reshape(1, -1) for c in torch.meshgrid(centre, centre, indexing="ij"))      # [1, S*S], column = iv*S + iu
    stride = torch.tensor([1, S, S * S], dtype=torch.int64, device=dev)
    chunk = max(1, (1 << 21) // (S * S))
    for n in range(N):
        flat = vol[n].reshape(-1).to(torch.int64)
        for lo in range(off[n], off[n + 1], chunk):
            hi = min(lo + chunk, off[n + 1])
            t = tris[lo:hi].to(torch.int64).view(-1, 3, 3)
            nrm = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).abs()
            m = torch.where((nrm[:, 0] >= nrm[:, 1]) & (nrm[:, 0] >= nrm[:, 2]), 0,
                            torch.where(nrm[:, 1] >= nrm[:, 2], 1, 2))
            axes = torch.stack([m, (m + 1) % 3, (m + 2) % 3], 1)                            # [n, 3]: m, u, v
            q = torch.gather(t, 2, axes.unsqueeze(1).expand(-1, 3, -1))
            st = stride[axes]                                                               # strides of m, u, v
            a, b, c = q[:, 0], q[:, 1], q[:, 2]
            area2 = (b[:, 1] - a[:, 1]) * (c[:, 2] - a[:, 2]) - (b[:, 2] - a[:, 2]) * (c[:, 1] - a[:, 1])
            flip = (area2 < 0).unsqueeze(1)
            b, c = torch.where(flip, c, b), torch.where(flip, b, c)
            live = nrm.any(1)                                                               # then area2 != 0
            inside = live.unsqueeze(1).expand(-1, S * S).clone()
            for p, r in ((a, b), (b, c), (c, a)):
                du, dv = (r[:, 1] - p[:, 1]).unsqueeze(1), (r[:, 2] - p[:, 2]).unsqueeze(1)
                E = du * (pv - p[:, 2:3]) - dv * (pu - p[:, 1:2])
                inside &= (E > 0) | ((E == 0) & ((du > 0) | ((du == 0) & (dv < 0))))
            pl = torch.linalg.cross(b - a, c - a)                                           # pl[:, 0] = |area2|
            ti, col = inside.nonzero(as_tuple=True)
            nx = pl[ti, 0]
            A = pl[ti, 1] * (pu[0, col] - a[ti, 1]) + pl[ti, 2] * (pv[0, col] - a[ti, 2])
            k = -torch.div(-(a[ti, 0] * nx - A - 8 * nx), 16 * nx, rounding_mode="floor")   # ceil, not clamped
            covered = torch.bincount(ti, minlength=len(t))
            # the centroid vote of the triangles that cover nothing
            lone = (live & (covered == 0)).nonzero().squeeze(1)
            s = q[lone].sum(1)
            ti = torch.cat([ti, lone])
            k = torch.cat([k, -torch.div(-(s[:, 0] - 24), 48, rounding_mode="floor")])
            iu = torch.cat([col % S, torch.div(s[:, 1], 48, rounding_mode="floor")])
            iv = torch.cat([col // S, torch.div(s[:, 2], 48, rounding_mode="floor")])
            column_in = (iu >= 0) & (iu < S) & (iv >= 0) & (iv < S)
            who, what = [], []
            for kk in (k - 1, k):
                ok = column_in & (kk >= 0) & (kk < S)
                lin = kk[ok] * st[ti[ok], 0] + iu[ok] * st[ti[ok], 1] + iv[ok] * st[ti[ok], 2]
                val = flat[lin]
                who.append(ti[ok][val != 0])
                what.append(val[val != 0])
            who, what = torch.cat(who), torch.cat(what)
            rows = out[lo:hi]
            rows[:, 2] = covered
            if len(who):
                pairs, count = torch.unique(torch.stack([who, what], 1), dim=0, return_counts=True)   # by (who, what)
                order = torch.argsort(count, descending=True, stable=True)                  # most votes first,
                order = order[torch.argsort(pairs[order, 0], stable=True)]                  # ... within a triangle
                w = pairs[order, 0]
                head = torch.ones_like(w, dtype=torch.bool)
                head[1:] = w[1:] != w[:-1]
                rows[w[head], 0] = pairs[order, 1][head]
                rows[w[head], 1] = count[order][head]
    return out.to(torch.int32)


ISOLATE_NCOL = 14         # n id | box z0 y0 x0 z1 y1 x1 | window z0 y0 x0 Lz Ly Lx
ISOLATE_MAX_S = 256        # longest grid axis and largest output size isolate_instances takes
_ISOLATE_CHUNK = 1 << 24   # output voxels that isolate_instances gathers at a time


def isolate_check(ids: torch.Tensor, sel: torch.Tensor, size, fmt) -> int:
    """The argument checks of ``isolate_instances`` that need no value of ``sel`` -> ``S``."""
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 4:
        got = f"{ids.dtype} {tuple(ids.shape)}" if isinstance(ids, torch.Tensor) else type(ids).__name__
        raise ValueError(f"isolate_instances: ids must be an int32 [N, D, H, W] tensor, not {got}")
    if not isinstance(sel, torch.Tensor) or sel.dtype != torch.int32 or sel.dim() != 2 \
            or sel.shape[1] != ISOLATE_NCOL:
        got = f"{sel.dtype} {tuple(sel.shape)}" if isinstance(sel, torch.Tensor) else type(sel).__name__
        raise ValueError(f"isolate_instances: sel must be an int32 [M, {ISOLATE_NCOL}] tensor, not {got}")
    if sel.device != ids.device:
        raise ValueError(f"isolate_instances: ids ({ids.device}) and sel ({sel.device}) must be on one device")
    if isinstance(size, bool) or not isinstance(size, int) or size < 8 or size > ISOLATE_MAX_S or size % 8:
        raise ValueError(f"isolate_instances: size must be a multiple of 8 in [8, {ISOLATE_MAX_S}], not {size!r}")
    if fmt not in (0, 1, 2):
        raise ValueError(f"isolate_instances: fmt must be 0 (packed bits), 1 (uint8) or 2 (bf16), not {fmt!r}")
    if max(ids.shape[1:]) > ISOLATE_MAX_S:
        raise ValueError(f"isolate_instances: every grid axis must be at most {ISOLATE_MAX_S}, not "
                         f"{tuple(ids.shape[1:])}")
    if ids.numel() >= 1 << 31:
        raise ValueError("isolate_instances: a batch must have fewer than 2^31 voxels; split it by samples")
    return int(size)


def isolate_bad_rows(sel: torch.Tensor, shape) -> torch.Tensor:
    """bool ``[M]``: the rows of ``sel`` whose sample or window does not lie in a grid of ``shape = (N, D, H,
    W)``, on the device of ``sel``."""
    N = int(shape[0])
    dims = torch.tensor([int(s) for s in shape[1:]], dtype=torch.int64, device=sel.device)
    s = sel.to(torch.int64)
    w0, L = s[:, 8:11], s[:, 11:14]
    return (s[:, 0] < 0) | (s[:, 0] >= N) | ((L < 1) | (w0 < 0) | (w0 + L > dims)).any(1)


def isolate_instances(ids: torch.Tensor, sel: torch.Tensor, size: int, fmt: int = 1) -> torch.Tensor:
    """Each selected instance alone in a solid stock block, at the classifier's resolution.

    ``ids`` int32 ``[N, D, H, W]`` (``instance_table``'s), ``sel`` int32 ``[M, 14]``, a row being ``n, id``
    (the sample and the instance's number in it), ``bz0, by0, bx0, bz1, by1, bx1`` (an inclusive box in the
    source grid) and ``wz0, wy0, wx0, Lz, Ly, Lx`` (the source window that becomes the stock block: ``L >=
    1``, inside the grid).  Output voxel ``o`` of an axis of part ``m`` looks, with ``Lmax = max(Lz, Ly, Lx)``
    and ``L``, ``w0`` those of the axis, at the window's voxel

        ``s = floor_div((2 o + 1) Lmax - (Lmax - L) S, 2 S)``

    -- the centre of ``o`` under the one scale ``Lmax / S``, the shorter axes centred, a centre on a source
    boundary going to the higher index.  A voxel with ``s < 0`` or ``s >= L`` on any axis lies outside the
    stock and is 0 (free space); otherwise its source voxel is ``v = w0 + s``, and it is 0 (the feature) iff
    ``v`` lies in the box and ``ids[n, v] == id``, else 1 (material, also where the source holds another
    instance).  With ``L == Lmax == S`` and ``w0 == 0`` the part is ``ids[n] != id`` inside the box.

    ``fmt`` 0: bits, uint8 ``[M, S^3 / 8]``, bit ``i & 7`` of byte ``i >> 3`` for ``i = (Z S + Y) S + X``; 1:
    uint8 ``[M, S, S, S]``; 2: bfloat16 ``[M, S, S, S, 1]``.  Exact integers: the oracle of ``isolate_parts``
    and the CPU path of ``ops.isolate``."""
    S = isolate_check(ids, sel, size, fmt)
    N, D, H, W = ids.shape
    M, dev = sel.shape[0], ids.device
    if M and bool(isolate_bad_rows(sel, ids.shape).any()):
        raise ValueError(f"isolate_instances: a row of sel names a sample or a window outside the grid "
                         f"{tuple(ids.shape)}")
    out = torch.empty(M, S, S, S, dtype=torch.uint8, device=dev)
    s64 = sel.to(torch.int64)
    o = torch.arange(S, dtype=torch.int64, device=dev)
    step = max(1, _ISOLATE_CHUNK // S ** 3)
    for lo in range(0, M, step):
        r = s64[lo:lo + step]
        L, w0 = r[:, 11:14], r[:, 8:11]
        Lmax = L.amax(1, keepdim=True)
        num = (2 * o + 1) * Lmax[:, :, None] - ((Lmax - L) * S)[:, :, None]          # [m, 3, S]
        s = torch.div(num, 2 * S, rounding_mode="floor")
        inside = (s >= 0) & (s < L[:, :, None])
        v = w0[:, :, None] + s
        inbox = (v >= r[:, 2:5, None]) & (v <= r[:, 5:8, None])
        dims = torch.tensor([D, H, W], dtype=torch.int64, device=dev).view(1, 3, 1)
        vc = torch.minimum(v.clamp(min=0), dims - 1)
        got = ids[r[:, 0].view(-1, 1, 1, 1), vc[:, 0, :, None, None], vc[:, 1, None, :, None],
                  vc[:, 2, None, None, :]]
        cube = lambda t: t[:, 0, :, None, None] & t[:, 1, None, :, None] & t[:, 2, None, None, :]   # noqa: E731
        stock = cube(inside)
        feature = stock & cube(inbox) & (got == r[:, 1].view(-1, 1, 1, 1))
        out[lo:lo + step] = (stock & ~feature).to(torch.uint8)
    if fmt == 1:
        return out
    if fmt == 2:
        return out.to(torch.bfloat16).unsqueeze(-1)
    weights = 1 << torch.arange(8, dtype=torch.int32, device=dev)
    return (out.reshape(M, S ** 3 // 8, 8).to(torch.int32) * weights).sum(-1).to(torch.uint8)


WS_MAX_S = 256             # longest axis the watershed takes


def _ws_check(ids: torch.Tensor, height: torch.Tensor, what: str) -> None:
    if ids.dim() != 4 or ids.dtype != torch.int32:
        raise ValueError(f"{what}: ids must be int32 [N, D, H, W], not {ids.dtype} {tuple(ids.shape)}")
    if height.shape != ids.shape or height.dtype != torch.int32 or height.device != ids.device:
        raise ValueError(f"{what}: height must be int32 {tuple(ids.shape)} on {ids.device}, not {height.dtype} "
                         f"{tuple(height.shape)} on {height.device}")
    if max(ids.shape[1:]) > WS_MAX_S:
        raise ValueError(f"{what}: each of D, H, W is at most {WS_MAX_S}, not {tuple(ids.shape[1:])}")


def _ws_shifts(D: int, H: int, W: int, forward: bool):
    """``(dst, src)`` slices of ``[N, D, H, W]`` for the 26 offsets (the 13 with ``(dz, dy, dx) > (0, 0, 0)`` when
    ``forward``): voxel ``dst`` has its neighbour at that offset in ``src``."""
    for dz, dy, dx in _ccl_offsets(26):
        if forward and (dz, dy, dx) < (0, 0, 0):
            continue

        def sl(n, d):
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (zd, zs), (yd, ys), (xd, xs) = sl(D, dz), sl(H, dy), sl(W, dx)
        yield (slice(None), zd, yd, xd), (slice(None), zs, ys, xs)


def watershed_parents(ids: torch.Tensor, height: torch.Tensor) -> torch.Tensor:
    """One step of the steepest ascent inside the components of an id volume -> ``parent`` int32 ``[N, D, H, W]``.

    ``ids`` int32 ``[N, D, H, W]`` (a voxel with ``ids > 0`` belongs to that component of its sample) and
    ``height`` int32 of the same shape, ``h(v) = max(height[v], 0)``.  ``key(v) = h(v) << 32 | (0xFFFFFFFF -
    index of v in its sample)``: the higher voxel wins, then the lower index.  ``u`` is a neighbour of ``v``
    when it is one of its 26 neighbours in the grid and the sample and ``ids[u] == ids[v]``; ``parent[v]`` is 1
    + the index of the neighbour of the largest key when that key exceeds ``key(v)``, else of ``v`` itself, and 0
    where ``ids <= 0``.  Each axis is at most ``WS_MAX_S``.  One maximum over 26 shifted views: the oracle of
    ``ws_ascend``."""
    _ws_check(ids, height, "watershed_parents")
    N, D, H, W = ids.shape
    V, dev = D * H * W, ids.device
    if N * V == 0:
        return torch.zeros_like(ids)
    lin = torch.arange(V, device=dev).view(1, D, H, W)
    key = height.clamp(min=0).to(torch.int64) << 32 | (0xFFFFFFFF - lin)
    fg = ids > 0
    best = key.clone()
    for dst, src in _ws_shifts(D, H, W, False):
        ok = fg[dst] & (ids[dst] == ids[src])
        best[dst] = torch.where(ok, torch.maximum(best[dst], key[src]), best[dst])
    return torch.where(fg, 0xFFFFFFFF - (best & 0xFFFFFFFF) + 1, 0).to(torch.int32)


def watershed_ascend(ids: torch.Tensor, height: torch.Tensor) -> torch.Tensor:
    """Steepest ascent inside the components of an id volume -> ``roots`` int32 ``[N, D, H, W]``: 1 + the index
    of the end of every voxel's chain of :func:`watershed_parents` (keys are distinct and grow along it, so it
    ends), 0 where ``ids <= 0``.  The voxels of one root are a *basin*, and a root has ``roots[v] == v + 1``.

    Pointer doubling over the parents to a fixed point: the oracle of ``ws_ascend`` + ``ws_resolve`` and the CPU
    path of ``ops.watershed.ascend``."""
    parent = watershed_parents(ids, height)
    N, V = ids.shape[0], ids[0].numel() if ids.shape[0] else 0
    if N * V == 0:
        return parent
    lin = torch.arange(V, device=ids.device).expand(N, V)
    p = torch.where(parent.view(N, V) > 0, parent.view(N, V).to(torch.int64) - 1, lin)
    while True:
        q = p.gather(1, p)
        if torch.equal(q, p):
            break
        p = q
    return torch.where(ids > 0, p.view(ids.shape) + 1, 0).to(torch.int32)


def watershed_saddles(ids: torch.Tensor, basin_ids: torch.Tensor, offsets: torch.Tensor,
                      height: torch.Tensor) -> torch.Tensor:
    """Saddles between the basins of each component -> ``pairs`` int64 ``[P, 3]``.

    ``ids`` and ``height`` as for :func:`watershed_ascend`; ``basin_ids`` int32 of the same shape and ``offsets``
    int64 ``[N + 1]`` as :func:`instance_table` gives them over the watershed's roots (``T = offsets[-1]``).  Over
    every pair ``(u, v)`` of 26-adjacent voxels of one sample with ``ids[u] == ids[v] > 0`` whose basin rows
    ``offsets[n] + basin_ids - 1`` both lie in the table and differ, ``saddle(a, b)`` is the largest ``min(h(u),
    h(v))`` between the rows ``a`` and ``b``.  One row ``(row_a, row_b, saddle)`` per pair of rows that occurs,
    0-based with ``row_a < row_b``, sorted by ``(row_a, row_b)``.  Shifted views, ``torch.unique`` and a scatter
    maximum: the oracle of ``ws_saddle`` and the CPU path of ``ops.watershed.saddle_pairs``."""
    _ws_check(ids, height, "watershed_saddles")
    N, D, H, W = ids.shape
    dev = ids.device
    T = int(offsets[-1])
    none = torch.zeros(0, 3, dtype=torch.int64, device=dev)
    if T == 0 or ids.numel() == 0:
        return none
    row = basin_ids.to(torch.int64) + offsets.to(torch.int64)[:-1].view(N, 1, 1, 1) - 1
    live = (ids > 0) & (basin_ids > 0) & (row >= 0) & (row < T)
    h = height.clamp(min=0).to(torch.int64)
    keys, vals = [], []
    for dst, src in _ws_shifts(D, H, W, True):
        ok = live[dst] & live[src] & (ids[dst] == ids[src]) & (row[dst] != row[src])
        a, b = row[dst][ok], row[src][ok]
        keys.append(torch.minimum(a, b) << 32 | torch.maximum(a, b))
        vals.append(torch.minimum(h[dst][ok], h[src][ok]))
    key, which = torch.unique(torch.cat(keys), return_inverse=True)
    if key.numel() == 0:
        return none
    saddle = torch.full_like(key, -1).scatter_reduce(0, which, torch.cat(vals), "amax")
    return torch.stack([key >> 32, key & 0xFFFFFFFF, saddle], 1)
