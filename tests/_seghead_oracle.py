"""A plain float64 oracle of the fused head + loss kernels: ``seghead_loss_kernel``
(``csrc/kernels/seghead.hip``) and the XENT instance of ``pw_fwd_kernel``
(``csrc/kernels/pointwise.hip``), with the input builders their tests share.

Elementwise arithmetic, matmul, ``logsumexp`` and reductions on float64 tensors only: no library
loss, no autograd.  The comparison helpers are those of ``_bn_pool_oracle`` (re-exported here).

One voxel row:  u = y * sc + sh,  z = act(u),  l = z w^T + b,
                off = smoothing / NC,  on = 1 - smoothing + off,  tgt = off, on at the label,
                loss = -sum_c tgt_c (l_c - lse),  d = (softmax(l) - tgt) * xscale,
                hit = [first arg-max of l == label].
A label outside [0, NC) has no target class: tgt = off for every class (the row's loss is
smoothing * lse - off * sum_c l_c, 0 without smoothing) and the row is never a hit.

Inputs live on dyadic grids (``build_general`` and the builders on top of it) so that z and the
logits are bf16 values: the kernels' fp32 logits are then exact sums whatever the MFMA's order,
the bf16 store of them is exact, ties between logits are real ties and the ReLU mask is decided
without a tolerance.
"""
from __future__ import annotations

import torch

import _bn_pool_oracle as O

ACT_NONE, ACT_RELU = O.ACT_NONE, O.ACT_RELU
# the comparison helpers, shared with the BN / pooling oracle
check_exact, check_one_rounding, check_reduction = O.check_exact, O.check_one_rounding, O.check_reduction
check_fp32, slab_rows_exact, bf16_round = O.check_fp32, O.slab_rows_exact, O.bf16_round

ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu"}
K_HEAD = 32                                      # seghead_loss: decoder channels
TILE = 256                                       # rows per tile of both kernels


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def _act(u, act):
    return torch.where(u > 0, u, torch.zeros_like(u)) if act == ACT_RELU else u


def first_argmax(l):
    """Lowest index among the equal maxima of every row."""
    n = l.shape[1]
    idx = torch.arange(n, device=l.device)
    return torch.where(l == l.amax(1, keepdim=True), idx, n).amin(1)


def last_argmax(l):
    idx = torch.arange(l.shape[1], device=l.device)
    return torch.where(l == l.amax(1, keepdim=True), idx, -1).amax(1)


def targets(labels, NC, smoothing, dtype=torch.float64):
    """tgt [M, NC] and the in-range mask [M]; an out-of-range row gets ``off`` everywhere."""
    lab = labels.to(torch.int64)
    off = smoothing / NC
    on = 1.0 - smoothing + off
    yin = (lab >= 0) & (lab < NC)
    cls = torch.arange(NC, device=lab.device)
    hot = (cls[None, :] == lab[:, None]) & yin[:, None]
    tgt = torch.where(hot, torch.full((), on, dtype=dtype), torch.full((), off, dtype=dtype))
    return tgt, yin


def logits(y, sc, sh, act, w, bias):
    u = y if sc is None else y * sc + sh
    z = u if sc is None else _act(u, act)
    l = z @ w.t()
    return u, z, l if bias is None else l + bias


def forward(y, sc, sh, act, w, bias, labels, xscale, smoothing):
    """Everything of the forward half; ``sc`` None = no prologue (z = u = y).  ``loss_bound`` is
    the per-row allowance of an fp32 evaluation: 2^-18 (|mx| + |log se| + |l_y| + off sum |l|)."""
    u, z, l = logits(y, sc, sh, act, w, bias)
    NC = w.shape[0]
    tgt, yin = targets(labels, NC, smoothing)
    off = smoothing / NC
    mx = l.amax(1)
    lse = torch.logsumexp(l, 1)
    loss = -(tgt * (l - lse[:, None])).sum(1)
    p = torch.exp(l - lse[:, None])
    d = (p - tgt) * xscale
    am = first_argmax(l)
    hit = yin & (am == labels.to(torch.int64))
    ly = torch.where(yin, l.gather(1, labels.to(torch.int64).clamp(0, NC - 1)[:, None])[:, 0], torch.zeros_like(mx))
    bound = 2.0 ** -18 * (mx.abs() + (lse - mx).abs() + ly.abs() + off * l.abs().sum(1))
    return {"u": u, "z": z, "l": l, "mx": mx, "lse": lse, "tgt": tgt, "yin": yin, "loss": loss, "loss_bound": bound,
            "d": d, "am": am, "hit": hit, "hits": int(hit.sum())}


def backward(z, w, d):
    """What the head's backward takes from a d [M, NC]; ``*_abs`` = each sum's sum |terms|.
    dWt is [ch][cls], as the kernel stores it."""
    return {"db": d.sum(0), "db_abs": d.abs().sum(0), "dWt": z.t() @ d, "dWt_abs": z.abs().t() @ d.abs(),
            "dz": d @ w, "dz_abs": d.abs() @ w.abs()}


def moments(dz, y, u, act):
    """The decoder BN's raw backward moments from a dz [M, K]: g = dz * [u > 0] (relu) or dz."""
    g = dz * (u > 0).to(dz.dtype) if act == ACT_RELU else dz
    return {"g": g, "sg": g.sum(0), "sg_abs": g.abs().sum(0), "sgy": (g * y).sum(0), "sgy_abs": (g * y).abs().sum(0)}


def slab_sums(terms, row_of, nb):
    """[nb, C]: the terms [R, C] added per slab row (workgroup) ``row_of`` [R]."""
    acc = torch.zeros(nb, terms.shape[1], dtype=torch.float64, device=terms.device)
    acc.index_add_(0, row_of.to(terms.device), terms)
    return acc


def row_blocks(M, nb):
    """The workgroup of every row under the kernels' grid-stride tile walk, and tiles per workgroup."""
    tile = torch.arange(M) // TILE
    return tile % nb, (int(tile[-1]) + nb) // nb


# ---------------------------------------------------------------------------
# inputs on dyadic grids
# ---------------------------------------------------------------------------
def _pick(values, shape, gen):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), tuple(shape), generator=gen)]


def _halves(shape, lim, gen):
    k = int(round(lim * 2))
    return torch.randint(-k, k + 1, tuple(shape), generator=gen).to(torch.float64) / 2


def sparse_rows(NC, ncols, gen, nnz=3):
    """[NC, ncols] with at most ``nnz`` entries of {+-1/2, +-1} per row (the rest 0)."""
    r = torch.zeros(NC, ncols, dtype=torch.float64)
    if ncols == 0:
        return r
    for c in range(NC):
        cols = torch.randperm(ncols, generator=gen)[: min(nnz, ncols)]
        r[c, cols] = _pick([0.0, 0.5, -0.5, 1.0, -1.0], (len(cols),), gen)
    return r


def build_general(M, K, NC, act, gen, pro=True, bias=True):
    """y halves |y| <= 2; sc from {0, +-1/2, +-1, +-2}; sh halves |sh| <= 1; bias quarters
    |b| <= 1; w sparse dyadic [NC, K].  ``pro`` False: no prologue (sc = sh = None)."""
    inp = {"M": M, "K": K, "NC": NC, "act": act,
           "y": _halves((M, K), 2.0, gen),
           "sc": _pick([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], (K,), gen) if pro else None,
           "sh": _halves((K,), 1.0, gen) if pro else None,
           "w": sparse_rows(NC, K, gen),
           "bias": torch.randint(-4, 5, (NC,), generator=gen).to(torch.float64) / 4 if bias else None}
    return inp


def build_readout(M, NC, act, gen, bias=True):
    """The readout head of ``seghead_loss`` (which emits dz = d w, not d): w = [P | R] with P a
    permutation matrix on NC of the 32 channels (w[c, perm[c]] = 1, the rest of those columns 0)
    and R sparse dyadic on the other channels, so dz[:, perm[c]] = d[:, c] bit for bit."""
    inp = build_general(M, K_HEAD, NC, act, gen, True, bias)
    order = torch.randperm(K_HEAD, generator=gen)
    perm, rest = order[:NC], order[NC:].sort().values
    w = torch.zeros(NC, K_HEAD, dtype=torch.float64)
    w[:, rest] = sparse_rows(NC, len(rest), gen)
    w[torch.arange(NC), perm] = 1.0
    inp.update(w=w, perm=perm, rest=rest)
    return inp


def build_tied(M, NC, act, gen):
    """Every class row of w the same and a constant bias: every logit of a row is equal, the
    first arg-max is class 0 on every row."""
    inp = build_general(M, K_HEAD, NC, act, gen, True, True)
    inp["w"] = sparse_rows(1, K_HEAD, gen, nnz=6).expand(NC, K_HEAD).contiguous()
    inp["bias"] = torch.full((NC,), 0.25, dtype=torch.float64)
    return inp


def build_uniform(M, NC, act, gen, bias=True):
    """The exact tier: a readout head whose R columns are equal across classes, with
    y[:, perm] constant per row under one (sc, sh) pair and a constant bias -- every logit of
    a row is equal, softmax = 1 / NC, and with NC and xscale powers of two and smoothing 0 or
    1/4, d = (1/NC - tgt) * xscale is a bf16 value."""
    assert NC & (NC - 1) == 0, "uniform logits need a power-of-two class count"
    inp = build_readout(M, NC, act, gen, bias)
    perm, rest = inp["perm"], inp["rest"]
    if len(rest):
        inp["w"][:, rest] = sparse_rows(1, len(rest), gen, nnz=6).expand(NC, len(rest))
    inp["y"][:, perm] = _halves((M, 1), 2.0, gen).expand(M, NC)
    inp["sc"][perm] = float(_pick([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], (1,), gen))
    inp["sh"][perm] = float(_halves((1,), 1.0, gen))
    if bias:
        inp["bias"] = torch.full((NC,), -0.75, dtype=torch.float64)
    return inp


def make_labels(inp, gen, out_of_range=None, mix=True):
    """int64 labels: a quarter of the rows the first arg-max, a quarter the last (a tied row's
    last maximum is a miss), the rest uniform (``mix`` False: all uniform).  ``out_of_range``:
    values dealt to every 8th row (-2 stands for 2^32 + the row's first arg-max)."""
    l = logits(inp["y"], inp["sc"], inp["sh"], inp["act"], inp["w"], inp["bias"])[2]
    f = {"l": l, "am": first_argmax(l)}
    M, NC = inp["M"], inp["NC"]
    lab = torch.randint(0, NC, (M,), generator=gen)
    how = torch.randint(0, 4, (M,), generator=gen)
    if mix:
        lab = torch.where(how == 0, f["am"], lab)
        lab = torch.where(how == 1, last_argmax(f["l"]), lab)
    if out_of_range:
        rows = torch.arange(3, M, 8)
        vals = torch.tensor(out_of_range, dtype=torch.int64)[torch.arange(len(rows)) % len(out_of_range)]
        vals = torch.where(vals == -2, (1 << 32) + f["am"][rows], vals)
        lab[rows] = vals
    return lab


def check_promises(inp, f):
    """What every builder promises of its inputs, asserted on the oracle's forward ``f``: z and the
    logits are bf16 values (so are y and w), and the logit spread of a row is at most 32."""
    for name in ("y", "w"):
        assert torch.equal(bf16_round(inp[name]), inp[name]), f"{name} is not a bf16 tensor"
    assert torch.equal(bf16_round(f["z"]), f["z"]), "z is not bf16-exact"
    assert torch.equal(bf16_round(f["l"]), f["l"]), "the logits are not bf16-exact"
    spread = float((f["l"].amax(1) - f["l"].amin(1)).max())
    assert spread <= 32.0, f"logit spread {spread}"
    return spread


def uniform_d(NC, tgt, xscale):
    """The exact d of the uniform-logit builder."""
    return (1.0 / NC - tgt) * xscale


def uniform_steps(NC, xscale):
    """The grids the exact tier's terms live on: d in multiples of xscale / (4 NC), z in quarters,
    y in halves -> (step of d and dz, step of z * d, step of g * y)."""
    sd = xscale / (4 * NC)
    return sd, sd / 4, sd / 2


def loss_chain(tiles_per_wg, nb):
    """Longest chain of additions behind the summed loss: a thread's rows, the wave sum (6
    shuffles), the 4 waves (2), the workgroups."""
    return tiles_per_wg + 6 + 2 + nb


def mfma_chain(tiles_per_wg, nb):
    """db / dWt: two 32-row MFMA steps per tile and wave, the 4 waves (2), the workgroups."""
    return 64 * tiles_per_wg + 2 + nb


def moment_chain(tiles_per_wg, nb):
    """Moments: 4 rows per tile and lane, 4 shuffles over the 16 lanes, the 4 waves (2), the workgroups."""
    return 4 * tiles_per_wg + 4 + 2 + nb


# ---------------------------------------------------------------------------
# per-workgroup sums, and the judges of a kernel's outputs (shared by the CPU file, which feeds
# them the oracle's own outputs with planted defects, and the GPU file)
# ---------------------------------------------------------------------------
PART_LEN = 2 + 32 + 32 * 32 + 64                 # [loss, hits | db 32 | dWt 32 x 32 | msum 32 | msq 32]
P_DB, P_DW, P_MS, P_MQ = 2, 34, 34 + 1024, 34 + 1024 + 32


def tile_mm(a, b):
    """[tiles, Ca, Cb]: a^T b over the rows of every 256-row tile."""
    M = a.shape[0]
    nt = (M + TILE - 1) // TILE
    pad = nt * TILE - M
    if pad:
        a = torch.cat([a, a.new_zeros(pad, a.shape[1])])
        b = torch.cat([b, b.new_zeros(pad, b.shape[1])])
    return torch.bmm(a.view(nt, TILE, -1).transpose(1, 2), b.view(nt, TILE, -1))


def wg_mm(a, b, nb):
    """[nb, Ca, Cb]: a^T b over the rows of every workgroup (tile t belongs to workgroup t mod nb)."""
    per_tile = tile_mm(a, b)
    out = per_tile.new_zeros(nb, per_tile.shape[1], per_tile.shape[2])
    out.index_add_(0, torch.arange(per_tile.shape[0]) % nb, per_tile)
    return out


def wg_sum(t, nb):
    """[nb, C]: the rows of t [M, C] (or [M]) added per workgroup."""
    t2 = t[:, None] if t.dim() == 1 else t
    r = wg_mm(torch.ones(t2.shape[0], 1, dtype=t2.dtype), t2, nb)[:, 0]
    return r[:, 0] if t.dim() == 1 else r


def tiles_per_wg(M, nb):
    return ((M + TILE - 1) // TILE + nb - 1) // nb


def seq_sum32(part):
    """The workgroup rows of an fp32 slab added in row order, in fp32."""
    acc = part[0].clone()
    for i in range(1, part.shape[0]):
        acc = acc + part[i]
    return acc


def judge_d(d_native, f, xscale, what):
    """Stage 1, d: one bf16 rounding of (softmax - tgt) * xscale.  With a logit spread <= 32 the
    fp32 exponent argument is off by <= 2^-19, e by <= 2^-19.5 relative and softmax <= 1: the
    2^-18 xscale term leaves 2.8x over the fast exp."""
    return check_one_rounding(d_native, f["d"], torch.full_like(f["d"], xscale), what + " d")


def judge_loss(loss_parts, f, M, nb, what):
    """Stage 1, loss: every workgroup's sum and the fp32 total, the per-row allowances added up."""
    t = tiles_per_wg(M, nb)
    a = check_reduction(loss_parts, wg_sum(f["loss"], nb), wg_sum(f["loss"].abs(), nb), t + 6 + 2,
                        what + " loss per workgroup", extra=wg_sum(f["loss_bound"], nb))
    b = check_reduction(loss_parts.to(torch.float32).sum(), f["loss"].sum(), f["loss"].abs().sum(), loss_chain(t, nb),
                        what + " loss total", extra=f["loss_bound"].sum())
    return max(a, b)


def judge_hits(hit_parts, f, nb, what):
    check_exact(hit_parts, wg_sum(f["hit"].to(torch.float64), nb), what + " hits per workgroup")
    assert int(hit_parts.to(torch.float64).sum()) == f["hits"], what + " hits"
    return 0.0


def judge_grads(part, z, d_native, NC, M, nb, what, reduced=None):
    """Stage 2, db and dWt against the oracle at the kernel's own d: every workgroup's row of
    ``part``, the rows added in order in fp32 and (``reduced``) part_reduce's result."""
    t = tiles_per_wg(M, nb)
    K = z.shape[1]
    part = part.to(torch.float64)
    db, dw = part[:, P_DB:P_DB + 32], part[:, P_DW:P_DW + 1024].view(nb, 32, 32)
    check_exact(db[:, NC:], torch.zeros(nb, 32 - NC), what + " db of the padded classes")
    check_exact(dw[:, :, NC:], torch.zeros(nb, 32, 32 - NC), what + " dWt of the padded classes")
    check_exact(dw[:, K:], torch.zeros(nb, 32 - K, 32), what + " dWt of the padded channels")
    rdb, rdb_abs = wg_sum(d_native, nb), wg_sum(d_native.abs(), nb)
    rdw, rdw_abs = wg_mm(z, d_native, nb), wg_mm(z.abs(), d_native.abs(), nb)
    worst = max(check_reduction(db[:, :NC], rdb, rdb_abs, mfma_chain(t, 0), what + " db per workgroup"),
                check_reduction(dw[:, :K, :NC], rdw, rdw_abs, mfma_chain(t, 0), what + " dWt per workgroup"))
    tots = [("row order", seq_sum32(part.to(torch.float32)))]
    if reduced is not None:
        tots.append(("part_reduce", reduced))
    for name, tot in tots:
        tot = tot.to(torch.float64)
        worst = max(worst,
                    check_reduction(tot[P_DB:P_DB + NC], rdb.sum(0), rdb_abs.sum(0), mfma_chain(t, nb), f"{what} db {name}"),
                    check_reduction(tot[P_DW:P_DW + 1024].view(32, 32)[:K, :NC], rdw.sum(0), rdw_abs.sum(0),
                                    mfma_chain(t, nb), f"{what} dWt {name}"))
    return worst


def judge_dz(dz, d_native, w, cols, what):
    """Stage 2, dz = d w on the columns ``cols`` (those outside the readout): one bf16 rounding."""
    return check_one_rounding(dz[:, cols], d_native @ w[:, cols], d_native.abs() @ w[:, cols].abs(), what + " dz")


def judge_moments(part, dz, y, u, act, M, nb, what, reduced=None):
    """Stage 2, the BN moments against the oracle at the kernel's own stored dz."""
    t = tiles_per_wg(M, nb)
    m = moments(dz, y, u, act)
    part = part.to(torch.float64)
    refs = [(P_MS, m["g"], "sum g"), (P_MQ, m["g"] * y, "sum g y")]
    worst = 0.0
    for off, terms, name in refs:
        r, ra = wg_sum(terms, nb), wg_sum(terms.abs(), nb)
        worst = max(worst, check_reduction(part[:, off:off + 32], r, ra, moment_chain(t, 0), f"{what} {name} per workgroup"))
        tots = [seq_sum32(part.to(torch.float32))] + ([reduced] if reduced is not None else [])
        for tot in tots:
            worst = max(worst, check_reduction(tot.to(torch.float64)[off:off + 32], r.sum(0), ra.sum(0),
                                               moment_chain(t, nb), f"{what} {name} total"))
    return worst


def simulate(inp, f, nb):
    """What a correct kernel returns, from the oracle: d and dz rounded to bf16, fp32 partials."""
    d = bf16_round(f["d"])
    dz = bf16_round(d @ inp["w"])
    m = moments(dz, inp["y"], f["u"], inp["act"])
    part = torch.zeros(nb, PART_LEN, dtype=torch.float64)
    NC, K = inp["NC"], inp["K"]
    part[:, 0] = wg_sum(f["loss"], nb)
    part[:, 1] = wg_sum(f["hit"].to(torch.float64), nb)
    part[:, P_DB:P_DB + NC] = wg_sum(d, nb)
    part[:, P_DW:P_DW + 1024].view(nb, 32, 32)[:, :K, :NC] = wg_mm(f["z"], d, nb)
    part[:, P_MS:P_MS + K] = wg_sum(m["g"], nb)
    part[:, P_MQ:P_MQ + K] = wg_sum(m["g"] * inp["y"], nb)
    return {"d": d, "dz": dz, "part": part.to(torch.float32)}


def judge_all(inp, f, out, xscale, nb, what, hits=True, reduced=None):
    """Both stages on the outputs ``out`` = {d, dz, part} of a readout-head case; returns
    {check: worst error / bound}."""
    M, NC = inp["M"], inp["NC"]
    d, dz, part = out["d"].to(torch.float64), out["dz"].to(torch.float64), out["part"]
    res = {"d": judge_d(d, f, xscale, what), "loss": judge_loss(part[:, 0], f, M, nb, what)}
    if hits:
        res["hits"] = judge_hits(part[:, 1], f, nb, what)
    res["db/dWt"] = judge_grads(part, f["z"], d, NC, M, nb, what, reduced)
    if len(inp["rest"]):
        res["dz"] = judge_dz(dz, d, inp["w"], inp["rest"], what)
    res["moments"] = judge_moments(part, dz, inp["y"], f["u"], inp["act"], M, nb, what, reduced)
    return res


def exact_tier_preconditions(inp, f, d, xscale, nb):
    """The exact tier (``build_uniform``): every term of every sum is a multiple of a power of
    two and no sum of |terms| -- of a workgroup, or of the whole slab -- reaches 2^24 of them, so
    every fp32 partial sum is exact in any order.  Returns the worst fraction of 2^24 steps."""
    sd = xscale / (4 * inp["NC"])                # d; z in quarters, w and y in halves
    dz = d @ inp["w"]
    assert torch.equal(bf16_round(dz), dz), "the uniform dz is not a bf16 value"
    g = moments(dz, inp["y"], f["u"], inp["act"])["g"]
    ones = torch.ones(inp["M"], 1, dtype=torch.float64)
    worst = 0.0
    for terms, step in ((tile_mm(ones, d.abs()), sd), (tile_mm(f["z"].abs(), d.abs()), sd / 4),
                        (tile_mm(ones, g.abs()), sd / 2), (tile_mm(ones, (g * inp["y"]).abs()), sd / 4)):
        assert bool((terms / step == torch.round(terms / step)).all()), "terms off their grid"
        flat = terms.reshape(terms.shape[0], -1)
        tile = torch.arange(flat.shape[0])
        worst = max(worst, slab_rows_exact(flat, tile % nb, nb, step), slab_rows_exact(flat, tile * 0, 1, step))
    return worst


def judge_exact(inp, f, d, out, nb, what, reduced=None):
    """The exact tier: d, dz, hits, db, dWt and the moments bit for bit -- per workgroup, added in
    row order and through part_reduce -- and the loss under its stage-1 bound."""
    ref = simulate(inp, dict(f, d=d), nb)
    check_exact(out["d"], d, what + " d")
    check_exact(out["dz"], ref["dz"], what + " dz")
    check_exact(out["part"][:, 1:], ref["part"][:, 1:], what + " part")
    tot = ref["part"].to(torch.float64).sum(0)[1:]
    check_exact(seq_sum32(out["part"])[1:], tot, what + " part in row order")
    if reduced is not None:
        check_exact(reduced[1:], tot, what + " part_reduce")
    return judge_loss(out["part"][:, 0], f, inp["M"], nb, what)


# ---------------------------------------------------------------------------
# the case tables shared by the CPU and the GPU file
# ---------------------------------------------------------------------------
def _sh(name, act, NC, bias=True, smoothing=0.0, hits=1, xone=False, inst=""):
    return {"name": name, "act": act, "NC": NC, "bias": bias, "smoothing": smoothing, "hits": hits, "xone": xone,
            "inst": inst}


# seghead_loss: every case runs with int64 and with uint8 labels (T = long long / unsigned char) at
# the four M values; ``inst`` is the SH_LAUNCH instance the host dispatch picks.  xone: xscale = 1.
SEGHEAD_CASES = [
    _sh("relu-nc25-lean", ACT_RELU, 25, hits=0, inst="<ACT_RELU, T, 25, false>"),
    _sh("none-nc25-lean-nobias", ACT_NONE, 25, bias=False, hits=0, inst="<ACT_NONE, T, 25, false>"),
    _sh("relu-nc25-smooth", ACT_RELU, 25, smoothing=0.125, inst="<ACT_RELU, T, 25>"),
    _sh("relu-nc25-smooth-nohits", ACT_RELU, 25, bias=False, smoothing=0.125, hits=0, inst="<ACT_RELU, T, 25>"),
    _sh("none-nc25-hits", ACT_NONE, 25, inst="<ACT_NONE, T, 25>"),
    _sh("relu-nc2", ACT_RELU, 2, inst="<ACT_RELU, T> NC 2"),
    _sh("none-nc2-nohits", ACT_NONE, 2, bias=False, hits=0, inst="<ACT_NONE, T> NC 2 (no lean instance: hits counted)"),
    _sh("none-nc3-smooth", ACT_NONE, 3, smoothing=0.125, inst="<ACT_NONE, T> NC 3"),
    _sh("relu-nc16-nobias", ACT_RELU, 16, bias=False, inst="<ACT_RELU, T> NC 16"),
    _sh("none-nc17-smooth", ACT_NONE, 17, smoothing=0.125, inst="<ACT_NONE, T> NC 17"),
    _sh("relu-nc17-xscale1", ACT_RELU, 17, xone=True, inst="<ACT_RELU, T> NC 17, xscale 1"),
    _sh("relu-nc24-smooth", ACT_RELU, 24, smoothing=0.125, inst="<ACT_RELU, T> NC 24"),
    _sh("none-nc32", ACT_NONE, 32, inst="<ACT_NONE, T> NC 32 (no padded class)"),
    _sh("relu-nc32-smooth-nobias", ACT_RELU, 32, bias=False, smoothing=0.125, inst="<ACT_RELU, T> NC 32"),
]
EXACT_CASES = [(NC, act, s) for NC in (2, 8, 32) for act in (ACT_NONE, ACT_RELU) for s in (0.0, 0.25)]


def _xe(K, N, pro, bias, smoothing):
    """pro: None = plain input (PRO = -1), else the prologue's activation."""
    p = "plain" if pro is None else "bn-" + ACT_NAMES[pro]
    return {"name": f"k{K}-n{N}-{p}-{'bias' if bias else 'nobias'}-s{smoothing}", "K": K, "NC": N, "pro": pro,
            "bias": bias, "smoothing": smoothing,
            "inst": f"pw_fwd_kernel<32, 32, ACT_NONE, {str(bias).lower()}, {-1 if pro is None else pro}, -1, true>"}


# pw_fwd_xent: (K, N) x prologue none / BN / BN + ReLU x bias x smoothing, every variant of the
# (HAS_BIAS, PRO) template pair named at least once
XENT_CASES = [
    _xe(32, 25, None, True, 0.0), _xe(32, 25, ACT_NONE, True, 0.125), _xe(32, 25, ACT_RELU, True, 0.0),
    _xe(32, 25, None, False, 0.125), _xe(32, 25, ACT_NONE, False, 0.0), _xe(32, 25, ACT_RELU, False, 0.125),
    _xe(32, 2, ACT_RELU, True, 0.125), _xe(32, 2, None, False, 0.0),
    _xe(16, 3, ACT_NONE, True, 0.0), _xe(16, 3, ACT_RELU, False, 0.125), _xe(16, 3, None, True, 0.125),
    _xe(8, 32, ACT_RELU, True, 0.0), _xe(8, 32, ACT_NONE, False, 0.125), _xe(8, 32, None, True, 0.0),
    _xe(6, 5, None, True, 0.125), _xe(6, 5, None, False, 0.0),
]


def m_values(nb_big):
    """One ragged tile, one full tile, a full and a ragged one, and a workgroup that walks two
    tiles with the prefetch in flight (``nb_big``: the grid of a large launch)."""
    return [8, 256, 264, TILE * (nb_big + 1) + 8]
