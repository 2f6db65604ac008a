"""A plain float64 oracle of the BN and pooling kernels (``csrc/kernels/bn_pool.hip``).

Everything here is elementwise arithmetic, padding, ``unfold`` / reshape and reductions on
float64 tensors -- no library pooling or batch-norm op -- so it shares no code with the kernels
it judges, nor with ``ops/reference.py``.  It runs wherever its inputs live (CPU, or the GPU
for the one large case).

Activations are channels-last ``[N, D, H, W, C]``; a pooling geometry is a ``PoolSpec``.

Besides every result the oracle returns its *magnitude*: the sum of the absolute values of the
terms that are added before the kernel's final rounding.  The comparison helpers at the end
are written against it:

* ``check_exact``        -- bit-for-bit (inputs on dyadic grids: see ``grid``);
* ``check_one_rounding`` -- ``|a - r| <= 2^-8 |r| + 2^-18 magnitude`` (bf16's half ulp 2^-9,
  doubled for double rounding, plus the few fp32 roundings in front of it);
* ``check_reduction``    -- ``|a - r| <= (n + 8) 2^-24 sum|terms|`` for an fp32 sum whose
  longest chain of additions has n links.

Each returns the largest observed error as a fraction of its bound and raises
``AssertionError`` above 1 (a NaN counts as above).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_TANH: "tanh", ACT_SIGMOID: "sigmoid"}


# ---------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------
def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """float64 -> the float64 value of its bf16 rounding (through fp32, as the kernels store)."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def bf16_ulp(t: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 (8 significant bits) at |t|, float64."""
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def grid(shape, step: float, lim: float, gen: torch.Generator) -> torch.Tensor:
    """float64 multiples of ``step`` in [-lim, lim], uniform, on the generator's device."""
    k = int(round(lim / step))
    return torch.randint(-k, k + 1, tuple(shape), generator=gen, device=gen.device).to(torch.float64) * step


# ---------------------------------------------------------------------------
# the prologue: z = act(y * scale + shift), act' through z (common.h)
# ---------------------------------------------------------------------------
def act_fwd(u: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == ACT_TANH:
        return torch.tanh(u)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-u))
    return u


def act_bwd_from_out(z: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)               # relu' at 0 is 0
    if act == ACT_TANH:
        return 1.0 - z * z
    if act == ACT_SIGMOID:
        return z * (1.0 - z)
    return torch.ones_like(z)


def act_bwd_mag(z: torch.Tensor, act: int) -> torch.Tensor:
    """Sum of the absolute terms act' is added up from: 1 - z^2 -> 1 + z^2, z - z^2 -> |z| + z^2."""
    if act == ACT_TANH:
        return 1.0 + z * z
    if act == ACT_SIGMOID:
        return z.abs() + z * z
    return act_bwd_from_out(z, act)


def prologue(y: torch.Tensor, scale, shift, act: int):
    """(z, act'(z)); ``scale`` None = no prologue at all (z = y, act' = 1), as the kernels
    treat a null scale pointer.  scale / shift broadcast over the last (channel) dim."""
    if scale is None:
        return y, torch.ones_like(y)
    z = act_fwd(y * scale + shift, act)
    return z, act_bwd_from_out(z, act)


# ---------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------
def _hi_pads(s):
    return (max((s.OD - 1) * s.sd + s.KD - s.D - s.pd, 0), max((s.OH - 1) * s.sh + s.KH - s.H - s.ph, 0),
            max((s.OW - 1) * s.sw + s.KW - s.W - s.pw, 0))


def windows(x5: torch.Tensor, s, fill: float) -> torch.Tensor:
    """[N, OD, OH, OW, C, KD*KH*KW]: every window's members in (kd, kh, kw) scan order; positions
    outside the input hold ``fill``."""
    hd, hh, hw = _hi_pads(s)
    xp = F.pad(x5, (0, 0, s.pw, hw, s.ph, hh, s.pd, hd), value=fill)
    w = xp.unfold(1, s.KD, s.sd).unfold(2, s.KH, s.sh).unfold(3, s.KW, s.sw)[:, : s.OD, : s.OH, : s.OW]
    return w.reshape(x5.shape[0], s.OD, s.OH, s.OW, x5.shape[4], s.KD * s.KH * s.KW)


def valid_mask(s, device="cpu") -> torch.Tensor:
    """[1, OD, OH, OW, 1, K] float64: 1 where the window member lies inside the input."""
    return windows(torch.ones(1, s.D, s.H, s.W, 1, dtype=torch.float64, device=device), s, 0.0)


def _fold(dwin: torch.Tensor, s) -> torch.Tensor:
    """Adjoint of ``windows``: add every window member back onto its input position
    (overlapping windows accumulate, uncovered inputs stay 0, padded positions are cut off)."""
    hd, hh, hw = _hi_pads(s)
    N, C = dwin.shape[0], dwin.shape[4]
    out = torch.zeros(N, s.D + s.pd + hd, s.H + s.ph + hh, s.W + s.pw + hw, C, dtype=dwin.dtype, device=dwin.device)
    k = 0
    for kd in range(s.KD):
        for kh in range(s.KH):
            for kw in range(s.KW):
                out[:, kd: kd + s.sd * s.OD: s.sd, kh: kh + s.sh * s.OH: s.sh, kw: kw + s.sw * s.OW: s.sw] += dwin[..., k]
                k += 1
    return out[:, s.pd: s.pd + s.D, s.ph: s.ph + s.H, s.pw: s.pw + s.W].contiguous()


def pool_fwd(z5: torch.Tensor, s, kind: str, count_pad: bool = False, tie: str = "first") -> dict:
    """out, mag [N, OD, OH, OW, C]; ``sel`` [.., K]: what each window member receives of the
    window's output gradient (the arg-max indicator, or valid / divisor)."""
    K = s.KD * s.KH * s.KW
    if kind == "max":
        win = windows(z5, s, float("-inf"))      # padded positions never win
        out = win.amax(-1)
        eq = win == out.unsqueeze(-1)
        cs = eq.to(torch.int32).cumsum(-1)
        pick = (cs == 1) if tie == "first" else (cs == cs[..., -1:])
        return {"out": out, "mag": out.abs(), "sel": (eq & pick).to(z5.dtype), "win": win}
    win = windows(z5, s, 0.0)
    valid = valid_mask(s, z5.device)
    div = torch.full_like(valid[..., 0], float(K)) if count_pad else valid.sum(-1).clamp_min(1.0)
    return {"out": win.sum(-1) / div, "mag": win.abs().sum(-1) / div, "sel": valid / div.unsqueeze(-1), "win": win}


def pool_bwd(dout5: torch.Tensor, s, sel: torch.Tensor) -> dict:
    """dx, mag [N, D, H, W, C] from the forward's ``sel``."""
    dwin = dout5.unsqueeze(-1) * sel
    return {"dx": _fold(dwin, s), "mag": _fold(dwin.abs(), s)}


def window_gap(win: torch.Tensor) -> float:
    """Smallest difference between the two largest DISTINCT candidates of any window (inf when
    every window is constant): the near-tie precondition of the tanh / sigmoid cases."""
    top = win.amax(-1, keepdim=True)
    second = torch.where(win < top, win, torch.full_like(win, float("-inf"))).amax(-1, keepdim=True)
    gap = (top - second).flatten()
    gap = gap[torch.isfinite(gap)]
    return float(gap.min()) if gap.numel() else float("inf")


# ---------------------------------------------------------------------------
# batch norm
# ---------------------------------------------------------------------------
def bn_stats(y2: torch.Tensor) -> dict:
    """mean, biased var, unbiased var of the rows of [M, C]."""
    M = y2.shape[0]
    mean = y2.sum(0) / M
    var = ((y2 - mean) ** 2).sum(0) / M
    return {"mean": mean, "var": var, "unbiased": var * M / (M - 1) if M > 1 else var}


def bn_running(run: torch.Tensor, stat: torch.Tensor, momentum: float) -> torch.Tensor:
    return (1.0 - momentum) * run + momentum * stat


def bn_params(mean, var, gamma, beta, eps: float) -> dict:
    invstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones_like(mean) if gamma is None else gamma
    b = torch.zeros_like(mean) if beta is None else beta
    scale = g * invstd
    return {"mean": mean, "invstd": invstd, "scale": scale, "shift": b - mean * scale,
            "shift_mag": b.abs() + (mean * scale).abs()}


def bn_bwd_sums(g2: torch.Tensor, y2: torch.Tensor, mean, invstd, g_abs=None) -> dict:
    """dbeta = sum g, dgamma = sum g*xhat, the raw moments (sum g, sum g*y), and each sum's
    sum of absolute terms (``*_abs``; ``g_abs``: the magnitude of g where g = dz * act' is itself
    a difference, see ``act_bwd_mag``)."""
    xhat = (y2 - mean) * invstd
    ga = g2.abs() if g_abs is None else g_abs
    return {"dbeta": g2.sum(0), "dgamma": (g2 * xhat).sum(0), "sg": g2.sum(0), "sgy": (g2 * y2).sum(0),
            "dbeta_abs": ga.sum(0), "dgamma_abs": (ga * xhat.abs()).sum(0), "sg_abs": ga.sum(0),
            "sgy_abs": (ga * y2.abs()).sum(0)}


def bn_dy(g: torch.Tensor, y: torch.Tensor, scale, mean, invstd, dbeta, dgamma, inv_count: float, g_abs=None) -> dict:
    """dy = k1*g + k2*y + k3 (channels last); the three terms, their sum, and the magnitude
    (k3 counted by its own two terms, g by ``g_abs`` when given)."""
    k2 = -scale * invstd * dgamma * inv_count
    k3a = -scale * dbeta * inv_count
    k3b = scale * mean * invstd * dgamma * inv_count
    t1, t2, t3 = scale * g, k2 * y, (k3a + k3b).expand_as(y)
    t1m = t1.abs() if g_abs is None else (scale * g_abs).abs()
    return {"t1": t1, "t2": t2, "t3": t3, "dy": t1 + t2 + t3,
            "mag": t1m + t2.abs() + (k3a.abs() + k3b.abs()).expand_as(y)}


# ---------------------------------------------------------------------------
# comparison helpers: return the worst error / bound, raise above 1
# ---------------------------------------------------------------------------
def _f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float64)


def check_exact(a: torch.Tensor, r: torch.Tensor, what: str = "") -> float:
    a, r = _f64(a), _f64(r).to(a.device)
    assert a.shape == r.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(r.shape)}"
    bad = ~(a == r)                              # (NaN is never equal)
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {a.numel()} differ; first at flat {i}: "
                             f"got {a.flatten()[i].item()!r} want {r.flatten()[i].item()!r}")
    return 0.0


def _worst(err: torch.Tensor, bound: torch.Tensor, what: str, keep=None) -> float:
    ok = err <= bound                            # (False for NaN)
    if keep is not None:
        ok = ok | ~keep
    if not bool(ok.all()):
        i = int((~ok).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {err.numel()} above the bound; first at flat {i}: "
                             f"err {err.flatten()[i].item():.3e} bound {bound.flatten()[i].item():.3e}")
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    if keep is not None:
        frac = torch.where(keep, frac, torch.zeros_like(frac))
    return float(frac.max()) if frac.numel() else 0.0


def check_one_rounding(a, r, mag, what: str = "", keep=None, extra=None) -> float:
    """One bf16 rounding of a value built from a few fp32 terms.  ``keep``: elements to judge;
    ``extra``: what the (bounded) error of the value's own inputs adds, per element."""
    a = _f64(a)
    r, mag = _f64(r).to(a.device), _f64(mag).to(a.device)
    assert a.shape == r.shape == mag.shape, f"{what}: shapes {tuple(a.shape)} {tuple(r.shape)} {tuple(mag.shape)}"
    bound = 2.0 ** -8 * r.abs() + 2.0 ** -18 * mag
    if extra is not None:
        bound = bound + _f64(extra).to(a.device)
    return _worst((a - r).abs(), bound, what, keep)


def check_reduction(a, r, sum_abs, n: int, what: str = "", extra=None) -> float:
    """An fp32 sum through a chain of n additions; ``extra`` widens the bound per element."""
    a = _f64(a)
    r, sum_abs = _f64(r).to(a.device), _f64(sum_abs).to(a.device)
    assert a.shape == r.shape == sum_abs.shape, f"{what}: shapes {tuple(a.shape)} {tuple(r.shape)}"
    bound = (n + 8) * 2.0 ** -24 * sum_abs
    if extra is not None:
        bound = bound + _f64(extra).to(a.device)
    return _worst((a - r).abs(), bound, what)


def check_fp32(a, r, ulps: float, what: str = "", mag=None, extra=None) -> float:
    """An fp32 result of a float64 computation: ``ulps`` fp32 ulps (2^-23) of max(|r|, mag), plus
    ``extra`` (the float64 side's own cancellation)."""
    a = _f64(a)
    r = _f64(r).to(a.device)
    ref = r.abs() if mag is None else torch.maximum(r.abs(), _f64(mag).to(a.device))
    bound = ulps * 2.0 ** -23 * ref
    if extra is not None:
        bound = bound + _f64(extra).to(a.device)
    return _worst((a - r).abs(), bound, what)


def slab_rows_exact(abs_terms: torch.Tensor, row_of: torch.Tensor, nb: int, step: float) -> float:
    """Precondition of the exact slab checks: with every term a multiple of ``step``, an fp32
    partial sum inside one slab row is exact while the row's sum |terms| / step stays below
    2^24.  ``abs_terms`` [R, C] float64, ``row_of`` [R] the slab row (workgroup) that adds term
    row r.  Returns the largest row sum / (2^24 step); asserts it is below 1."""
    acc = torch.zeros(nb, abs_terms.shape[1], dtype=torch.float64, device=abs_terms.device)
    acc.index_add_(0, row_of.to(abs_terms.device), abs_terms)
    worst = float(acc.max()) / (2.0 ** 24 * step)
    assert worst < 1.0, f"slab rows are not exactly summable: {worst:.3f} of 2^24 steps"
    return worst


# ---------------------------------------------------------------------------
# the geometry table shared by the CPU and the GPU file
#   shape N, D, H, W, C | kernel | stride (None = kernel) | padding | kinds
#   dagger: also tanh / sigmoid | stats: pool_bwd_stats_blocks > 0 | fused: pool_bn_bwd_apply
#   takes it (else it refuses with -2) | kernels: what the host dispatch picks
# ---------------------------------------------------------------------------
def _case(name, shape, kernel, stride=None, padding="valid", kinds=("max",), dagger=False, stats=False,
          fused=False, count_pad=(False,), kernels=""):
    return {"name": name, "shape": shape, "kernel": kernel, "stride": stride, "padding": padding, "kinds": kinds,
            "dagger": dagger, "stats": stats, "fused": fused, "count_pad": count_pad, "kernels": kernels}


POOL_CASES = [
    _case("cube2_c64", (2, 8, 8, 8, 64), 2, kinds=("max", "avg"), dagger=True, stats=True, fused=True,
          kernels="pool2_fwd<2>, pool_bwd_tiled<8>, pool_bn_moments8<int>, pool_bn_bwd_apply<int>"),
    _case("flat2_c32", (3, 1, 10, 12, 32), (1, 2, 2), dagger=True, stats=True, fused=True,
          kernels="pool2_fwd<1>, pool_bwd_tiled<8>, pool_bn_moments8<int>, pool_bn_bwd_apply<int>"),
    _case("odd2_c16", (2, 9, 7, 11, 16), 2, kinds=("max", "avg"),
          kernels="pool2_fwd<2> on odd extents, gather pool_bwd<8> (zeroes the uncovered planes)"),
    _case("cube2_c24", (2, 6, 6, 6, 24), 2, kernels="cpr 3: pool_fwd<8>, pool_bwd_tiled<8>, no stats"),
    _case("cube2_c40", (2, 6, 6, 6, 40), 2, kernels="cpr 5: pool_fwd<8>, pool_bwd_tiled<8>, no stats"),
    _case("win6_c8", (2, 4, 6, 8, 8), (1, 3, 2), dagger=True, stats=True, fused=True,
          kernels="pool_fwd<8>, pool_bwd_tiled<8>, moments8 / apply with 6 of 8 window lanes"),
    _case("win8_c8", (2, 4, 6, 8, 8), (1, 2, 4), dagger=True, stats=True, fused=True,
          kernels="pool_fwd<8>, pool_bwd_tiled<8>, moments8 / apply with 8 window lanes (1x2x4)"),
    _case("win2w_c8", (2, 4, 6, 8, 8), (1, 1, 2), dagger=True, stats=True, fused=True,
          kernels="pool_fwd<8>, pool_bwd_tiled<8>, moments8 / apply with 2 of 8 window lanes"),
    _case("win2d_c8", (2, 4, 6, 8, 8), (2, 1, 1), dagger=True, stats=True, fused=True,
          kernels="pool_fwd<8>, pool_bwd_tiled<8>, moments8 / apply with 2 of 8 window lanes (along D)"),
    _case("cube3_c16", (2, 6, 6, 6, 16), 3, stats=True,
          kernels="27 positions: pool_fwd<8>, pool_bwd_tiled<8>, pool_bwd_stats -> pool_bwd_tiled<8,true>"),
    _case("over3_s2_same_c16", (2, 1, 9, 9, 16), (1, 3, 3), (1, 2, 2), "same", kinds=("max", "avg"),
          kernels="padded, overlapping: pool_fwd<8>, gather pool_bwd<8>"),
    _case("over2_s1_c18", (2, 1, 9, 9, 18), (1, 2, 2), 1, kernels="overlapping: pool_fwd<1>, gather pool_bwd<2>"),
    _case("over2_s1_c6", (2, 1, 9, 9, 6), (1, 2, 2), 1, kernels="overlapping: pool_fwd<1>, gather pool_bwd<2>"),
    _case("over2_s1_c3", (2, 1, 9, 9, 3), (1, 2, 2), 1, kernels="overlapping: pool_fwd<1>, gather pool_bwd<1>"),
    _case("sub_k1_s2_c16", (4, 1, 8, 8, 16), 1, (1, 2, 2), kernels="subsample: pool_fwd<8>, gather pool_bwd<8>"),
    _case("avg3_s1_same_c16", (3, 1, 9, 9, 16), (1, 3, 3), 1, "same", kinds=("avg",), count_pad=(False, True),
          kernels="border divisors: pool_fwd<8>, gather pool_bwd<8>"),
    _case("avg2_same_c6", (2, 1, 7, 7, 6), (1, 2, 2), None, "same", kinds=("avg",),
          kernels="border divisors: pool_fwd<1>, gather pool_bwd<2>"),
    _case("gap_c40", (3, 4, 5, 6, 40), (4, 5, 6), kinds=("avg",),
          kernels="global average, 120 positions: pool_fwd<8>, pool_bwd_tiled<8>"),
    _case("gap_c5", (3, 4, 5, 6, 5), (4, 5, 6), kinds=("avg",),
          kernels="global average, 120 positions: pool_fwd<1>, pool_bwd_tiled<1>"),
]
# 2,112,000 windows > 8192 * 256: the second grid-stride round (GPU file; its geometry at N = 1 here)
LARGE_CASE = _case("large_c8", (33, 80, 80, 80, 8), 2, stats=True, fused=True,
                   kernels="second round of pool2_fwd<2>, pool_bwd_tiled<8>, moments8<int>, apply<int>")


def make_spec(case, N=None):
    from featurenet_amd.ops.spec import PoolSpec

    shape = tuple(case["shape"])
    if N is not None:
        shape = (N,) + shape[1:]
    return PoolSpec.make(shape, case["kernel"], case["stride"], case["padding"])
