"""A plain float64 oracle of the Dense kernels (``csrc/kernels/dense.hip``), the inputs that make
them exact, the case table, and a Python mirror of the launchers' arithmetic.

The oracle is float64 ``matmul`` and nothing else -- no ``torch.nn.functional.linear``, no
autograd, nothing from ``ops/``:

    y  = act(x @ bf16_round(w).T + b)
    dx = g' @ bf16_round(w)
    dW = g'.T @ x
    db = g'.sum(0)
    g' = bf16_round(dy * act_bwd_from_out(ya))  when ya is given (one rounding, as the kernels'
         ``f2bf`` when they load g), else dy

Why the comparisons need no tolerance
-------------------------------------
Every input lies on a dyadic grid (``make_inputs``):

* ``x``, ``dy``  integers in [-4, 4] (bf16 values)
* ``w``     the fp32 master weights: multiples of 2^-9 in [-1, 1], never zero (a zero weight
  hides a mis-addressed product).  Deliberately NOT all bf16 values: an odd multiple of 2^-9
  with magnitude in (1/2, 1) has nine significant bits and lies exactly half way between two
  bf16 values, so the kernels' in-loop conversion (``dn_cvt8``, ``f2bf`` in the dgrad staging)
  has to round, and every rounding is a tie.  A quarter of a uniform draw is such a value;
  ``bf16_round(w)`` is still a multiple of 2^-9 with |w| <= 1.  The bf16 weight copy of the
  inference path (``wbf16 = 1``) is ``bf16_round(w)``.
* ``bias``  multiples of 1/4 in [-1, 1]
* ``ya``    (the activation output handed to the backward entry points) relu: zero or a multiple
  of 1/4 in (0, 4]; tanh: multiples of 1/8 in [-1, 1]; sigmoid: multiples of 1/8 in [0, 1].
  ``1 - y^2`` and ``y (1 - y)`` are then multiples of 1/64, exact in fp32; the product with dy
  is a multiple of 1/64 of magnitude <= 4, of which ``g'`` is one defined rounding.

So every partial sum of a result, in any order, is a multiple of the result's step
(``step_of``): y 2^-9 (the bias 2^-2); dx 2^-9, or 2^-15 with ``ya``; dW and db 1, or 1/64
with ``ya``.  An fp32 sum of multiples of ``step`` is exact while ``sum |terms| / step < 2^24``
(``exact_margin``); the oracle returns ``sum |terms|`` of every sum as ``*_abs`` and
tests/test_dense_oracle_cpu.py asserts the condition for every case and quantity.

Exact quantities (``check_exact``): y and dx = ``bf16_round(oracle)``; y = the oracle as fp32
with ``out_fp32``; dW and db = the oracle as fp32.

Bounded quantities (``BOUNDED``, as ``(case, quantity)``): the tanh and the sigmoid forward
epilogue.  Their argument is the exact fp32 sum; what remains is ``tanhf`` / ``1 / (1 +
__expf(-u))`` and the output rounding.  Both are judged by ``check_one_rounding`` with the
magnitude |r| and no ``extra`` term -- the bound ``tests/_conv_oracle.py`` gives ``y_tanh`` and
``tests/test_bn_pool_oracle_gpu.py`` gives ``bn_apply`` with tanh and sigmoid.  The latter's
inputs keep |u| <= 4; here |u| exceeds a hundred (below ``SOFT_ARG_LIMIT``, asserted on the CPU).
``__expf(-u)`` is ``exp2(-u log2 e)``: one fp32 rounding of the product shifts the exponent by
at most |u| log2(e) 2^-24, a relative error of |u| 2^-24 in the result, 2^-16 at |u| = 192, next
to a few ulps of the hardware exp2, the add and the divide -- the bound's 2^-8 |r| is over two
hundred times that, so it carries over unchanged.  A relative bound speaks of normal numbers only: where
sigmoid(u) < 2^-126 (u < -87.3; ``__expf`` overflows to infinity from 88.7 on and the kernel
gives 0) the output is only required to lie in [0, 2^-125] (``SOFT_TINY``).  tanh saturates to
+-1 exactly on both sides.  profiles/dense_oracle.md records the observed worst error over the
bound.

``dense_wgrad_kernel<2>`` is unreachable (``nb`` is the constant 1 in ``fn_dense_wgrad``) and is
not tested.
"""
from __future__ import annotations

import zlib

import torch

from _bn_pool_oracle import (ACT_NAMES, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, act_bwd_from_out, act_fwd,  # noqa: F401
                             bf16_round, grid)
from _conv_oracle import BAND, SENTINEL, banded  # noqa: F401  (re-exported)

NONE, RELU, TANH, SIGMOID = ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID
W_STEP = 2.0 ** -9
SOFT_ARG_LIMIT = 192.0                           # |u| of every tanh / sigmoid forward case stays below
SOFT_TINY = 2.0 ** -126                          # smallest normal bf16 / fp32 value


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def g_prime(dy: torch.Tensor, ya, act: int) -> torch.Tensor:
    return dy if ya is None else bf16_round(dy * act_bwd_from_out(ya, act))


def forward(x: torch.Tensor, w: torch.Tensor, b, act: int = NONE) -> dict:
    """``pre`` = x @ bf16_round(w).T + b, ``y`` = act(pre), ``y_abs`` = sum |terms| of pre."""
    assert x.dtype == w.dtype == torch.float64
    wr = bf16_round(w)
    pre = x @ wr.T
    mag = x.abs() @ wr.abs().T
    if b is not None:
        pre, mag = pre + b, mag + b.abs()
    return {"pre": pre, "y": act_fwd(pre, act), "y_abs": mag}


def backward(x, w, gp: torch.Tensor, want=("dx", "dW")) -> dict:
    """dx [M, K], dW [N, K], db [N] of the gradient ``gp`` (= g') at the layer's pre-activation,
    each with its ``*_abs``."""
    out = {"db": gp.sum(0), "db_abs": gp.abs().sum(0)}
    if "dx" in want:
        wr = bf16_round(w)
        out["dx"], out["dx_abs"] = gp @ wr, gp.abs() @ wr.abs()
    if "dW" in want:
        out["dW"], out["dW_abs"] = gp.T @ x, gp.abs().T @ x.abs()
    return out


def step_of(q: str, ya: bool = False) -> float:
    if q == "y":
        return W_STEP
    if q == "dx":
        return 2.0 ** -15 if ya else W_STEP
    return 1.0 / 64 if ya else 1.0               # dW, db


def exact_margin(sum_abs: torch.Tensor, step: float) -> float:
    """Largest sum |terms| / (2^24 step): below 1, an fp32 sum of multiples of ``step`` is exact
    in any order."""
    return float(sum_abs.max()) / (2.0 ** 24 * step)


def on_grid(t: torch.Tensor, step: float) -> bool:
    return bool(((t / step).round() * step == t).all())


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def make_w(N: int, K: int, g: torch.Generator) -> torch.Tensor:
    w = grid((N, K), W_STEP, 1.0, g)
    # no zero weight; the replacement, 257 / 512, is itself a tie between two bf16 values
    return torch.where(w == 0, torch.full_like(w, 257 * W_STEP), w)


def make_ya(M: int, N: int, act: int, g: torch.Generator) -> torch.Tensor:
    if act == RELU:
        pos = torch.randint(1, 17, (M, N), generator=g).to(torch.float64) / 4
        return pos * torch.randint(0, 2, (M, N), generator=g).to(torch.float64)
    if act == TANH:
        return grid((M, N), 1 / 8, 1.0, g)
    assert act == SIGMOID
    return torch.randint(0, 9, (M, N), generator=g).to(torch.float64) / 8


def make_inputs(case: dict, need=("x", "w", "b", "dy", "ya")) -> dict:
    """float64 inputs of a case on the grids of the module docstring (CPU).  Every tensor has a
    generator of its own (seeded by the shape and the tensor's name), so cases of one shape
    share their data and a tensor that is not needed is not drawn."""
    M, N, K = case["M"], case["N"], case["K"]
    tag = f"dense-{M}-{N}-{K}"
    out = {}
    if "x" in need:
        out["x"] = grid((M, K), 1.0, 4.0, gen(tag + ":x"))
    if "w" in need:
        out["w"] = make_w(N, K, gen(tag + ":w"))
    if "b" in need:
        out["b"] = grid((N,), 0.25, 1.0, gen(tag + ":b"))
    if "dy" in need:
        out["dy"] = grid((M, N), 1.0, 4.0, gen(tag + ":dy"))
    if "ya" in need and case.get("ya"):
        out["ya"] = make_ya(M, N, case["ya"], gen(tag + f":ya{case['ya']}"))
    return out


# ---------------------------------------------------------------------------
# a mirror of the launchers' arithmetic (dense.hip, "host launchers")
# ---------------------------------------------------------------------------
def dn_ncw(M, N, K):
    if N <= 64 or M <= 128:
        return 1
    if K < 512 and -(-N // 128) * -(-M // 128) < 256:
        return 1
    return 2


def dense_splits(M, N, K):
    """fn_dense_splits."""
    ncw = dn_ncw(M, N, K)
    tiles = -(-N // (64 * ncw)) * -(-M // 128)
    target = 256 if M <= 128 else 512 // ncw
    S = -(-target // tiles)
    maxS = max(K // 256, 1)
    return max(1, min(S, maxS))


def dense_wgrad_slices(M, N, K):
    """fn_dense_wgrad_slices."""
    tiles = -(-K // 64) * -(-N // 64)
    S = -(-256 // tiles)
    maxS = max(M // 128, 1)
    return max(1, min(S, maxS))


def load8_width(n):
    """The dn_load8 path a row pitch of n elements takes: 8 (16-B), 4 (8-B), 2 (4-B) or 1."""
    return 8 if n % 8 == 0 else 4 if n % 4 == 0 else 2 if n % 2 == 0 else 1


def fwd_plan(M, N, K, S):
    """fn_dense_fwd: slice length, slices covering K, column waves, load form."""
    kc = -(-(-(-K // S)) // 32) * 32
    Sr = -(-K // kc)
    vec = K % 8 == 0
    return {"kc": kc, "Sr": Sr, "ncw": dn_ncw(M, N, K), "vec": vec, "D": 4 if vec else 1,
            "slices": [(s * kc, min(K, (s + 1) * kc)) for s in range(Sr)]}


def dgrad_plan(M, N, K):
    NP = -(-N // 32) * 32
    lds = 64 * (NP + 8) * 2
    mblk = -(-M // 64)
    mrep = min(mblk, 4) if -(-K // 64) >= 512 else 1
    return {"NP": NP, "lds": lds, "refused": lds > 160 * 1024, "mblk": mblk, "mrep": mrep,
            "grid_y": -(-mblk // mrep)}


def wgrad_plan(M, N, K, S):
    mc = (-(-M // S) + 31) & ~31
    Sr = -(-M // mc)
    MCH = mc if mc < 512 else 512
    slices = [(z * mc, min(M, (z + 1) * mc)) for z in range(Sr)]
    chunks = [[min(MCH, m1 - mb) for mb in range(m0, m1, MCH)] for m0, m1 in slices]
    return {"mc": mc, "Sr": Sr, "MCH": MCH, "slices": slices, "chunks": chunks, "lds": 128 * (MCH + 8) * 2}


# ---------------------------------------------------------------------------
# the case table: the smallest shapes that still reach each path
# ---------------------------------------------------------------------------
def _fwd(M, N, K, S, act, bias, out_fp32):
    s = "auto" if S is None else S
    return {"name": f"fwd-{M}x{N}x{K}-S{s}-{ACT_NAMES[act]}-b{int(bias)}-f{int(out_fp32)}", "M": M, "N": N, "K": K,
            "S": S, "act": act, "bias": bias, "out_fp32": out_fp32}


# S None: S = dense_splits(M, N, K), the production pairing of the two host functions.
# Every case runs with the fp32 master weights and with the bf16 copy (wbf16 = 1).
FWD_CASES = [
    # one slice (FINAL epilogue), 16-B loads and the 4-deep ring
    _fwd(20, 7, 40, 1, NONE, True, False),
    _fwd(129, 65, 64, 1, RELU, True, True),
    _fwd(16, 16, 32, 1, TANH, False, False),
    # one slice, element loads: K odd, even, % 4
    _fwd(20, 7, 45, 1, SIGMOID, True, False),
    _fwd(20, 7, 30, 1, RELU, False, False),
    _fwd(20, 7, 84, 1, NONE, True, True),
    # split K, 16-B loads: kc 32 and 17 slices (one unrolled reduce pass, then the tail; three of
    # four ring steps masked), the tail alone, idle reduce waves, kc rounded so that Sr = 9 < S
    _fwd(33, 65, 544, 17, RELU, True, False),
    _fwd(33, 65, 544, 5, TANH, True, True),
    _fwd(33, 65, 544, 2, SIGMOID, False, False),
    _fwd(33, 65, 544, 16, NONE, True, True),
    # kc 160: a full ring group, then a remainder of one step
    _fwd(20, 24, 800, 5, NONE, False, False),
    _fwd(20, 24, 800, None, RELU, True, False),
    # element loads, ragged last slice
    _fwd(20, 10, 1095, 4, RELU, True, True),
    # 128-column workgroups; in the second workgroup column wave 1 lies wholly past N
    _fwd(130, 130, 512, 1, RELU, True, False),
    _fwd(130, 130, 512, 1, TANH, True, True),
    _fwd(130, 130, 512, 2, NONE, True, False),
    # 128-column workgroups with element loads: one exact case per epilogue form, then the soft ones
    _fwd(130, 65, 516, 1, NONE, True, False),
    _fwd(130, 65, 516, 2, RELU, True, True),
    _fwd(130, 65, 516, 1, SIGMOID, True, True),
    _fwd(130, 65, 516, 2, TANH, True, False),
]
# The tanh / sigmoid cases say little about the sums in front of them: at these K most arguments
# saturate, and an fp32 output (f1) is still held to the bf16 bound 2^-8 |r|.  They cover the
# activation branch of the two epilogues; every template instance and every reduce path also has
# a none or relu case, compared bit for bit (asserted in tests/test_dense_oracle_cpu.py), and a
# later edit must keep it so.


def _bwd(kind, M, N, K, ya=0, S=1, db=True):
    name = f"{kind}-{M}x{N}x{K}" + (f"-S{S}" if kind == "wgrad" else "") + (f"-ya-{ACT_NAMES[ya]}" if ya else "")
    name += "" if db or kind != "wgrad" else "-nodb"
    return {"name": name, "M": M, "N": N, "K": K, "ya": ya, "S": S, "db": db}


DGRAD_CASES = [
    _bwd("dgrad", 20, 7, 45),                    # odd N; scalar stage and store, ragged kk tile
    _bwd("dgrad", 20, 10, 30),                   # even N
    _bwd("dgrad", 65, 84, 68),                   # N % 4; the kk + 4 <= K edge; a second row block of 1 row
    _bwd("dgrad", 64, 24, 64),                   # NP = 32: the last lane group lies past N
    _bwd("dgrad", 20, 40, 128),                  # two n0 steps
    _bwd("dgrad", 130, 8, 32768),                # mrep = 3
    _bwd("dgrad", 300, 8, 32768),                # mrep = 4; the second blockIdx.y covers one block, then breaks
    _bwd("dgrad", 16, 512, 64),                  # 66,560 B of LDS
] + [_bwd("dgrad", M, N, K, ya=a) for (M, N, K) in ((20, 10, 30), (64, 24, 64)) for a in (RELU, TANH, SIGMOID)]
DGRAD_REFUSED = (4, 1280, 8)                     # 64 * 1288 * 2 = 164,864 B > 160 KB: -4

WGRAD_CASES = [
    _bwd("wgrad", 20, 7, 45),                    # odd K and N
    _bwd("wgrad", 20, 10, 30, db=False),         # even K and N, no db
    _bwd("wgrad", 64, 24, 40),                   # K % 8, N % 8
    _bwd("wgrad", 33, 84, 84),                   # K % 4, N % 4
    _bwd("wgrad", 545, 24, 40),                  # two LDS chunks, 512 + 33 rows (MP = 64): 133,120 B of LDS
    _bwd("wgrad", 300, 24, 40, S=2),             # slices of 160 and 140 rows
    _bwd("wgrad", 400, 24, 40, S=3),             # 160, 160, 80
    _bwd("wgrad", 300, 24, 40, S=4),             # 96, 96, 96, 12
    _bwd("wgrad", 130, 24, 40, S=4),             # mc 64: the launcher makes it 3 slices
    _bwd("wgrad", 33, 130, 130),                 # 3 x 3 tiles, ragged in both dimensions
] + [_bwd("wgrad", M, N, K, ya=a) for (M, N, K) in ((64, 24, 40), (20, 7, 45)) for a in (RELU, TANH, SIGMOID)]

# LinearFn.apply, forward and torch.autograd.grad: (M, N, K, act, bias, out_fp32)
DISPATCH_CASES = [
    {"name": "fn-20x84x120-relu", "M": 20, "N": 84, "K": 120, "act": RELU, "bias": True, "out_fp32": False},
    {"name": "fn-16x24x4104-relu", "M": 16, "N": 24, "K": 4104, "act": RELU, "bias": True, "out_fp32": False},
    {"name": "fn-20x10x84-none-fp32", "M": 20, "N": 10, "K": 84, "act": NONE, "bias": False, "out_fp32": True},
]
INFER_SHAPES = [(130, 130, 512), (33, 65, 544)]  # linear_infer: NCW 2 and NCW 1
SPLITS_FC1 = (128, 128, 64000)

BOUNDED = [(c["name"], "y") for c in FWD_CASES if c["act"] in (TANH, SIGMOID)]


# ---------------------------------------------------------------------------
# path tags: what each case reaches, from the mirror above
# ---------------------------------------------------------------------------
def fwd_tags(c: dict, wbf16: int) -> set:
    M, N, K = c["M"], c["N"], c["K"]
    S = dense_splits(M, N, K) if c["S"] is None else c["S"]
    p = fwd_plan(M, N, K, S)
    t = {"fwd.vec_ring" if p["vec"] else "fwd.elem", "fwd.w_bf16" if wbf16 else "fwd.w_fp32", f"fwd.ncw{p['ncw']}"}
    out = "fp32" if c["out_fp32"] else "bf16"
    if p["Sr"] == 1:
        t |= {"fwd.final", f"fwd.final.{out}", f"fwd.final.act.{ACT_NAMES[c['act']]}",
              "fwd.final.bias" if c["bias"] else "fwd.final.nobias"}
    else:
        t |= {"fwd.split", f"red.{out}", f"red.act.{ACT_NAMES[c['act']]}", "red.bias_mod_N" if c["bias"] else "red.nobias"}
        # the reduce kernel: wave w walks slices w, w + 4, ..: the unrolled loop while s + 12 < Sr
        for wv in range(4):
            s = wv
            unrolled = 0
            while s + 12 < p["Sr"]:
                s += 16
                unrolled += 1
            tail = len(range(s, p["Sr"], 4))
            if unrolled:
                t.add("red.unrolled")
            if tail:
                t.add("red.tail")
            if unrolled and tail:
                t.add("red.unrolled_then_tail")
            if wv >= p["Sr"]:
                t.add("red.idle_wave")
    if p["Sr"] < S:
        t.add("fwd.Sr_lt_S")
    for k0, k1 in p["slices"]:
        steps = -(-(k1 - k0) // 32)
        if (k1 - k0) % 32:
            t.add("fwd.kok_chunk_past_kend")     # a consumed step with lane groups past kend
        if p["vec"] and steps % 4:
            t.add("fwd.ring_step_past_kend")     # ring steps loaded from chunk 0 and discarded
        if p["vec"] and steps > 4 and steps % 4:
            t.add("fwd.ring_group_then_remainder")
        if not p["vec"] and (k1 - k0) % 8:
            t.add("fwd.elem_masked_at_kend")
    if p["Sr"] > 1 and p["slices"][-1][1] - p["slices"][-1][0] < p["kc"]:
        t.add("fwd.ragged_last_slice")
    if M % 128:
        t.add("fwd.rows_past_M")
    if M > 128:
        t.add("fwd.row_blocks")
    if N % 16:
        t.add("fwd.cols_past_N_in_fragment")
    if N > 16 and N % 64 and N % 64 <= 48:
        t.add("fwd.fragment_past_N")
    if p["ncw"] == 2 and N % 128 and N % 128 <= 64:
        t.add("fwd.wave_past_N")
    return t


def dgrad_tags(c: dict) -> set:
    M, N, K = c["M"], c["N"], c["K"]
    p = dgrad_plan(M, N, K)
    t = {"dgrad.stage_float4" if K % 4 == 0 else "dgrad.stage_elem", "dgrad.store_8B" if K % 4 == 0 else "dgrad.store_elem",
         f"dgrad.n_w{load8_width(N)}"}
    if K % 64:
        t.add("dgrad.ragged_kk")
    if K % 4 == 0 and K % 64:
        t.add("dgrad.kk4_edge")
    if p["NP"] > N:
        t.add("dgrad.NP_pad")
    if N % 8 == 0 and p["NP"] - N >= 8:
        t.add("dgrad.lane_group_past_N")
    t.add("dgrad.g_16B" if N % 8 == 0 else "dgrad.g_load8")
    if p["NP"] >= 64:
        t.add("dgrad.n0_steps")
    if p["mrep"] > 1:
        t.add(f"dgrad.mrep{p['mrep']}")
        if p["grid_y"] * p["mrep"] > p["mblk"]:
            t.add("dgrad.mrep_break")
    if M > 64 and p["mrep"] == 1:
        t.add("dgrad.row_blocks")
    if M % 64:
        t.add("dgrad.rows_past_M")
    if p["lds"] > 64 * 1024:
        t.add("dgrad.lds_gt_64k")
    if c["ya"]:
        t |= {f"dgrad.ya.{ACT_NAMES[c['ya']]}", f"dgrad.ya.n_w{load8_width(N)}"}
    return t


def wgrad_tags(c: dict) -> set:
    M, N, K = c["M"], c["N"], c["K"]
    p = wgrad_plan(M, N, K, c["S"])
    t = {f"wgrad.n_w{load8_width(N)}", f"wgrad.k_w{load8_width(K)}", "wgrad.db" if c["db"] else "wgrad.nodb",
         "wgrad.store_float4" if K % 4 == 0 else "wgrad.store_elem", f"wgrad.slices{p['Sr']}"}
    if p["Sr"] < c["S"]:
        t.add("wgrad.S_recomputed")
    if p["Sr"] > 1 and c["db"]:
        t.add("wgrad.slices_db")
    for ch in p["chunks"]:
        if len(ch) > 1 and -(-ch[-1] // 32) * 32 < p["MCH"]:
            t.add("wgrad.second_chunk_short")
        if any(r % 32 for r in ch):
            t.add("wgrad.MP_pad")
    if p["lds"] > 64 * 1024:
        t.add("wgrad.lds_gt_64k")
    if N % 64:
        t.add("wgrad.ragged_N")
    if K % 64:
        t.add("wgrad.ragged_K")
    if N > 64 and K > 64:
        t.add("wgrad.tiles_2d")
    if c["ya"]:
        t |= {f"wgrad.ya.{ACT_NAMES[c['ya']]}", f"wgrad.ya.n_w{load8_width(N)}"}
        if c["db"]:
            t.add("wgrad.ya_db")
    return t


def all_tags() -> set:
    t = set()
    for c in FWD_CASES:
        t |= fwd_tags(c, 0) | fwd_tags(c, 1)
    for c in DGRAD_CASES:
        t |= dgrad_tags(c)
    if dgrad_plan(*DGRAD_REFUSED)["refused"]:
        t.add("dgrad.refused")
    for c in WGRAD_CASES:
        t |= wgrad_tags(c)
    return t


# one entry or more per bullet of the paths listed for dense.hip
REQUIRED_TAGS = {
    # forward: load forms, weight forms, workgroup widths, epilogue or slabs + reduce
    "fwd.vec_ring", "fwd.elem", "fwd.w_fp32", "fwd.w_bf16", "fwd.ncw1", "fwd.ncw2", "fwd.final", "fwd.split",
    "fwd.final.bf16", "fwd.final.fp32", "fwd.final.bias", "fwd.final.nobias",
    "fwd.final.act.none", "fwd.final.act.relu", "fwd.final.act.tanh", "fwd.final.act.sigmoid",
    # k-chunks past kend zeroed by kok, ring steps past kend discarded, masked element loads
    "fwd.kok_chunk_past_kend", "fwd.ring_step_past_kend", "fwd.ring_group_then_remainder", "fwd.elem_masked_at_kend",
    "fwd.ragged_last_slice",
    # rows and columns past M and N
    "fwd.rows_past_M", "fwd.row_blocks", "fwd.cols_past_N_in_fragment", "fwd.fragment_past_N", "fwd.wave_past_N",
    # kc rounding
    "fwd.Sr_lt_S",
    # reduce: unrolled loop and tail, idle waves, bias[i % N], activation, output type
    "red.unrolled", "red.tail", "red.unrolled_then_tail", "red.idle_wave", "red.bias_mod_N", "red.nobias",
    "red.act.none", "red.act.relu", "red.act.tanh", "red.act.sigmoid", "red.bf16", "red.fp32",
    # dn_load8: the four widths for g (dgrad, wgrad), x (wgrad) and ya
    "dgrad.n_w8", "dgrad.n_w4", "dgrad.n_w2", "dgrad.n_w1", "wgrad.n_w8", "wgrad.n_w4", "wgrad.n_w2", "wgrad.n_w1",
    "wgrad.k_w8", "wgrad.k_w4", "wgrad.k_w2", "wgrad.k_w1", "dgrad.ya.n_w8", "dgrad.ya.n_w2", "wgrad.ya.n_w8",
    "wgrad.ya.n_w1", "dgrad.lane_group_past_N",
    # dgrad
    "dgrad.stage_float4", "dgrad.stage_elem", "dgrad.ragged_kk", "dgrad.kk4_edge", "dgrad.store_8B", "dgrad.store_elem",
    "dgrad.NP_pad", "dgrad.g_16B", "dgrad.g_load8", "dgrad.n0_steps", "dgrad.mrep3", "dgrad.mrep4", "dgrad.mrep_break",
    "dgrad.row_blocks", "dgrad.rows_past_M", "dgrad.ya.relu", "dgrad.ya.tanh", "dgrad.ya.sigmoid", "dgrad.lds_gt_64k",
    "dgrad.refused",
    # wgrad
    "wgrad.slices1", "wgrad.slices2", "wgrad.slices3", "wgrad.slices4", "wgrad.S_recomputed", "wgrad.slices_db",
    "wgrad.second_chunk_short", "wgrad.MP_pad", "wgrad.db", "wgrad.nodb", "wgrad.ya_db", "wgrad.ya.relu",
    "wgrad.ya.tanh", "wgrad.ya.sigmoid", "wgrad.ragged_N", "wgrad.ragged_K", "wgrad.tiles_2d", "wgrad.store_float4",
    "wgrad.store_elem", "wgrad.lds_gt_64k",
}
