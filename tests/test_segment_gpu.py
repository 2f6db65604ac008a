"""The fused 1x1 head + arg-max kernel (``pw_argmax_kernel``) and the inference path built on it
(``FeatureNet3DSeg.predict``, ``fn.segment``) on the GPU.

Kernel checks, at the smallest shapes that reach every path (one partial tile, exactly one tile,
a tile plus an 8-row tail, and one more tile than the launch grid so a workgroup walks two tiles
and the prefetch runs):

* exact: the labels are the lowest-index arg-max of the bf16 logits ``pw_fwd`` (the unfused native
  head) stores for the same inputs and prologue, on every row; the confidence is the fp32
  ``softmax(logits_bf16).max`` within 2^-8 (a bf16 half-ulp on a value <= 1, doubled);
* oracle: against fp64 ``l = bf16(pact(x * psc + psh)) w^T + b`` the labels may differ only on rows
  whose oracle top-2 gap is below ``2^-7 max|l_row|`` (each bf16 logit is within 2^-9 relative, two
  competing logits 2^-8, times a 2x margin), and those rows stay <= 6 % of a case's rows (pooled
  over its M values: at M = 8 one row is 12.5 %);
* ``pw_fwd`` itself (the two kernels share the code up to the staged logit tile, so an error there
  would cancel in the exact check): every stored logit against the same fp64 oracle, within one
  bf16 rounding plus the fp32 accumulation error (``test_pw_fwd_against_fp64_oracle``).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import importlib  # noqa: E402

import featurenet_amd as fn  # noqa: E402
from featurenet_amd import _native  # noqa: E402
from featurenet_amd.models.featurenet3d import FeatureNet3DSeg  # noqa: E402
from featurenet_amd.ops import subpixel  # noqa: E402

C = importlib.import_module("featurenet_amd.ops.conv")

DEV = "cuda"
KN = [(32, 25), (32, 5), (8, 2), (16, 3), (64, 64)]
PRO = [None, 0, 1]                                # none, BN only, BN + ReLU


def lowest_argmax(l: torch.Tensor) -> torch.Tensor:
    n = l.shape[-1]
    idx = torch.arange(n, device=l.device)
    return torch.where(l == l.max(-1, keepdim=True).values, idx, n).min(-1).values.to(torch.uint8)


def make_inputs(M, K, N, pro, bias, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    b = (0.1 * torch.randn(N, generator=g)).to(DEV) if bias else None
    p = None
    if pro is not None:
        psc = (torch.rand(K, generator=g) + 0.5).to(DEV)
        psh = (0.3 * torch.randn(K, generator=g)).to(DEV)
        p = (psc, psh, pro)
    return x, w, b, p


def oracle_input(x, p):
    """z = bf16(pact(x * psc + psh)) in fp64 (x itself without a prologue)."""
    z = x.double()
    if p is not None:
        z = z * p[0].double() + p[1].double()
        if p[2] == 1:
            z = torch.relu(z)
        z = z.to(torch.bfloat16).double()
    return z


def oracle(x, w, b, p):
    """fp64 logits of z = bf16(pact(x * psc + psh))."""
    l = oracle_input(x, p) @ w.double().t()
    return l + b.double() if b is not None else l


def check_against_oracle(labels, l64):
    """-> (mismatches on rows the oracle decides, excluded rows)."""
    top2 = l64.topk(2, -1).values
    unsure = (top2[:, 0] - top2[:, 1]) < 2.0 ** -7 * l64.abs().max(-1).values
    bad = (labels != lowest_argmax(l64)) & ~unsure
    return int(bad.sum()), int(unsure.sum())


def grid_blocks(K, N):
    return int(_native.kernels().pw_argmax_blocks(1 << 30, K, N))


def m_values(K, N):
    return [8, 256, 264, 256 * (grid_blocks(K, N) + 1) + 8]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("pro", PRO, ids=["plain", "bn", "bnrelu"])
@pytest.mark.parametrize("kn", KN, ids=lambda kn: f"k{kn[0]}n{kn[1]}")
def test_kernel_exact_and_oracle(kn, pro, bias):
    K, N = kn
    rows = unsure = 0
    for i, M in enumerate(m_values(K, N)):
        x, w, b, p = make_inputs(M, K, N, pro, bias, 100 + i)
        assert C.pw_argmax_ok(M, K, N, p)
        labels, conf = C.pw_argmax(x, w, b, pro=p, want_conf=True)
        only_labels, none = C.pw_argmax(x, w, b, pro=p)
        logits = C.pw_fwd(x, w, b, 0, pro=p).float()
        torch.cuda.synchronize()
        assert none is None and labels.dtype == torch.uint8 and conf.dtype == torch.bfloat16
        want = lowest_argmax(logits)
        assert torch.equal(labels, want), (M, int((labels != want).sum()))
        assert torch.equal(only_labels, want), (M, int((only_labels != want).sum()))
        cerr = float((conf.float() - torch.softmax(logits, -1).max(-1).values).abs().max())
        assert cerr <= 2.0 ** -8, (M, cerr)
        bad, u = check_against_oracle(labels, oracle(x, w, b, p))
        assert bad == 0, (M, bad)
        rows, unsure = rows + M, unsure + u
    print(f"pw_argmax K={K} N={N} pro={pro} bias={bias}: oracle-undecided rows {100.0 * unsure / rows:.2f} %")
    assert unsure <= 0.06 * rows, unsure / rows


# K = 6: the 16-B chunks straddle rows (the prologue needs K % 8 == 0, so plain input only)
FWD_CASES = [(kn, pro) for kn in KN for pro in PRO] + [((6, 40), None)]
PRO_IDS = {None: "plain", 0: "bn", 1: "bnrelu"}


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: f"k{c[0][0]}n{c[0][1]}-{PRO_IDS[c[1]]}")
def test_pw_fwd_against_fp64_oracle(case, bias):
    """``pw_fwd`` (the front half ``pw_argmax_kernel`` shares) against the fp64 logits l, every row and
    element: |y - l| <= 2^-8 |l| + 2^-17 (sum_k |z_k w_k| + |b|) -- one bf16 rounding of the output
    (half-ulp 2^-9, doubled) plus fp32 accumulation over K <= 64 terms (64 * 2^-24, doubled)."""
    (K, N), pro = case
    for i, M in enumerate(m_values(K, N)):
        x, w, b, p = make_inputs(M, K, N, pro, bias, 100 + i)
        y = C.pw_fwd(x, w, b, 0, pro=p).double()
        l = oracle(x, w, b, p)
        mag = oracle_input(x, p).abs() @ w.double().abs().t()
        if b is not None:
            mag = mag + b.double().abs()
        excess = (y - l).abs() - (2.0 ** -8 * l.abs() + 2.0 ** -17 * mag)
        print(f"pw_fwd K={K} N={N} pro={pro} bias={bias} M={M}: max |y - l| {float((y - l).abs().max()):.3e}, "
              f"max (error - bound) {float(excess.max()):.3e}")
        assert y.shape == (M, N) and float(excess.max()) <= 0.0, (M, int((excess > 0).sum()))


@pytest.mark.parametrize("pro", PRO, ids=["plain", "bn", "bnrelu"])
def test_ties_go_to_the_lowest_index(pro):
    K, N, M = 32, 12, 264
    g = torch.Generator().manual_seed(5)
    w = torch.randn(N, K, generator=g)
    w[3] = w[7] = w.abs().sum(0)                         # rows 3 and 7 identical, the largest logit ...
    b = 0.1 * torch.randn(N, generator=g)
    b[3] = b[7] = 1.0                                    # ... with equal bias
    x = (torch.rand(M, K, generator=g) + 0.5).to(torch.bfloat16).to(DEV)
    p = None if pro is None else (torch.rand(K, generator=g).add(0.5).to(DEV),
                                  torch.rand(K, generator=g).mul(0.3).to(DEV), pro)   # (keeps z > 0)
    labels, _ = C.pw_argmax(x, w.to(DEV), b.to(DEV), pro=p)
    assert torch.all(labels == 3), labels.unique().tolist()
    # all-zero input, zero bias: every class ties at 0 (a BN shift of 0 keeps it so)
    p0 = None if pro is None else (p[0], torch.zeros(K, device=DEV), pro)
    labels, conf = C.pw_argmax(torch.zeros(M, K, dtype=torch.bfloat16, device=DEV), w.to(DEV),
                               torch.zeros(N, device=DEV), pro=p0, want_conf=True)
    assert torch.all(labels == 0)
    assert torch.all((conf.float() - 1.0 / N).abs() <= 2.0 ** -8)


class _Recorder:
    """Forwards to the real ``_C`` and records the entry points called."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


@pytest.mark.parametrize("shape", [(4096, 72, 25), (4100, 32, 25)], ids=["k72", "m4100"])
def test_unsupported_shape_takes_the_fallback(shape, monkeypatch):
    M, K, N = shape
    x, w, b, _ = make_inputs(M, K, N, None, True, 7)
    assert not C.pw_argmax_ok(M, K, N)
    Kn = _native.kernels()
    out = torch.zeros(M, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported configuration"):      # the kernel refuses it
        Kn.pw_argmax(x.data_ptr(), w.data_ptr(), 0, out.data_ptr(), 0, M, K, N, 0, 0, 0, _native.stream(x),
                     [x.numel(), M, 0])
    rec = _Recorder(Kn)
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    labels, conf = C.pw_argmax(x, w, b, want_conf=True)
    torch.cuda.synchronize()
    assert "pw_argmax" not in rec.calls and rec.calls
    assert labels.dtype == torch.uint8 and labels.shape == (M,) and conf.shape == (M,)
    bad, unsure = check_against_oracle(labels, oracle(x, w, b, None))
    assert bad == 0 and unsure <= 0.06 * M, (bad, unsure)


def test_kernel_is_repeatable():
    K, N = 32, 25
    M = m_values(K, N)[-1]
    x, w, b, p = make_inputs(M, K, N, 1, True, 11)
    l1, c1 = C.pw_argmax(x, w, b, pro=p, want_conf=True)
    l2, c2 = C.pw_argmax(x, w, b, pro=p, want_conf=True)
    assert torch.equal(l1, l2) and torch.equal(c1.view(torch.int16), c2.view(torch.int16))


# ---------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------
S = 32


def make_model(nc: int, seed: int = 0) -> FeatureNet3DSeg:
    """A CPU fp32 model whose BN folds are not the identity."""
    torch.manual_seed(seed)
    m = FeatureNet3DSeg(S, num_classes=nc).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for c in list(m.enc) + [m.dec]:
            c.running_mean.copy_(torch.randn(c.cout, generator=g) * 0.1)
            c.running_var.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.gamma.copy_(torch.rand(c.cout, generator=g) + 0.5)
            c.beta.copy_(torch.randn(c.cout, generator=g) * 0.1)
        m.head.bias.copy_(torch.randn(nc, generator=g) * 0.1)
    return m


def voxels(n: int, seed: int = 3) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, S, S, S, generator=g) < 0.4)


def gpu_copy(m: FeatureNet3DSeg) -> FeatureNet3DSeg:
    mg = FeatureNet3DSeg(S, num_classes=m.num_classes)
    mg.load_state_dict(m.state_dict())
    return mg.to(DEV).eval()


def test_predict_fallback_decoder_is_exact(monkeypatch):
    """27-tap decoder layer + fused head: the decoder output is the forward's and the head bits are
    pw_fwd's, so the labels equal the arg-max of the model's logits exactly."""
    monkeypatch.setenv("FN_SUBPIXEL", "0")
    mg = gpu_copy(make_model(5))
    x = voxels(2).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        want = lowest_argmax(mg(x).float())
    rec = _Recorder(_native.kernels())
    monkeypatch.setattr(_native, "kernels", lambda: rec)
    labels, conf = mg.predict(x, want_conf=True)
    torch.cuda.synchronize()
    assert rec.calls.count("pw_argmax") == 1
    assert labels.shape == (2, S, S, S) and labels.dtype == torch.uint8 and conf.shape == (2, S, S, S)
    assert torch.equal(labels, want), int((labels != want).sum())
    assert len(labels.unique()) > 1


@pytest.mark.parametrize("nc", [25, 5])
def test_predict_subpixel_decoder_agreement(nc):
    """Sub-pixel decoder + fused head with the folded-BN prologue.  The folded sub-pixel weights
    are rounded to bf16 once more than the 27-tap weights, so no bit equality with the unfused
    forward: against the fp32 CPU model's arg-max (the oracle), predict's agreement must be no
    lower than the unfused GPU forward's minus 0.5 percentage points."""
    m = make_model(nc)
    xb = voxels(2)
    with torch.no_grad():
        want = lowest_argmax(m(xb.float())).to(DEV)
    mg = gpu_copy(m)
    x = xb.to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        z = x.unsqueeze(-1)
        for c in mg.enc:
            z = c(z)
        assert subpixel.infer_ok(z, mg.dec.cout, z.shape[-1])       # (the path under test is taken)
        unfused = lowest_argmax(mg(x).float())
    labels = mg.predict(x)
    torch.cuda.synchronize()
    assert labels.dtype == torch.uint8 and labels.shape == (2, S, S, S)
    assert int(labels.max()) < nc
    a_pred = float((labels == want).float().mean())
    a_unf = float((unfused == want).float().mean())
    print(f"seg predict S={S} classes={nc}: agreement with the fp32 CPU arg-max: predict {100 * a_pred:.3f} %, "
          f"unfused GPU forward {100 * a_unf:.3f} %")
    assert a_pred >= a_unf - 0.005, (a_pred, a_unf)
    assert torch.equal(mg.predict(x), labels)                       # repeatable


@pytest.mark.parametrize("bs", [1, 3])
def test_segment_end_to_end(bs, tmp_path):
    n = 5
    m = make_model(5)
    path = fn.save(m, tmp_path / "seg.fnk", {"model_kind": "featurenet3d_seg", "input_size": S, "in_channels": 1,
                                             "num_classes": 5})
    xb = voxels(n)
    packed = np.packbits(xb.numpy().reshape(n, -1), axis=1, bitorder="little")
    labels, conf = fn.segment(str(path), packed, batch_size=bs, device=DEV, packed_size=S, return_confidence=True)
    assert labels.dtype == np.uint8 and labels.shape == (n, S, S, S)
    assert conf.dtype == np.float32 and conf.shape == (n, S, S, S)
    mg = gpu_copy(m)
    x = xb.to(DEV).to(torch.bfloat16)
    for i in range(0, n, bs):
        lb, cf = mg.predict(x[i:i + bs], want_conf=True)
        assert np.array_equal(labels[i:i + bs], lb.cpu().numpy())
        assert np.array_equal(conf[i:i + bs], cf.float().cpu().numpy())
    again, _ = fn.segment(str(path), packed, batch_size=bs, device=DEV, packed_size=S)
    assert again.tobytes() == labels.tobytes()
