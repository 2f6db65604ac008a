"""Sub-pixel segmentation decoder on the GPU (ops/subpixel.py): the 8 parity-class forward
convs (tile kernel, strided output view), the BN backward written as the shifted
space-to-depth dy, the decoder dgrad over it (tile kernel) and the sub-pixel weight
gradient (conv_wtile SP form) against the fp32 references; then the whole
decoder + BN + head autograd node against the materialised-upsample path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from featurenet_amd import _native  # noqa: E402
from featurenet_amd.ops import bn as bn_ops  # noqa: E402
from featurenet_amd.ops import conv_wtile as cw  # noqa: E402
from featurenet_amd.ops import subpixel as sp  # noqa: E402


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _bf(t):
    return t.to(torch.bfloat16)


@pytest.mark.parametrize("N,S", [(2, 12), (3, 16)])
def test_upconv_forward_and_stats(N, S):
    assert _native.kernels_available()
    torch.manual_seed(0)
    x = _bf(torch.randn(N, S, S, S, 64, device="cuda"))
    w = torch.randn(32, 3, 3, 3, 64, device="cuda") * 0.05
    y, slab = sp.upconv_forward(x, w)
    want = sp.ref_forward(x.float(), w)
    assert _rel(y, want) < 1e-2
    s = slab.sum(0)
    yf = y.float().reshape(-1, 32)
    torch.testing.assert_close(s[0], yf.sum(0), rtol=2e-3, atol=2e-1)
    torch.testing.assert_close(s[1], (yf * yf).sum(0), rtol=2e-3, atol=2e-1)


@pytest.mark.parametrize("shape", [(2, 12, 12, 12, 32), (3, 10, 14, 8, 64), (4, 64, 64, 64, 32), (2, 8, 8, 48, 64),
                                   (1, 2, 2, 4, 512)])
def test_bn_backward_shifted_layout_matches_natural(shape):
    """bn_bwd_apply_s2d == the natural BN backward, shifted (incl. non-cubic grids, 64 channels;
    rows of 1056 and 1600 16-B chunks: the 5- and 8-chunk-per-thread instances; 512 channels, past
    the row form's 32 chunks, on the smallest even grid: border zeros on every side)."""
    torch.manual_seed(1)
    K = shape[-1]
    y = _bf(torch.randn(*shape, device="cuda"))
    dz = _bf(torch.randn(*shape, device="cuda"))
    prm = torch.stack([torch.randn(K), torch.rand(K) + 0.5, torch.randn(K), torch.randn(K)]).cuda()
    db, dg = torch.randn(K, device="cuda"), torch.randn(K, device="cuda")
    y2, dz2 = y.reshape(-1, K), dz.reshape(-1, K)
    nat = bn_ops._bwd_input(dz2, y2, prm, db, dg, 1, True).reshape(y.shape)
    sh = sp.bn_bwd_to_shifted(dz2, y2, prm, db, dg, 1, y.shape)
    assert torch.equal(sh.cpu(), sp.shift_s2d(nat.cpu()))


@pytest.mark.parametrize("N,S", [(2, 12), (3, 16)])
def test_upconv_dgrad(N, S):
    torch.manual_seed(2)
    w = torch.randn(32, 3, 3, 3, 64, device="cuda") * 0.05
    dy = _bf(torch.randn(N, 2 * S, 2 * S, 2 * S, 32, device="cuda"))
    dsh = sp.shift_s2d(dy).contiguous()
    dx = sp.upconv_dgrad(dsh, w, (N, S, S, S, 64))
    want = sp.ref_dgrad(dy.float(), w)
    assert _rel(dx, want) < 1e-2


@pytest.mark.parametrize("N,S", [(2, 12), (4, 16)])
def test_subpixel_wgrad(N, S):
    torch.manual_seed(3)
    x = _bf(torch.randn(N, S, S, S, 64, device="cuda"))
    dy = _bf(torch.randn(N, 2 * S, 2 * S, 2 * S, 32, device="cuda"))
    p = cw.plan_subpixel(N, (S, S, S), 64, 32)
    assert p is not None and p.sp
    dwf = cw.conv_wgrad_subpixel(sp.shift_s2d(dy).contiguous(), x, p)
    want = sp.ref_wgrad_classes(dy.float(), x.float())
    assert _rel(dwf, want) < 5e-3
    rel_fold = _rel(sp.fold_weight_grad(dwf), sp.fold_weight_grad(want))
    assert rel_fold < 5e-3


def test_decoder_head_matches_upsample_path():
    """Forward logits and every gradient of the fused node vs upsample2x + conv + the fused
    BN/head node (the previous path), same parameters."""
    from featurenet_amd.models.featurenet3d import FeatureNet3DSeg

    torch.manual_seed(4)
    N, S = 2, 24
    m = FeatureNet3DSeg(input_size=S, num_classes=25).cuda().train()
    x = (torch.rand(N, S, S, S, 1, device="cuda") < 0.3).to(torch.bfloat16)
    outs, grads = [], []
    for flag in ("1", "0"):
        import os
        os.environ["FN_SUBPIXEL"] = flag
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        out = m(x)
        g = torch.randn_like(out.float())
        (out.float() * g).sum().backward()
        outs.append(out.float())
        grads.append({k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None})
    os.environ.pop("FN_SUBPIXEL", None)
    # (measured, scripts/diag_model_tolerances.py: outputs 4.7e-3 apart; every upstream gradient
    # 2.8-4.5e-2 apart -- the decoder BN's backward removes the mean components of a random dz and
    # amplifies the two paths' different bf16 roundings; BOTH paths are 13-18 % from the same model
    # run in fp32 on the CPU and 4.4e-2 from each other, so neither carries an error of its own.
    # The gradient bound leaves 1.8x margin for boxes whose schedules round differently.)
    assert _rel(outs[0], outs[1]) < 1e-2
    for k in grads[1]:
        assert k in grads[0], k
        r = _rel(grads[0][k], grads[1][k])
        assert r < 8e-2, (k, r)


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_fused_head_xent_matches_softmax_xent(monkeypatch, smoothing, mode):
    """FeatureNet3DSeg.loss with the loss fused into the head vs the unfused head + softmax_xent:
    mode 1 = the head's whole backward in the forward kernel (seghead.hip: dz, weight / bias
    gradient and BN-moment partials), mode 2 = the loss-only epilogue (pw_fwd XENT instance:
    d(logits) stored).  Same loss, top-1 hits and every parameter gradient; the loss is scaled by
    3 before backward to check the dloss scaling of what the forward stored."""
    from featurenet_amd.models.featurenet3d import FeatureNet3DSeg

    torch.manual_seed(6)
    N, S = 2, 24
    m = FeatureNet3DSeg(input_size=S, num_classes=25).cuda().train()
    x = (torch.rand(N, S, S, S, 1, device="cuda") < 0.3).to(torch.bfloat16)
    lab = torch.randint(0, 25, (N, S, S, S), device="cuda")
    res = []
    for flag in (mode, "0"):
        monkeypatch.setenv("FN_SEG_XENT", flag)
        m.zero_grad(set_to_none=True)
        loss, hits = m.loss(x, lab, smoothing, with_correct=True)
        (loss * 3.0).backward()
        res.append((float(loss), int(hits.sum()), {k: p.grad.detach().float().clone() for k, p in m.named_parameters()
                                                    if p.grad is not None}))
    (l1, h1, g1), (l0, h0, g0) = res
    assert l1 == pytest.approx(l0, rel=1e-4)
    assert abs(h1 - h0) <= max(2, h0 // 1000)        # (identical logits up to bf16 ties)
    for k in g0:
        assert k in g1, k
        r = _rel(g1[k], g0[k])
        assert r < 2e-2, (k, r)


def test_decoder_bn_identity_matches_colstats(monkeypatch):
    """The encoder's last BN (relu(bn(y)) feeding the sub-pixel decoder) takes its backward from
    the statistics identity: the decoder dgrad sums g = dx * mask and S = sum W_class . dW_class
    comes from the class weight gradients.  Every parameter gradient matches the colstats path
    (FN_BN_IDENTITY=0), and the identity offer is actually made."""
    from featurenet_amd.models.featurenet3d import FeatureNet3DSeg
    from featurenet_amd.ops import bnfuse

    torch.manual_seed(7)
    N, S = 2, 24
    m = FeatureNet3DSeg(input_size=S, num_classes=25).cuda().train()
    x = (torch.rand(N, S, S, S, 1, device="cuda") < 0.3).to(torch.bfloat16)
    lab = torch.randint(0, 25, (N, S, S, S), device="cuda")
    offers = []
    orig = bnfuse.offer
    monkeypatch.setattr(bnfuse, "offer", lambda dz, slab, y: (offers.append(slab[0] if isinstance(slab, tuple)
                                                                             else "raw"), orig(dz, slab, y)))
    monkeypatch.setenv("FN_SEG_XENT", "1")
    res = []
    for flag in ("0", "1", "1"):                     # (warm-up pass, then the identity pass compared)
        monkeypatch.setenv("FN_BN_IDENTITY", flag)
        m.zero_grad(set_to_none=True)
        loss = m.loss(x, lab)
        loss.backward()
        res.append({k: p.grad.detach().float().clone() for k, p in m.named_parameters() if p.grad is not None})
    assert offers.count("identity") >= 2 * 4 - 2      # 3 encoder convs + the decoder, per identity pass
    g0, g1 = res[0], res[2]
    for k in g0:
        r = _rel(g1[k], g0[k])
        assert r < 2e-2, (k, r)


def test_weight_maps_native_match_einsum():
    """The native sub-pixel weight maps (class weights, dgrad weights, folded weight gradient;
    conv_halo.hip subpixel_wmap) against the einsum forms on the CPU."""
    from featurenet_amd.ops import subpixel as sp

    torch.manual_seed(21)
    K, C = 32, 64
    w = torch.randn(K, 3, 3, 3, C)
    dwf = torch.randn(8, K, 2, 2, 2, C)
    for fn, arg in ((sp.forward_weights, w), (sp.dgrad_weights, w), (sp.fold_weight_grad, dwf)):
        ref = fn(arg)
        got = fn(arg.cuda()).cpu()
        assert got.shape == ref.shape, fn.__name__
        torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-5)


def test_fused_head_loss_uint8_labels_match_int64():
    """The fused head + loss with uint8 per-voxel labels (the seg bench's label format) gives the
    same loss, hits and gradients bit for bit as with int64 labels."""
    from featurenet_amd.models.featurenet3d import FeatureNet3DSeg

    torch.manual_seed(7)
    N, S = 2, 24
    m = FeatureNet3DSeg(input_size=S, num_classes=25).cuda().train()
    x = (torch.rand(N, S, S, S, 1, device="cuda") < 0.3).to(torch.bfloat16)
    lab = torch.randint(0, 25, (N, S, S, S), device="cuda")
    res = []
    for lb in (lab, lab.to(torch.uint8)):
        m.zero_grad(set_to_none=True)
        loss, hits = m.loss(x, lb, 0.0, with_correct=True)
        loss.backward()
        res.append((loss.detach().clone(), hits.clone(),
                    {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


@pytest.mark.parametrize("S", [24, 20])
def test_fused_head_lean_instance_matches_full(monkeypatch, S):
    """A training step asks for neither top-1 hits nor label smoothing: seghead.hip's lean
    instance (no arg-max, no logit sum) must give the loss and every gradient bit for bit as the
    full instance (hits requested), and both must match the unfused head + softmax_xent.
    S = 20: 2 x 20^3 voxels, a partial last 256-row tile (the zero-row branch)."""
    from featurenet_amd.models.featurenet3d import FeatureNet3DSeg
    from featurenet_amd.ops import subpixel as sp

    torch.manual_seed(11)
    N = 2
    m = FeatureNet3DSeg(input_size=S, num_classes=25).cuda().train()
    x = (torch.rand(N, S, S, S, 1, device="cuda") < 0.3).to(torch.bfloat16)
    lab = torch.randint(0, 25, (N, S, S, S), device="cuda").to(torch.uint8)
    calls = []
    orig = sp.decoder_head_xent
    monkeypatch.setattr(sp, "decoder_head_xent", lambda *a, **k: (calls.append(k.get("want_hits")), orig(*a, **k))[1])
    res = []
    for flag, with_correct in (("1", True), ("1", False), ("0", False)):
        monkeypatch.setenv("FN_SEG_XENT", flag)
        m.zero_grad(set_to_none=True)
        out = m.loss(x, lab, 0.0, with_correct=with_correct)
        loss = out[0] if with_correct else out
        loss.backward()
        res.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()
                                            if p.grad is not None}))
    assert calls[:2] == [True, False], calls          # both fused passes took the seghead path
    (lf, gf), (ll, gl), (lu, gu) = res
    assert torch.equal(lf, ll)
    for k in gf:
        assert torch.equal(gf[k], gl[k]), k
    assert float(ll) == pytest.approx(float(lu), rel=1e-4)
    for k in gu:
        r = _rel(gl[k].float(), gu[k].float())
        assert r < 2e-2, (k, r)


@pytest.mark.parametrize("N,S", [(2, 12), (3, 16)])
def test_upconv_dgrad_64_column_workgroups_match_32(N, S):
    """The sub-pixel dgrad on 64-column workgroups (conv_tile MT 4 x NT 4: one halo DMA for all
    64 columns) against the 32-column-block plan, with and without the relu-mask BN-statistics
    epilogue.  At these small grids the 32-column plan takes 16-channel slices (two taps per
    k-step) where the 64-column one takes 32, so the MFMA sums group differently: measured 0.02 %
    of dx elements 1 bf16 ulp apart (rel 3e-5); the partial rows of the statistics differ in
    number, their column sums agree to rounding."""
    torch.manual_seed(9)
    C, K = 64, 32
    w = torch.randn(K, 3, 3, 3, C, device="cuda") * 0.05
    dsh = _bf(torch.randn(N, S + 1, S + 1, S + 1, 8 * K, device="cuda"))
    mask = torch.randint(0, 256, (N * S * S * S * C // 8,), dtype=torch.uint8, device="cuda")
    res = {}
    for flag in ("0", "1"):
        nt4 = flag == "1"
        p = sp._dgrad_plan((N, S, S, S, C), K, nt4)
        assert p.NT == (4 if nt4 else 2), p
        dx = sp.upconv_dgrad(dsh, w, (N, S, S, S, C), nt4=nt4)
        dxm, slab = sp.upconv_dgrad(dsh, w, (N, S, S, S, C), mask=mask, nt4=nt4)
        torch.cuda.synchronize()
        res[flag] = (dx, dxm, slab.sum(0))
    for i in (0, 1):
        a, b = res["0"][i].float(), res["1"][i].float()
        assert ((a - b).norm() / a.norm()).item() < 1e-4
        assert ((a - b) != 0).float().mean().item() < 2e-3
    assert torch.equal(res["1"][0], res["1"][1])           # (dx is stored unmasked)
    torch.testing.assert_close(res["1"][2], res["0"][2], rtol=1e-3, atol=1e-2)
