"""BN + activation of a conv's input inside conv_wtile's x-halo prologue (``conv_wtile.hip``
``xform_x``, experiment builds only) against the separate ``bn_apply`` pass.

The prologue applies the same fma, activation and bf16 rounding as ``bn_apply_kernel``, so the
weight gradient must be bit-identical to bn_apply followed by the plain weight gradient -- at the
FeatureNet-3D layer shapes (valid convs: every halo interior) and same-padded shapes (border
tiles: the zero page's padding must stay zero, not act(shift)).  (The matching conv_tile forward
prologue and its tests were removed: profiles/r6_bn_prologue.md.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from featurenet_amd import _native  # noqa: E402
from featurenet_amd.ops.spec import ConvSpec  # noqa: E402

CASES = [
    # (N, D, H, W, C, K, kernel, padding, act)
    (2, 29, 29, 29, 32, 32, (5, 5, 5), "valid", 1),   # FeatureNet-3D conv2 (input: the stem's BN + ReLU)
    (2, 25, 25, 25, 32, 64, (4, 4, 4), "valid", 1),   # conv3
    (3, 22, 22, 22, 64, 64, (3, 3, 3), "valid", 1),   # conv4: 2 slices per tile, 2 column blocks
    (3, 11, 12, 13, 16, 48, (3, 3, 3), "same", 1),    # border tiles: zero-page padding positions
    (2, 9, 10, 11, 64, 64, (3, 3, 3), "same", 1),     # 64 input channels: CS 32/64
    (3, 10, 11, 12, 8, 16, (3, 3, 3), "same", 1),     # 8-channel slices
]


@pytest.mark.parametrize("nw", ["8", "4"])
@pytest.mark.parametrize("case", CASES)
def test_wgrad_prologue_matches_bn_apply(case, nw, monkeypatch):
    """conv_wtile with the prologue (x = y, normalised in LDS by whoever DMA'd the slots: each wave
    in the loaderless form, the loader wave in the 4-wave form) against the weight gradient of the
    bn_apply output, bit for bit."""
    from featurenet_amd.ops import conv_wtile as cw

    N, D, H, W, C, K, k, pad, act = case
    monkeypatch.setenv("FN_WTILE_NW", nw)
    monkeypatch.setattr(cw, "_PLANS", {})
    torch.manual_seed(2)
    dev = "cuda"
    y = torch.randn(N, D, H, W, C, device=dev).to(torch.bfloat16)
    prm = torch.stack([torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.randn(C, device=dev),
                       torch.randn(C, device=dev) * 0.5]).contiguous()
    Kn = _native.kernels()
    z_ref = torch.empty_like(y)
    Kn.bn_apply(y.data_ptr(), prm[2].data_ptr(), prm[3].data_ptr(), z_ref.data_ptr(), y.numel(), C, act,
                _native.stream(y), 0, 0)
    spec = ConvSpec.make(y.shape, K, k, 1, pad)
    if not _native.kernels().conv_wtile_prologue_built():
        pytest.skip("conv_wtile's x-halo prologue is in experiment builds only (FN_BUILD_EXPERIMENTS=1)")
    p = cw.plan(spec)
    if p is None or not cw.prologue_ok(p):
        pytest.skip("no conv_wtile plan with the prologue form for this shape")
    dy = torch.randn(spec.out_shape5, device=dev).to(torch.bfloat16)
    dw_ref = cw.conv_wgrad(dy, z_ref, spec, p).clone()
    dw = cw.conv_wgrad(dy, y, spec, p, pro=(prm, act))
    torch.cuda.synchronize()
    assert torch.equal(dw, dw_ref), float((dw - dw_ref).norm() / dw_ref.norm())
