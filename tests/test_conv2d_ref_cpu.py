"""The fp64 reference of tests/conv2d_ref.py (the bound tests/test_gpu_conv2d_routes.py holds every 2D-convolution route to) on the CPU:
  * the per-element bound discriminates: each plausible kernel mistake of conv2d_ref.MISTAKES, evaluated by the same reference, fails it
    against the correct result even at the loosest route constant, while the correct result rounded to fp32 sits far inside it;
  * the reference agrees with nn.Conv2d + BatchNorm2d (eval) + ReLU (and nn.Upsample, sigmoid) evaluated in float64 on the same parameters,
    with scale / shift folded by packing.fold_bn_fp32 as the plans fold them;
  * the sampled-pixel form equals the whole-map form."""
import pytest
import torch
import torch.nn as nn

import conv2d_ref as R
from test_gpu_conv2d_routes import C_ROUTE

C_MAX = max(C_ROUTE.values())
SHAPES = [(1, 9, 17), (2, 7, 15)]          # ragged against the 8 x 16 tiles and the 16-pixel rows of the kernels


def _bn(n, g):
    bn = nn.BatchNorm2d(n).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(n, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(n, generator=g) + 0.5)
    return bn


def _folded(bn):
    from estdepth_amd import packing
    return packing.fold_bn_fp32(bn, list(range(bn.num_features)))


# the convolution that exposes each mistake: (k, stride, pad, dilation, residual + relu_after, upsample)
SETUP = {"drop_corner_tap": (3, 1, 1, 1, True, False), "right_pad_wraps": (3, 1, 1, 1, True, False), "stride2_from_1": (3, 2, 1, 1, False, False),
         "dilation_1": (3, 1, 2, 2, True, False), "relu_before_residual": (3, 1, 1, 1, True, False), "ignore_residual": (1, 1, 0, 1, True, False),
         "shift_before_scale": (5, 2, 2, 1, False, False), "neighbour_shift": (1, 2, 0, 1, True, False), "bilinear_upsample": (3, 1, 1, 1, False, True)}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_bound_rejects_each_plausible_kernel_mistake(shape, mistake):
    g = torch.Generator().manual_seed(len(mistake))
    k, stride, pad, dil, res, up = SETUP[mistake]
    N, H, W = shape
    cin, cout = (16, 16) if up else (48, 64)
    x = torch.randn(N, H, W, cin, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (k * cin ** 0.5)
    sc, sh = _folded(_bn(cout, g))
    Ho, Wo = R.out_size(H, W, k, stride, pad, dil, up)
    kw = dict(stride=stride, pad=pad, dilation=dil, upsample=up, relu_after=True,
              residual=torch.randn(N, Ho, Wo, cout, generator=g) if res else None)
    good, A = R.conv2d_ref(x, w, sc, sh, **kw)
    bad, _ = R.conv2d_ref(x, w, sc, sh, mistake=mistake, **kw)
    assert R.bound_ratio(good.float(), good, A) <= 1.0            # fp32 rounding of the exact result: half an ulp of |ref| <= A
    ratio = R.bound_ratio(bad.float(), good, A)
    assert ratio > C_MAX, "%s slips under the bound (worst ratio %.1f <= %g)" % (mistake, ratio, C_MAX)
    if mistake == "bilinear_upsample":                            # ... and in the disparity head's output upscaling
        wd, b = torch.randn(1, cin, 3, 3, generator=g) * 0.3, torch.randn(1, generator=g)
        good, A = R.disp_head_ref(x, wd, b, 10.0, 2)
        bad, _ = R.disp_head_ref(x, wd, b, 10.0, 2, mistake=mistake)
        assert R.bound_ratio(good.float(), good, A) <= 1.0
        ratio = R.bound_ratio(bad.float(), good, A)
        assert ratio > C_MAX, "disp_head %s slips under the bound (worst ratio %.1f <= %g)" % (mistake, ratio, C_MAX)


# (cin, cout, k, stride, dilation, relu_before, residual, relu_after, upsample): the contracts of the kernels
MODULES = [(32, 64, 3, 1, 1, True, False, False, False),       # Conv2dPlan, relu_before_residual
           (32, 32, 3, 1, 2, False, True, True, False),        # Conv2dPlan, dilation 2, residual + relu_after
           (48, 64, 1, 2, 1, False, True, True, False),        # conv1x1 / taps k = 1, stride 2
           (16, 32, 5, 2, 1, False, False, True, False),       # taps k = 5, stride 2
           (3, 64, 7, 2, 1, False, False, True, False),        # stem 7x7 / 2
           (3, 32, 3, 2, 1, False, False, True, False),        # stem 3x3 / 2
           (32, 16, 3, 1, 1, False, False, True, True)]        # conv2d_k3_to16 on the nearest-x2 upsampled input


@pytest.mark.parametrize("m", MODULES)
def test_reference_agrees_with_the_float64_modules(m):
    cin, cout, k, stride, dil, rb, res, ra, up = m
    g = torch.Generator().manual_seed(cin + cout + k)
    pad = dil * (k // 2)
    conv = nn.Conv2d(cin, cout, k, stride, pad, dil, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, k, k, generator=g) / (k * cin ** 0.5))
    bn = _bn(cout, g)
    x = torch.randn(2, 9, 17, cin, generator=g)
    xm = x.permute(0, 3, 1, 2).double()
    if up:
        xm = nn.Upsample(scale_factor=2, mode="nearest")(xm)
    want = bn.double()(conv.double()(xm))
    if rb:
        want = torch.relu(want)
    r = torch.randn(*want.permute(0, 2, 3, 1).shape, generator=g) if res else None
    if r is not None:
        want = want + r.permute(0, 3, 1, 2).double()
    if ra:
        want = torch.relu(want)
    want = want.permute(0, 2, 3, 1)
    sc, sh = _folded(bn.float())
    got, A = R.conv2d_ref(x, conv.weight.float(), sc, sh, stride=stride, pad=pad, dilation=dil, relu_before=rb, residual=r, relu_after=ra,
                          upsample=up)
    assert got.shape == want.shape
    # the fp32 folding of BatchNorm is the only difference: a few 2^-24 A
    assert R.bound_ratio(want, got, A) <= 4.0


def test_disp_head_agrees_with_the_float64_modules():
    g = torch.Generator().manual_seed(4)
    conv = nn.Conv2d(32, 1, 3, padding=1).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(1, 32, 3, 3, generator=g) * 0.2)
        conv.bias.copy_(torch.randn(1, generator=g))
    x = torch.randn(2, 9, 17, 32, generator=g)
    for up in (1, 2):
        want = 10.0 * torch.sigmoid(conv(x.permute(0, 3, 1, 2).double()))
        if up == 2:
            want = nn.Upsample(scale_factor=2, mode="nearest")(want)
        got, A = R.disp_head_ref(x, conv.weight, conv.bias, 10.0, up)
        assert got.shape == want.shape
        assert R.bound_ratio(want, got, A) <= 1e-6


def test_sampled_pixels_equal_the_whole_map():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 9, 17, 32, generator=g)
    pts = lambda Ho, Wo: torch.tensor([[1, Ho - 1, Wo - 1], [0, 0, 0], [1, 0, Wo - 1], [0, Ho - 1, 0], [1, Ho // 2, 3]])   # noqa: E731
    for k, stride, pad, dil, up in ((3, 1, 2, 2, False), (5, 2, 2, 1, False), (1, 2, 0, 1, False), (3, 1, 1, 1, True), (7, 2, 3, 1, False)):
        w = torch.randn(48, 32, k, k, generator=g)
        sc, sh = torch.rand(48, generator=g) + 0.5, torch.randn(48, generator=g)
        Ho, Wo = R.out_size(9, 17, k, stride, pad, dil, up)
        r = torch.randn(2, Ho, Wo, 48, generator=g)
        kw = dict(stride=stride, pad=pad, dilation=dil, upsample=up, residual=r, relu_after=True)
        full, fa = R.conv2d_ref(x, w, sc, sh, **kw)
        p = pts(Ho, Wo)
        part, pa = R.conv2d_ref(x, w, sc, sh, points=p, **kw)
        at = lambda t: t[p[:, 0], p[:, 1], p[:, 2]]                               # noqa: E731
        assert torch.allclose(part, at(full), rtol=1e-12, atol=1e-12) and torch.allclose(pa, at(fa), rtol=1e-12, atol=1e-12)
    wd, b = torch.randn(1, 32, 3, 3, generator=g), torch.randn(1, generator=g)
    for up in (1, 2):
        full, fa = R.disp_head_ref(x, wd, b, 10.0, up)
        p = pts(9 * up, 17 * up)
        part, pa = R.disp_head_ref(x, wd, b, 10.0, up, points=p)
        at = lambda t: t[p[:, 0], 0, p[:, 1], p[:, 2]]                            # noqa: E731
        assert torch.allclose(part, at(full), rtol=1e-12, atol=1e-12) and torch.allclose(pa, at(fa), rtol=1e-12, atol=1e-12)
