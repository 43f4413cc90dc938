"""fp64 reference of the 2D convolution contracts of the library (include/estd_hip.h) on NHWC maps, as the ops spell them:
``ops.Conv2dPlan(conv, bn, relu_before, relu_after).run(x, residual)`` (3x3, stride 1, dilation 1|2, padding = dilation),
``ops.conv1x1_nhwc`` (stride 1|2), ``ops.conv2d_taps_nhwc`` (k 1|3|5, stride 1|2, any pad), ``ops.stem7x7s2_nhwc`` (7x7 / 2 / pad 3 + BN +
ReLU), ``ops.stem3x3s2_nhwc`` (3x3 / 2 / pad 1 + BN + ReLU), ``ops.conv2d_small_nhwc`` (SMALL_CONV_SHAPES, pad k // 2),
``ops.conv2d_k3_to16_nhwc`` (3x3 / pad 1 + BN + ReLU, optionally on the nearest-x2 upsampled input) and ``ops.disp_head_nhwc``.
A plain helper module of the test suite (not a conftest).

Order of the operations, per output pixel p and output channel o (``conv2d_ref``):

    1. input   x, or its nearest-x2 upsampling (``upsample``: pixel (y, x) of the upsampled map is x[y // 2, x // 2]; never materialised
               by the kernel);
    2. z       = conv2d(x, w) in float64 with zero padding ``pad`` on every side, ``stride``, ``dilation``;
    3. y       = z * scale[o] + shift[o]          (scale None: 1; shift None: 0 -- ``scale=None`` + a shift is a bias, the pre0 channel mix);
    4.         y = relu(y) if relu_before          (Conv2dPlan's relu_before_residual);
    5.         y = y + residual[p][o]              (if any);
    6.         y = relu(y) if relu_after           (the ReLU of conv1x1 / taps / stems / small / to16; Conv2dPlan's relu_after_residual).

Steps 3-6 are the epilogues of csrc/conv1x1.hip, csrc/conv2d_taps.hip and csrc/conv2d_mfma.hip (``fmaf(acc, sc, sh)``, + residual, max).

``disp_head_ref``: out = depth_max * sigmoid(conv3x3(x, w, pad 1) + b), then nearest x``upscale`` of the output map.

Error magnitude ``A`` (the same pipeline on absolute values): A = (|w| * |x|) * |scale| + |shift| + |residual| (a ReLU does not add to it);
``disp_head``: A = depth_max * (A_conv / 4 + 1), since |sigmoid'| <= 1/4 carries the convolution's error and the sigmoid itself errs by a
few ulp of a value <= 1.  A kernel passes when every element satisfies |gpu - ref| <= c_route * 2^-24 * A.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
# test-only knob: plausible kernel mistakes (tests/test_conv2d_ref_cpu.py asserts the bound rejects each)
MISTAKES = ("drop_corner_tap", "right_pad_wraps", "stride2_from_1", "dilation_1", "relu_before_residual", "ignore_residual",
            "shift_before_scale", "neighbour_shift", "bilinear_upsample")


def _cpu64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def out_size(H, W, k, stride, pad, dilation=1, upsample=False):
    u = 2 if upsample else 1
    span = dilation * (k - 1) + 1
    return (u * H + 2 * pad - span) // stride + 1, (u * W + 2 * pad - span) // stride + 1


def _padded(x, pad, mistake):
    """x float64 [N,C,H,W] -> zero-padded [N,C,H+2p,W+2p]; ``right_pad_wraps``: the right padding columns hold the first pixels of the next
    row (a flat pixel index without the column bound check; the last row wraps to zeros)"""
    xp = F.pad(x, (pad, pad, pad, pad))
    if mistake == "right_pad_wraps" and pad > 0:
        H, W = x.shape[2], x.shape[3]
        nxt = torch.cat([x[:, :, 1:, :pad], torch.zeros_like(x[:, :, :1, :pad])], 2)
        xp[:, :, pad:pad + H, pad + W:] = nxt
    return xp


def conv2d_ref(x, weight, scale=None, shift=None, *, stride=1, pad=None, dilation=1, relu_before=False, residual=None, relu_after=False,
               upsample=False, points=None, mistake=None):
    """Expected result of the convolution (module docstring) in float64 and its error magnitude A.
    x NHWC [N,H,W,cin] (any device); weight [cout,cin,k,k] as nn.Conv2d holds it; residual NHWC of the output shape.
    ``points`` (long [P,3] of output pixels (n, y, x)): evaluate there only, from the input gathered on the device.
    ``mistake``: one of MISTAKES, a deliberately wrong variant for the discrimination test (whole-map form only).
    Returns (ref, A): float64 CPU [N,Ho,Wo,cout], or [P,cout] with ``points``."""
    assert mistake is None or mistake in MISTAKES, mistake
    k = weight.shape[2]
    pad = dilation * (k // 2) if pad is None else pad
    w = _cpu64(weight)
    cout = w.shape[0]
    sc = _cpu64(scale) if scale is not None else torch.ones(cout, dtype=torch.float64)
    sh = _cpu64(shift) if shift is not None else torch.zeros(cout, dtype=torch.float64)
    if points is None:
        xc = _cpu64(x).permute(0, 3, 1, 2)
        if upsample:
            xc = F.interpolate(xc, scale_factor=2, mode="bilinear" if mistake == "bilinear_upsample" else "nearest")
        wv, dil, pv = w, dilation, pad
        if mistake == "drop_corner_tap":
            wv = w.clone()
            wv[:, :, k - 1, k - 1] = 0.0
        if mistake == "dilation_1":
            dil, pv = 1, pad - (dilation - 1) * (k // 2)
        xp = _padded(xc, pv, mistake)
        if mistake == "stride2_from_1" and stride == 2:
            xp = F.pad(xp[:, :, 1:, 1:], (0, 1, 0, 1))
        z = F.conv2d(xp, wv, stride=stride, dilation=dil).permute(0, 2, 3, 1)
        za = F.conv2d(_padded(xc.abs(), pad, None), w.abs(), stride=stride, dilation=dilation).permute(0, 2, 3, 1)
        res = _cpu64(residual)
    else:
        if mistake is not None:
            raise ValueError("mistakes are evaluated on whole maps only")
        z, za = _sampled(x, w, points, stride, pad, dilation, upsample)
        res = None
        if residual is not None:
            p = points.to(residual.device)
            res = residual[p[:, 0], p[:, 1], p[:, 2]].double().cpu()
    if mistake == "shift_before_scale":
        y = (z + sh) * sc
    elif mistake == "neighbour_shift":
        y = z * sc + torch.roll(sh, -1)
    else:
        y = z * sc + sh
    A = za * sc.abs() + sh.abs()
    if relu_before or (mistake == "relu_before_residual" and relu_after and residual is not None):
        y = y.clamp_min(0.0)
    if res is not None and mistake != "ignore_residual":
        y = y + res
    if res is not None:
        A = A + res.abs()
    if relu_after:
        y = y.clamp_min(0.0)
    return y, A


def _sampled(x, w, points, stride, pad, dilation, upsample):
    """z and |w| * |x| at output pixels ``points`` [P,3]: the k x k windows gathered from x on its device (zero outside the map)"""
    N, H, W, C = x.shape
    k = w.shape[2]
    u = 2 if upsample else 1
    p = points.to(x.device)
    zs, zas = 0.0, 0.0
    for ky in range(k):
        for kx in range(k):
            yy = p[:, 1] * stride - pad + ky * dilation
            xx = p[:, 2] * stride - pad + kx * dilation
            ok = (yy >= 0) & (yy < u * H) & (xx >= 0) & (xx < u * W)
            v = x[p[:, 0], (yy.clamp(0, u * H - 1) // u), (xx.clamp(0, u * W - 1) // u)].double()
            v = torch.where(ok[:, None], v, torch.zeros_like(v)).cpu()
            zs = zs + v @ w[:, :, ky, kx].t()
            zas = zas + v.abs() @ w[:, :, ky, kx].abs().t()
    return zs, zas


def disp_head_ref(x, weight, bias, depth_max, upscale=1, points=None, mistake=None):
    """depth_max * sigmoid(conv3x3(x, weight, pad 1) + bias), nearest x``upscale`` -> (ref, A) float64 CPU [N,1,uH,uW], or [P] at output
    pixels ``points`` [P,3] = (n, Y, X) of the upscaled map.  ``mistake="bilinear_upsample"``: bilinear instead of nearest."""
    assert mistake in (None, "bilinear_upsample"), mistake
    if points is not None:
        if mistake is not None:
            raise ValueError("mistakes are evaluated on whole maps only")
        q = points.clone()
        q[:, 1:] //= upscale
        z, za = _sampled(x, _cpu64(weight), q, 1, 1, 1, False)
        z, za = z[:, 0] + float(bias.reshape(-1)[0]), za[:, 0] + abs(float(bias.reshape(-1)[0]))
        return depth_max * torch.sigmoid(z), depth_max * (za / 4.0 + 1.0)
    z, za = conv2d_ref(x, weight, None, bias.reshape(-1), stride=1, pad=1)
    z, za = z.permute(0, 3, 1, 2), za.permute(0, 3, 1, 2)
    y, A = depth_max * torch.sigmoid(z), depth_max * (za / 4.0 + 1.0)
    if upscale != 1:
        y = F.interpolate(y, scale_factor=upscale, mode="bilinear" if mistake == "bilinear_upsample" else "nearest")
        A = F.interpolate(A, scale_factor=upscale, mode="nearest")
    return y, A


def bound_ratio(got, ref, A):
    """max over the elements of |got - ref| / (2^-24 A) (inf where got is NaN and ref is not)"""
    got = got.detach().to("cpu", torch.float64)
    err = (got - ref).abs()
    err = torch.where(torch.isnan(got) & ~torch.isnan(ref), torch.full_like(err, math.inf), err)
    return float((err / (U * A.clamp_min(1e-300))).max()) if err.numel() else 0.0


def check_bound(got, ref, A, c_route, what=""):
    """the per-element bound |got - ref| <= c_route 2^-24 A; returns the worst per-element ratio"""
    ratio = bound_ratio(got, ref, A)
    assert ratio <= c_route, "%s: |gpu - ref| reaches %.2f x 2^-24 A (bound %g)" % (what, ratio, c_route)
    return ratio
