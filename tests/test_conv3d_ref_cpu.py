"""The fp64 reference of tests/conv3d_ref.py (the bound tests/test_gpu_conv3d_routes.py holds every 3D-convolution route to) on the CPU:
  * the per-element bound discriminates: each plausible kernel mistake of conv3d_ref.MISTAKES, evaluated by the same reference, fails it
    against the correct result even at the loosest route constant;
  * the reference agrees with the pinned oracle's Conv3d + BatchNorm3d + activation (oracle/ref_model.convbn3d) for relu, tanh and none;
  * the sampled-voxel form (gathered 3x3x3 patches) equals the whole-volume form."""
import numpy as np
import pytest
import torch

import conv3d_ref as R
from test_gpu_conv3d_routes import C_ROUTE

SHAPES = [(1, 3, 9, 17), (2, 2, 7, 15)]          # ragged against the 8 x 16 / 16 x 16 tiles of the kernels
C_MAX = max(C_ROUTE.values())


def _plan(n_in, n_out, seed, extra=False):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n_out, n_in, 3, 3, 3, generator=g, dtype=torch.float64).float() / np.sqrt(27.0 * n_in)
    sc = torch.rand(n_out, generator=g) + 0.5
    sh = torch.randn(n_out, generator=g) * 0.3
    if n_out == 33:       # dres2's layout: scalar channel first in the input, output channel 32 last
        return dict(weight=w, main_idx=list(range(1, 33)), extra_idx=0, out_idx=list(range(33)), n_tiles=3, scale=sc, shift=sh)
    return dict(weight=w, main_idx=list(range(32)), extra_idx=32 if extra else None, out_idx=list(range(n_out)),
                n_tiles=n_out // 16, scale=sc, shift=sh)


def _inputs(dims, seed, n_tiles=2, extra=False, stride=32):
    g = torch.Generator().manual_seed(seed)
    N, D, H, W = dims
    t = lambda *s: torch.randn(*s, generator=g)                               # noqa: E731
    kw = dict(x=t(N, D, H, W, 32), dims=dims, out=t(N, D, H, W, stride), out_stride=stride)
    if extra or n_tiles == 3:
        kw["in_extra"] = t(N, D, H, W)
    if n_tiles == 3:
        kw["out_extra"] = torch.empty(N, D, H, W)
    return kw, (t(N, D, H, W, stride), t(N, D, H, W, stride))


def _rejected(good, bad, key):
    ratio = R.bound_ratio(bad[key].float(), good[key], good[key + "_A"])
    return ratio > C_MAX, ratio


@pytest.mark.parametrize("dims", SHAPES)
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_bound_rejects_each_plausible_kernel_mistake(dims, mistake):
    # the case that exposes the mistake: a 33 -> 33 plan for the channel-32 activation, the full read-back epilogue otherwise
    if mistake == "xout_identity":
        plan = dict(_plan(33, 33, 1), act_a="relu")
        kw, _ = _inputs(dims, 2, n_tiles=3)
        key = "extra"
    else:
        plan = dict(_plan(32, 32, 3), act_a="tanh", act_b="relu", act_split=16)
        kw, (r1, r2) = _inputs(dims, 4)
        kw.update(residual=r1, residual2=r2, out_scale=0.5, accumulate=True)
        key = "out"
    good = R.conv3d_ref(**plan, **kw)
    bad = R.conv3d_ref(**plan, **kw, mistake=mistake)
    # the correct result itself, rounded to fp32, sits far inside the bound
    assert R.bound_ratio(good[key].float(), good[key], good[key + "_A"]) <= 2.0
    rej, ratio = _rejected(good, bad, key)
    assert rej, "%s slips under the bound (worst ratio %.1f <= %g)" % (mistake, ratio, C_MAX)


@pytest.mark.parametrize("act", ["relu", "tanh", "none"])
def test_reference_agrees_with_the_oracle_convbn3d(act):
    from oracle import ref_model as M
    dims = (2, 3, 9, 17)
    g = torch.Generator().manual_seed(11)
    w = torch.randn(32, 32, 3, 3, 3, generator=g) * 0.06
    bn = (torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.3, torch.randn(32, generator=g) * 0.1,
          torch.rand(32, generator=g) + 0.5)
    P = {"l.0.weight": w.numpy(), "l.1.weight": bn[0].numpy(), "l.1.bias": bn[1].numpy(), "l.1.running_mean": bn[2].numpy(),
         "l.1.running_var": bn[3].numpy()}
    x = torch.randn(*dims, 32, generator=g)
    want = M.convbn3d(P, "l", x.permute(0, 4, 1, 2, 3).numpy(), act)            # [N, C, D, H, W] float32
    sc = bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)
    sh = bn[1].double() - bn[2].double() * sc
    got = R.conv3d_ref(w, list(range(32)), None, list(range(32)), 2, sc, sh, act_a=act, x=x, dims=dims, out=torch.zeros(*dims, 32))
    ref = got["out"].permute(0, 4, 1, 2, 3).numpy()
    assert np.abs(want - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    # and the oracle's fp32 result lies inside the direct kernel's bound
    assert R.bound_ratio(torch.from_numpy(want).permute(0, 2, 3, 4, 1), got["out"], got["out_A"]) <= C_MAX


def test_sampled_voxels_equal_the_whole_volume():
    dims = (2, 3, 9, 17)
    for n_out, extra in ((33, True), (32, False)):
        plan = dict(_plan(33 if extra else 32, n_out, 5, extra=extra), act_a="tanh", act_b="relu", act_split=32 if n_out == 33 else 20)
        kw, (r1, _) = _inputs(dims, 6, n_tiles=plan["n_tiles"], extra=extra)
        if n_out == 32:
            kw.update(residual=r1, accumulate=True, out_scale=0.25)
        ru = torch.randn(*dims, 32)
        gate = (ru, torch.tensor([0.1, 1.3, 0.0, 0.0]), torch.rand(16) + 0.5, torch.randn(16) * 0.2) if n_out == 32 else None
        full = R.conv3d_ref(**plan, **kw, gate=gate)
        pts = torch.tensor([[1, 2, 8, 16], [0, 0, 0, 0], [1, 1, 4, 15], [0, 2, 8, 0], [1, 0, 3, 7]])
        part = R.conv3d_ref(**plan, **kw, gate=gate, points=pts)
        at = lambda t: t[pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]]           # noqa: E731
        for k in ("out", "out_A") + (("extra", "extra_A") if n_out == 33 else ()):
            assert torch.allclose(part[k], at(full[k]), rtol=1e-12, atol=1e-12), k
