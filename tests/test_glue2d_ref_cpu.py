"""The fp64 reference of tests/glue2d_ref.py (the bound tests/test_gpu_glue2d_routes.py holds every 2D glue kernel to) on the CPU:
  * ``compare`` discriminates: each plausible kernel mistake of glue2d_ref.MISTAKES, evaluated by the same reference, is rejected at the
    route's own constant, while the reference rounded to fp32 passes against itself;
  * the references agree with the torch modules they stand for (BatchNorm2d + add + ReLU, F.interpolate(bilinear, align_corners=False),
    MaxPool2d(3, 2, 1), AvgPool2d(k, k), cat / permute, nearest x2) evaluated in float64;
  * the position term of the bilinear blend vanishes where the coordinates are exact, and covers a coordinate evaluated in fp32."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue2d_ref as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _spp_inputs(seed, N=2, H=5, W=7, cr=4, cs=4, cb=4, maps=((1, 1), (2, 3))):
    g = _g(seed)
    raw, skip = torch.randn(N, H, W, cr, generator=g), torch.randn(N, H, W, cs, generator=g)
    return raw, skip, [torch.randn(N, bh, bw, cb, generator=g) for bh, bw in maps]


def _pair(mistake):
    """-> (route constant, good (ref, A, pos), bad value) on inputs that expose the mistake"""
    g = _g(len(mistake))
    if mistake in ("relu_before_residual", "neighbour_group_affine"):
        x, r = torch.randn(2, 7, 9, 36, generator=g), torch.randn(2, 7, 9, 36, generator=g)
        s, t = torch.rand(36, generator=g) + 0.5, torch.randn(36, generator=g) * 0.3
        good = R.bn_act_ref(x, s, t, r, True) + (None,)
        return R.C_ROUTE["bn_act"], good, R.bn_act_ref(x, s, t, r, True, mistake=mistake)[0]
    if mistake in ("align_corners_true", "branch_order_swapped", "y1_not_clamped"):
        raw, skip, brs = _spp_inputs(7, maps=((2, 3), (3, 2)))
        return R.C_ROUTE["spp_upsample_cat"], R.spp_upsample_cat_ref(raw, skip, brs), R.spp_upsample_cat_ref(raw, skip, brs, mistake=mistake)[0]
    if mistake in ("avgpool_ceil", "avgpool_valid_divisor"):
        x = torch.randn(2, 7, 9, 4, generator=g)
        return R.c_avgpool(2), R.avgpool_ref(x, 2) + (None,), R.avgpool_ref(x, 2, mistake=mistake)[0]
    if mistake in ("maxpool_zero_pad", "maxpool_drops_nan"):
        x = torch.randn(2, 7, 8, 4, generator=g) - 3.0            # mostly negative: a zero padding wins the border windows
        x[0, 3, 3, 1] = math.nan
        x[1, :3, :3, 2] = -math.inf                                # the window of output (0, 0) is all -inf
        return R.C_ROUTE["maxpool"], R.maxpool3x3s2_ref(x) + (None,), R.maxpool3x3s2_ref(x, mistake=mistake)[0]
    if mistake == "upsample_round_up":
        x, skip = torch.randn(2, 3, 5, 4, generator=g), torch.randn(2, 6, 10, 12, generator=g)
        return R.C_ROUTE["upsample2_cat"], R.upsample2_cat_ref(x, skip) + (None,), R.upsample2_cat_ref(x, skip, mistake=mistake)[0]
    if mistake in ("relu_on_a", "planes_tail_dropped"):
        a, b = torch.randn(2, 3, 5, 13, generator=g), torch.randn(2, 2, 5, 13, generator=g)
        return R.C_ROUTE["planes_cat"], R.planes_cat_ref(a, b, True) + (None,), R.planes_cat_ref(a, b, True, mistake=mistake)[0]
    assert mistake == "normalise_scale_folded"
    imgs = torch.rand(2, 3, 16, 16, generator=g) * 255.0
    return R.C_ROUTE["normalise"], R.normalise_ref(imgs) + (None,), R.normalise_ref(imgs, mistake=mistake)[0]


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_compare_rejects_each_plausible_kernel_mistake(mistake):
    c, (good, A, pos), bad = _pair(mistake)
    assert R.compare(good.float(), good, A, c, pos, "reference against itself") <= 1.0
    if mistake.startswith("avgpool"):           # mistakes of the output size: the shape check rejects them, the common windows are right
        assert bad.shape != good.shape and torch.equal(bad[:, :good.shape[1], :good.shape[2]], good)
    else:
        assert bad.shape == good.shape          # every other mistake is rejected by a value
    with pytest.raises(AssertionError):
        R.compare(bad.float(), good, A, c, pos, mistake)


def test_mistakes_cover_what_the_suite_promises():
    """one entry per mistake the GPU suite's docstring names"""
    assert len(set(R.MISTAKES)) == len(R.MISTAKES) >= 11
    assert R.c_avgpool(1) == 1.0 and R.c_avgpool(8) == 64.0


# ------------------------------------------------------------------------------------------------ the references against torch in fp64
@pytest.mark.parametrize("relu,res", [(r, s) for r in (False, True) for s in (False, True)])
def test_bn_act_ref_is_batchnorm_add_relu(relu, res):
    g = _g(3)
    bn = torch.nn.BatchNorm2d(8).eval().double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(8, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(8, generator=g))
        bn.running_mean.copy_(torch.randn(8, generator=g))
        bn.running_var.copy_(torch.rand(8, generator=g) + 0.5)
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    t = bn.bias - bn.running_mean * s
    x, r = torch.randn(2, 3, 5, 8, generator=g), torch.randn(2, 3, 5, 8, generator=g)
    with torch.no_grad():
        want = bn(x.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    if res:
        want = want + r.double()
    if relu:
        want = torch.relu(want)
    got, A = R.bn_act_ref(x, s.detach(), t.detach(), r if res else None, relu)
    assert torch.allclose(got, want, rtol=0, atol=1e-13)
    assert bool((A >= got.abs() - 1e-13).all())


def test_bn_act_ref_relu_turns_nan_into_zero():
    x = torch.tensor([[math.nan, -1.0, 2.0, math.nan]])
    one, zero = torch.ones(4), torch.zeros(4)
    assert R.bn_act_ref(x, one, zero, None, True)[0].tolist() == [[0.0, 0.0, 2.0, 0.0]]
    assert bool(torch.isnan(R.bn_act_ref(x, one, zero, None, False)[0][0, 0]))
    a, b = torch.zeros(1, 1, 1, 2), torch.tensor([math.nan, -2.0]).reshape(1, 1, 1, 2)
    assert R.planes_cat_ref(a, b, True)[0][0, 0, :, 1].tolist() == [0.0, 0.0]
    assert bool(torch.isnan(R.planes_cat_ref(a, b, False)[0][0, 0, 0, 1]))


@pytest.mark.parametrize("maps,hw", [(((1, 1), (2, 3)), (5, 7)), (((5, 7),), (5, 7)), (((1, 1),), (1, 1)), (((7, 10), (3, 5)), (30, 40))])
def test_spp_ref_is_bilinear_interpolate_and_cat(maps, hw):
    raw, skip, brs = _spp_inputs(11, H=hw[0], W=hw[1], maps=maps)
    ref, A, pos = R.spp_upsample_cat_ref(raw, skip, brs)
    ups = [F.interpolate(b.double().permute(0, 3, 1, 2), size=hw, mode="bilinear", align_corners=False).permute(0, 2, 3, 1) for b in brs]
    want = torch.cat([raw.double(), skip.double()] + ups, 3)
    assert ref.shape == want.shape
    # torch evaluates the source coordinate in fp64 from an fp64 scale; the reference from the kernel's fp32 scale: within the position term
    assert bool(((ref - want).abs() <= pos + 1e-12).all())
    assert bool((A[..., :8] == 0).all()) and bool((pos[..., :8] == 0).all())
    for k, (bh, bw) in enumerate(maps):
        if (bh, bw) == hw:            # exact coordinates: a copy, no position term
            sl = slice(8 + 4 * k, 12 + 4 * k)
            assert torch.equal(ref[..., sl], brs[k].double()) and bool((pos[..., sl] == 0).all())


def test_spp_position_term_covers_an_fp32_coordinate():
    """the blend evaluated at coordinates computed in fp32, contracted (one rounding) or not (two), stays within pos of the reference"""
    raw, skip, brs = _spp_inputs(5, H=30, W=40, maps=((7, 10), (3, 5)))
    ref, A, pos = R.spp_upsample_cat_ref(raw, skip, brs)
    for contracted in (False, True):
        outs = [raw.double(), skip.double()]
        for b in brs:
            bh, bw = b.shape[1:3]
            coords = []
            for n_src, n_dst in ((bh, 30), (bw, 40)):
                sc = np.float32(n_src) / np.float32(n_dst)
                d = np.arange(n_dst, dtype=np.float32) + np.float32(0.5)
                if contracted:
                    s = (sc.astype(np.float64) * d.astype(np.float64) - 0.5).astype(np.float32)
                else:
                    s = (sc * d).astype(np.float32) - np.float32(0.5)
                coords.append(torch.from_numpy(np.maximum(s, np.float32(0)).astype(np.float64)))
            sy, sx = coords
            y0, y1, ly = R._cell(sy, bh)
            x0, x1, lx = R._cell(sx, bw)
            ly, lx = ly.reshape(1, -1, 1, 1), lx.reshape(1, 1, -1, 1)
            bd = b.double()
            r0, r1 = bd.index_select(1, y0), bd.index_select(1, y1)
            outs.append((1 - ly) * ((1 - lx) * r0.index_select(2, x0) + lx * r0.index_select(2, x1))
                        + ly * ((1 - lx) * r1.index_select(2, x0) + lx * r1.index_select(2, x1)))
        got = torch.cat(outs, 3)
        assert bool(((got - ref).abs() <= pos + 1e-13 * A).all()), contracted
    assert float(pos.max()) < 1e-4          # a few ulp of a coordinate (< 10) times a texel difference (< 8): no room for a wrong tap


@pytest.mark.parametrize("H,W", [(1, 1), (2, 7), (7, 8), (8, 2)])
def test_maxpool_ref_is_maxpool2d(H, W):
    x = torch.randn(2, H, W, 4, generator=_g(H * 10 + W))
    x[0, 0, 0, 0] = -math.inf
    want = F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    got, A = R.maxpool3x3s2_ref(x)
    assert torch.equal(got, want) and bool((A == 0).all())
    x[1, H // 2, W // 2, 1] = math.nan
    got = R.maxpool3x3s2_ref(x)[0]
    want = F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got).any())


@pytest.mark.parametrize("k,H,W", [(1, 3, 5), (2, 7, 9), (5, 5, 13), (8, 8, 17)])
def test_avgpool_ref_is_avgpool2d(k, H, W):
    x = torch.randn(2, H, W, 4, generator=_g(k))
    got, A = R.avgpool_ref(x, k)
    assert got.shape == (2, H // k, W // k, 4)
    win = x.double()[:, :k, :k].sum((1, 2)) / (k * k)
    assert torch.allclose(got[:, 0, 0], win, rtol=0, atol=1e-14)
    assert bool((A >= got.abs() - 1e-14).all())


def test_layout_refs_are_cat_and_permute():
    g = _g(2)
    a, b = torch.randn(2, 3, 4, 5, generator=g), torch.randn(2, 2, 4, 5, generator=g)
    assert torch.equal(R.planes_cat_ref(a, b, True)[0], torch.cat([a, torch.relu(b)], 1).permute(0, 2, 3, 1).double())
    x = torch.randn(2, 4, 5, 6, generator=g)
    assert torch.equal(R.nhwc_to_planes_ref(x)[0], x.permute(0, 3, 1, 2).double())
    lo, skip = torch.randn(2, 2, 3, 4, generator=g), torch.randn(2, 4, 6, 8, generator=g)
    up = F.interpolate(lo.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(R.upsample2_cat_ref(lo, skip)[0], torch.cat([up, skip], 3).double())
    imgs = torch.rand(1, 3, 4, 4, generator=g) * 255.0
    assert torch.equal(R.normalise_ref(imgs)[0].float(), (2 * (imgs / 255.) - 1.).permute(0, 2, 3, 1))


def test_compare_rejects_a_wrong_shape_and_a_flipped_bit():
    x = torch.randn(1, 2, 2, 4, generator=_g(1))
    ref, A = R.nhwc_to_planes_ref(x)
    with pytest.raises(AssertionError):
        R.compare(x, ref, A, 0.0)
    y = ref.float().clone()
    assert R.compare(y, ref, A, 0.0) == 0.0
    y.view(torch.int32)[0, 0, 0, 0] ^= 1
    with pytest.raises(AssertionError):
        R.compare(y, ref, A, 0.0)
