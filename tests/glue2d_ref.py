"""fp64 reference of the 2D glue contracts of the library (include/estd_hip.h) as the ops spell them: ``ops.bn_act_nhwc_``,
``ops.spp_upsample_cat``, ``ops.maxpool3x3s2_nhwc``, ``ops.avgpool_nhwc``, ``ops.planes_cat_nhwc``, ``ops.nhwc_to_planes``,
``ops.upsample2_cat_nhwc`` and ``ops.normalise_nhwc``.  A plain helper module of the test suite (not a conftest).

Every function evaluates its contract in float64 from the fp32 inputs and returns ``(ref, A)`` (``spp_upsample_cat_ref``: ``(ref, A, pos)``):
the expected value, the error magnitude per element and, for the bilinear blend, a position term.  ``compare`` asserts, element by element,

    |gpu - ref| <= C * 2^-24 * A + pos

with the route constant C of ``C_ROUTE`` (``c_avgpool(k)`` for the average).  u = 2^-24 is the unit roundoff of fp32; a correctly rounded
operation errs by at most u |result|, and a sum of n terms evaluated in any order by at most (n - 1) u sum|x_i| (Rump 2012, no
second-order term).  C = 0 means bits: every element equals the fp32 value of the reference bit for bit (a NaN included).

The constants, from the rounding count of each contract:

    planes_cat, nhwc_to_planes, upsample2_cat     copies (and a ReLU, which rounds nothing): C = 0.
    maxpool3x3s2    a selection, no rounding: C = 0.  The window is scanned in row-major order with ATen's comparison
                    (v > m or v is NaN) from m = -inf: taps outside the map are skipped (padding = -inf), a NaN in the window is the
                    result, a window of -inf gives -inf.
    normalise       2 * (x / 255) - 1 in three fp32 roundings, contraction off: the reference IS the three fp32 CPU ops of the model
                    (``x / 255.0``, ``2 * q``, ``d - 1``), so C = 0 keeps the bit identity the existing test has.
    bn_act          y = x * s + t: one rounding of the product (u |x s|) and one of the sum (u |x s + t|), or one in all when the
                    compiler contracts them to an fma; + residual: one more (u |y + r|); the ReLU rounds nothing.  With
                    A = |x| |s| + |t| + |r| every rounded intermediate is <= A, so the error is <= 3 u A: C = 3 (2 without residual, 1
                    contracted -- both pass under 3).
    avgpool         k * k - 1 additions (the first adds to an exact 0) and one division: with A = sum|x| / k^2 the sum errs by
                    (k^2 - 1) u sum|x| and the division by u |s / k^2| <= u A: C = k * k - 1 + 1 = ``c_avgpool(k)``.
    spp_upsample_cat  raw / skip: copies, A = 0 (bits).  A branch channel is v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)
                    with lx = sx - x0, ly = sy - y0 (exact: sx >= 0 and x0 = floor(sx)), hx = fl(1 - lx), hy = fl(1 - ly) (one
                    rounding each).  The longest path (v00) passes hx (u), hx * v00 (u), the inner sum (u), hy (u), the product with
                    hy (u) and the outer sum (u): with A = hy (hx |v00| + lx |v01|) + ly (hx |v10| + lx |v11|) the blend errs by at most
                    6 u A, fewer where fmas are contracted: C = 6.
                    The source coordinate s = scale * (dst + 0.5) - 0.5, scale = fl(bh / H), clamped at 0, is evaluated in fp32 by the
                    kernel -- contracted to one fma or not -- and in fp64 here along the same sequence; the running bound e of its fp32
                    roundings (``sweep_fusion_ref.E``, the non-contracted sequence: the larger one) gives the position tolerance
                    delta = C_POS * e per axis, and pos = delta_y G_y + delta_x G_x with G the largest |difference of neighbouring texels|
                    along that axis in the cells the tolerance can reach (the blend is continuous across a cell edge and across the
                    clamp at 0, so a floor taken on the other side of an integer is covered by the same term).  A branch of the output's
                    own size has scale = 1 and exact coordinates: pos = 0.

ReLU and NaN: ``bn_act`` (``fmaxf(v, 0)``) and ``planes_cat`` (``v > 0 ? v : 0``) turn a NaN into 0 where torch's ReLU propagates it; the
references spell the kernels' form (``where(v > 0, v, 0)``).
"""
import math

import torch
import torch.nn.functional as F

import sweep_fusion_ref as S

U = 2.0 ** -24
C_POS = S.C_POS
_f64 = torch.float64

# per-element bound constants, in units of 2^-24 A (derivations above; the worst ratios measured on an MI355X are beside the routes in
# tests/test_gpu_glue2d_routes.py)
C_ROUTE = {
    "bn_act": 3.0,                # measured 1.925
    "spp_upsample_cat": 6.0,      # measured 3.570
    "maxpool": 0.0,
    "planes_cat": 0.0,
    "nhwc_to_planes": 0.0,
    "upsample2_cat": 0.0,
    "normalise": 0.0,
}


def c_avgpool(k):
    """k * k - 1 additions and one division (measured: k = 2 1.815 of 4, k = 4 3.619 of 16, k = 5 2.255 of 25, k = 8 4.288 of 64)"""
    return float(k * k - 1 + 1)


# test-only knob: plausible kernel mistakes (tests/test_glue2d_ref_cpu.py asserts the bound rejects each)
MISTAKES = ("relu_before_residual", "neighbour_group_affine", "align_corners_true", "branch_order_swapped", "y1_not_clamped",
            "avgpool_ceil", "avgpool_valid_divisor", "maxpool_zero_pad", "maxpool_drops_nan", "upsample_round_up", "relu_on_a",
            "planes_tail_dropped", "normalise_scale_folded")


def _c64(t):
    return None if t is None else t.detach().to("cpu", _f64)


def _relu(y):
    """the kernels' ReLU: a NaN becomes 0"""
    return torch.where(y > 0, y, torch.zeros_like(y))


# ------------------------------------------------------------------------------------------------------------------------ bn_act
def bn_act_ref(x, scale, shift, residual=None, relu=False, mistake=None):
    """x[..., C] * scale[C] + shift[C] (+ residual) (ReLU) -> (ref, A) float64 CPU of x's shape.  x may be the whole NHWC map or rows
    gathered from it ([P, C])."""
    assert mistake in (None, "relu_before_residual", "neighbour_group_affine"), mistake
    xc, s, t, r = _c64(x), _c64(scale), _c64(shift), _c64(residual)
    sv, tv = s, t
    if mistake == "neighbour_group_affine":          # scale[c + 1] of the float4 view: the next group of four channels
        sv, tv = torch.roll(s, -4), torch.roll(t, -4)
    y = xc * sv + tv
    A = xc.abs() * s.abs() + t.abs()
    if mistake == "relu_before_residual" and relu:
        y = _relu(y)
    if r is not None:
        y = y + r
        A = A + r.abs()
    if relu:
        y = _relu(y)
    return y, A


# ------------------------------------------------------------------------------------------------------------- spp_upsample_cat
def _src_coord(n_src, n_dst, mistake=None):
    """source coordinate of every destination index along one axis -> (s float64 [n_dst] clamped at 0, delta [n_dst])"""
    d = torch.arange(n_dst, dtype=_f64)
    if mistake == "align_corners_true":
        s = d * ((n_src - 1) / (n_dst - 1)) if n_dst > 1 else torch.zeros_like(d)
        return s, torch.zeros_like(s)
    scale = S.div(S.E(torch.tensor(float(n_src), dtype=_f64)), S.E(torch.tensor(float(n_dst), dtype=_f64)))
    s = S.sub(S.mul(scale, S.E(d + 0.5)), 0.5)        # the non-contracted sequence (the contracted one rounds once less)
    return s.v.clamp_min(0.0), C_POS * s.e


def _cell(s, n):
    """floor index, its clamped upper neighbour and the fraction of the source coordinates s along an axis of n texels"""
    i0 = torch.floor(s).long().clamp_max(n - 1)
    return i0, i0 + (i0 < n - 1).long(), s - i0.to(_f64)


def _G(t, i0, axis):
    """largest |difference of neighbouring texels| of t along ``axis`` in the cells i0 - 1 .. i0 + 1 (clamped), the axis resampled to
    len(i0)"""
    n = t.shape[axis]
    G = None
    for o in (-1, 0, 1):
        a = (i0 + o).clamp(0, n - 1)
        d = (t.index_select(axis, (a + 1).clamp_max(n - 1)) - t.index_select(axis, a)).abs()
        G = d if G is None else torch.maximum(G, d)
    return G


def spp_upsample_cat_ref(raw, skip, branches, mistake=None):
    """cat(raw, skip, bilinear(branch_k -> H x W, align_corners=False) ...) over the channels of NHWC maps -> (ref, A, pos) float64 CPU
    [N,H,W,Cr + Cs + nb Cb]"""
    assert mistake in (None, "align_corners_true", "branch_order_swapped", "y1_not_clamped"), mistake
    r, k = _c64(raw), _c64(skip)
    N, H, W = r.shape[:3]
    vals, As, poss = [r, k], [torch.zeros_like(r), torch.zeros_like(k)], [torch.zeros_like(r), torch.zeros_like(k)]
    brs = [_c64(b) for b in branches]
    if mistake == "branch_order_swapped":
        brs = brs[::-1]
    for b in brs:
        bh, bw = b.shape[1:3]
        sy, dy = _src_coord(bh, H, mistake)
        sx, dx = _src_coord(bw, W, mistake)
        y0, y1, ly = _cell(sy, bh)
        x0, x1, lx = _cell(sx, bw)
        ly, hy, dy = ly.reshape(1, H, 1, 1), (1.0 - ly).reshape(1, H, 1, 1), dy.reshape(1, H, 1, 1)
        lx, hx, dx = lx.reshape(1, 1, W, 1), (1.0 - lx).reshape(1, 1, W, 1), dx.reshape(1, 1, W, 1)
        row0 = b.index_select(1, y0)
        if mistake == "y1_not_clamped":
            # row y0 + 1 read without the clamp: past the last row lies the first row of the next image (zeros after the last image)
            ext = torch.cat([b, torch.cat([b[1:, :1], torch.zeros_like(b[:1, :1])], 0)], 1)
            row1 = ext.index_select(1, y0 + 1)
        else:
            row1 = b.index_select(1, y1)
        v00, v01, v10, v11 = row0.index_select(2, x0), row0.index_select(2, x1), row1.index_select(2, x0), row1.index_select(2, x1)
        vals.append(hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11))
        As.append(hy * (hx * v00.abs() + lx * v01.abs()) + ly * (hx * v10.abs() + lx * v11.abs()))
        Gy = _G(b, y0, 1)                   # [N,H,bw,C]: over the columns x0 - 1 .. x1 + 1 a tolerance in x may reach
        Gy = torch.stack([Gy.index_select(2, (x0 + o).clamp(0, bw - 1)) for o in (-1, 0, 1, 2)]).amax(0)
        Gx = _G(b, x0, 2)                   # [N,bh,W,C]
        Gx = torch.stack([Gx.index_select(1, (y0 + o).clamp(0, bh - 1)) for o in (-1, 0, 1, 2)]).amax(0)
        poss.append(dy * Gy + dx * Gx)
    return torch.cat(vals, 3), torch.cat(As, 3), torch.cat(poss, 3)


# --------------------------------------------------------------------------------------------------------------------- pooling
def maxpool3x3s2_ref(x, mistake=None):
    """MaxPool2d(3, 2, 1) of an NHWC map with ATen's NaN rule -> (ref, A = 0) float64 CPU [N,(H-1)//2+1,(W-1)//2+1,C]"""
    assert mistake in (None, "maxpool_zero_pad", "maxpool_drops_nan"), mistake
    xc = _c64(x)
    N, H, W, C = xc.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad_v = 0.0 if mistake == "maxpool_zero_pad" else -math.inf
    xp = torch.full((N, H + 2, W + 2, C), pad_v, dtype=_f64)
    xp[:, 1:H + 1, 1:W + 1] = xc
    m = torch.full((N, Ho, Wo, C), pad_v if mistake == "maxpool_zero_pad" else -math.inf, dtype=_f64)
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][:, :Ho, :Wo]
            take = v > m
            if mistake != "maxpool_drops_nan":
                take = take | torch.isnan(v)
            m = torch.where(take, v, m)
    return m, torch.zeros_like(m)


def avgpool_ref(x, k, mistake=None):
    """AvgPool2d(k, k) of an NHWC map, floor output size, divisor k * k -> (ref, A) float64 CPU [N,H//k,W//k,C].
    The two mistakes are mistakes of the output SIZE: with the floor size and no padding every window is full, so the windows both
    variants share with the contract hold the contract's values and a valid-tap divisor equals k * k there.  What they get wrong is
    the ragged last row / column of windows that must not exist; ``compare`` rejects them by its shape assertion, not by the value
    bound (tests/test_glue2d_ref_cpu.py asserts exactly that: equal values on the common region, a different shape)."""
    assert mistake in (None, "avgpool_ceil", "avgpool_valid_divisor"), mistake
    xc = _c64(x).permute(0, 3, 1, 2)
    if mistake is None:
        y = F.avg_pool2d(xc, k, k)
        A = F.avg_pool2d(xc.abs(), k, k)
    else:       # ceil output size: the ragged last windows exist; their divisor is k * k (zero padded) or the count of valid taps
        y = F.avg_pool2d(xc, k, k, ceil_mode=True, count_include_pad=True,
                         divisor_override=k * k if mistake == "avgpool_ceil" else None)
        A = F.avg_pool2d(xc.abs(), k, k, ceil_mode=True)
    return y.permute(0, 2, 3, 1).contiguous(), A.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------- layouts
def planes_cat_ref(a, b, relu_b=False, mistake=None):
    """cat([a, relu?(b)], 1) of NCHW stacks as the NHWC map -> (ref, A = 0) float64 CPU [N,H,W,Ca + Cb]"""
    assert mistake in (None, "relu_on_a", "planes_tail_dropped"), mistake
    ac, bc = _c64(a), _c64(b)
    if relu_b:
        if mistake == "relu_on_a":
            ac = _relu(ac)
        else:
            bc = _relu(bc)
    y = torch.cat([ac, bc], 1).permute(0, 2, 3, 1).contiguous()
    if mistake == "planes_tail_dropped":               # the ragged last tile of 64 pixels never written (zeros)
        N, H, W, C = y.shape
        y = y.reshape(N, H * W, C).clone()
        y[:, H * W - (H * W) % 64:] = 0.0
        y = y.reshape(N, H, W, C)
    return y, torch.zeros_like(y)


def nhwc_to_planes_ref(x):
    """NHWC [N,H,W,C] -> NCHW planes -> (ref, A = 0) float64 CPU [N,C,H,W]"""
    y = _c64(x).permute(0, 3, 1, 2).contiguous()
    return y, torch.zeros_like(y)


def upsample2_cat_ref(x, skip, mistake=None):
    """cat([nearest_x2(x), skip], channels) on NHWC maps: out[y][x] reads x[y >> 1][x >> 1] -> (ref, A = 0) float64 CPU [N,H,W,Cx + Cs]"""
    assert mistake in (None, "upsample_round_up"), mistake
    xc, sc = _c64(x), _c64(skip)
    H, W = sc.shape[1:3]
    ys, xs = torch.arange(H), torch.arange(W)
    if mistake == "upsample_round_up":                  # (y + 1) >> 1, clamped to the map
        iy, ix = ((ys + 1) >> 1).clamp_max(H // 2 - 1), ((xs + 1) >> 1).clamp_max(W // 2 - 1)
    else:
        iy, ix = ys >> 1, xs >> 1
    up = xc.index_select(1, iy).index_select(2, ix)
    y = torch.cat([up, sc], 3)
    return y, torch.zeros_like(y)


def normalise_ref(imgs, mistake=None):
    """[N,3,H,W] images in 0..255 -> 2 * (imgs / 255) - 1 as NHWC [N,H,W,3], in the model's three fp32 CPU ops (module docstring)
    -> (ref, A = 0) float64 CPU (every value an fp32 value)"""
    assert mistake in (None, "normalise_scale_folded"), mistake
    x = imgs.detach().to("cpu", torch.float32)
    if mistake == "normalise_scale_folded":             # x * (2 / 255) - 1: two roundings, not the model's three
        y = x * (2.0 / 255.0) - 1.0
    else:
        y = 2 * (x / 255.0) - 1.0
    y = y.permute(0, 2, 3, 1).contiguous().double()
    return y, torch.zeros_like(y)


# ------------------------------------------------------------------------------------------------------------------- the bound
def bits_equal(got, ref):
    """got (fp32) equals the fp32 value of ref bit for bit, NaNs included"""
    g = got.detach().to("cpu", torch.float32).contiguous()
    r = ref.to(torch.float32).contiguous()
    return g.shape == r.shape and torch.equal(g.view(torch.int32), r.view(torch.int32))


def bound_ratio(got, ref, A, pos=None):
    """max over the elements of (|got - ref| - pos)+ / (2^-24 A); inf where an element with A = 0 differs beyond pos, where got is NaN
    and ref is not (or the reverse), or where an infinity does not match"""
    g = got.detach().to("cpu", _f64)
    assert g.shape == ref.shape, "shape %s, expected %s" % (tuple(g.shape), tuple(ref.shape))
    if g.numel() == 0:
        return 0.0
    pos = torch.zeros_like(ref) if pos is None else pos
    same = (g == ref) | (torch.isnan(g) & torch.isnan(ref))
    err = torch.where(same, torch.zeros_like(ref), (g - ref).abs())
    err = torch.nan_to_num(err, nan=math.inf, posinf=math.inf)
    over = (err - pos).clamp_min(0.0)
    ratio = torch.where(over == 0, torch.zeros_like(over), over / (U * A).clamp_min(1e-300))
    ratio = torch.where((A == 0) & (over > 0), torch.full_like(over, math.inf), ratio)
    return float(ratio.max())


def compare(got, ref, A, c, pos=None, what=""):
    """asserts |got - ref| <= c 2^-24 A + pos element by element (c = 0 and no pos: bit identity with the fp32 value of ref); returns the
    worst ratio"""
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(ref.shape))
    if c == 0 and pos is None:
        assert bits_equal(got, ref), "%s: differs from the reference (bits)" % what
        return 0.0
    ratio = bound_ratio(got, ref, A, pos)
    assert ratio <= c, "%s: |gpu - ref| reaches %.3f x 2^-24 A (bound %g)" % (what, ratio, c)
    return ratio
