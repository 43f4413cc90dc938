"""fp64 reference of the plane-sweep and EST-fusion contracts of the library (csrc/plane_sweep.hip, csrc/est_fusion.hip) as the ops
spell them: ``ops.homo_warping_chw`` / ``homo_warping_px_chw``, ``ops.mix1x1``, ``ops.homo_warp_costvol``, ``ops.warp_volume_cdhw`` /
``warp_volume_ex_cdhw``, ``ops.warp_attention`` / ``attention_prewarped``, ``ops.groupnorm_finalize``, ``ops.gru_reset_apply`` /
``gru_blend``, ``ops.softargmin_up``, ``ops.cam_*`` and ``ops.cdhw_to_vol`` / ``vol_to_cdhw``.  A plain helper module of the test suite
(not a conftest).

Every function evaluates its contract in float64 and returns a ``Ref``: the expected value ``val``, the error magnitude ``A`` and a
position term ``pos`` (both in the units of the bound), and for sampling ops the samples that lie within their tolerance of a mask edge
(``amb``) with the value the other side of the mask gives (``alt``).  An element passes when

    |got - val| <= c_route * 2^-24 * A + pos          (or, for an ambiguous sample, the same against alt).

The functions take whole tensors (any device) and evaluate every output element, or ``points`` (long [P] flat output voxel / pixel
indices) to evaluate only there; sources may be given as getters ``get(flat long [...]) -> float64 [..., C]`` so that volumes that only
exist on the device (or as a closed form) are read at the texels a sample needs.

Sample positions (``_sweep_pos``, ``_volume_pos``)
    The kernels repeat the reference's fp32 rounding sequence op for op (``sweep_coords`` / ``volume_coords_base``), and the
    |n| > 1 masks are discontinuous.  Positions are evaluated in float64 from the fp32 matrices, depths and constants the kernel receives,
    along that same sequence, and each operation carries a first-order running bound of the fp32 rounding it makes (class ``E``):
        fl(a + b): e_a + e_b + u|a + b|        fl(a * b): |a| e_b + |b| e_a + u|ab|        fma(a, b, c): |a| e_b + |b| e_a + e_c + u|ab + c|
        fl(a / b): (e_a + |a / b| e_b) / |b| + u|a / b|
    with u = 2^-24 and no rounding term where the inputs are exact and the result is representable in fp32 (identity geometries give
    exact positions).  The position tolerance of an axis is delta = C_POS * e.  A sample is ambiguous when its normalised coordinate lies
    within delta of +-1 or its denominator within C_POS * e_den of 0; ``alt`` then masks the ambiguous axes.
    Sampling: bilinear / trilinear, zero padding, align_corners=False (i = ((n + 1) * size - 1) / 2), a masked coordinate becomes n = 2;
    ``border`` (warp_volume_ex) clips i to [0, size - 1] and reads padding_value on the outer voxel layer.  A non-finite position (den == 0
    exactly) samples zero.

Error magnitudes (``A``; u = 2^-24)
    sample            A = sum_k w_k |t_k| (the interpolation on absolute values);  pos = sum_axis delta_axis * G_axis, G_axis = the largest
                      |difference of neighbouring texels along that axis| in the 4-texel window around the sample (the cell and the cells a
                      delta may move it into).
    homo_warping      the sample.                       mix1x1: A = sum_c |w||in| + |bias|.
    homo_warp_costvol A = |ref_mix| + sample A.         warp_volume / warp_volume_ex: the sample.
    attention         corr_j = <K_t, Kw_j>, a = softmax(corr), h = sum_j a_j Vw_j / n.  A_corr_j = sum |K_t| A(Kw_j);
                      |d a_j / d corr_k| <= a_j (delta_jk + a_k), so
                      A_h = sum_j a_j (A(Vw_j) + |Vw_j| (1 + A_corr_j + sum_k a_k A_corr_k)) / n, and pos likewise with the position terms.
                      The V_t half of the record is a copy: A = 0.
    groupnorm_finalize  mean = S / count, rstd = 1 / sqrt(Q / count - mean^2 + eps) from fp64 sums of the partials (``depth`` sequential
                      fp64 additions per sum).  A_mean = |mean| + 2^-29 depth sum|S_b| / count;
                      A_rstd = rstd (1 + 2^-29 (depth + 3) (Q / count + mean^2) / (var + eps)).  With (Q/count + mean^2)/var = 1 + 2 (mean/std)^2
                      the fp32 results hold to a few ulp for |mean| / std <= GN_RANGE = 2^11 (the extra term <= 2 ulp at 8193 blocks).
    gru_reset_apply   z = (r - mean) rstd g + b, A_z = (|r| + |mean|) |rstd| |g| + |b|;  out = [x | sigmoid(z) h]:
                      A = |h| (A_z / 4 + sigmoid(z)) (|sigmoid'| <= 1/4); the x half is a copy (A = 0).
    gru_blend         out = s h + (1 - s) y, s = sigmoid(z_u), y = tanh(z_o):
                      A = s|h| + (1 - s)|y| + |h - y| (A_zu / 4 + s) + (1 - s)(A_zo + |y|) (|tanh'| <= 1).
                      FAST instances (v_exp / v_rcp, absolute error <= 2e-7 each): + (|h - y| + (1 - s)) * FAST_ABS.
    softargmin_up     p = softmax(l), depth = sum p_d d_d, prob = max p = 1 / sum exp(l - max); n_add = ceil(D / 8) + 8 sequential fp32 adds:
                      A_depth = n_add sum_d p_d (|d_d| + |depth|) (1 + |l_d - max|),  A_prob = prob (1 + n_add + sum_d p_d |l_d - max|).
    cam_*             the same products / inverses with the fp32 roundings of the intermediates the kernels keep; an fp32 intermediate may
                      round the other way, so A carries one ulp of every rounded intermediate through the products, and an inverse
                      multiplies its input's error by cond(X) (``_inv``).
    cdhw_to_vol / vol_to_cdhw   exact copies: A = 0.
"""
import math
from fractions import Fraction

import numpy as np
import torch

U = 2.0 ** -24
C_POS = 2.0                     # position tolerance delta = C_POS * running rounding bound
GN_RANGE = 2.0 ** 11            # |mean| / std up to which groupnorm_finalize's fp32 results hold to a few ulp
FAST_ABS = 4.0                  # 2e-7 absolute (ESTD_GRU_FAST transcendentals) in units of 2^-24
EPS_SWEEP = float(np.float32(1e-8))
EPS_VOL = float(np.float32(1e-10))
# test-only knob: plausible kernel mistakes (tests/test_sweep_fusion_ref_cpu.py asserts the bound rejects each)
MISTAKES = ("align_corners_true", "corner_xy_swapped", "far_corner_dropped", "mask_ge_1", "den_no_eps", "softmax_no_max",
            "no_mean_over_views", "blend_u_swapped", "reset_on_x", "depth_plane_off_by_one", "neighbour_gamma")

_f64 = torch.float64


def _c64(t):
    return t.detach().to("cpu", _f64) if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=_f64)


def fl32(x):
    """the fp32 value of a python float (the constants the kernels hold)"""
    return float(np.float32(x))


class Ref:
    """expected value, error magnitude A, position term pos; ambiguous samples (bool, per element) with their other-side value"""

    def __init__(self, val, A, pos=None, alt=None, amb=None, n_amb=0, n_samples=None):
        self.val, self.A = val, A
        self.pos = torch.zeros_like(val) if pos is None else pos
        self.alt, self.amb = alt, amb
        self.n_amb = n_amb                              # ambiguous samples (sample positions, not elements)
        self.n_samples = n_samples if n_samples is not None else val.shape[0]

    def map(self, f):
        g = lambda t: None if t is None else f(t)       # noqa: E731
        return Ref(g(self.val), g(self.A), g(self.pos), g(self.alt), g(self.amb), self.n_amb, self.n_samples)

    def reshape(self, *shape):
        return self.map(lambda t: t.reshape(*shape))


# ------------------------------------------------------------------------------------------------------ running rounding bounds
class E:
    """an fp64 value and a first-order bound of the fp32 rounding error the kernel's evaluation of it has made"""

    def __init__(self, v, e=None):
        self.v = _c64(v)
        # a non-finite value (a division by an exact zero) is what the kernel holds too: no error to carry
        self.e = torch.zeros_like(self.v) if e is None else torch.where(torch.isfinite(self.v), e, torch.zeros_like(e))


def _k(a):
    return a if isinstance(a, E) else E(torch.tensor(float(a), dtype=_f64))


def _rnd(v, e_in):
    """u|v| unless the operands were exact and v is an fp32 value (then the kernel's result is exact)"""
    exact = ((e_in == 0) & (v.float().double() == v)) | ~torch.isfinite(v)      # NaN / inf: a division by an exact zero
    return torch.where(exact, torch.zeros_like(v), U * v.abs())


def add(a, b):
    a, b = _k(a), _k(b)
    v = a.v + b.v
    e = a.e + b.e
    return E(v, e + _rnd(v, e))


def sub(a, b):
    b = _k(b)
    return add(a, E(-b.v, b.e))


def mul(a, b):
    a, b = _k(a), _k(b)
    v = a.v * b.v
    e = a.v.abs() * b.e + b.v.abs() * a.e
    return E(v, e + _rnd(v, e))


def fma(a, b, c):
    a, b, c = _k(a), _k(b), _k(c)
    v = a.v * b.v + c.v
    e = a.v.abs() * b.e + b.v.abs() * a.e + c.e
    return E(v, e + _rnd(v, e))


def div(a, b):
    a, b = _k(a), _k(b)
    v = a.v / b.v
    e = torch.nan_to_num((a.e + v.abs() * b.e) / b.v.abs(), nan=math.inf)
    e = torch.where((b.v == 0) & (b.e == 0) & (a.e == 0), torch.zeros_like(e), e)     # an exact division by an exact zero
    return E(v, e + _rnd(v, e))


# ------------------------------------------------------------------------------------------------------------- positions
def _axis(n, size, mistake, scale2=False):
    """normalised coordinate n (E) -> (position E unmasked, masked, ambiguous, position when masked) along an axis of ``size``"""
    mask_hi = (n.v >= 1.0) | (n.v <= -1.0) if mistake == "mask_ge_1" else (n.v > 1.0) | (n.v < -1.0)
    amb = ((n.v.abs() - 1.0).abs() <= C_POS * n.e) & (n.e > 0) & torch.isfinite(n.v)
    if mistake == "align_corners_true":
        i = mul(mul(add(n, 1.0), 0.5), float(size - 1))
        i_m = 1.5 * (size - 1)
    else:
        i = mul(sub(mul(add(n, 1.0), float(size)), 1.0), 0.5)
        i_m = (3.0 * size - 1.0) * 0.5
    return i, mask_hi, amb, i_m


def _sweep_pos(P, dv, x, y, H, W, mistake=None):
    """csrc/plane_sweep.hip sweep_coords in fp64 with running bounds -> [(i, masked, amb, i_masked) for y, x], den ambiguity"""
    P = [E(torch.tensor(float(p), dtype=_f64)) for p in _c64(P).reshape(-1)]
    fx, fy, dv = E(x.double()), E(y.double()), E(dv)
    r = [add(fma(P[3 * i + 1], fy, mul(P[3 * i], fx)), P[3 * i + 2]) for i in range(3)]
    p = [add(mul(r[i], dv), P[9 + i]) for i in range(3)]
    den = p[2] if mistake == "den_no_eps" else add(p[2], EPS_SWEEP)
    px, py = div(p[0], den), div(p[1], den)
    xn = sub(div(px, fl32((W - 1) * 0.5)), 1.0)
    yn = sub(div(py, fl32((H - 1) * 0.5)), 1.0)
    amb_den = (den.v.abs() <= C_POS * den.e) & (den.e > 0)
    return [_axis(yn, H, mistake), _axis(xn, W, mistake)], amb_den


def _volume_pos(M, dep, x, y, D, H, W, dmin, dint, disp=None, mistake=None):
    """csrc/est_fusion.hip volume_coords_base (and warp_volume_ex's disparity planes) in fp64 -> [axis tuples for z, y, x], den ambiguity"""
    M = [E(torch.tensor(float(m), dtype=_f64)) for m in _c64(M).reshape(-1)]
    fx, fy, dep = E(x.double()), E(y.double()), E(dep)
    c = [mul(add(fma(M[3 * i + 1], fy, mul(M[3 * i], fx)), M[3 * i + 2]), dep) for i in range(3)]
    s = [add(fma(M[9 + 4 * i + 2], c[2], fma(M[9 + 4 * i + 1], c[1], mul(M[9 + 4 * i], c[0]))), M[9 + 4 * i + 3]) for i in range(3)]
    q = [fma(M[21 + 3 * i + 2], s[2], fma(M[21 + 3 * i + 1], s[1], mul(M[21 + 3 * i], s[0]))) for i in range(3)]
    den = q[2] if mistake == "den_no_eps" else add(q[2], EPS_VOL)
    X, Y, Z = div(q[0], den), div(q[1], den), q[2]
    xn = sub(div(mul(2.0, X), float(W - 1)), 1.0)
    yn = sub(div(mul(2.0, Y), float(H - 1)), 1.0)
    if disp is not None:
        zz = div(sub(div(1.0, add(Z, EPS_VOL)), fl32(disp[0])), fl32(disp[1]))
    else:
        zz = div(sub(Z, fl32(dmin)), fl32(dint))
    zn = sub(div(mul(2.0, zz), float(D - 1)), 1.0)
    amb_den = (den.v.abs() <= C_POS * den.e) & (den.e > 0)
    return [_axis(zn, D, mistake), _axis(yn, H, mistake), _axis(xn, W, mistake)], amb_den


# -------------------------------------------------------------------------------------------------------------- sampling
def _sample(get, dims, pos, border=False, pad_value=0.0, mistake=None):
    """multilinear sample at fp64 positions ``pos`` (one [P] tensor per axis, outermost first) of the source ``get`` with ``dims``
    -> (val [P,C], A [P,C], G [naxes][P,C])"""
    nd = len(dims)
    P = pos[0].shape[0]
    if border:                                                       # fminf(size - 1, fmaxf(i, 0)): NaN -> 0
        pos = [torch.clamp(torch.nan_to_num(p, nan=0.0), 0.0, float(n - 1)) for p, n in zip(pos, dims)]
    fin = torch.ones(P, dtype=torch.bool)
    for p in pos:
        fin &= torch.isfinite(p)
    flo = [torch.where(fin, torch.floor(p), torch.full_like(p, -8.0)) for p in pos]
    frac = [torch.where(fin, p - f, torch.zeros_like(p)) for p, f in zip(pos, flo)]
    offs = torch.tensor([-1, 0, 1, 2])
    idx = [f.long()[:, None] + offs for f in flo]                       # [P,4] per axis
    ok = [(i >= 0) & (i < n) for i, n in zip(idx, dims)]
    # the 4^nd window, flat texel indices in (outer..inner) order
    shp = [P] + [4] * nd
    flat = torch.zeros(shp, dtype=torch.long)
    valid = torch.ones(shp, dtype=torch.bool)
    edge = torch.zeros(shp, dtype=torch.bool)
    for a in range(nd):
        view = [P] + [1] * nd
        view[a + 1] = 4
        ia = idx[a].clamp(0, dims[a] - 1).reshape(view)
        flat = flat * dims[a] + ia
        valid = valid & ok[a].reshape(view)
        edge = edge | ((idx[a] == 0) | (idx[a] == dims[a] - 1)).reshape(view)
    total = int(np.prod(dims))
    tex = get(torch.where(valid, flat, torch.zeros_like(flat)).reshape(P, -1)).reshape(shp + [-1])
    valid_c = valid[..., None]
    if mistake == "far_corner_dropped":
        valid_c = valid_c & (flat != total - 1)[..., None]
    tex = torch.where(valid_c, tex, torch.zeros_like(tex))
    if border:
        tex = torch.where((edge & valid)[..., None], torch.full_like(tex, float(fl32(pad_value))), tex)
    # corners of the cell: window offsets 1, 2 on every axis
    cell = tex[(slice(None),) + (slice(1, 3),) * nd]
    if mistake == "corner_xy_swapped":                               # corner (dy = 0, dx = 1) reads (dy = 1, dx = 0)
        cell = cell.clone()
        cell[(slice(None),) + (slice(None),) * (nd - 2) + (0, 1)] = cell[(slice(None),) + (slice(None),) * (nd - 2) + (1, 0)]
    wgt = torch.ones([P] + [2] * nd, dtype=_f64)
    for a in range(nd):
        view = [P] + [1] * nd
        view[a + 1] = 2
        t = frac[a][:, None]
        wgt = wgt * torch.cat([1.0 - t, t], 1).reshape(view)
    wgt = wgt[..., None]
    red = tuple(range(1, nd + 1))
    val = (wgt * cell).sum(red)
    A = (wgt * cell.abs()).sum(red)
    G = []
    for a in range(nd):
        dif = (tex.narrow(a + 1, 1, 3) - tex.narrow(a + 1, 0, 3)).abs()
        G.append(dif.amax(red))
    return val, A, G


def _sample_at(get, dims, axes, amb_den, border=False, pad_value=0.0, mistake=None):
    """sample through the mask logic -> (val, A, pos, alt, amb [P])"""
    pos_in, pos_alt, amb = [], [], amb_den.clone()
    for (i, masked, a_amb, i_m) in axes:
        im = torch.full_like(i.v, i_m)
        pos_in.append(torch.where(masked, im, i.v))
        pos_alt.append(torch.where(amb_den, im, torch.where(a_amb, torch.where(masked, i.v, im), pos_in[-1])))
        amb |= a_amb
    val, A, G = _sample(get, dims, pos_in, border, pad_value, mistake)
    delta = [torch.where(masked, torch.zeros_like(i.e), C_POS * i.e) for (i, masked, _, _) in axes]
    pos = sum(torch.nan_to_num(d[:, None] * g, nan=math.inf) for d, g in zip(delta, G))
    alt = val.clone()
    if bool(amb.any()):
        sel = amb.nonzero()[:, 0]
        alt[sel] = _sample(get, dims, [p[sel] for p in pos_alt], border, pad_value, mistake)[0]
    return val, A, pos, alt, amb


def _dhw(points, D, H, W):
    d = torch.div(points, H * W, rounding_mode="floor")
    rem = points - d * H * W
    return d, torch.div(rem, W, rounding_mode="floor"), rem % W


def _getter(t, C):
    """a [..., C]-record (channels-last) source on any device -> get(flat) float64 CPU [..., C]"""
    flat_view = t.reshape(-1, C)
    return lambda f: flat_view[f.to(t.device)].to("cpu", _f64)


def _getter_planes(t):
    """a [C, ...] (channels-first) source -> get(flat) [..., C]"""
    C = t.shape[0]
    flat_view = t.reshape(C, -1)
    return lambda f: flat_view[:, f.to(t.device).reshape(-1)].t().reshape(*f.shape, C).to("cpu", _f64)


def _all(n):
    return torch.arange(n, dtype=torch.long)


# ------------------------------------------------------------------------------------------------------- hand-built geometries
T_SWEEP, T_VOL = 2.0 ** -26, 2.0 ** -33          # powers of two with T - eps an fp32 value: den = (T - eps) + eps = T exactly


def exact_sweep_proj():
    """proj12 whose positions are exact in fp32 and fp64: den = T, px = x * dv, py = y * dv (n = +-1 exactly where x * dv = W - 1)"""
    return torch.tensor([T_SWEEP, 0, 0, 0, T_SWEEP, 0, 0, 0, 0, 0, 0, T_SWEEP - EPS_SWEEP], dtype=torch.float32)


def exact_volume_mats():
    """mats30 with exact positions: den = T, X = x * dep, Y = y * dep, Z = T - eps (depth_min = Z puts every sample on n_z = -1)"""
    M = torch.zeros(30, dtype=torch.float32)
    M[[0, 4, 8]] = 1.0
    M[9], M[14], M[20] = T_VOL, T_VOL, T_VOL - EPS_VOL
    M[[21, 25, 29]] = 1.0
    return M, fl32(T_VOL - EPS_VOL)


def den0_sweep_proj():
    """proj12 with projected depth exactly -eps on every plane: den = 0, px = 0 / 0 (NaN), py = +-inf (NaN at y = 0... x = 0)"""
    return torch.tensor([0, 0, 0, 0.5, 1, 0, 0, 0, 0, 0, 0, -EPS_SWEEP], dtype=torch.float32)


def den0_volume_mats():
    """mats30 with q2 = -eps exactly: den = 0, X = 0 / 0, Y = +-inf"""
    M = torch.zeros(30, dtype=torch.float32)
    M[[0, 4, 8]] = 1.0
    M[[13, 14]] = 1.0
    M[20] = -EPS_VOL
    M[[21, 25, 29]] = 1.0
    return M


# ------------------------------------------------------------------------------------------------------------- plane sweep
def homo_warping_ref(src_chw, proj12, depth, D=None, points=None, mistake=None):
    """ops.homo_warping_chw (depth [D] planes) / homo_warping_px_chw (depth [D,H,W]): src [C,H,W] -> [C,D,H,W], or [P,C] at flat
    output voxels ``points`` of (d, y, x)"""
    C, H, W = src_chw.shape
    dep = _c64(depth)
    per_pixel = dep.dim() == 3
    D = dep.shape[0] if per_pixel else D
    pts = _all(D * H * W) if points is None else points.cpu()
    d, y, x = _dhw(pts, D, H, W)
    dv = dep.reshape(-1)[pts] if per_pixel else dep.reshape(-1)[d]
    axes, amb_den = _sweep_pos(proj12, dv, x, y, H, W, mistake)
    val, A, pos, alt, amb = _sample_at(_getter_planes(src_chw), (H, W), axes, amb_den, mistake=mistake)
    r = Ref(val, A, pos, alt, amb[:, None].expand_as(val), int(amb.sum()))
    return r if points is not None else r.map(lambda t: t.t().reshape(C, D, H, W))


def costvol_ref(src_mix, ref_mix, proj12, dvals, D, points=None, mistake=None):
    """ops.homo_warp_costvol: ref_mix[y,x] + bilinear(src_mix) at the homography of plane d -> [D,H,W,32] or [P,32]"""
    H, W, C = src_mix.shape
    pts = _all(D * H * W) if points is None else points.cpu()
    d, y, x = _dhw(pts, D, H, W)
    axes, amb_den = _sweep_pos(proj12, _c64(dvals).reshape(-1)[d], x, y, H, W, mistake)
    val, A, pos, alt, amb = _sample_at(_getter(src_mix, C), (H, W), axes, amb_den, mistake=mistake)
    rf = _getter(ref_mix, C)(y * W + x)
    r = Ref(val + rf, A + rf.abs(), pos, alt + rf, amb[:, None].expand_as(val), int(amb.sum()))
    return r if points is not None else r.reshape(D, H, W, C)


def mix1x1_ref(in_chw, w, bias=None):
    """ops.mix1x1: out[y,x,o] = sum_c w[o,c] in[c,y,x] + bias[o] -> [H,W,Cout]"""
    x = _c64(in_chw)
    Cin, H, W = x.shape
    w = _c64(w)
    b = _c64(bias) if bias is not None else torch.zeros(w.shape[0], dtype=_f64)
    xf = x.reshape(Cin, -1).t()
    val = xf @ w.t() + b
    A = xf.abs() @ w.abs().t() + b.abs()
    return Ref(val.reshape(H, W, -1), A.reshape(H, W, -1))


# ------------------------------------------------------------------------------------------------------------- volume warp
def warp_volume_ref(vol, mats30, depth, dmin, dint, points=None, disp=None, border=False, padding_value=0.0, mistake=None):
    """ops.warp_volume_cdhw (depth [D] planes) / warp_volume_ex_cdhw (depth [D] or per voxel [D,H,W]; ``disp`` = (disp_min,
    disp_interval); ``border`` + padding_value): vol [C,D,H,W] -> [C,D,H,W] or [P,C]"""
    C, D, H, W = vol.shape
    dep = _c64(depth).reshape(-1)
    pts = _all(D * H * W) if points is None else points.cpu()
    d, y, x = _dhw(pts, D, H, W)
    dv = dep[pts] if dep.numel() == D * H * W and D * H * W > D else dep[d]
    axes, amb_den = _volume_pos(mats30, dv, x, y, D, H, W, dmin, dint, disp, mistake)
    val, A, pos, alt, amb = _sample_at(_getter_planes(vol), (D, H, W), axes, amb_den, border, padding_value, mistake)
    r = Ref(val, A, pos, alt, amb[:, None].expand_as(val), int(amb.sum()))
    return r if points is not None else r.map(lambda t: t.t().reshape(C, D, H, W))


def _softmax_h(corr, Ac, pc, Vw, AV, pV, n, mistake):
    """attention over views from per-view corr [P,n], A_corr, pos_corr [P,n] and warped values Vw / A / pos [P,n,16] -> (h, A, pos)"""
    if mistake == "softmax_no_max":
        e = torch.exp(corr).float().double()                          # overflows fp32 as expf(corr) would
        a = e / e.sum(1, keepdim=True)
    else:
        a = torch.softmax(corr, 1)
    nn_ = 1.0 if mistake == "no_mean_over_views" else float(n)
    h = (a[..., None] * Vw).sum(1) / nn_
    sAc = (a * Ac).sum(1, keepdim=True)
    spc = (a * pc).sum(1, keepdim=True)
    A = (a[..., None] * (AV + Vw.abs() * (1.0 + Ac + sAc)[..., None])).sum(1) / n
    pos = (a[..., None] * (pV + Vw.abs() * (pc + spc)[..., None])).sum(1) / n
    return h, A, pos


def warp_attention_ref(kv_t, kv_srcs, mats, dvals, dmin, dint, points=None, mistake=None, dims=None):
    """ops.warp_attention: target [D,H,W,32] = [V | K] records, sources (tensors of that shape or getters with ``dims`` = (D,H,W)),
    mats [n,30] -> xh [D,H,W,32] = [V_t | h] or [P,32]"""
    D, H, W = dims if dims is not None else kv_t.shape[:3]
    n = len(kv_srcs)
    pts = _all(D * H * W) if points is None else points.cpu()
    d, y, x = _dhw(pts, D, H, W)
    tgt = kv_t if callable(kv_t) else _getter(kv_t, 32)
    rec = tgt(pts)
    Vt, Kt = rec[:, :16], rec[:, 16:]
    dv = _c64(dvals).reshape(-1)[d]
    mats = _c64(mats).reshape(n, 30)
    cols = {k: [] for k in ("corr", "Ac", "pc", "V", "AV", "pV", "corr_alt", "V_alt")}
    amb = torch.zeros(pts.shape[0], dtype=torch.bool)
    for j in range(n):
        axes, amb_den = _volume_pos(mats[j], dv, x, y, D, H, W, dmin, dint, None, mistake)
        get = kv_srcs[j] if callable(kv_srcs[j]) else _getter(kv_srcs[j], 32)
        val, A, pos, alt, a_j = _sample_at(get, (D, H, W), axes, amb_den, mistake=mistake)
        amb |= a_j
        cols["corr"].append((Kt * val[:, 16:]).sum(1))
        cols["corr_alt"].append((Kt * alt[:, 16:]).sum(1))
        cols["Ac"].append((Kt.abs() * A[:, 16:]).sum(1))
        cols["pc"].append((Kt.abs() * pos[:, 16:]).sum(1))
        cols["V"].append(val[:, :16])
        cols["V_alt"].append(alt[:, :16])
        cols["AV"].append(A[:, :16])
        cols["pV"].append(pos[:, :16])
    st = {k: torch.stack(v, 1) for k, v in cols.items()}
    h, A, pos = _softmax_h(st["corr"], st["Ac"], st["pc"], st["V"], st["AV"], st["pV"], n, mistake)
    h_alt, _, _ = _softmax_h(st["corr_alt"], st["Ac"], st["pc"], st["V_alt"], st["AV"], st["pV"], n, mistake)
    z = torch.zeros_like(Vt)
    r = Ref(torch.cat([Vt, h], 1), torch.cat([z, A], 1), torch.cat([z, pos], 1), torch.cat([Vt, h_alt], 1),
            torch.cat([torch.zeros_like(Vt, dtype=torch.bool), amb[:, None].expand_as(h)], 1), int(amb.sum()))
    return r if points is not None else r.reshape(D, H, W, 32)


def attention_prewarped_ref(kv_t, kv_srcs, mistake=None):
    """ops.attention_prewarped: attention over already warped [.., 32] records -> [.., 32]"""
    shape = kv_t.shape
    t = _c64(kv_t).reshape(-1, 32)
    Vt, Kt = t[:, :16], t[:, 16:]
    S = [_c64(s).reshape(-1, 32) for s in kv_srcs]
    corr = torch.stack([(Kt * s[:, 16:]).sum(1) for s in S], 1)
    Ac = torch.stack([(Kt.abs() * s[:, 16:].abs()).sum(1) for s in S], 1)
    V = torch.stack([s[:, :16] for s in S], 1)
    h, A, _ = _softmax_h(corr, Ac, torch.zeros_like(Ac), V, V.abs(), torch.zeros_like(V), len(S), mistake)
    return Ref(torch.cat([Vt, h], 1).reshape(shape), torch.cat([torch.zeros_like(Vt), A], 1).reshape(shape))


# ---------------------------------------------------------------------------------------------------------- GroupNorm / GRU
def gn_depth(n_blocks):
    """sequential fp64 additions per sum in groupnorm_finalize_kernel (per-thread loop + the 10-level tree of 1024 threads)"""
    return -(-n_blocks // 1024) + 10


def groupnorm_finalize_ref(partials, count, eps):
    """ops.groupnorm_finalize: partials [n_blocks, 4] = (sum, sum of squares) of group 0 and group 1 -> Ref [4] = (mean0, rstd0, mean1,
    rstd1).  Sums are exact (math.fsum), mean and variance rational, the square root in fp64."""
    p = _c64(partials).reshape(-1, 4)
    depth = gn_depth(p.shape[0])
    val, A = [], []
    for g in range(2):
        S = math.fsum(p[:, 2 * g].tolist())
        Q = math.fsum(p[:, 2 * g + 1].tolist())
        Sa = math.fsum(p[:, 2 * g].abs().tolist())
        mean = Fraction(S) / Fraction(count)
        var = Fraction(Q) / Fraction(count) - mean * mean
        var = max(var, Fraction(0))
        ve = float(var + Fraction(fl32(eps)))
        rstd = 1.0 / math.sqrt(ve)
        m = float(mean)
        val += [m, rstd]
        A += [abs(m) + 2.0 ** -29 * depth * Sa / count,
              rstd * (1.0 + 2.0 ** -29 * (depth + 3) * (Q / count + m * m) / ve)]
    return Ref(torch.tensor(val, dtype=_f64), torch.tensor(A, dtype=_f64))


def _gate(r, mean, rstd, g, b):
    z = (r - mean) * rstd * g + b
    Az = (r.abs() + abs(mean)) * abs(rstd) * g.abs() + b.abs()
    return z, Az


def _rows(t, C, points):
    if points is None:
        return _c64(t).reshape(-1, C)
    return _getter(t, C)(points)


def gru_reset_ref(xh, ru, stats4, gamma, beta, fast=False, points=None, mistake=None):
    """ops.gru_reset_apply: [x | sigmoid(GN(r)) h] -> [n_vox, 32] (or [P,32] at voxels ``points``)"""
    X, R = _rows(xh, 32, points), _rows(ru, 32, points)
    st, g, b = _c64(stats4).reshape(-1), _c64(gamma).reshape(16), _c64(beta).reshape(16)
    if mistake == "neighbour_gamma":
        g = torch.roll(g, -1)
    z, Az = _gate(R[:, :16], float(st[0]), float(st[1]), g, b)
    s = torch.sigmoid(z)
    x, h = X[:, :16], X[:, 16:]
    if mistake == "reset_on_x":
        out = torch.cat([s * x, h], 1)
    else:
        out = torch.cat([x, s * h], 1)
    A = h.abs() * (Az / 4.0 + s + (FAST_ABS if fast else 0.0))
    return Ref(out, torch.cat([torch.zeros_like(x), A], 1))


def gru_blend_ref(xh, ru, o_raw, st_ru, st_o, gu, bu, go, bo, fast=False, points=None, mistake=None):
    """ops.gru_blend: u h + (1 - u) tanh(GN(o)), u = sigmoid(GN(u_raw)) -> [n_vox, 16] (or [P,16])"""
    X, R, O = _rows(xh, 32, points), _rows(ru, 32, points), _rows(o_raw, 16, points)
    sr, so = _c64(st_ru).reshape(-1), _c64(st_o).reshape(-1)
    gu, bu, go, bo = (_c64(t).reshape(16) for t in (gu, bu, go, bo))
    if mistake == "neighbour_gamma":
        gu = torch.roll(gu, -1)
    zu, Azu = _gate(R[:, 16:], float(sr[2]), float(sr[3]), gu, bu)
    zo, Azo = _gate(O, float(so[0]), float(so[1]), go, bo)
    s, yv, h = torch.sigmoid(zu), torch.tanh(zo), X[:, 16:]
    out = (1.0 - s) * h + s * yv if mistake == "blend_u_swapped" else s * h + (1.0 - s) * yv
    A = s * h.abs() + (1.0 - s) * yv.abs() + (h - yv).abs() * (Azu / 4.0 + s) + (1.0 - s) * (Azo + yv.abs())
    if fast:
        A = A + ((h - yv).abs() + (1.0 - s)) * FAST_ABS
    return Ref(out, A)


# ------------------------------------------------------------------------------------------------------------- soft-argmin
def softargmin_ref(logits, dvals, scale, mistake=None):
    """ops.softargmin_up: logits [N,D,H,W] -> (depth, prob) Refs, each [N,1,scale*H,scale*W]"""
    l = _c64(logits)
    N, D, H, W = l.shape
    dv = _c64(dvals).reshape(-1)[:D]
    if mistake == "depth_plane_off_by_one":
        dv = _c64(dvals).reshape(-1)[torch.clamp(torch.arange(D) + 1, max=D - 1)]
    mx = l.amax(1, keepdim=True)
    p = torch.softmax(l, 1)
    dvv = dv.view(1, D, 1, 1)
    dep = (p * dvv).sum(1, keepdim=True)
    prob = p.amax(1, keepdim=True)
    gap = torch.where(p > 0, (l - mx).abs(), torch.zeros_like(l))
    n_add = -(-D // 8) + 8
    A_dep = n_add * (p * (dvv.abs() + dep.abs()) * (1.0 + gap)).sum(1, keepdim=True)
    A_prob = prob * (1.0 + n_add + (p * gap).sum(1, keepdim=True))
    up = lambda t: t.repeat_interleave(scale, 2).repeat_interleave(scale, 3)      # noqa: E731
    return Ref(up(dep), up(A_dep)), Ref(up(prob), up(A_prob))


# ------------------------------------------------------------------------------------------------------------- camera algebra
def _np(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64)


def _r32(v, e):
    """round an fp64 intermediate to fp32 as the kernel does: the value, and one more ulp of error (it may round the other way)"""
    return v.astype(np.float32).astype(np.float64), e + U * np.abs(v)


def _inv(X, eX):
    """fp64 inverse and its error: cond(X) * |X^-1| * (2^-53 + |eX| / |X|) propagated as |X^-1| |eX| |X^-1| + 2^-50 cond |X^-1|"""
    Xi = np.linalg.inv(X)
    cond = np.linalg.cond(X)
    return Xi, np.abs(Xi) @ eX @ np.abs(Xi) + 2.0 ** -50 * cond * np.abs(Xi)


def _mm(a, ea, b, eb):
    return a @ b, np.abs(a) @ eb + ea @ np.abs(b) + 2.0 ** -50 * (np.abs(a) @ np.abs(b))


def _pose_to_proj(pose, K):
    e, ee = _inv(_np(pose), np.zeros((4, 4)))
    e, ee = _r32(e, ee)
    Kd = _np(K)
    pr, epr = _mm(Kd, np.zeros((3, 3)), e[:3], ee[:3])
    pr, epr = _r32(pr, epr)
    proj, eproj = e.copy(), ee.copy()
    proj[:3], eproj[:3] = pr, epr
    return proj, eproj


def _pair(sp, esp, rp, erp):
    ri, eri = _inv(rp, erp)
    ri, eri = _r32(ri, eri)
    pr, epr = _mm(sp, esp, ri, eri)
    out = np.concatenate([pr[:3, :3].reshape(-1), pr[:3, 3]])
    eo = np.concatenate([epr[:3, :3].reshape(-1), epr[:3, 3]])
    return out, eo


def _cam_ref(v, e):
    """-> Ref: A in units of 2^-24 (the final fp32 rounding: |v|, plus the carried error)"""
    return Ref(torch.from_numpy(v), torch.from_numpy(np.abs(v) + e / U))


def cam_pair_proj_ref(src_proj, ref_proj):
    """ops.cam_pair_proj: rot | trans of src_proj @ fl32(inverse(ref_proj)) -> Ref [12]"""
    return _cam_ref(*_pair(_np(src_proj), np.zeros((4, 4)), _np(ref_proj), np.zeros((4, 4))))


def cam_sweep_proj_ref(ref_pose, src_pose, K):
    """ops.cam_sweep_proj: proj(pose) = [fl32(K fl32(inv(pose))[:3]) ; fl32(inv(pose))[3]], then the pair projection -> Ref [12]"""
    sp, esp = _pose_to_proj(src_pose, K)
    rp, erp = _pose_to_proj(ref_pose, K)
    return _cam_ref(*_pair(sp, esp, rp, erp))


def cam_volume_mats_ref(pose_j, pose_i, K):
    """ops.cam_volume_mats: [fl32(inv(K)) | fl32(inv(rel))[:3] | K], rel = fl32(pose_j @ fl32(inv(pose_i))) (pose_i None: rel = pose_j)
    -> Ref [30]"""
    if pose_i is not None:
        ii, eii = _r32(*_inv(_np(pose_i), np.zeros((4, 4))))
        rel, erel = _r32(*_mm(_np(pose_j), np.zeros((4, 4)), ii, eii))
    else:
        rel, erel = _np(pose_j), np.zeros((4, 4))
    m, em = _inv(rel, erel)
    ki, eki = _inv(_np(K), np.zeros((3, 3)))
    v = np.concatenate([ki.reshape(-1), m[:3].reshape(-1), _np(K).reshape(-1)])
    e = np.concatenate([eki.reshape(-1), em[:3].reshape(-1), np.zeros(9)])
    r = _cam_ref(v, e)
    r.A[21:] = 0.0                                                     # K is copied
    return r


# ------------------------------------------------------------------------------------------------------------- checking
def bound_ratio(got, ref):
    """-> (worst ratio, ambiguous elements): per element max(|got - val| - pos, 0) / (2^-24 A), an ambiguous element taking the closer of
    val and alt (inf where got is NaN and the reference is not, or where the error is non-zero and A = pos = 0)"""
    got = got.detach().to("cpu", _f64).reshape(ref.val.shape)

    def excess(v):
        err = (got - v).abs()
        both_nan = torch.isnan(got) & torch.isnan(v)
        err = torch.where(both_nan, torch.zeros_like(err), torch.nan_to_num(err, nan=math.inf))
        return (err - ref.pos).clamp_min(0.0)

    ex = excess(ref.val)
    if ref.amb is not None and ref.alt is not None:
        ex = torch.where(ref.amb, torch.minimum(ex, excess(ref.alt)), ex)
    denom = U * ref.A
    ratio = torch.where(ex == 0, torch.zeros_like(ex), ex / torch.where(denom > 0, denom, torch.full_like(denom, 1e-300)))
    return (float(ratio.max()) if ratio.numel() else 0.0), ref.n_amb


def check_bound(got, ref, c_route, what=""):
    """|got - val| <= c_route 2^-24 A + pos per element; returns (worst ratio, ambiguous samples)"""
    ratio, n_amb = bound_ratio(got, ref)
    assert ratio <= c_route, "%s: |gpu - ref| reaches %.3g x 2^-24 A beyond the position term (bound %g)" % (what, ratio, c_route)
    return ratio, n_amb
