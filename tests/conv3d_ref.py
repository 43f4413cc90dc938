"""fp64 reference of the whole 3x3x3 convolution descriptor contract (include/estd_hip.h, ``estd_conv3d_desc``), as the arguments of
``ops.Conv3dPlan(...)`` followed by ``.run(...)`` spell it.  A plain helper module of the test suite (not a conftest).

Order of the operations, per output position o (channel o of the plan; row ``out_idx[o]`` of ``weight``) and voxel v:

    1. input   x_c = in_main[v][c] for c < cin_main (main channel c is weight column main_idx[c]), plus in_extra[v] (column extra_idx);
               with ``gate`` = (ru, stats, gamma, beta): main channels 16..31 are multiplied by
               sigmoid((ru[v][c - 16] - stats[0]) * stats[1] * gamma[c - 16] + beta[c - 16]) first (the ConvGRU reset gate);
    2. z       = conv3d(x, w) in float64, stride 1, zero padding 1;
    3. y_raw   = z * scale[o] + shift[o]                      (GroupNorm partials: of y_raw, channels 0..15 / 16..31);
    4. y       = act(y_raw), act = act_a if o < act_split else act_b (act_b None: act_a everywhere);
    5. head    = sum_{o < 16} head_w[o] * y[o] + head_b      (out_head; independent of out_main);
    6. main    for o < out_channels:  out[v][o] = (y + residual[v][o] + residual2[v][o]) * out_scale  (+ prior out[v][o] if accumulate);
               channels out_channels .. out_stride - 1 keep their prior content;
    7. extra   output channel 32 (n_tiles == 3) -> out_extra[v] = y[32]; no residual / scale / accumulation applies to it.

Steps 3 and 6 are the direct kernel's order (csrc/conv3d_mfma.hip epilogue: ``acc * sc + sh``, statistics before the activation, then
residual, residual2, ``*= out_scale``, ``+= out``), which the header leaves implicit.

Error magnitude ``A`` (same pipeline on absolute values): A = (|w| * |x|) * |scale| + |shift|; a tanh channel adds 1 (|tanh'| <= 1 carries
the input error through; the tanh evaluation itself errs by a few ulp of a value <= 1); the main output adds |r1| + |r2|, multiplies by
|out_scale| and adds |prior out| when accumulating; the head is sum |head_w| A + |head_b|.  A kernel passes when every element satisfies
|gpu - ref| <= c_route * 2^-24 * A.
"""
import math

import torch

U = 2.0 ** -24
ACTS = ("none", "relu", "tanh")
# test-only knob of conv3d_ref: plausible kernel mistakes (tests/test_conv3d_ref_cpu.py asserts the bound rejects each)
MISTAKES = ("drop_face_tap", "xout_identity", "shift_before_scale", "ignore_residual2", "accumulate_overwrites", "act_split_plus_2")


def _cpu64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def _records(t, dims, stride):
    """[N,D,H,W,stride] view of a contiguous channels-last tensor (or of a flat base of one)"""
    n = dims[0] * dims[1] * dims[2] * dims[3]
    return t.reshape(-1)[: n * stride].view(*dims, stride)


def _act(v, name):
    if name == "relu":
        return v.clamp_min(0.0)
    if name == "tanh":
        return torch.tanh(v)
    return v


def gather_patches(vol, points):
    """vol [N,D,H,W,C] (any device / dtype), points long [P,4] = (n, d, h, w) -> float64 CPU [P, 27, C] of the 3x3x3 neighbourhoods
    (tap t = (kd * 3 + kh) * 3 + kw), zero outside the volume."""
    N, D, H, W, C = vol.shape
    p = points.to(vol.device)
    out = []
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                d, h, w = p[:, 1] + kd - 1, p[:, 2] + kh - 1, p[:, 3] + kw - 1
                ok = (d >= 0) & (d < D) & (h >= 0) & (h < H) & (w >= 0) & (w < W)
                v = vol[p[:, 0], d.clamp(0, D - 1), h.clamp(0, H - 1), w.clamp(0, W - 1)].double()
                out.append(torch.where(ok[:, None], v, torch.zeros_like(v)))
    return torch.stack(out, 1).cpu()


def _at(vol, points):
    """values of vol [N,D,H,W(,C)] at points [P,4] -> float64 CPU [P(,C)]"""
    p = points.to(vol.device)
    return vol[p[:, 0], p[:, 1], p[:, 2], p[:, 3]].double().cpu()


def conv3d_ref(weight, main_idx, extra_idx, out_idx, n_tiles, scale, shift, act_a="none", act_b=None, act_split=0,
               head_w=None, head_b=None, *, x, dims, in_stride=None, in_extra=None, out=None, out_stride=None, out_channels=None,
               residual=None, residual2=None, out_scale=1.0, accumulate=False, out_extra=None, out_head=None, stats_partials=None,
               gate=None, points=None, mistake=None):
    """Expected results of ``Conv3dPlan(weight, ..., head_b).run(x, dims, ...)`` in float64 (module docstring), with their error
    magnitudes.  ``out`` / ``out_extra`` / ``out_head`` / ``stats_partials`` only say whether the output exists (``out``: and its prior
    content); nothing is written.  ``points`` (long [P,4] of (n, d, h, w)): evaluate at these voxels only, from gathered 3x3x3 patches
    (no statistics then).  ``mistake``: one of MISTAKES, a deliberately wrong variant for the discrimination test.

    Returns a dict with ``out`` / ``out_A`` ([N,D,H,W,out_stride] or [P,out_stride]: the whole record, prior content past out_channels),
    ``extra`` / ``extra_A``, ``head`` / ``head_A`` ([N,D,H,W] or [P]) for the outputs that exist, and ``stats`` / ``stats_A``
    (float64 [4] = mean_g0, rstd_g0, mean_g1, rstd_g1 as ops.groupnorm_finalize writes them, and their first-order error magnitudes)."""
    assert mistake is None or mistake in MISTAKES, mistake
    N, D, H, W = dims
    cin = len(main_idx)
    n_out = len(out_idx)
    in_stride = in_stride if in_stride is not None else cin
    out_stride = out_stride if out_stride is not None else 16 * min(n_tiles, 2)
    out_channels = out_channels if out_channels is not None else 16 * min(n_tiles, 2)
    acts = [act_a if (act_b is None or o < act_split + (2 if mistake == "act_split_plus_2" else 0)) else act_b for o in range(n_out)]
    if mistake == "xout_identity" and n_out == 33:
        acts[32] = "none"
    cols = list(main_idx) + ([extra_idx] if extra_idx is not None else [])
    w = _cpu64(weight)[list(out_idx)][:, cols]                                  # [n_out, cin(+1), 3, 3, 3]
    sc, sh = _cpu64(scale)[:n_out], _cpu64(shift)[:n_out]

    # ---- input (+ the reset gate)
    xm = _records(x, dims, in_stride)[..., :cin]
    g_r = None
    if gate is not None:
        ru, gst, gga, gbe = gate
        g_r = _records(ru, dims, 32)[..., :16]
        gst, gga, gbe = _cpu64(gst), _cpu64(gga), _cpu64(gbe)

    def gated(xv, rv):                     # xv [..., cin], rv [..., 16] float64
        if rv is None:
            return xv
        g = torch.sigmoid((rv - gst[0]) * gst[1] * gga + gbe)
        return torch.cat([xv[..., :16], xv[..., 16:32] * g, xv[..., 32:]], -1)

    if points is None:
        xin = gated(_cpu64(xm), _cpu64(g_r) if g_r is not None else None)
        if in_extra is not None:
            xin = torch.cat([xin, _cpu64(in_extra).reshape(-1)[: N * D * H * W].view(N, D, H, W, 1)], -1)
        xc = xin.permute(0, 4, 1, 2, 3)
        z = torch.nn.functional.conv3d(xc, w, padding=1).permute(0, 2, 3, 4, 1)
        za = torch.nn.functional.conv3d(xc.abs(), w.abs(), padding=1).permute(0, 2, 3, 4, 1)
        if mistake == "drop_face_tap" and W >= 2:
            # the tap (kd, kh, kw) = (1, 1, 2) of the voxels in column W - 2 reads column W - 1 -- treated as padding
            z[:, :, :, W - 2] -= torch.einsum("ndhc,oc->ndho", xin[:, :, :, W - 1], w[:, :, 1, 1, 2])
        at = lambda t: _cpu64(t)                                                # noqa: E731
    else:
        pat = gather_patches(xm, points)                                       # [P, 27, cin]
        if g_r is not None:
            pat = gated(pat, gather_patches(g_r, points))
        if in_extra is not None:
            pat = torch.cat([pat, gather_patches(in_extra.reshape(-1)[: N * D * H * W].view(N, D, H, W, 1), points)], -1)
        wt = w.reshape(n_out, w.shape[1], 27)
        z = torch.einsum("ptc,oct->po", pat, wt)
        za = torch.einsum("ptc,oct->po", pat.abs(), wt.abs())
        if mistake == "drop_face_tap":
            sel = points[:, 3] == W - 2
            z[sel] -= torch.einsum("pc,oc->po", pat[sel, 14], w[:, :, 1, 1, 2])      # tap (1, 1, 2)
        at = lambda t: _at(t, points)                                           # noqa: E731

    # ---- BN, statistics, activation
    if mistake == "shift_before_scale":
        y_raw = (z + sh) * sc
    else:
        y_raw = z * sc + sh
    A = za * sc.abs() + sh.abs()
    res = {}
    if stats_partials is not None:
        if points is not None:
            raise ValueError("GroupNorm statistics need the whole volume")
        st, st_a = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
        for g in range(min(n_out, 32) // 16):
            v, a = y_raw[..., 16 * g:16 * g + 16], A[..., 16 * g:16 * g + 16]
            mean = v.mean()
            var = (v * v).mean() - mean * mean
            rstd = 1.0 / math.sqrt(float(var) + 1e-5)
            st[2 * g], st[2 * g + 1] = mean, rstd
            st_a[2 * g] = a.mean()
            st_a[2 * g + 1] = rstd ** 3 * float((v.abs() * a).mean() + mean.abs() * a.mean())    # d rstd = -rstd^3 / 2 * d var
        st_a += st.abs()                                                         # (+ the float32 rounding of the finalised values)
        res["stats"], res["stats_A"] = st, st_a
    y = torch.empty_like(y_raw)
    for o in range(n_out):
        y[..., o] = _act(y_raw[..., o], acts[o])
        if acts[o] == "tanh":
            A[..., o] += 1.0

    # ---- head
    if out_head is not None and head_w is not None:
        hw, hb = _cpu64(head_w), _cpu64(head_b)
        res["head"] = (y[..., :16] * hw).sum(-1) + hb[0]
        res["head_A"] = (A[..., :16] * hw.abs()).sum(-1) + hb[0].abs()

    # ---- main output
    if out is not None:
        oc = out_channels
        prior = at(_records(out, dims, out_stride))
        m, ma = y[..., :oc].clone(), A[..., :oc].clone()
        if residual is not None:
            r = at(_records(residual, dims, out_stride))[..., :oc]
            m, ma = m + r, ma + r.abs()
        if residual2 is not None and mistake != "ignore_residual2":
            r = at(_records(residual2, dims, out_stride))[..., :oc]
            m, ma = m + r, ma + r.abs()
        m, ma = m * float(out_scale), ma * abs(float(out_scale))
        if accumulate and mistake != "accumulate_overwrites":
            m, ma = m + prior[..., :oc], ma + prior[..., :oc].abs()
        full, full_a = prior.clone(), torch.zeros_like(prior)
        full[..., :oc], full_a[..., :oc] = m, ma
        res["out"], res["out_A"] = full, full_a

    # ---- output channel 32
    if n_tiles == 3 and out_extra is not None:
        res["extra"], res["extra_A"] = y[..., 32], A[..., 32]
    return res


def bound_ratio(got, ref, A):
    """max over the elements of |got - ref| / (2^-24 A) (inf where got is NaN)"""
    got = got.detach().to("cpu", torch.float64)
    err = (got - ref).abs()
    err = torch.where(torch.isnan(got) & ~torch.isnan(ref), torch.full_like(err, math.inf), err)
    return float((err / (U * A.clamp_min(1e-300))).max()) if err.numel() else 0.0


def check_bound(got, ref, A, c_route, what=""):
    """the per-element bound |got - ref| <= c_route 2^-24 A and the max-relative bar |got - ref| < 3e-6 max |ref|; returns the
    worst per-element ratio"""
    got64 = got.detach().to("cpu", torch.float64)
    ratio = bound_ratio(got64, ref, A)
    assert ratio <= c_route, "%s: |gpu - ref| reaches %.1f x 2^-24 A (bound %g)" % (what, ratio, c_route)
    mag = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got64 - ref).abs().max()) if ref.numel() else 0.0
    assert err < 3e-6 * mag or err == 0.0, "%s: max error %.3g vs max |ref| %.3g" % (what, err, mag)
    return ratio
