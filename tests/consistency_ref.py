"""float64 reference of the cross-view consistency contract of the library (csrc/depth_consistency.hip, include/estd_hip.h:
estd_depth_consistency), in the style of tests/tsdf_raycast_ref.py.  A plain helper module of the test suite (not a conftest); numpy only.

``evaluate`` evaluates the contract in float64 FROM THE fp32 MATRICES, MAPS AND CONSTANTS THE KERNEL RECEIVES and returns, per target pixel,
the expected views / visible / depth / rel_err, first-order rounding bounds of the two averaged outputs, the ``valid`` mask and the pixels
that are ``amb``iguous: a discontinuous decision of some source lies within the fp32 rounding of the kernel's evaluation, so either outcome
is right and the pixel is left out of the comparison.  ``dtype=np.float32`` evaluates the same contract in numpy fp32 arithmetic (the CPU
stand-in for the kernel; numpy has no fused multiply-add, so every product rounds on its own).  ``compare`` is THE comparison of the suite
(GPU results and the stand-in alike): ambiguous pixels <= AMB_CAP of the valid target pixels; invalid pixels exactly zero in all four
outputs; on every other pixel views and visible exact and
    |depth - ref| <= C_CONS e_depth                |rel_err - ref| <= C_CONS e_relerr.

Rounding bounds (first order, u = 2^-24; the counts are the unfused ones, a fused multiply-add rounds once where they count twice)
    row(M, j; x, y, z) = z r_j + M_j3 with r_j = M_j0 x + M_j1 y + M_j2, S_j = |M_j0 x| + |M_j1 y| + |M_j2|:
        e_r_j = 4 u S_j + |M_j0| e_x + |M_j1| e_y      (as tsdf_ref's dot products: any association order; e_x = e_y = 0 for the integer
                                                        target pixel, e_us / e_vs on the way back)
        e_row = |z| e_r_j + |r_j| e_z + u (2 |z r_j| + |M_j3|)         (the product, the sum; e_z = 0 for the target's own depth d)
    a, b, c = rows 0, 1, 2 of F at (u, v, d):  e_a, e_b, e_c as above.
    us = a / c:      e_us = (e_a + |us| e_c) / |c| + u |us|;   vs likewise.
    The cell x0 = min(floor(us), W - 2) and fx = us - x0 are exact functions of the computed us (x0 <= us <= 2 x0 or x0 = 0: the
        subtraction is exact).  ds = lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy) on taps of magnitude <= m: 5 u m per level (the
        difference, the product, the sum; 3 u m fused), two levels, and the interpolant moves with us, vs by at most the tap differences
        s_x = max(|t10 - t00|, |t11 - t01|), s_y = max(|t01 - t00|, |t11 - t10|):
            e_ds = 10 u m + s_x e_us + s_y e_vs.
        Where us or vs is within C_POS of its bound of an integer the kernel may have taken the neighbouring cell: the bilinear
        interpolant is continuous across the face, but its slope is the neighbour's, so s_x = s_y = the range of the valid depths in
        the 3 x 3 pixels around the rounded position there.
    a', b', c' = rows of B at (us, vs, ds): the same expressions with e_x = e_us, e_y = e_vs, e_z = e_ds.
    u' = a' / c':    e_u' = (e_a' + |u'| e_c') / |c'| + u |u'|;   v' likewise.
    e2 = (u' - u)^2 + (v' - v)^2 with du = u' - u: e_du = e_u' + u |du|;   e_e2 = 2 |du| e_du + 2 |dv| e_dv + 3 u e2.
    rel = |c' - d| / d:   e_rel = (e_c' + u |c' - d|) / d + u rel.
    depth = (d + sum c') / (1 + views), all terms positive, one rounding per addition: e_depth = (sum_s (e_c'_s + u partial_s)) / (1 + views)
        + u depth;  rel_err likewise from e_rel.
    C_CONS = 2: for what first order leaves out (the bounds are evaluated at the reference's own values; products of two errors).  Every
    count above is already the unfused one.  C_POS = 2 as in tsdf_ref.py.
Ambiguity: for a source that has reached the decision in the reference's evaluation,
    |c - z_near| < C_POS e_c;   us or vs within C_POS e_us / e_vs of 0 or of the far edge W - 1 / H - 1;
    us or vs within C_POS of its bound of an integer while some depth in the 3 x 3 source pixels around the rounded position is invalid
    (the neighbouring cell has another set of taps; with all of them valid the value is continuous and the bound above holds);
    |c' - z_near| < C_POS e_c';   |e2 - px_max^2| < C_POS e_e2;   |rel - rel_max| < C_POS e_rel.
    The validity of the target's depth and of a tap compares stored fp32 values and is exact.

Figures of the numpy-fp32 stand-in against this reference (tests/test_consistency_ref_cpu.py prints them per case): ambiguous share of the
valid pixels 0.0002 - 0.0028 (cap 0.03); largest depth error 0.14 - 0.23 of the unscaled bound per case, largest rel_err error 0.12 - 0.25
(bar C_CONS = 2).  The device's figures (0.13 - 0.19 and 0.09 - 0.19): profiles/consistency_gpu_tests.txt.
"""
import functools

import numpy as np

import tsdf_ref as R

U = 2.0 ** -24
C_POS = 2.0                  # decision tolerance = C_POS * rounding bound (as in tsdf_ref.py)
C_CONS = 2.0                 # route constant of the depth / rel_err bounds, from the derivation above
AMB_CAP = 0.03               # ambiguous pixels: at most this share of the valid target pixels in every case
NOISE = 0.004                # multiplicative Gaussian noise of the cases' depth maps: both outcomes occur at px_max = 1, rel_max = 0.01
PX_MAX, REL_MAX, Z_NEAR = 1.0, 0.01, 1e-3

# name: size (H, W), sources, extras.  The middle frame of tsdf_ref.scene_poses(S + 1) is the target, the others are the sources.
CASES = {
    "s2": dict(hw=(60, 80), S=2),
    "s4": dict(hw=(120, 160), S=4, holes=True),
    "s8": dict(hw=(119, 157), S=8),
    "tiny": dict(hw=(24, 32), S=8),
    "kdiff": dict(hw=(120, 160), S=2, kdiff=True),
}
FULL_CASE = dict(hw=(480, 640), S=4)
# the route suite's maps: the smallest the contract allows and the edges of the kernel's 16 x 16 tiles, under 1 and 8 sources each
# (make_case(hw, S, seed=S + hw[0])); tests/test_consistency_ref_cpu.py checks their ambiguous share
ROUTE_SIZES, ROUTE_SOURCES = [(2, 2), (15, 17), (16, 16), (17, 33)], (1, 8)


def matrices64(pose_t, K_t, poses_s, K_s):
    """F_s = [K_s R_st K_t^-1 | K_s t_st] and B_s (the same the other way) in float64, rounded to fp32 [S,2,3,4] (what
    estdepth_amd.camera.consistency_matrices hands the kernel); K_s [3,3] or [S,3,3]"""
    Pt, Kt = np.asarray(pose_t, np.float64).reshape(4, 4), np.asarray(K_t, np.float64).reshape(3, 3)
    Ps, Ks = np.asarray(poses_s, np.float64).reshape(-1, 4, 4), np.asarray(K_s, np.float64).reshape(-1, 3, 3)
    out = []
    for s in range(Ps.shape[0]):
        K = Ks[s if Ks.shape[0] > 1 else 0]
        pair = []
        for Ka, Pa, Kb, Pb in ((Kt, Pt, K, Ps[s]), (K, Ps[s], Kt, Pt)):
            rel = np.linalg.inv(Pb) @ Pa
            pair.append(np.concatenate([Kb @ rel[:3, :3] @ np.linalg.inv(Ka), (Kb @ rel[:3, 3])[:, None]], 1))
        out.append(np.stack(pair))
    return np.stack(out).astype(np.float32)


def depth_valid(d, z_near=Z_NEAR):
    """the contract's validity of a stored depth: finite and > z_near (compared as fp32 values: exact)"""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > np.float32(z_near))


def _window3(a, fn, fill):
    """fn over the 3 x 3 window around every pixel of ``a`` [H,W]; pixels outside the map count as ``fill``"""
    H, W = a.shape
    pad = np.pad(a, 1, constant_values=fill)
    return fn([pad[i:i + H, j:j + W] for i in range(3) for j in range(3)], axis=0)


def _rows(M, M64, x, y, z, e_x, e_y, e_z):
    """rows 0..2 of the 3x4 matrix at (x, y, z): values in the dtype of M / x / y / z, bounds in float64"""
    x64, y64, z64 = (np.asarray(t, np.float64) for t in (x, y, z))
    val, err = [], []
    for j in range(3):
        r = M[j, 0] * x + (M[j, 1] * y + M[j, 2])
        val.append(z * r + M[j, 3])
        r64 = np.asarray(r, np.float64)
        S = np.abs(M64[j, 0] * x64) + np.abs(M64[j, 1] * y64) + np.abs(M64[j, 2])
        e_r = 4 * U * S + np.abs(M64[j, 0]) * e_x + np.abs(M64[j, 1]) * e_y
        err.append(np.abs(z64) * e_r + np.abs(r64) * e_z + U * (2 * np.abs(z64 * r64) + np.abs(M64[j, 3])))
    return val, err


def _lerp(a, b, t):
    return t * (b - a) + a


def evaluate(target, sources, mats, px_max=PX_MAX, rel_max=REL_MAX, z_near=Z_NEAR, dtype=np.float64, variant=None):
    """target [H,W] and sources [S,H,W] float32; mats [S,2,3,4] float32; the three constants as the kernel receives them (rounded to fp32
    here).  Returns a dict of [H,W] arrays: views, visible, depth, rel_err (``dtype``), valid, amb (bool), tol_depth, tol_rel_err (float64,
    absolute, to be scaled by C_CONS).  ``variant`` evaluates a deliberately WRONG contract (the tests' wrong kernels): "nearest" reads the
    nearest source pixel instead of the bilinear blend, "ge" lets a depth equal to z_near pass as valid (>= where the contract has >),
    "swap" exchanges F and B."""
    f = dtype
    tgt = np.asarray(target, np.float32)
    srcs = np.asarray(sources, np.float32)
    H, W = tgt.shape
    M32 = np.asarray(mats, np.float32).reshape(-1, 2, 3, 4)
    assert srcs.shape == (M32.shape[0], H, W) and H >= 2 and W >= 2
    zn32, rm32 = np.float32(z_near), np.float32(rel_max)
    px2_32 = np.float32(px_max) * np.float32(px_max)
    zn, rm, px2 = f(zn32), f(rm32), f(px2_32)
    zn64, rm64, px264 = float(zn32), float(rm32), float(px2_32)

    def ok(m):
        with np.errstate(invalid="ignore"):
            return np.isfinite(m) & ((m >= zn32) if variant == "ge" else (m > zn32))
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    uf, vf = uu.astype(f), vv.astype(f)
    valid = ok(tgt)
    d = np.where(valid, tgt, np.float32(1.0)).astype(f)
    d64 = d.astype(np.float64)
    zero = np.zeros((H, W))
    views, visible, sum_rel = np.zeros((H, W), f), np.zeros((H, W), f), np.zeros((H, W), f)
    sum_c = d.copy()
    e_sum_c, e_sum_rel = np.zeros((H, W)), np.zeros((H, W))
    amb = np.zeros((H, W), bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(M32.shape[0]):
            Fm, Bm = (M32[s, 1], M32[s, 0]) if variant == "swap" else (M32[s, 0], M32[s, 1])
            src = srcs[s]
            alive = valid.copy()
            (a, b, c), (e_a, e_b, e_c) = _rows(Fm.astype(f), Fm.astype(np.float64), uf, vf, d, zero, zero, zero)
            c64 = c.astype(np.float64)
            amb |= alive & (np.abs(c64 - zn64) < C_POS * e_c)
            alive &= c > zn
            cs = np.where(alive, c, f(1.0))
            us, vs = a / cs, b / cs
            us64, vs64, cs64 = us.astype(np.float64), vs.astype(np.float64), np.abs(cs.astype(np.float64))
            e_us = (e_a + np.abs(us64) * e_c) / cs64 + U * np.abs(us64)
            e_vs = (e_b + np.abs(vs64) * e_c) / cs64 + U * np.abs(vs64)
            amb |= alive & ((np.abs(us64) < C_POS * e_us) | (np.abs(us64 - (W - 1)) < C_POS * e_us)
                            | (np.abs(vs64) < C_POS * e_vs) | (np.abs(vs64 - (H - 1)) < C_POS * e_vs))
            alive &= (us >= 0) & (us <= f(W - 1)) & (vs >= 0) & (vs <= f(H - 1))
            us, vs = np.where(alive, us, f(0.0)), np.where(alive, vs, f(0.0))
            us64, vs64 = us.astype(np.float64), vs.astype(np.float64)
            x0, y0 = np.minimum(np.floor(us), f(W - 2)), np.minimum(np.floor(vs), f(H - 2))
            xi, yi = x0.astype(np.int64), y0.astype(np.int64)
            t00, t10, t01, t11 = src[yi, xi], src[yi, xi + 1], src[yi + 1, xi], src[yi + 1, xi + 1]
            src_ok = ok(src)
            near = (np.abs(us64 - np.rint(us64)) < C_POS * e_us) | (np.abs(vs64 - np.rint(vs64)) < C_POS * e_vs)
            rx, ry = np.clip(np.rint(us64), 0, W - 1).astype(np.int64), np.clip(np.rint(vs64), 0, H - 1).astype(np.int64)
            amb |= alive & near & _window3(~src_ok, np.any, False)[ry, rx]
            alive &= src_ok[yi, xi] & src_ok[yi, xi + 1] & src_ok[yi + 1, xi] & src_ok[yi + 1, xi + 1]
            t00, t10, t01, t11 = (np.where(alive, t, np.float32(1.0)).astype(f) for t in (t00, t10, t01, t11))
            fx, fy = us - x0, vs - y0
            if variant == "nearest":
                ds = np.where(alive, src[ry, rx], np.float32(1.0)).astype(f)
            else:
                ds = _lerp(_lerp(t00, t10, fx), _lerp(t01, t11, fx), fy)
            taps = np.stack([t.astype(np.float64) for t in (t00, t10, t01, t11)])
            s_x = np.maximum(np.abs(taps[1] - taps[0]), np.abs(taps[3] - taps[2]))
            s_y = np.maximum(np.abs(taps[2] - taps[0]), np.abs(taps[3] - taps[1]))
            rng3 = (_window3(np.where(src_ok, src.astype(np.float64), -np.inf), np.max, -np.inf)
                    - _window3(np.where(src_ok, src.astype(np.float64), np.inf), np.min, np.inf))[ry, rx]
            s_x, s_y = np.where(near, np.maximum(rng3, s_x), s_x), np.where(near, np.maximum(rng3, s_y), s_y)
            e_ds = 10 * U * np.abs(taps).max(0) + s_x * e_us + s_y * e_vs
            (a2, b2, c2), (e_a2, e_b2, e_c2) = _rows(Bm.astype(f), Bm.astype(np.float64), us, vs, ds, e_us, e_vs, e_ds)
            c264 = c2.astype(np.float64)
            amb |= alive & (np.abs(c264 - zn64) < C_POS * e_c2)
            alive &= c2 > zn
            c2s = np.where(alive, c2, f(1.0))
            u2, v2 = a2 / c2s, b2 / c2s
            c2a = np.abs(c2s.astype(np.float64))
            e_u2 = (e_a2 + np.abs(u2.astype(np.float64)) * e_c2) / c2a + U * np.abs(u2.astype(np.float64))
            e_v2 = (e_b2 + np.abs(v2.astype(np.float64)) * e_c2) / c2a + U * np.abs(v2.astype(np.float64))
            visible = visible + alive.astype(f)
            du, dv = u2 - uf, v2 - vf
            e2 = du * du + dv * dv
            rel = np.abs(c2s - d) / d
            du64, dv64, e264, rel64 = (t.astype(np.float64) for t in (du, dv, e2, rel))
            e_e2 = 2 * np.abs(du64) * (e_u2 + U * np.abs(du64)) + 2 * np.abs(dv64) * (e_v2 + U * np.abs(dv64)) + 3 * U * e264
            e_rel = (e_c2 + U * np.abs(c2s.astype(np.float64) - d64)) / d64 + U * rel64
            amb |= alive & ((np.abs(e264 - px264) < C_POS * e_e2) | (np.abs(rel64 - rm64) < C_POS * e_rel))
            cons = alive & (e2 < px2) & (rel < rm)
            views = views + cons.astype(f)
            sum_c = np.where(cons, sum_c + c2s, sum_c)
            sum_rel = np.where(cons, sum_rel + rel, sum_rel)
            e_sum_c += np.where(cons, e_c2 + U * sum_c.astype(np.float64), 0.0)
            e_sum_rel += np.where(cons, e_rel + U * sum_rel.astype(np.float64), 0.0)
        depth = np.where(valid, sum_c / (f(1.0) + views), f(0.0)).astype(f)
        rel_err = np.where(views > 0, sum_rel / np.maximum(views, f(1.0)), f(0.0)).astype(f)
    n64 = views.astype(np.float64)
    return {"views": np.where(valid, views, f(0.0)), "visible": np.where(valid, visible, f(0.0)), "depth": depth, "rel_err": rel_err,
            "valid": valid, "amb": amb & valid,
            "tol_depth": e_sum_c / (1.0 + n64) + U * np.abs(depth.astype(np.float64)),
            "tol_rel_err": e_sum_rel / np.maximum(n64, 1.0) + U * np.abs(rel_err.astype(np.float64))}


def compare(got, ref, label=""):
    """THE comparison of the suite.  ``got``: dict(views, visible, depth, rel_err) of fp32 [H,W] arrays; ``ref`` from evaluate(dtype=float64).
    Returns a dict of figures after asserting what the module docstring states."""
    g = {k: np.asarray(got[k]) for k in ("views", "visible", "depth", "rel_err")}
    for k, a in g.items():
        assert a.shape == ref[k].shape, (k, a.shape)
        assert np.isfinite(a).all(), "%s: output %s is not finite" % (label, k)
    valid, amb = ref["valid"], ref["amb"]
    n_valid, n_amb = int(valid.sum()), int(amb.sum())
    fig = {"valid": n_valid, "ambiguous": n_amb, "amb_share": n_amb / max(n_valid, 1)}
    assert n_amb <= AMB_CAP * n_valid, "%s: %d ambiguous pixels exceed %.2f of the %d valid pixels" % (label, n_amb, AMB_CAP, n_valid)
    zero = all((a[~valid] == 0).all() for a in g.values())
    keep = valid & ~amb
    for k in ("views", "visible"):
        wrong = keep & (g[k].astype(np.float64) != ref[k].astype(np.float64))
        fig[k + "_mismatch"] = int(wrong.sum())
    for k in ("depth", "rel_err"):
        err = np.abs(g[k].astype(np.float64) - ref[k].astype(np.float64))[keep]
        ratio = err / np.maximum(ref["tol_" + k][keep], 1e-300)
        fig[k + "_ratio"] = float(ratio.max()) if ratio.size else 0.0
        fig[k + "_err"] = float(err.max()) if err.size else 0.0
    fig["consistent_share"] = float(ref["views"].sum() / max(ref["visible"].sum(), 1))
    print("depth_consistency compare %s: valid %d ambiguous %d (%.4f) consistent %.3f of visible; mismatches views %d visible %d; max error / bound "
          "(bar %.1f): depth %.3g (%.3g m) rel_err %.3g (%.3g)" % (label, n_valid, n_amb, fig["amb_share"], fig["consistent_share"], fig["views_mismatch"],
                                                                  fig["visible_mismatch"], C_CONS, fig["depth_ratio"], fig["depth_err"],
                                                                  fig["rel_err_ratio"], fig["rel_err_err"]))
    assert zero, "%s: an invalid pixel is not exactly zero" % label
    for k in ("views", "visible"):
        assert fig[k + "_mismatch"] == 0, "%s: %s differs on %d unambiguous pixels" % (label, k, fig[k + "_mismatch"])
    for k in ("depth", "rel_err"):
        assert fig[k + "_ratio"] <= C_CONS, "%s: %s error at %.3f of its bound (bar %.1f)" % (label, k, fig[k + "_ratio"], C_CONS)
    return fig


# ------------------------------------------------------------------------------------------------------------ the cases of the suite
def noisy(depth, rng, sigma=NOISE):
    return (depth * (1.0 + sigma * rng.randn(*depth.shape))).astype(np.float32)


def make_case(hw, S, holes=False, kdiff=False, noise=NOISE, seed=0, name=""):
    """dict(target [H,W], sources [S,H,W] f32, mats [S,2,3,4] f32, pose_t, K_t, poses_s [S,4,4], K_s [S,3,3], depths [S+1,H,W], poses, t)"""
    H, W = hw
    T = S + 1
    t = T // 2
    poses = R.scene_poses(T, seed=seed)
    K = R.intrinsics(H, W)
    Ks = np.stack([R.intrinsics(H, W, 0.8 + 0.05 * i) if (kdiff and i != t) else K for i in range(T)])
    rng = np.random.RandomState(11 + seed)
    clean = np.stack([R.raycast_scene(poses[i], Ks[i], H, W) for i in range(T)])
    depths = noisy(clean, rng, noise) if noise else clean.astype(np.float32)
    if holes:
        depths[:, 10:30, 20:60] = 0.0
        depths[:, 50:70, 80:120] = np.nan
        depths[:, 90:110, 30:70] = np.inf
        depths[:, 40:45, 5:15] = -1.0
    src = [i for i in range(T) if i != t]
    return dict(name=name, target=depths[t], sources=depths[src], mats=matrices64(poses[t], K, poses[src], Ks[src]), pose_t=poses[t], K_t=K,
                poses_s=poses[src], K_s=Ks[src], depths=depths, poses=poses, t=t)


@functools.lru_cache(maxsize=None)
def build_case(name):
    c = FULL_CASE if name == "full" else CASES[name]
    return make_case(c["hw"], c["S"], c.get("holes", False), c.get("kdiff", False), seed=len(name), name=name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 evaluation of a case, computed once and shared"""
    c = build_case(name)
    return evaluate(c["target"], c["sources"], c["mats"])


def corrupted_stack(T=5, hw=(120, 160), share=0.05, seed=3):
    """T noise-free frames of the scene, ``share`` of each map's pixels replaced by the depth times a factor drawn from
    [0.6, 0.85] u [1.2, 1.5] -> dict(clean, depths [T,H,W] f32, bad [T,H,W] bool, poses [T,4,4], K)"""
    H, W = hw
    poses, K = R.scene_poses(T, seed=seed), R.intrinsics(H, W)
    clean = np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)
    rng = np.random.RandomState(seed)
    bad = rng.uniform(size=clean.shape) < share
    low = rng.uniform(size=clean.shape) < 0.5
    factor = np.where(low, rng.uniform(0.6, 0.85, size=clean.shape), rng.uniform(1.2, 1.5, size=clean.shape))
    return dict(clean=clean, depths=np.where(bad, clean * factor, clean).astype(np.float32), bad=bad, poses=poses, K=K)


def window_sources(t, T, radius, cap=8):
    """the neighbours frame t of a T-frame stack is checked against: up to ``radius`` on either side, nearest first, at most ``cap``"""
    out = []
    for k in range(1, radius + 1):
        out += [i for i in (t - k, t + k) if 0 <= i < T]
    return sorted(out[:cap])
