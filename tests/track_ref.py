"""float64 reference of the frame-to-model alignment contract of the library (csrc/track/frame_align.hip, include/estd_hip.h:
estd_frame_align), in the style of tests/consistency_ref.py.  A plain helper module of the test suite (not a conftest); numpy only.

``evaluate`` evaluates the contract in float64 FROM THE fp32 MATRICES, MAPS AND CONSTANTS THE KERNEL RECEIVES and returns, per live pixel,
the expected ``match`` and ``residual``, the Jacobian row, first-order rounding bounds, the ``valid`` mask (step 1 of the contract) and the
pixels that are ``amb``iguous: a discontinuous decision lies within the fp32 rounding of the kernel's evaluation, so either outcome is
right and the pixel is left out of the per-pixel comparison.  ``dtype=np.float32`` evaluates the same contract in numpy fp32 arithmetic
(the CPU stand-in for the kernel; numpy has no fused multiply-add, so every product rounds on its own).  With ``match=`` the decisions
are TAKEN from a given match map and only the values are computed: that is how the 29 sums of a device run are checked -- the reference
recomputes them from the device's own decisions, so no left-out pixel enters them.  ``compare`` is THE comparison of the suite (GPU
results and the stand-in alike): ambiguous pixels <= AMB_CAP of the valid pixels; on every other pixel ``match`` exact and
    |residual - ref| <= C_TRACK e_r;
wherever ``match`` is -1 the residual is exactly 0; sums[28] equals the number of matched pixels exactly and every other sum
    |sum_k - ref_k(given the match map)| <= C_TRACK sum over the matched pixels of e_term_k.

Rounding bounds (first order, u = 2^-24; the counts are the unfused ones, a fused multiply-add rounds once where they count twice)
    row(M, j; x, y, z) = z r_j + M_j3 with r_j = M_j0 x + M_j1 y + M_j2, S_j = |M_j0 x| + |M_j1 y| + |M_j2|; x, y integers (the live
        pixel, the model pixel) and z a stored depth, all exact:
            e_row = 4 u |z| S_j + u (2 |z r_j| + |M_j3|)                             (consistency_ref's e_row with e_x = e_y = e_z = 0)
        p_j = row(L, j; u, v, d) and q_j = row(Bm, j; um, vm, dm): e_p_j, e_q_j as above.
    a = Fm_00 p_x + Fm_01 p_y + Fm_02 p_z + Fm_03, S_a = the sum of the absolute terms: three nested fused multiply-adds or products that
        round on their own, any association order (tsdf_ref's dot product), and the points' own error:
            e_a = 4 u S_a + sum_k |Fm_0k| e_p_k;     b, c likewise.
    x = a / c + 0.5:  e_x = (e_a + |a / c| e_c) / |c| + u |a / c| + u |x|            (tsdf_ref's e_q).
    e_j = q_j - p_j:  e_e_j = e_q_j + e_p_j + u |e_j|.
    e2 = e_x^2 + e_y^2 + e_z^2:  e_e2 = sum_j 2 |e_j| e_e_j + 3 u e2                  (the products' roundings sum to <= u e2, two additions).
    r = n . e, S_r = sum_j |n_j e_j|:  e_r = sum_j |n_j| e_e_j + 3 u S_r             (the normal is a stored value: exact).
    w = p x n, per component two products and a difference, S_w = |p_y n_z| + |p_z n_y| (and cyclic):
            e_w_x = |n_z| e_p_y + |n_y| e_p_z + 2 u S_w_x.     J = (n, w): e_J = (0, 0, 0, e_w).
    The terms of the sums, each ONE fp32 product:  e(J_i J_j) = |J_i| e_J_j + |J_j| e_J_i + u |J_i J_j|;   e(J_i r) = |J_i| e_r + |r| e_J_i
        + u |J_i r|;   e(r^2) = 2 |r| e_r + u r^2;   the count is exact.  The float64 additions add <= 2^-53 n per term: n 2^-53 sum |term|.
    C_TRACK = 2: for what first order leaves out (the bounds are evaluated at the reference's own values; products of two errors), as
        consistency_ref's C_CONS -- every count above is already the unfused one.  Not above the ray caster's C_RAY = 4.
Decisions and their tolerances (C_POS = 2 as in tsdf_ref.py); a pixel that has reached the decision in the reference is ambiguous when
    |c - z_near| < C_POS e_c;
    a / c + 0.5 or b / c + 0.5 lies within C_POS e_x of an integer: the kernel may read the neighbouring model pixel.  The image edges
        (0 and Wm, 0 and Hm) are integers of x and fall under the same rule, and so does ``dm > 0``: the comparison of a stored value is
        exact, WHICH value is read is the pixel decision;
    |e2 - dist_max^2| < C_POS e_e2 -- unless the gate is EXACT at the pixel: the numpy-fp32 evaluation reproduces the float64 values of
        p, q, e and e2 bit for bit.  Then every fp32 operation on the way was exact, any evaluation order, fused or not, gives those very
        values, and the gate compares two stored numbers (the case "tie": e2 == dist_max^2 passes the contract's <=).
    The validity of d, the confidence gate and dm > 0 compare stored fp32 values and are exact.

The scene is this module's own: tsdf_ref.raycast_scene's plane and sphere PLUS a second sphere at another (x, y).  A plane and one sphere
leave the rotation about the plane's normal through the sphere's centre free, and sum J J^T would be singular along it;
tests/test_track_ref_cpu.py asserts that the eigenvalues of the reference's A / count on the convergence fixture lie within COND_FIXTURE
of each other.

Figures of the numpy-fp32 stand-in against this reference (tests/test_track_ref_cpu.py prints them per case): see that file's docstring.
"""
import functools

import numpy as np

import placement as PL
import tsdf_ref as R

U = 2.0 ** -24
C_POS = 2.0                  # decision tolerance = C_POS * rounding bound (as in tsdf_ref.py)
C_TRACK = 2.0                # route constant of the residual / sum bounds, from the derivation above
AMB_CAP = 0.03               # ambiguous pixels: at most this share of the valid pixels in every case
N_SUMS = 29
Z_NEAR = 1e-3
DIST_MAX = 4 * R.VOXEL       # the truncation distance of the suite's volumes
COND_FIXTURE = 1e3           # eigenvalues of A / count on the convergence fixture: largest <= COND_FIXTURE * smallest
MISTAKES = ("truncation", "swap_fb", "cross_nxp", "normal_negated", "gate_lt")
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]

PLANE_Z = 2.6
SPHERES = (((0.1, 0.05, 2.0), 0.55), ((-0.6, -0.3, 2.15), 0.3))
HELD_OUT_POSE = R.look_at((0.12, -0.08, -0.05), (0.1, 0.0, 2.2))             # tsdf_raycast_ref.HELD_OUT_POSE
# the fixed perturbation of the guess: about 1 cm and 0.5 degrees, xi = (t, omega) in world axes
TWIST = np.array([0.006, -0.005, 0.006, 0.005, -0.004, 0.006])


# ------------------------------------------------------------------------------------------------------------ analytic fixture
def scene_maps(pose, K, H, W):
    """depth [H,W] (z-depth along the optical axis, pixel centres on integers) and unit normals [H,W,3] (world axes, towards the camera)
    of the three-body scene, ray-cast in float64 from the camera-to-world ``pose``"""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = (np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T) @ pose[:3, :3].T
    o = pose[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (PLANE_Z - o[2]) / rays[..., 2]
    t = np.where(np.isfinite(t) & (t > 0), t, np.inf)
    normal = np.zeros((H, W, 3))
    normal[..., 2] = -1.0
    for centre, radius in SPHERES:
        centre = np.asarray(centre, np.float64)
        oc = o - centre
        qa, qb, qc = (rays * rays).sum(-1), 2.0 * (rays @ oc), oc @ oc - radius * radius
        disc = qb * qb - 4 * qa * qc
        ts = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / (2 * qa), np.inf)
        ts = np.where(ts > 0, ts, np.inf)
        nearer = ts < t
        hit = o + rays * np.where(nearer, ts, 0.0)[..., None]
        normal = np.where(nearer[..., None], (hit - centre) / radius, normal)
        t = np.minimum(t, ts)
    ok = np.isfinite(t)
    return np.where(ok, t, 0.0), np.where(ok[..., None], normal, 0.0)


def scene_poses(T, seed=0):
    return R.scene_poses(T, seed=seed)


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_se3(xi):
    """Exp of the twist xi = (t, omega) -> [4,4] float64: R = Rodrigues(omega), translation V t with
    V = I + (1 - cos th) / th^2 [omega]x + (th - sin th) / th^3 [omega]x^2 (series below 1e-6 rad)"""
    xi = np.asarray(xi, np.float64)
    t, w = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    Wx = hat(w)
    if th < 1e-6:
        A, B, C = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        A, B, C = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th ** 3)
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + A * Wx + B * (Wx @ Wx)
    out[:3, 3] = (np.eye(3) + B * Wx + C * (Wx @ Wx)) @ t
    return out


def pose_error(P, P_true):
    """(translation in metres, angle in radians) of P relative to P_true"""
    D = np.asarray(P, np.float64) @ np.linalg.inv(np.asarray(P_true, np.float64))
    return float(np.linalg.norm(D[:3, 3])), float(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


def matrices64(pose_guess, K, model_pose, K_m):
    """L = [R_g K^-1 | c_g], Fm = K_m [R|t]_world->model, Bm = [R_m K_m^-1 | c_m] in float64, rounded to fp32 [3,3,4] (what
    estdepth_amd.camera.frame_align_matrices hands the kernel)"""
    Pg, Pm = np.asarray(pose_guess, np.float64).reshape(4, 4), np.asarray(model_pose, np.float64).reshape(4, 4)
    Kg, Km = np.asarray(K, np.float64).reshape(3, 3), np.asarray(K_m, np.float64).reshape(3, 3)
    L = np.concatenate([Pg[:3, :3] @ np.linalg.inv(Kg), Pg[:3, 3:4]], 1)
    Fm = Km @ np.linalg.inv(Pm)[:3, :4]
    Bm = np.concatenate([Pm[:3, :3] @ np.linalg.inv(Km), Pm[:3, 3:4]], 1)
    return np.stack([L, Fm, Bm]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the contract
def _rows(M, M64, x, y, z):
    """rows 0..2 of the 3x4 matrix at the exact (x, y, z): values in the dtype of M / x / y / z, bounds in float64"""
    x64, y64, z64 = (np.asarray(t, np.float64) for t in (x, y, z))
    val, err = [], []
    for j in range(3):
        val.append(z * (M[j, 0] * x + (M[j, 1] * y + M[j, 2])) + M[j, 3])
        r64 = M64[j, 0] * x64 + M64[j, 1] * y64 + M64[j, 2]
        S = np.abs(M64[j, 0] * x64) + np.abs(M64[j, 1] * y64) + np.abs(M64[j, 2])
        err.append(4 * U * np.abs(z64) * S + U * (2 * np.abs(z64 * r64) + np.abs(M64[j, 3])))
    return val, err


def _point_rows(M, M64, p, e_p):
    val, err = [], []
    p64 = [np.asarray(t, np.float64) for t in p]
    for j in range(3):
        val.append(M[j, 0] * p[0] + (M[j, 1] * p[1] + (M[j, 2] * p[2] + M[j, 3])))
        S = sum(np.abs(M64[j, k] * p64[k]) for k in range(3)) + np.abs(M64[j, 3])
        err.append(4 * U * S + sum(np.abs(M64[j, k]) * e_p[k] for k in range(3)))
    return val, err


def evaluate(c, dtype=np.float64, mistake=None, match=None, _exact=True):
    """``c``: dict(depth [H,W] f32, conf [H,W] f32 or None, conf_min, m_depth [Hm,Wm] f32, m_normal [Hm,Wm,3] f32, mats [3,3,4] f32 (L, Fm, Bm),
    dist_max, z_near) -- the constants as the kernel receives them (rounded to fp32 here).  Returns a dict: match (int64 [H,W], -1 =
    skipped), residual (``dtype``), J [H,W,6], valid, amb (bool), tol_r (float64, absolute, to be scaled by C_TRACK), sums (float64 [29],
    each per-pixel term ONE product in ``dtype``, added in float64) and tol_sums.  ``mistake``: one of MISTAKES, a deliberately WRONG
    contract (the tests' wrong kernels).  ``match``: take the decisions from this map instead of making them."""
    assert mistake is None or mistake in MISTAKES, mistake
    f = dtype
    depth = np.asarray(c["depth"], np.float32)
    m_depth, m_normal = np.asarray(c["m_depth"], np.float32), np.asarray(c["m_normal"], np.float32)
    H, W = depth.shape
    Hm, Wm = m_depth.shape
    assert m_normal.shape == (Hm, Wm, 3)
    M32 = np.asarray(c["mats"], np.float32).reshape(3, 3, 4)
    L32, F32, B32 = (M32[0], M32[2], M32[1]) if mistake == "swap_fb" else (M32[0], M32[1], M32[2])
    L, F, B = L32.astype(f), F32.astype(f), B32.astype(f)
    L64, F64, B64 = (m.astype(np.float64) for m in (L32, F32, B32))
    zn32 = np.float32(c["z_near"])
    d2_32 = np.float32(c["dist_max"]) * np.float32(c["dist_max"])
    zn, zn64, dist2, dist264 = f(zn32), float(zn32), f(d2_32), float(d2_32)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    uf, vf = uu.astype(f), vv.astype(f)
    amb = np.zeros((H, W), bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if match is None:
            valid = np.isfinite(depth) & (depth > zn32)
            if c.get("conf") is not None:
                valid &= np.asarray(c["conf"], np.float32) >= np.float32(c["conf_min"])
        else:
            match = np.asarray(match, np.int64)
            assert match.shape == (H, W) and match.max(initial=-1) < Hm * Wm and match.min(initial=0) >= -1
            valid = match >= 0
        alive = valid.copy()
        d = np.where(valid, depth, np.float32(1.0)).astype(f)
        p, e_p = _rows(L, L64, uf, vf, d)
        if match is None:
            (a, b, cc), (e_a, e_b, e_c) = _point_rows(F, F64, p, e_p)
            c64 = cc.astype(np.float64)
            amb |= alive & (np.abs(c64 - zn64) < C_POS * e_c)
            alive &= cc > zn
            cs = np.where(alive, cc, f(1.0))
            cabs = np.abs(cs.astype(np.float64))
            pix, near = [], np.zeros((H, W), bool)
            for t, e_t in ((a, e_a), (b, e_b)):
                ratio = t / cs
                x = ratio if mistake == "truncation" else ratio + f(0.5)
                r64, x64 = np.abs(ratio.astype(np.float64)), x.astype(np.float64)
                e_x = (e_t + r64 * e_c) / cabs + U * r64 + U * np.abs(x64)
                near |= np.abs(x64 - np.rint(x64)) < C_POS * e_x
                pix.append(np.floor(x))
            amb |= alive & near & np.isfinite(pix[0].astype(np.float64)) & np.isfinite(pix[1].astype(np.float64))
            um, vm = pix
            alive &= (um >= 0) & (um < Wm) & (vm >= 0) & (vm < Hm)
            iu, iv = np.where(alive, um, 0).astype(np.int64), np.where(alive, vm, 0).astype(np.int64)
        else:
            iv, iu = np.where(valid, match, 0) // Wm, np.where(valid, match, 0) % Wm
        dm32 = m_depth[iv, iu]
        if match is None:
            alive &= dm32 > 0
        dm = np.where(alive & np.isfinite(dm32), dm32, np.float32(1.0)).astype(f)
        n = [m_normal[iv, iu, k].astype(f) for k in range(3)]
        if mistake == "normal_negated":
            n = [-t for t in n]
        q, e_q = _rows(B, B64, iu.astype(f), iv.astype(f), dm)
        e = [q[k] - p[k] for k in range(3)]
        e64 = [t.astype(np.float64) for t in e]
        e_e = [e_q[k] + e_p[k] + U * np.abs(e64[k]) for k in range(3)]
        e2 = e[0] * e[0] + (e[1] * e[1] + e[2] * e[2])
        e264 = e2.astype(np.float64)
        if match is None:
            e_e2 = sum(2 * np.abs(e64[k]) * e_e[k] for k in range(3)) + 3 * U * e264
            close = np.abs(e264 - dist264) < C_POS * e_e2
            if f is np.float64 and _exact and close.any():
                s = evaluate(c, np.float32, mistake, None, _exact=False)            # the gate is exact where fp32 reproduces every value
                same = (s["e2"].astype(np.float64) == e264)
                for k in range(3):
                    same &= (s["p"][k].astype(np.float64) == p[k]) & (s["q"][k].astype(np.float64) == q[k]) & (s["e"][k].astype(np.float64) == e[k])
                close &= ~same
            amb |= alive & np.isfinite(dm32) & close
            alive &= np.isfinite(dm32) & ((e2 < dist2) if mistake == "gate_lt" else (e2 <= dist2))
        n64, p64 = [t.astype(np.float64) for t in n], [t.astype(np.float64) for t in p]
        r = n[0] * e[0] + (n[1] * e[1] + n[2] * e[2])
        S_r = sum(np.abs(n64[k] * e64[k]) for k in range(3))
        e_r = sum(np.abs(n64[k]) * e_e[k] for k in range(3)) + 3 * U * S_r
        w, e_w = [], []
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            w.append(p[i] * n[j] - p[j] * n[i])
            e_w.append(np.abs(n64[j]) * e_p[i] + np.abs(n64[i]) * e_p[j] + 2 * U * (np.abs(p64[i] * n64[j]) + np.abs(p64[j] * n64[i])))
        if mistake == "cross_nxp":
            w = [-t for t in w]
        zero = np.zeros((H, W))
        J = [np.where(alive, t, f(0.0)) for t in n + w]
        e_J = [zero, zero, zero] + e_w
        r = np.where(alive, r, f(0.0))
        J64, r64 = [t.astype(np.float64) for t in J], r.astype(np.float64)
        terms = [(J[i] * J[j], np.abs(J64[i]) * e_J[j] + np.abs(J64[j]) * e_J[i] + U * np.abs(J64[i] * J64[j])) for i, j in TRIU]
        terms += [(J[i] * r, np.abs(J64[i]) * e_r + np.abs(r64) * e_J[i] + U * np.abs(J64[i] * r64)) for i in range(6)]
        terms += [(r * r, 2 * np.abs(r64) * e_r + U * r64 * r64), (alive.astype(f), zero)]
        n_match = int(alive.sum())
        sums = np.array([t.astype(np.float64)[alive].sum() for t, _ in terms])
        tol_sums = np.array([tol[alive].sum() + n_match * 2.0 ** -53 * np.abs(t.astype(np.float64)[alive]).sum() for t, tol in terms])
    return {"match": np.where(alive, iv * Wm + iu, -1), "residual": r, "J": np.stack(J, -1), "valid": valid, "amb": amb & valid,
            "tol_r": np.where(alive, e_r, 0.0), "sums": sums, "tol_sums": tol_sums, "e2": e2, "p": p, "q": q, "e": e, "count": n_match}


def compare(got, c, ref=None, label=""):
    """THE comparison of the suite.  ``got``: dict(residual f32 [H,W], match int32 [H,W], sums f64 [29]); ``c`` the case, ``ref`` its
    evaluate(c) (computed here when not given).  Returns a dict of figures after asserting what the module docstring states."""
    ref = evaluate(c) if ref is None else ref
    res, mt, sums = np.asarray(got["residual"]), np.asarray(got["match"]).astype(np.int64), np.asarray(got["sums"], np.float64)
    assert res.shape == ref["residual"].shape and mt.shape == res.shape and sums.shape == (N_SUMS,), (res.shape, mt.shape, sums.shape)
    Hm, Wm = np.asarray(c["m_depth"]).shape
    valid, amb = ref["valid"], ref["amb"]
    n_valid, n_amb = int(valid.sum()), int(amb.sum())
    fig = {"valid": n_valid, "ambiguous": n_amb, "amb_share": n_amb / max(n_valid, 1), "matched": int((mt >= 0).sum()),
           "matched_share": int((mt >= 0).sum()) / max(n_valid, 1)}
    in_range = bool(((mt >= -1) & (mt < Hm * Wm)).all())
    finite = bool(np.isfinite(res).all()) and bool(np.isfinite(sums).all())
    keep = ~amb
    fig["match_mismatch"] = int((keep & (mt != ref["match"])).sum())
    skipped_zero = bool((res[mt < 0] == 0).all())
    both = keep & (mt >= 0) & (ref["match"] == mt)
    err = np.abs(res.astype(np.float64) - ref["residual"].astype(np.float64))[both]
    ratio = err / np.maximum(ref["tol_r"][both], 1e-300)
    fig["residual_ratio"] = float(ratio.max()) if ratio.size else 0.0
    fig["residual_err"] = float(err.max()) if err.size else 0.0
    fig["sum_ratio"], fig["count_exact"] = float("inf"), False
    if in_range and finite:
        given = evaluate(c, match=mt)
        fig["count_exact"] = sums[28] == float((mt >= 0).sum())
        d = np.abs(sums[:28] - given["sums"][:28])
        fig["sum_ratio"] = float(np.max(np.where(d == 0, 0.0, d / np.maximum(given["tol_sums"][:28], 1e-300))))
    print("frame_align compare %s: valid %d ambiguous %d (%.4f) matched %d; match mismatches %d; max error / bound (bar %.1f): residual %.3g "
          "(%.3g m) sums %.3g" % (label, n_valid, n_amb, fig["amb_share"], fig["matched"], fig["match_mismatch"], C_TRACK, fig["residual_ratio"],
                                  fig["residual_err"], fig["sum_ratio"]))
    assert in_range, "%s: a match outside -1 .. Hm Wm - 1" % label
    assert finite, "%s: an output is not finite" % label
    assert n_amb <= AMB_CAP * n_valid, "%s: %d ambiguous pixels exceed %.2f of the %d valid pixels" % (label, n_amb, AMB_CAP, n_valid)
    assert fig["match_mismatch"] == 0, "%s: match differs on %d unambiguous pixels" % (label, fig["match_mismatch"])
    assert skipped_zero, "%s: a skipped pixel's residual is not exactly zero" % label
    assert fig["residual_ratio"] <= C_TRACK, "%s: residual error at %.3f of its bound (bar %.1f)" % (label, fig["residual_ratio"], C_TRACK)
    assert fig["count_exact"], "%s: sums[28] = %r but %d pixels are matched" % (label, sums[28], fig["matched"])
    assert fig["sum_ratio"] <= C_TRACK, "%s: a sum is at %.3f of its bound (bar %.1f)" % (label, fig["sum_ratio"], C_TRACK)
    return fig


# ------------------------------------------------------------------------------------------------------------ Gauss-Newton, float64
def unpack(sums):
    """the 29 sums -> (A [6,6] symmetric, b [6], sum r^2, count)"""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(TRIU):
        A[i, j] = A[j, i] = sums[k]
    return A, np.asarray(sums[21:27], np.float64).copy(), float(sums[27]), int(round(float(sums[28])))


def step(depth, K, pose_guess, model, conf=None, conf_min=0.0, dist_max=DIST_MAX, z_near=Z_NEAR, dtype=np.float64):
    """one evaluation of the system at ``pose_guess``; ``model`` = dict(depth, normal, pose, K) -> dict(A, b, count, rmse, ...)"""
    c = dict(depth=depth, conf=conf, conf_min=conf_min, m_depth=model["depth"], m_normal=model["normal"],
             mats=matrices64(pose_guess, K, model["pose"], model["K"]), dist_max=dist_max, z_near=z_near)
    out = evaluate(c, dtype=dtype, _exact=False)
    A, b, rr, count = unpack(out["sums"])
    out.update(A=A, b=b, count=count, rmse=float(np.sqrt(rr / count)) if count else 0.0)
    return out


def pivoted(A, b, pivot):
    """(A, b) of twists about the world origin -> about ``pivot`` c: G = [[I, 0], [-[c]x, I]], A_c = G A G^T, b_c = G b (None: unchanged)"""
    if pivot is None:
        return A, b
    G = np.eye(6)
    G[3:, :3] = -hat(np.asarray(pivot, np.float64).reshape(3))
    Ac = G @ A @ G.T
    return 0.5 * (Ac + Ac.T), G @ b


def pivot_step(xi, pivot):
    """C Exp(xi) C^-1 with C the translation by the pivot: the twist applied about the pivot (None: about the world origin)"""
    E = exp_se3(xi)
    if pivot is not None:
        c = np.asarray(pivot, np.float64).reshape(3)
        E[:3, 3] += c - E[:3, :3] @ c
    return E


def refine(depth, K, pose_guess, model, iters=10, pivot=None, **kw):
    """``iters`` Gauss-Newton steps P <- Exp(xi) P with A xi = b (Cholesky), no stopping rule -> (pose, [rmse per evaluation]).
    ``pivot``: every system is re-expressed about it and the step is the twist about it, as tracking.gauss_newton does (None: the world
    origin, the method before the pivot)"""
    P, trace = np.asarray(pose_guess, np.float64).copy(), []
    for _ in range(iters):
        s = step(depth, K, P, model, **kw)
        trace.append(s["rmse"])
        A, b = pivoted(s["A"], s["b"], pivot)
        Lc = np.linalg.cholesky(A)
        xi = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
        P = pivot_step(xi, pivot) @ P
    return P, trace


def refine_stopped(depth, K, pose_guess, model, max_iter=10, min_count=100, pivot=None, cond_max=1e6, step_t=1e-5, step_r=1e-5, **kw):
    """tracking.refine_pose in this module's words: the refusals (count, cholesky, condition at ``cond_max``) and the stopping rule of
    tracking.gauss_newton on the float64 systems -> dict(pose, converged, reason, iterations, cond = cond(A_c) of the first system)"""
    guess = np.asarray(pose_guess, np.float64).copy()
    P, reason, done, cond = guess.copy(), "max_iter", 0, None
    for it in range(max_iter):
        s = step(depth, K, P, model, **kw)
        if s["count"] < min_count:
            return dict(pose=guess, converged=False, reason="count", iterations=it, cond=cond)
        A, b = pivoted(s["A"], s["b"], pivot)
        cond = float(np.linalg.cond(A)) if cond is None else cond
        try:
            Lc = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return dict(pose=guess, converged=False, reason="cholesky", iterations=it, cond=cond)
        ev = np.linalg.eigvalsh(A)
        if not ev[0] > 0 or ev[-1] > cond_max * ev[0]:
            return dict(pose=guess, converged=False, reason="condition", iterations=it, cond=cond)
        xi = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
        P = pivot_step(xi, pivot) @ P
        done = it + 1
        if np.linalg.norm(xi[:3]) < step_t and np.linalg.norm(xi[3:]) < step_r:
            reason = "converged"
            break
    return dict(pose=P, converged=reason == "converged", reason=reason, iterations=done, cond=cond)


# ------------------------------------------------------------------------------------------------------------ the cases of the suite
# name: live size, extras.  hw_m: the model maps' size (default: the live maps'); model: the model camera ("true": the frame's own pose,
# "other": a neighbouring pose); conf: a confidence map gated at 0.3; holes: invalid depths in both maps; away: the guess looks away
ROUTE_SIZES = [(1, 1), (15, 17), (16, 16), (17, 33), (10, 270)]
CASES = {"r%dx%d" % hw: dict(hw=hw) for hw in ROUTE_SIZES}
CASES.update({
    "mid": dict(hw=(120, 160), holes=True),
    "mid-conf": dict(hw=(120, 160), conf=True, model="other"),
    "mid-model90": dict(hw=(120, 160), hw_m=(90, 120), model="other"),
    "small-model": dict(hw=(17, 33), hw_m=(40, 56), conf=True),
    "away": dict(hw=(33, 40), away=True),
})
FULL_CASE = dict(hw=(480, 640), holes=True, model="other")
NOISE = 0.002                # multiplicative Gaussian noise of the live depth: residuals of a few millimetres beside the twist's


def perturbed(pose, scale=1.0):
    return exp_se3(scale * TWIST) @ np.asarray(pose, np.float64)


def make_case(hw, hw_m=None, model="true", conf=False, holes=False, away=False, noise=NOISE, seed=0, name="", place=None):
    """``place`` (placement.py): the same case in the placed world.  A depth map does not change when the world moves with its camera;
    the poses become W P and the model's normals, which are in world axes, W's rotation of them, in float64 before the one rounding"""
    H, W = hw
    Hm, Wm = hw_m or hw
    K, K_m = R.intrinsics(H, W), R.intrinsics(Hm, Wm)
    pose = HELD_OUT_POSE
    model_pose = pose if model == "true" else R.look_at((0.07, -0.05, -0.02), (0.12, 0.02, 2.2))
    rng = np.random.RandomState(23 + seed)
    depth = scene_maps(pose, K, H, W)[0]
    depth = (depth * (1.0 + noise * rng.randn(H, W))).astype(np.float32)
    m_depth, m_normal = scene_maps(model_pose, K_m, Hm, Wm)
    guess = perturbed(pose)
    if PL.key(place) is not None:
        m_normal = PL.vectors(m_normal, place)
        pose, model_pose, guess = PL.pose(pose, place), PL.pose(model_pose, place), PL.pose(guess, place)
    m_depth, m_normal = m_depth.astype(np.float32), m_normal.astype(np.float32)
    if holes:
        depth[H // 12:H // 4, W // 8:W // 3] = 0.0
        depth[H // 2:H // 2 + H // 8, W // 2:W // 2 + W // 4] = np.nan
        depth[3 * H // 4:3 * H // 4 + H // 10, W // 5:W // 2] = np.inf
        depth[H // 3:H // 3 + 5, 5:15] = -1.0
        m_depth[Hm // 3:Hm // 2, 2 * Wm // 3:5 * Wm // 6] = 0.0
        m_normal[Hm // 3:Hm // 2, 2 * Wm // 3:5 * Wm // 6] = 0.0
    if away:
        guess = guess @ np.diag([-1.0, 1.0, -1.0, 1.0])            # half a turn about y: the frame looks away from the model
    cf = rng.uniform(0.0, 1.0, size=(H, W)).astype(np.float32) if conf else None
    return dict(name=name, depth=depth, conf=cf, conf_min=0.3 if conf else 0.0, m_depth=m_depth, m_normal=m_normal, K=K, K_m=K_m, pose=pose,
                guess=guess, model_pose=model_pose, mats=matrices64(guess, K, model_pose, K_m), dist_max=DIST_MAX, z_near=Z_NEAR)


def tie_case():
    """A 16 x 16 fronto-parallel plane at 2.25 m as the model, the live map at 2.0 m, identical poses, f = 64, principal point (8, 8):
    every value of the chain is exact in fp32, e = 0.25 (x, y, 1) with x = (u - 8) / 64, and dist_max = 0.25 is met with equality at
    pixel (8, 8) alone: the contract's <= matches it, every other pixel is farther away"""
    H = W = 16
    K = np.array([[64.0, 0.0, 8.0], [0.0, 64.0, 8.0], [0.0, 0.0, 1.0]])
    P = np.eye(4)
    normal = np.zeros((H, W, 3), np.float32)
    normal[..., 2] = -1.0
    return dict(name="tie", depth=np.full((H, W), 2.0, np.float32), conf=None, conf_min=0.0, m_depth=np.full((H, W), 2.25, np.float32),
                m_normal=normal, K=K, K_m=K, pose=P, guess=P, model_pose=P, mats=matrices64(P, K, P, K), dist_max=0.25, z_near=Z_NEAR)


@functools.lru_cache(maxsize=None)
def build_case(name, place=None):
    """the case ``name``; ``place``: the same case built at that placement (not the tie)"""
    if name == "tie":
        assert PL.key(place) is None
        return tie_case()
    c = dict(FULL_CASE if name == "full" else CASES[name])
    if PL.key(place) is not None:
        return make_case(c.pop("hw"), seed=len(name), name="%s@%s" % (name, PL.label(place)), place=PL.key(place), **c)
    return make_case(c.pop("hw"), seed=len(name), name=name, **c)


@functools.lru_cache(maxsize=None)
def reference(name, place=None):
    """the float64 evaluation of a case, computed once and shared"""
    return evaluate(build_case(name, place))


# the placed case of the feature suite: the smallest value case, 64 m and 128 m out -- not 512 m: the reference's own ambiguous share
# passes AMB_CAP beyond 128 m (tests/test_placement_ref_cpu.py measures it: 0.029 at 128 m, 0.056 at 256 m)
PLACED_CASE, PLACED_AT = "mid", (64, 128)


@functools.lru_cache(maxsize=None)
def convergence_fixture(hw=(120, 160), place=None):
    """the held-out frame against the analytic model maps at the true pose, the guess off by TWIST -> dict(depth, K, pose, guess, model,
    centre).  ``place`` (placement.py): the same frame, model and guess in the placed world -- the poses W P, the normals turned in
    float64 before their one rounding, the twist of the guess conjugated (the same motion of the camera); ``centre``: the placed point
    the error of a pose is measured at"""
    H, W = hw
    K = R.intrinsics(H, W)
    depth, normal = scene_maps(HELD_OUT_POSE, K, H, W)
    centre = np.array(SCENE_CENTRE)
    if PL.key(place) is not None:
        pose, normal, centre = PL.pose(HELD_OUT_POSE, place), PL.vectors(normal, place), PL.points(centre, place)
        guess = PL.pose(perturbed(HELD_OUT_POSE), place)
    else:
        pose, guess = HELD_OUT_POSE, perturbed(HELD_OUT_POSE)
    model = dict(depth=depth.astype(np.float32), normal=normal.astype(np.float32), pose=pose, K=K)
    return dict(depth=depth.astype(np.float32), K=K, pose=pose, guess=guess, model=model, centre=centre)


SCENE_CENTRE = (0.0, 0.0, 2.2)               # between the spheres and the plane: where a pose's error is measured in metres


def pose_error_at(P, P_true, centre):
    """(metres at ``centre``, radians) of the pose P relative to P_true: how far the motion P P_true^-1 moves the world point ``centre``,
    and its angle.  pose_error measures the translation at the world origin, where an angle error of a placed scene is multiplied by
    the scene's distance"""
    D = np.asarray(P, np.float64) @ np.linalg.inv(np.asarray(P_true, np.float64))
    c = np.asarray(centre, np.float64)
    return float(np.linalg.norm(D[:3, :3] @ c + D[:3, 3] - c)), float(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
