"""float64 reference of the colour contracts of the library (csrc/tsdf.hip, csrc/tsdf_raycast.hip; include/estd_hip.h: estd_tsdf_integrate_color,
estd_tsdf_edge_colors, estd_tsdf_raycast_color), beside tests/tsdf_ref.py and tests/tsdf_raycast_ref.py.  A plain helper module of the test suite
(not a conftest); numpy only.

``integrate`` restates the decisions of ``tsdf_ref.integrate`` (steps 1-6) and adds step 7; tests/test_tsdf_color_ref_cpu.py asserts that its
D, Wt, ``updated`` and ``amb`` equal tsdf_ref's exactly on every case, so the two cannot drift apart.  Colour adds no decision of its own: the
pixel is the one the depth was read at, so the ambiguous voxels are tsdf_ref's and their share stays under tsdf_ref.AMB_CAP.

Colour bound (first order, u = 2^-24), per update of a voxel with m = max(|C|, |col|) over the three channels' own values:
    C' = (C Wt + col w) / (Wt + w).  The kernel rounds col w, the fused multiply-add, Wt + w (exact in unweighted mode) and the quotient: four
    roundings, each of a value that is at most m after the division, so 4 u m; the error C already carries is passed on with the
    weight Wt / (Wt + w):                   A_c' = A_c Wt / (Wt + w) + 4 m,          |C - C_ref| <= C_COLOR u A_c.
    C_COLOR: 1 would cover the kernel with exact weights.  The numpy-fp32 stand-in has no fused multiply-add and rounds C Wt as well: 5 / 4.
    In weighted mode the kernel's Wt is itself a rounded sum (relative error <= (n - 1) u after n updates) where the reference's is exact;
    d C' / d Wt = w (C - col) / (Wt + w)^2 and |C - col| <= 2 m, Wt w / (Wt + w)^2 <= 1 / 4, so this moves C' by at most (n - 1) u m / 2 =
    (n - 1) / 8 of the update's 4 m: 3 / 8 for the four updates at most that the weighted case of the suite applies to a voxel.
    5 / 4 + 3 / 8 = 1.625, rounded up for what first order leaves out:            C_COLOR = 2.
    (Weighted fusion of many more frames onto one voxel grows the (n - 1) / 8 term; the constant is stated for the cases of the suite.)

``edge_colors``: out = C0 + s (C1 - C0) with s = D0 / (D0 - D1): the expression of the extraction's point weight, so its bound
    C_EXTRACT u (|C0| + |C1|) applies as it stands (tsdf_ref.py).

``render_colors``: the colour of tsdf_raycast_ref.raycast's hit.  (k, s) are recovered from that reference's own float64 depth = t_{k-1} + dt s:
    q = (depth - t_min) / dt, k - 1 = floor(q), s = q - floor(q).  The blend is continuous across a sample boundary (s = 1 on the pair
    (k - 1, k) and s = 0 on (k, k + 1) both give Cb_k), so the only pixels left out are those whose remainder lies within C_RAY tol_depth / dt
    of 0 or 1 (the kernel's pair may be the neighbouring one, whose far cell need not be observed); they count as ambiguous, under
    tsdf_raycast_ref.AMB_CAP together with that module's own.
    Cb = the trilinear blend of a cell's corner colours, e_Cb = 16 u max|corner| + (max corner - min corner) sum_j e_p_j (the bound of Wb);
    colour = Cb0 + s (Cb1 - Cb0):  tol = |Cb1 - Cb0| e_s + e_Cb0 + e_Cb1 + 3 u (|Cb0| + |Cb1|), e_s <= tol_depth / dt; compared at C_RAY tol.
"""
import functools

import numpy as np

import tsdf_ref as R
import tsdf_raycast_ref as RR

U = R.U
C_POS = R.C_POS
# Route constant of the colour bound, from the derivation above.  It holds for unweighted fusion of any number of frames and for weighted
# fusion of at most four updates per voxel (the suite's cases); weighted fusion of n updates needs color_constant(n).
C_COLOR = 2.0


def color_constant(n_updates, weighted=True):
    """the constant of the colour bound for ``n_updates`` updates of a voxel: 5 / 4 (unfused evaluation) + (n - 1) / 8 in weighted mode
    (the rounded weight sums), rounded up to the next multiple of 1 / 2 and never below C_COLOR"""
    c = 1.25 + (max(int(n_updates), 1) - 1) / 8.0 * bool(weighted)
    return max(C_COLOR, float(np.ceil(2 * c) / 2))
# test-only knob: plausible kernel mistakes (tests/test_tsdf_color_ref_cpu.py asserts that compare rejects each on some case)
MISTAKES = ("color_weight_after",)
CASES = ("t1", "t3", "t8", "gated", "weighted", "second", "holes", "odd")
NORMALISED = ("t3", "weighted")          # cases that are also run with images normalised to negative values
MEDIAN_FACTOR = 1.25         # the semantic bar: median colour error at the extracted points <= this x the float64 reference's own median
OMEGA = 3.0                  # rad / m of the texture


# ------------------------------------------------------------------------------------------------------------ analytic texture
def texture(xyz):
    """[..., 3] world points -> [..., 3] colour: three sinusoids around 127.5 +- 100"""
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    return 127.5 + 100.0 * np.stack([np.sin(OMEGA * (x + 0.3 * z)), np.sin(OMEGA * (y - 0.2 * x) + 1.0),
                                     np.sin(OMEGA * (z + 0.5 * x + 0.5 * y) + 2.0)], -1)


def case_images(case, normalised=False):
    """[T,3,H,W] float32: the texture at the back-projected depth of every pixel, zero where the depth is invalid; ``normalised``:
    (value - 127.5) / 100 where valid (negative values)"""
    out = []
    for t in range(case["depths"].shape[0]):
        d = case["depths"][t]
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(d) & (d > 0)
        pts = RR.backproject(np.where(ok, d, 1.0), case["poses"][t], case["K"])
        col = texture(pts)
        if normalised:
            col = (col - 127.5) / 100.0
        out.append(np.where(ok[..., None], col, 0.0).transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------ integrate
def integrate(D0, W0, C0, mats, depths, images, confs=None, *, trunc, z_near=1e-3, conf_min=0.0, weighted=False, w_max=64.0, dtype=np.float64,
              z_block=16, mistake=None):
    """D0, W0 [Z,Y,X], C0 [3,Z,Y,X] float32 (before the call); mats [T,3,4] float32; depths / confs [T,H,W], images [T,3,H,W] float32.
    ``dtype=np.float32`` evaluates the contract in numpy fp32 arithmetic (the CPU stand-in for the kernel).
    ``mistake``: one of MISTAKES, a deliberately wrong variant for the discrimination test.
    Returns dict(D, Wt, C (``dtype``), A_c [Z,Y,X] (float64, units of 2^-24), updated, amb (bool))."""
    assert mistake is None or mistake in MISTAKES, mistake
    f = dtype
    D0, W0, C0 = np.asarray(D0, dtype=np.float32), np.asarray(W0, dtype=np.float32), np.asarray(C0, dtype=np.float32)
    mats = np.asarray(mats, dtype=np.float32).reshape(-1, 3, 4)
    depths, images = np.asarray(depths, dtype=np.float32), np.asarray(images, dtype=np.float32)
    T, H, W = depths.shape
    assert mats.shape[0] == T and images.shape == (T, 3, H, W)
    Z, Y, X = D0.shape
    trunc32, znear32, cmin32, wmax32 = (np.float32(v) for v in (trunc, z_near, conf_min, w_max))
    dvalid = np.where(np.isfinite(depths) & (depths > 0), depths.astype(np.float64), -np.inf)
    pad = np.pad(dvalid, ((0, 0), (1, 1), (1, 1)), constant_values=-np.inf)
    dmax3 = np.max([pad[:, i:i + H, j:j + W] for i in range(3) for j in range(3)], axis=0)
    out = {"D": np.empty((Z, Y, X), dtype=f), "Wt": np.empty((Z, Y, X), dtype=f), "C": np.empty((3, Z, Y, X), dtype=f), "A_c": np.zeros((Z, Y, X)),
           "updated": np.zeros((Z, Y, X), dtype=bool), "amb": np.zeros((Z, Y, X), dtype=bool)}
    for zb in range(0, Z, z_block):
        sl = slice(zb, min(Z, zb + z_block))
        iz, iy, ix = np.meshgrid(np.arange(sl.start, sl.stop, dtype=np.float64), np.arange(Y, dtype=np.float64),
                                 np.arange(X, dtype=np.float64), indexing="ij")
        D, Wt, C = D0[sl].astype(f), W0[sl].astype(f), C0[:, sl].astype(f)
        Ac = np.zeros(D.shape)
        upd = np.zeros(D.shape, dtype=bool)
        amb = np.zeros(D.shape, dtype=bool)
        for t in range(T):
            # ---- steps 1-6: the decisions of tsdf_ref.integrate, restated
            a, Sa = R._dot4(mats[t, 0], ix, iy, iz, f)
            b, Sb = R._dot4(mats[t, 1], ix, iy, iz, f)
            c, Sc = R._dot4(mats[t, 2], ix, iy, iz, f)
            ea, eb, ec = 4 * U * Sa, 4 * U * Sb, 4 * U * Sc
            front = c > f(znear32)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                qa, qb = a / c, b / c
                qu, qv = qa + f(0.5), qb + f(0.5)
                c64 = np.abs(c.astype(np.float64))
                e_qu = (ea + np.abs(qa.astype(np.float64)) * ec) / c64 + U * np.abs(qa.astype(np.float64)) + U * np.abs(qu.astype(np.float64))
                e_qv = (eb + np.abs(qb.astype(np.float64)) * ec) / c64 + U * np.abs(qb.astype(np.float64)) + U * np.abs(qv.astype(np.float64))
                fu, fv = np.floor(qu), np.floor(qv)
            inimg = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            d_c = C_POS * ec
            maybe_front = c.astype(np.float64) > float(znear32) - d_c
            with np.errstate(invalid="ignore"):
                near_img = maybe_front & (qu >= -1) & (qu <= W + 1) & (qv >= -1) & (qv <= H + 1)
                fr_u = np.abs(qu.astype(np.float64) - np.round(qu.astype(np.float64)))
                fr_v = np.abs(qv.astype(np.float64) - np.round(qv.astype(np.float64)))
                uc = np.clip(np.nan_to_num(np.floor(qu.astype(np.float64)), nan=0.0), 0, W - 1).astype(np.int64)
                vc = np.clip(np.nan_to_num(np.floor(qv.astype(np.float64)), nan=0.0), 0, H - 1).astype(np.int64)
                reach = dmax3[t][vc, uc] - c.astype(np.float64) >= -float(trunc32) - C_POS * (ec + U * np.abs(c.astype(np.float64)))
                amb |= near_img & reach & ((fr_u < C_POS * e_qu) | (fr_v < C_POS * e_qv))
            amb |= np.abs(c.astype(np.float64) - float(znear32)) < d_c
            ui = np.where(inimg, fu, 0).astype(np.int64)
            vi = np.where(inimg, fv, 0).astype(np.int64)
            d = depths[t][vi, ui]
            with np.errstate(invalid="ignore"):
                ok = inimg & (d > 0) & np.isfinite(d)
            w = np.ones(D.shape, dtype=f)
            if confs is not None:
                cf = np.asarray(confs[t], dtype=np.float32)[vi, ui]
                with np.errstate(invalid="ignore"):
                    amb |= ok & (np.abs(cf.astype(np.float64) - float(cmin32)) <= 2.0 ** -23 * abs(float(cmin32)))
                    ok &= ~(cf < cmin32)
                    if weighted:
                        w = cf.astype(f)
                        ok &= (cf > 0) & np.isfinite(cf)
            d = np.where(ok, d, np.float32(1.0))
            with np.errstate(invalid="ignore", over="ignore"):
                sdf = d.astype(f) - c
                e_sdf = ec + U * np.abs(sdf.astype(np.float64))
                amb |= ok & (np.abs(sdf.astype(np.float64) + float(trunc32)) < C_POS * e_sdf)
                ok &= ~(sdf < -f(trunc32))
                tsdf = np.minimum(f(1.0), sdf / f(trunc32))
            w = np.where(ok, w, f(1.0))
            tsdf = np.where(ok, tsdf, f(0.0))
            den = Wt + w
            Dn = (D * Wt + tsdf * w) / den
            # ---- step 7: the colour of the pixel the depth was read at, blended with the weight BEFORE step 6
            m = np.zeros(D.shape)
            for k in range(3):
                col = images[t, k][vi, ui].astype(f)
                m = np.maximum(m, np.maximum(np.abs(C[k].astype(np.float64)), np.abs(col.astype(np.float64))))
                if mistake == "color_weight_after":          # blended with the weight the D update leaves behind, not the one it starts from
                    Wn = np.minimum(den, f(wmax32))
                    C[k] = np.where(ok, (C[k] * Wn + col * w) / (Wn + w), C[k])
                    continue
                C[k] = np.where(ok, (C[k] * Wt + col * w) / den, C[k])
            Ac = np.where(ok, Ac * Wt.astype(np.float64) / den.astype(np.float64) + 4.0 * m, Ac)
            D = np.where(ok, Dn, D)
            Wt = np.where(ok, np.minimum(den, f(wmax32)), Wt)
            upd |= ok
        out["D"][sl], out["Wt"][sl], out["C"][:, sl], out["A_c"][sl], out["updated"][sl], out["amb"][sl] = D, Wt, C, Ac, upd, amb
    return out


def compare(got_C, ref, C_before=None):
    """THE colour comparison of the suite.  got_C [3,Z,Y,X] fp32; ``ref`` from integrate(dtype=float64).  Asserts the ambiguous share <=
    tsdf_ref.AMB_CAP, |C - C_ref| <= C_COLOR 2^-24 A_c on unambiguous updated voxels and, with ``C_before``, that voxels the reference
    leaves alone keep their bits.  Returns the figures."""
    got_C = np.asarray(got_C)
    amb, upd = ref["amb"], ref["updated"]
    n_upd, n_amb = int(upd.sum()), int(amb.sum())
    fig = {"updated": n_upd, "ambiguous": n_amb, "amb_share": n_amb / max(n_upd, 1)}
    assert n_amb <= R.AMB_CAP * max(n_upd, 1), "ambiguous share %.4f of %d updated voxels exceeds %.2f" % (fig["amb_share"], n_upd, R.AMB_CAP)
    sel = ~amb & upd
    err = np.abs(got_C.astype(np.float64) - ref["C"].astype(np.float64)).max(0)
    ratio = np.where(sel, err / (U * np.maximum(ref["A_c"], 1e-30)), 0.0)
    fig["max_ratio"] = float(ratio.max()) if sel.any() else 0.0
    fig["max_abs"] = float(err[sel].max()) if sel.any() else 0.0
    print("tsdf colour compare: updated %d ambiguous %d (%.4f) max |dC| %.3g max ratio %.3f (bound %.1f)"
          % (n_upd, n_amb, fig["amb_share"], fig["max_abs"], fig["max_ratio"], C_COLOR))
    assert np.isfinite(got_C).all(), "a colour is not finite"
    assert fig["max_ratio"] <= C_COLOR, "max |C - C_ref| / (2^-24 A_c) = %.3f > %.1f" % (fig["max_ratio"], C_COLOR)
    if C_before is not None:
        still = ~amb & ~upd
        for k in range(3):
            assert np.array_equal(got_C[k].view(np.uint32)[still], np.asarray(C_before)[k].view(np.uint32)[still]), "an untouched voxel's colour changed"
    return fig


# ------------------------------------------------------------------------------------------------------------ edge colours
def edge_colors(D32, C32, edge):
    """D32 [Z,Y,X], C32 [3,Z,Y,X] float32; edge [N] int64 -> (colour [N,3] float64, tol [N,3] absolute); ids outside the volume give zeros"""
    D32, C32, edge = np.asarray(D32, np.float32), np.asarray(C32, np.float32), np.asarray(edge, np.int64)
    Z, Y, X = D32.shape
    n_vox = Z * Y * X
    idx, k = edge // 3, edge % 3
    x, y, z = idx % X, (idx // X) % Y, idx // (X * Y)
    q = np.stack([x, y, z], -1)
    dims, strides = np.array([X, Y, Z]), np.array([1, X, X * Y])
    ok = (edge >= 0) & (edge < 3 * n_vox)
    ok &= np.where(ok, q[np.arange(len(edge)), k] + 1 < dims[k], False)
    i0 = np.where(ok, idx, 0)
    i1 = np.where(ok, idx + strides[k], 0)
    Df, Cf = D32.reshape(-1).astype(np.float64), C32.reshape(3, -1).astype(np.float64)
    d0, d1 = Df[i0], Df[i1]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = d0 / (d0 - d1)
    c0, c1 = Cf[:, i0].T, Cf[:, i1].T
    with np.errstate(invalid="ignore"):
        col = np.where(ok[:, None], c0 + s[:, None] * (c1 - c0), 0.0)
    tol = R.C_EXTRACT * U * (np.abs(c0) + np.abs(c1))
    return col, np.where(ok[:, None], tol, 0.0)


def compare_edge_colors(got, edge, D32, C32):
    col, tol = edge_colors(D32, C32, edge)
    err = np.abs(np.asarray(got, np.float64) - col)
    ratio = err / np.maximum(tol, 1e-300)
    worst = float(np.where(tol > 0, ratio, 0.0).max()) * R.C_EXTRACT if len(edge) else 0.0
    print("tsdf edge colours: %d records, worst error in units of 2^-24 (|C0| + |C1|): %.3f (bound %.1f)" % (len(edge), worst, R.C_EXTRACT))
    assert (err <= tol).all(), "edge colour: worst error %.3g at %.3f of its bound" % (err.max(), ratio[tol > 0].max() if (tol > 0).any() else np.inf)
    return worst


def median_error(xyz, color):
    """the semantic score: per point the largest channel error against the analytic texture -> (median, 95th percentile)"""
    e = np.abs(np.asarray(color, np.float64) - texture(np.asarray(xyz, np.float64))).max(-1)
    return float(np.median(e)), float(np.percentile(e, 95))


def reference_median(ref, case, w_min=1.0):
    """(median, p95) of the float64 reference's own colour at its own extracted points"""
    D32, W32 = ref["D"].astype(np.float32), ref["Wt"].astype(np.float32)
    pts = R.extract(D32, W32, w_min, case["voxel"], case["origin"])
    col, _ = edge_colors(D32, ref["C"].astype(np.float32), pts["edge"])
    return median_error(pts["xyz"], col)


# ------------------------------------------------------------------------------------------------------------ render colour
def render_colors(D, Wt, C, view, w_min, ray=None):
    """D, Wt [Z,Y,X], C [3,Z,Y,X] float32; ``view`` from tsdf_raycast_ref.view -> dict(color [H,W,3] float64, tol_color [H,W,3] (absolute, to be
    scaled by C_RAY), amb [H,W] (tsdf_raycast_ref's own and the pixels next to a sample boundary), ray: that module's result)"""
    D, Wt, C = np.asarray(D, np.float32), np.asarray(Wt, np.float32), np.asarray(C, np.float32)
    H, W = view["H"], view["W"]
    if ray is None:
        ray = RR.raycast(D, Wt, view["M"], H, W, view["t_min"], view["dt"], view["n_steps"], w_min)
    M = np.asarray(view["M"], np.float32).astype(np.float64).reshape(3, 4)
    tmin, dt = float(np.float32(view["t_min"])), float(np.float32(view["dt"]))
    hit = ray["hit"]
    v, u = np.nonzero(hit)
    q = (ray["depth"][hit].astype(np.float64) - tmin) / dt
    k0 = np.floor(q)
    s = q - k0
    margin = RR.C_RAY * ray["tol_depth"][hit] / dt
    near = (s < margin) | (s > 1 - margin)
    r = np.stack([M[j, 0] * u + (M[j, 1] * v + M[j, 2]) for j in range(3)], 1)
    S = np.stack([np.abs(M[j, 0] * u) + np.abs(M[j, 1] * v) + np.abs(M[j, 2]) for j in range(3)], 1)
    Z, Y, X = D.shape
    C64 = C.astype(np.float64)
    Cb, eCb = [], []
    for kk in (k0, k0 + 1):
        t = tmin + kk * dt
        p = M[None, :, 3] + t[:, None] * r
        e_p = U * (4 * t[:, None] * S + 4 * np.abs(t[:, None] * r) + np.abs(M[None, :, 3]))
        fl = np.floor(p)
        ii = fl.astype(np.int64)
        inside = ((ii >= 0) & (ii <= np.array([X - 2, Y - 2, Z - 2])[None])).all(1)
        near |= ~inside
        ii = np.where(inside[:, None], ii, 0)
        fx, fy, fz = (p - fl).T
        ix, iy, iz = ii.T
        c = {(dx, dy, dz): C64[:, iz + dz, iy + dy, ix + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}           # [3,n] each
        L = RR._lerp
        blend = L(L(L(c[0, 0, 0], c[1, 0, 0], fx), L(c[0, 1, 0], c[1, 1, 0], fx), fy),
                  L(L(c[0, 0, 1], c[1, 0, 1], fx), L(c[0, 1, 1], c[1, 1, 1], fx), fy), fz)
        cs = np.stack(list(c.values()))
        Cb.append(blend.T)
        eCb.append((16 * U * np.abs(cs).max(0) + (cs.max(0) - cs.min(0)) * e_p.sum(1)[None]).T)
    col = Cb[0] + s[:, None] * (Cb[1] - Cb[0])
    tol = np.abs(Cb[1] - Cb[0]) * (ray["tol_depth"][hit] / dt)[:, None] + eCb[0] + eCb[1] + 3 * U * (np.abs(Cb[0]) + np.abs(Cb[1]))
    out = {"color": np.zeros((H, W, 3)), "tol_color": np.zeros((H, W, 3)), "amb": ray["amb"].copy(), "ray": ray}
    out["color"][hit], out["tol_color"][hit] = col, tol
    out["amb"][v[near], u[near]] = True
    return out


def compare_render(got_color, ref, label=""):
    """got_color [H,W,3] fp32 against render_colors' result: ambiguous share <= AMB_CAP of the hit pixels, no-hit pixels exactly zero,
    |colour - ref| <= C_RAY tol on the others"""
    g = np.asarray(got_color)
    hit, amb = ref["ray"]["hit"], ref["amb"]
    n_hit, n_amb = int(hit.sum()), int(amb.sum())
    assert n_amb <= RR.AMB_CAP * n_hit, "%s: %d ambiguous pixels exceed %.2f of the %d hit pixels" % (label, n_amb, RR.AMB_CAP, n_hit)
    assert np.isfinite(g).all(), "a rendered colour is not finite"
    assert (g[~amb & ~hit] == 0).all(), "%s: a pixel without a hit has a colour" % label
    sel = ~amb & hit
    err = np.abs(g.astype(np.float64) - ref["color"])[sel]
    ratio = err / np.maximum(ref["tol_color"][sel], 1e-300)
    worst = float(ratio.max()) if ratio.size else 0.0
    print("tsdf render colour %s: hit %d ambiguous %d (%.4f) max error / bound %.3f (bar %.1f), max |dC| %.3g"
          % (label, n_hit, n_amb, n_amb / max(n_hit, 1), worst, RR.C_RAY, float(err.max()) if err.size else 0.0))
    assert worst <= RR.C_RAY, "%s: colour error at %.3f of its bound (bar %.1f)" % (label, worst, RR.C_RAY)
    return {"hit": n_hit, "ambiguous": n_amb, "amb_share": n_amb / max(n_hit, 1), "color_ratio": worst}


# ------------------------------------------------------------------------------------------------------------ the fixtures of the suite
def sentinel(dims, seed):
    """a pattern that no update produces by accident, for planes the kernel must leave alone"""
    return np.random.RandomState(seed).uniform(-0.9, 0.9, size=dims).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture(name, normalised=False):
    """One case of tsdf_ref.CASES with its images, the matrices the kernel receives, the sentinel-filled planes the tests start from (D and
    colour a pattern, weight zero) and the float64 reference of the FIRST call on them; computed once and shared by the tests that need it
    (treat as read-only)."""
    import torch
    from estdepth_amd import camera
    case = R.build_case(name)
    images = case_images(case, normalised)
    mats = camera.tsdf_matrices(torch.from_numpy(case["poses"]), torch.from_numpy(case["K"]), case["origin"], case["voxel"]).numpy().reshape(-1, 3, 4)
    D0, W0 = sentinel(case["dims"], 11), np.zeros(case["dims"], np.float32)
    C0 = sentinel((3,) + tuple(case["dims"]), 12)
    ref = integrate(D0, W0, C0, mats, case["depths"], images, case["confs"], **case["params"])
    return {"case": case, "images": images, "mats": mats, "D0": D0, "W0": W0, "C0": C0, "ref": ref}
