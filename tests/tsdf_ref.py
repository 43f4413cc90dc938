"""float64 reference of the TSDF contracts of the library (csrc/tsdf.hip, include/estd_hip.h: estd_tsdf_integrate and
estd_tsdf_extract_points), in the style of tests/sweep_fusion_ref.py.  A plain helper module of the test suite (not a conftest); numpy only.

``integrate`` evaluates the update rule in float64 FROM THE fp32 MATRICES, DEPTH MAPS AND CONSTANTS THE KERNEL RECEIVES and returns, per
voxel, the expected ``D`` and ``Wt``, an error magnitude ``A`` (in units of 2^-24), the voxels some frame ``updated`` and the voxels that are
``amb``iguous: a discontinuous decision of some frame lies within the fp32 rounding of the kernel's evaluation, so either side is right and
the voxel is left out of the value comparison.  ``compare`` is THE comparison of the suite (GPU results and the numpy-fp32 evaluation alike):

    Wt exact (unweighted: small integers; weighted: |Wt - ref| <= C_INTEGRATE 2^-24 n_updates Wt)      |D - D_ref| <= C_INTEGRATE 2^-24 A

Rounding bounds (first order, u = 2^-24; the ``E``-class idiom of sweep_fusion_ref.py, written out for the one expression chain there is)
    a = A0 ix + A1 iy + A2 iz + A3: four terms t_j, S = sum |t_j|.  The kernel nests three fused multiply-adds (three roundings, each of a
        partial sum <= S); an evaluation with separate products rounds each t_j as well (<= u S in total).  e_a = 4 u S_a covers both, any
        association order included; the indices are exact.  Likewise b and c.
    q = a / c + 0.5: e_q = (e_a + |a / c| e_c) / |c| + u |a / c| + u |q|.             delta_pix = C_POS e_q   (a few 1e-4 px at 640 px)
    sdf = d - c:     e_sdf = e_c + u |sdf|.                                          delta_sdf = C_POS e_sdf;  delta_c = C_POS e_c
    A voxel is ambiguous when, in any frame whose depth c > z_near - delta_c, with the projection within a pixel of the image:
    a / c + 0.5 or b / c + 0.5 lies within delta_pix of an integer (and some pixel of the 3 x 3 around the projection holds a valid depth
    not more than trunc + delta_sdf in front of the voxel: otherwise either pixel choice skips it); or, at the pixel it reads,
    |sdf + trunc| < delta_sdf; or
    |c - z_near| < delta_c; or the confidence lies within an ulp of conf_min.
    tsdf = min(1, sdf / trunc): error <= u (4 S_c + |sdf| + ...) / trunc: per contributing frame A_f = (S_c + d) / trunc + 1, and
    C_INTEGRATE = 5 (four for the dot product, one for the subtraction; the division's and the clamp's ulp of |tsdf| <= 1 is the "+ 1").
    blend D' = (D Wt + tsdf w) / (Wt + w): three roundings of values <= 1 and one of Wt + w (weighted mode): A' = (A Wt + A_f w) / (Wt + w) + 4.

``extract`` evaluates the zero-crossing contract in float64 on an fp32 volume; the crossing decision compares stored fp32 values and is
exact.  ``compare_points`` checks records against it within the interpolation bounds
    s = D0 / (D0 - D1): two roundings, |s| <= 1.      xyz_j = (idx_j + 0.5 + s) voxel + origin_j: C_EXTRACT u (|origin_j| + (idx_j + 1.5) voxel)
    weight = W0 + s (W1 - W0): C_EXTRACT u (|W0| + |W1|)
    g_j = g0_j + s (g1_j - g0_j): e_gj <= 5 u G_j, G_j = |g0_j| + |g1_j|;  n = g / |g|: C_EXTRACT u ((G_j + sum_k G_k) / |g| + 1); a normal whose
    |g| is within 16 u sum_k G_k of zero is not compared (cancellation: the fp32 blend may or may not vanish).
"""
import numpy as np

U = 2.0 ** -24
C_POS = 2.0                  # decision tolerance = C_POS * running rounding bound (as in sweep_fusion_ref.py)
C_INTEGRATE = 5.0            # route constant of the integrate bound, from the derivation above
C_EXTRACT = 8.0              # route constant of the extraction bounds
AMB_CAP = 0.03               # ambiguous voxels: at most this share of the updated voxels in every case
# test-only knob: plausible kernel mistakes (tests/test_tsdf_ref_cpu.py asserts that compare / compare_points reject each on some case)
MISTAKES = ("pixel_truncation", "wt_uncapped", "cap_before_blend", "cross_counted_twice", "normal_negated", "one_sided_gradient")
INTEGRATE_MISTAKES, EXTRACT_MISTAKES = MISTAKES[:3], MISTAKES[3:]


# ------------------------------------------------------------------------------------------------------------ analytic fixture
def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """camera-to-world pose [4,4] float64 of a camera at ``eye`` looking at ``target`` (x right, y down, z forward)"""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)            # y is DOWN: right = down x forward ... (-up) x z
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def intrinsics(H, W, fov_scale=0.9):
    f = fov_scale * W
    return np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])


def raycast_scene(pose, K, H, W, plane_z=2.6, centre=(0.1, 0.05, 2.0), radius=0.55):
    """depth map [H,W] float64 (z-depth along the optical axis) of the analytic scene: the plane z_world = plane_z and a sphere in front
    of it, ray-cast in float64 from the camera-to-world ``pose``; pixel centres on integers.  Rays that hit nothing get 0."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    Kinv = np.linalg.inv(K)
    rays_c = np.stack([u, v, np.ones_like(u)], -1) @ Kinv.T              # z component 1: t along the ray IS the z-depth
    R, o = pose[:3, :3], pose[:3, 3]
    rays = rays_c @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        t_plane = (plane_z - o[2]) / rays[..., 2]
    t_plane = np.where(np.isfinite(t_plane) & (t_plane > 0), t_plane, np.inf)
    oc = o - np.asarray(centre, dtype=np.float64)
    qa = (rays * rays).sum(-1)
    qb = 2.0 * (rays @ oc)
    qc = oc @ oc - radius * radius
    disc = qb * qb - 4 * qa * qc
    t_sph = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / (2 * qa), np.inf)
    t_sph = np.where(t_sph > 0, t_sph, np.inf)
    t = np.minimum(t_plane, t_sph)
    return np.where(np.isfinite(t), t, 0.0)


def scene_poses(T, seed=0):
    """T camera-to-world poses a few centimetres and degrees apart, looking at the scene from around the origin"""
    rng = np.random.RandomState(seed)
    poses = []
    for t in range(T):
        eye = np.array([0.06 * t - 0.03 * (T - 1), 0.02 * np.sin(1.3 * t), 0.03 * np.cos(0.7 * t) - 0.03]) + 0.01 * rng.randn(3)
        target = np.array([0.1 + 0.05 * np.sin(t), 0.05 * np.cos(2.0 * t), 2.2])
        poses.append(look_at(eye, target))
    return np.stack(poses)


def tsdf_matrices64(poses, K, origin, voxel_size):
    """A = K [R|t]_world->camera V in float64, rounded to fp32 [T,3,4] (what estdepth_amd.camera.tsdf_matrices hands the kernel)"""
    V = np.eye(4)
    V[:3, :3] *= voxel_size
    V[:3, 3] = np.asarray(origin, dtype=np.float64) + 0.5 * voxel_size
    out = []
    for P in np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4):
        out.append((np.asarray(K, dtype=np.float64).reshape(3, 3) @ np.linalg.inv(P)[:3, :4]) @ V)
    return np.stack(out).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ integrate
def _dot4(A_row, ix, iy, iz, f):
    """the kernel's a = fma(A0, ix, fma(A1, iy, fma(A2, iz, A3))) in dtype ``f`` (no fused operations in numpy: products round on their
    own in fp32) and S = the sum of the absolute terms (float64)"""
    t0, t1, t2 = A_row[0].astype(f) * ix.astype(f), A_row[1].astype(f) * iy.astype(f), A_row[2].astype(f) * iz.astype(f)
    val = t0 + (t1 + (t2 + A_row[3].astype(f)))
    S = (np.abs(np.float64(A_row[0]) * ix) + np.abs(np.float64(A_row[1]) * iy) + np.abs(np.float64(A_row[2]) * iz)
         + np.abs(np.float64(A_row[3])))
    return val, S


def integrate(D0, W0, mats, depths, confs=None, *, trunc, z_near=1e-3, conf_min=0.0, weighted=False, w_max=64.0, dtype=np.float64,
              z_block=16, voxel_range=None, mistake=None):
    """D0, W0 [Z,Y,X] float32 (the volume before the call); mats [T,3,4] float32; depths / confs [T,H,W] float32.
    ``dtype=np.float32`` evaluates the same contract in numpy fp32 arithmetic (the CPU stand-in for the kernel).
    ``voxel_range`` = ((z0, z1), (y0, y1), (x0, x1)): D0, W0 (and every result) are the brick [z0:z1, y0:y1, x0:x1] of a larger volume,
    evaluated at the voxel indices of that volume with the volume's own matrices (a cropped volume with a shifted origin would hand the
    kernel other fp32 matrices).  ``mistake``: one of INTEGRATE_MISTAKES, a deliberately wrong variant for the discrimination test.
    Returns dict(D, Wt (``dtype``), A (float64, units of 2^-24), updated, amb (bool), n_updates (int))."""
    assert mistake is None or mistake in INTEGRATE_MISTAKES, mistake
    f = dtype
    D0, W0 = np.asarray(D0, dtype=np.float32), np.asarray(W0, dtype=np.float32)
    mats = np.asarray(mats, dtype=np.float32).reshape(-1, 3, 4)
    depths = np.asarray(depths, dtype=np.float32)
    T, H, W = depths.shape
    assert mats.shape[0] == T
    Z, Y, X = D0.shape
    (z0, z1), (y0, y1), (x0, x1) = voxel_range if voxel_range is not None else ((0, Z), (0, Y), (0, X))
    assert (z1 - z0, y1 - y0, x1 - x0) == (Z, Y, X), "D0 / W0 must have the shape of voxel_range"
    trunc32, znear32, cmin32, wmax32 = (np.float32(v) for v in (trunc, z_near, conf_min, w_max))
    # the farthest valid depth in the 3 x 3 pixels around each pixel (-inf where none is valid)
    dvalid = np.where(np.isfinite(depths) & (depths > 0), depths.astype(np.float64), -np.inf)
    pad = np.pad(dvalid, ((0, 0), (1, 1), (1, 1)), constant_values=-np.inf)
    dmax3 = np.max([pad[:, i:i + H, j:j + W] for i in range(3) for j in range(3)], axis=0)
    out = {"D": np.empty((Z, Y, X), dtype=f), "Wt": np.empty((Z, Y, X), dtype=f), "A": np.zeros((Z, Y, X)),
           "updated": np.zeros((Z, Y, X), dtype=bool), "amb": np.zeros((Z, Y, X), dtype=bool), "n_updates": np.zeros((Z, Y, X), dtype=np.int32)}
    for zb in range(0, Z, z_block):
        sl = slice(zb, min(Z, zb + z_block))
        iz, iy, ix = np.meshgrid(np.arange(z0 + sl.start, z0 + sl.stop, dtype=np.float64), np.arange(y0, y1, dtype=np.float64),
                                 np.arange(x0, x1, dtype=np.float64), indexing="ij")
        D, Wt = D0[sl].astype(f), W0[sl].astype(f)
        A = np.zeros(D.shape)
        upd = np.zeros(D.shape, dtype=bool)
        amb = np.zeros(D.shape, dtype=bool)
        nup = np.zeros(D.shape, dtype=np.int32)
        for t in range(T):
            a, Sa = _dot4(mats[t, 0], ix, iy, iz, f)
            b, Sb = _dot4(mats[t, 1], ix, iy, iz, f)
            c, Sc = _dot4(mats[t, 2], ix, iy, iz, f)
            ea, eb, ec = 4 * U * Sa, 4 * U * Sb, 4 * U * Sc
            front = c > f(znear32)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                qa, qb = a / c, b / c
                qu, qv = qa + f(0.5), qb + f(0.5)
                c64 = np.abs(c.astype(np.float64))
                e_qu = (ea + np.abs(qa.astype(np.float64)) * ec) / c64 + U * np.abs(qa.astype(np.float64)) + U * np.abs(qu.astype(np.float64))
                e_qv = (eb + np.abs(qb.astype(np.float64)) * ec) / c64 + U * np.abs(qb.astype(np.float64)) + U * np.abs(qv.astype(np.float64))
                fu, fv = np.floor(qu), np.floor(qv)
                if mistake == "pixel_truncation":                      # (int)(a / c): the pixel by truncation, not floor(x + 0.5)
                    fu, fv = np.trunc(qa), np.trunc(qb)
            inimg = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            # ---- ambiguity of the discontinuous decisions
            d_c = C_POS * ec
            maybe_front = c.astype(np.float64) > float(znear32) - d_c
            with np.errstate(invalid="ignore"):
                near_img = maybe_front & (qu >= -1) & (qu <= W + 1) & (qv >= -1) & (qv <= H + 1)
                fr_u = np.abs(qu.astype(np.float64) - np.round(qu.astype(np.float64)))
                fr_v = np.abs(qv.astype(np.float64) - np.round(qv.astype(np.float64)))
                # ... which matters only where one of the pixels around the projection can update the voxel at all (behind every
                # surface of the 3 x 3 neighbourhood by more than trunc, either pixel choice skips it)
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
            Dn = (D * Wt + tsdf * w) / (np.minimum(den, f(wmax32)) if mistake == "cap_before_blend" else den)
            A_f = (Sc + d.astype(np.float64)) / float(trunc32) + 1.0
            An = (A * Wt.astype(np.float64) + A_f * w.astype(np.float64)) / den.astype(np.float64) + 4.0
            D = np.where(ok, Dn, D)
            A = np.where(ok, An, A)
            Wt = np.where(ok, den if mistake == "wt_uncapped" else np.minimum(den, f(wmax32)), Wt)
            upd |= ok
            nup += ok
        out["D"][sl], out["Wt"][sl], out["A"][sl], out["updated"][sl], out["amb"][sl], out["n_updates"][sl] = D, Wt, A, upd, amb, nup
    return out


def compare(got_D, got_W, ref, weighted=False, D_before=None, W_before=None):
    """THE comparison of the suite.  got_* [Z,Y,X] fp32 arrays; ``ref`` from integrate(dtype=float64).  Returns a dict of figures after
    asserting: the ambiguous share <= AMB_CAP of the updated voxels; on every other voxel Wt exact (weighted: within its bound) and
    |D - D_ref| <= C_INTEGRATE 2^-24 A; with ``*_before``: voxels the reference leaves alone keep their bits."""
    got_D, got_W = np.asarray(got_D), np.asarray(got_W)
    amb, upd = ref["amb"], ref["updated"]
    n_upd, n_amb = int(upd.sum()), int((amb & upd).sum() + (amb & ~upd).sum())
    fig = {"updated": n_upd, "ambiguous": n_amb, "amb_share": n_amb / max(n_upd, 1)}
    if n_upd:
        assert n_amb <= AMB_CAP * n_upd, "ambiguous share %.4f of %d updated voxels exceeds %.2f" % (fig["amb_share"], n_upd, AMB_CAP)
    keep = ~amb
    if weighted:
        tol_w = C_INTEGRATE * U * np.maximum(ref["n_updates"], 1) * np.abs(ref["Wt"])
        bad_w = keep & ~(np.abs(got_W.astype(np.float64) - ref["Wt"]) <= tol_w)
    else:
        bad_w = keep & (got_W.astype(np.float64) != ref["Wt"].astype(np.float64))
    assert not bad_w.any(), "%d voxels with a wrong weight, first at %s" % (int(bad_w.sum()), np.argwhere(bad_w)[0])
    err = np.abs(got_D.astype(np.float64) - ref["D"].astype(np.float64))
    sel = keep & upd
    ratio = np.where(sel, err / (U * np.maximum(ref["A"], 1e-30)), 0.0)
    fig["max_ratio"] = float(ratio.max()) if sel.any() else 0.0
    fig["max_abs"] = float(err[sel].max()) if sel.any() else 0.0
    print("tsdf compare: updated %d ambiguous %d (%.4f) max |dD| %.3g max ratio %.3f (bound %.1f)"
          % (n_upd, n_amb, fig["amb_share"], fig["max_abs"], fig["max_ratio"], C_INTEGRATE))
    assert fig["max_ratio"] <= C_INTEGRATE, "max |D - D_ref| / (2^-24 A) = %.3f > %.1f" % (fig["max_ratio"], C_INTEGRATE)
    still = keep & ~upd
    if D_before is not None:
        assert np.array_equal(got_D.view(np.uint32)[still], np.asarray(D_before).view(np.uint32)[still]), "an untouched voxel's D changed"
        assert np.array_equal(got_W.view(np.uint32)[still], np.asarray(W_before).view(np.uint32)[still]), "an untouched voxel's Wt changed"
    else:
        assert not (keep & ~upd & (err != 0)).any(), "a voxel the reference leaves alone changed"
    return fig


# ------------------------------------------------------------------------------------------------------------ extraction
def _gradient(D, obs, mistake=None):
    """per-axis (x, y, z) gradient of D [Z,Y,X] float64 with the contract's central / one-sided / zero choice -> [3][Z,Y,X]"""
    g = []
    for axis in (2, 1, 0):                       # x, y, z
        Dm = np.moveaxis(D, axis, 0)
        om = np.moveaxis(obs, axis, 0)
        lo = np.zeros_like(om)
        hi = np.zeros_like(om)
        lo[1:] = om[:-1]
        hi[:-1] = om[1:]
        dl, dh = Dm.copy(), Dm.copy()
        dl[1:] = np.where(lo[1:], Dm[:-1], Dm[1:])
        dh[:-1] = np.where(hi[:-1], Dm[1:], Dm[:-1])
        gk = np.where(lo & hi, 0.5 * (dh - dl), dh - dl)
        if mistake == "one_sided_gradient":          # D[q + 1] - D[q] wherever the upper neighbour is observed, the central difference never
            gk = np.where(hi, dh - Dm, dh - dl)
        g.append(np.moveaxis(gk, 0, axis))
    return g


def extract(D32, W32, w_min, voxel_size, origin, mistake=None, voxel_range=None, dims=None):
    """D32, W32 [Z,Y,X] float32.  Returns dict sorted by edge id: edge (int64), xyz, normal [N,3], weight [N] (float64) and the bound
    magnitudes tol_xyz, tol_normal [N,3], tol_weight [N] (absolute), skip_normal [N] (bool).  ``mistake``: one of EXTRACT_MISTAKES.
    ``voxel_range`` = ((z0, z1), (y0, y1), (x0, x1)) with ``dims`` = the (Z, Y, X) of the whole volume: D32, W32 are that brick of the
    volume; edge ids, positions and their bounds are the whole volume's.  The brick's outer voxel layers see no neighbour beyond the
    brick: records within two voxels of a face of the brick that is no face of the volume are the caller's to discard."""
    assert mistake is None or mistake in EXTRACT_MISTAKES, mistake
    D32, W32 = np.asarray(D32, dtype=np.float32), np.asarray(W32, dtype=np.float32)
    Z, Y, X = D32.shape
    vs, org = float(np.float32(voxel_size)), np.asarray(origin, dtype=np.float32).astype(np.float64)
    D, Wt = D32.astype(np.float64), W32.astype(np.float64)
    obs = W32 >= np.float32(w_min)
    g = _gradient(D, obs, mistake)
    if voxel_range is None:
        off, lin = np.zeros(3), np.arange(Z * Y * X, dtype=np.int64).reshape(Z, Y, X)
    else:
        (z0, z1), (y0, y1), (x0, x1) = voxel_range
        assert (z1 - z0, y1 - y0, x1 - x0) == (Z, Y, X), "D32 / W32 must have the shape of voxel_range"
        off = np.array([x0, y0, z0], dtype=np.float64)
        gz, gy, gx = np.meshgrid(np.arange(z0, z1, dtype=np.int64), np.arange(y0, y1, dtype=np.int64), np.arange(x0, x1, dtype=np.int64), indexing="ij")
        lin = (gz * dims[1] + gy) * dims[2] + gx
    recs = {k: [] for k in ("edge", "xyz", "normal", "weight", "tol_xyz", "tol_normal", "tol_weight", "skip_normal")}
    for k, axis in enumerate((2, 1, 0)):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        d0, d1 = D[a], D[b]
        cr = obs[a] & obs[b] & (((d0 < 0) & (0 <= d1)) | ((d1 < 0) & (0 <= d0)))
        if mistake == "cross_counted_twice":         # d0 <= 0 <= d1: a voxel at exactly 0 closes one edge and opens the next
            cr = obs[a] & obs[b] & (((d0 <= 0) & (0 <= d1)) | ((d1 <= 0) & (0 <= d0))) & ((d0 != 0) | (d1 != 0))
        sel = np.nonzero(cr)
        d0, d1 = d0[sel], d1[sel]
        s = d0 / (d0 - d1)
        idx3 = np.stack([sel[2], sel[1], sel[0]], -1).astype(np.float64) + off    # (x, y, z) of the edge's first voxel
        cell = idx3 + 0.5
        cell[:, k] += s
        g0 = np.stack([gj[a][sel] for gj in g], -1)
        g1 = np.stack([gj[b][sel] for gj in g], -1)
        gg = g0 + s[:, None] * (g1 - g0)
        G = np.abs(g0) + np.abs(g1)
        length = np.sqrt((gg * gg).sum(-1))
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.where(length[:, None] > 0, gg / length[:, None], 0.0)
            if mistake == "normal_negated":
                n = -n
            tol_n = C_EXTRACT * U * ((G + G.sum(-1, keepdims=True)) / length[:, None] + 1.0)
        skip = (length <= 16 * U * G.sum(-1)) & (G.sum(-1) > 0)
        w0, w1 = Wt[a][sel], Wt[b][sel]
        recs["edge"].append(3 * lin[a][sel] + k)
        recs["xyz"].append(cell * vs + org)
        recs["normal"].append(n)
        recs["weight"].append(w0 + s * (w1 - w0))
        recs["tol_xyz"].append(C_EXTRACT * U * (np.abs(org) + (idx3 + 1.5) * vs))
        recs["tol_normal"].append(np.where(np.isfinite(tol_n), tol_n, 0.0))
        recs["tol_weight"].append(C_EXTRACT * U * (np.abs(w0) + np.abs(w1)))
        recs["skip_normal"].append(skip)
    out = {k: np.concatenate(v) for k, v in recs.items()}
    order = np.argsort(out["edge"], kind="stable")
    return {k: v[order] for k, v in out.items()}


def compare_points(got, ref):
    """``got``: dict(edge, xyz, normal, weight) numpy arrays of records whose edge ids all occur in ``ref`` (a subset when the capacity was
    too small).  Each record is compared with the reference record of the same edge id."""
    order = np.argsort(got["edge"], kind="stable")
    edge = got["edge"][order]
    assert len(np.unique(edge)) == len(edge), "an edge was emitted twice"
    pos = np.searchsorted(ref["edge"], edge)
    assert (pos < len(ref["edge"])).all() and np.array_equal(ref["edge"][np.minimum(pos, len(ref["edge"]) - 1)], edge), \
        "a record's edge id is not a crossing of the reference"
    fig = {}
    for name in ("xyz", "weight", "normal"):
        g, r, tol = got[name][order].astype(np.float64), ref[name][pos], ref["tol_" + name][pos]
        err = np.abs(g - r)
        if name == "normal":
            keep = ~ref["skip_normal"][pos]
            err, tol = err[keep], tol[keep]
        ratio = err / np.maximum(tol, 1e-300)
        fig[name] = float(ratio.max()) * C_EXTRACT if ratio.size else 0.0
        assert (err <= tol).all(), "%s: worst error %.3g at %.3f of its bound" % (name, err.max(), ratio.max())
    print("tsdf compare_points: %d records, worst ratio in units of 2^-24 magnitude: %s (bound %.1f)" % (len(edge), fig, C_EXTRACT))
    return fig


# ------------------------------------------------------------------------------------------------------------ the cases of the suite
# name: (T, (H, W), dims (Z, Y, X), origin, mode, extras).  3 cm voxels, trunc = 4 voxels.  The CPU suite checks the ambiguous share of
# every one of them; the GPU suite runs them.
VOXEL = 0.03
CASES = {
    "t1": dict(T=1, hw=(120, 160), dims=(96, 128, 128), origin=(-1.92, -1.92, 0.2)),
    "t3": dict(T=3, hw=(120, 160), dims=(96, 128, 128), origin=(-1.92, -1.92, 0.2)),
    "t8": dict(T=8, hw=(120, 160), dims=(96, 128, 128), origin=(-1.92, -1.92, 0.2)),
    "gated": dict(T=3, hw=(120, 160), dims=(96, 128, 128), origin=(-1.92, -1.92, 0.2), conf=True, conf_min=0.4),
    "weighted": dict(T=3, hw=(120, 160), dims=(96, 128, 128), origin=(-1.92, -1.92, 0.2), conf=True, conf_min=0.2, weighted=True),
    "second": dict(T=3, hw=(120, 160), dims=(96, 128, 128), origin=(-1.92, -1.92, 0.2), w_max=4.0, calls=2),
    "inside": dict(T=3, hw=(120, 160), dims=(96, 128, 128), origin=(-1.92, -1.92, -0.9)),
    "away": dict(T=3, hw=(120, 160), dims=(32, 64, 64), origin=(-0.96, -0.96, 0.5), away=True),
    "holes": dict(T=3, hw=(120, 160), dims=(96, 128, 128), origin=(-1.92, -1.92, 0.2), holes=True),
    "odd": dict(T=3, hw=(119, 157), dims=(96, 100, 132), origin=(-1.98, -1.5, 0.2)),
    "full": dict(T=3, hw=(480, 640), dims=(256, 256, 256), origin=(-3.84, -3.84, -0.5)),
}


# Small cases for a route suite of the integration: volumes at the edges of the integrate kernel's 64 x 16 x ZCHUNK (8) bricks -- one 16-byte
# group, one voxel short of a brick in every dimension, one voxel past it, exactly one brick -- under 1 and 8 frames and maps of 1 x 1,
# 3 x 5 and 120 x 160 pixels, placed where the sphere's near side runs through them.  A table of its own: the suites over CASES ask for
# more than a thousand updated voxels per case.  tests/test_tsdf_ref_cpu.py checks the ambiguous share of every one of them.
ROUTE_DIMS = {(1, 1, 4): (0.04, 0.035, 1.43), (7, 15, 60): (-0.8, -0.17, 1.36), (9, 17, 68): (-0.92, -0.2, 1.33), (8, 16, 64): (-0.86, -0.19, 1.35)}
ROUTE_CASES = {"r%dx%dx%d-t%d-%dx%d" % (dims + (T,) + hw): dict(T=T, hw=hw, dims=dims, origin=org)
               for dims, org in ROUTE_DIMS.items() for T in (1, 8) for hw in ((1, 1), (3, 5), (120, 160))}


PLACED_CASE = "t1"            # the case that is also built at placement.FAMILY_PLACES: the smallest volume and map the feature suite uses


def placed_origin(origin, place):
    """the volume's corner moved with the scene (placement.py; unturned placements only: a volume's axes are the world's) -> three floats
    that are fp32 values, so that the volume (which keeps its origin in fp32) and the host's float64 matrices start from the same corner"""
    import placement as PL
    if PL.key(place) is None:
        return tuple(origin)
    assert not place[1], "a volume cannot follow a turned world"
    return tuple(float(v) for v in (np.asarray(origin, np.float64) + PL.offset(place[0])).astype(np.float32))


def build_case(name, place=None):
    """dict(dims, origin, voxel, trunc, poses [T,4,4] f64, K [3,3] f64, depths [T,H,W] f32, confs or None, params for integrate()).
    ``place`` (placement.py): the cameras and the volume's origin moved with the scene; the depth maps do not change"""
    import placement as PL
    c = dict(CASES[name] if name in CASES else ROUTE_CASES[name])
    if PL.key(place) is not None:
        base = build_case(name)
        return dict(base, name="%s@%s" % (name, PL.label(place)), origin=placed_origin(base["origin"], place), poses=PL.pose(base["poses"], place))
    T, (H, W) = c["T"], c["hw"]
    K = intrinsics(H, W)
    poses = scene_poses(T, seed=len(name))
    if c.get("away"):
        flip = np.diag([-1.0, 1.0, -1.0, 1.0])                    # half a turn about y: the cameras look away from the volume
        poses = np.stack([P @ flip for P in poses])
        depths = np.full((T, H, W), 2.0, dtype=np.float32)
    else:
        depths = np.stack([raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)
    rng = np.random.RandomState(7 + T)
    if c.get("holes"):
        depths[:, 10:30, 20:60] = 0.0
        depths[:, 50:70, 80:120] = np.nan
        depths[:, 90:110, 30:70] = np.inf
        depths[:, 40:45, 5:15] = -1.0
    confs = rng.uniform(0.0, 1.0, size=depths.shape).astype(np.float32) if c.get("conf") else None
    params = dict(trunc=4 * VOXEL, z_near=1e-3, conf_min=c.get("conf_min", 0.0), weighted=c.get("weighted", False), w_max=c.get("w_max", 64.0))
    return dict(name=name, dims=c["dims"], origin=c["origin"], voxel=VOXEL, poses=poses, K=K, depths=depths, confs=confs, params=params,
                calls=c.get("calls", 1))
