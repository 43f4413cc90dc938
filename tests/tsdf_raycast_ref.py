"""float64 reference of the ray-casting contract of the library (csrc/tsdf_raycast.hip, include/estd_hip.h: estd_tsdf_raycast), in the style of
tests/tsdf_ref.py.  A plain helper module of the test suite (not a conftest); numpy only.

``raycast`` evaluates the contract in float64 FROM THE fp32 MATRIX, VOLUME AND CONSTANTS THE KERNEL RECEIVES and returns, per pixel, the expected
depth / normal / weight, first-order rounding bounds of each, the ``hit`` mask and the pixels that are ``amb``iguous: a discontinuous decision lies
within the fp32 rounding of the kernel's evaluation at some sample up to and including the hit, so either outcome is right and the pixel is
left out of the value comparison.  ``dtype=np.float32`` evaluates the same contract in numpy fp32 arithmetic (the CPU stand-in for the kernel;
numpy has no fused multiply-add, so every product rounds on its own).  ``compare`` is THE comparison of the suite (GPU results and the stand-in
alike): ambiguous pixels <= AMB_CAP of the hit pixels; on all others hit / no-hit agrees exactly, no-hit pixels are exactly zero and
    |depth - ref| <= C_RAY e_depth        |normal_j - ref| <= C_RAY e_n_j  (unless |g| cancels)        |weight - ref| <= C_RAY e_w.

Rounding bounds (first order, u = 2^-24; a fused multiply-add rounds once, the unfused stand-in twice: the counts below are the unfused ones)
    r_j = M_j0 u + M_j1 v + M_j2: S_j = |M_j0 u| + |M_j1 v| + |M_j2|; e_r_j = 4 u S_j (as tsdf_ref's dot products: any association order).
    t = k dt + t_min (k exact, all terms >= 0): e_t = 2 u t.
    p_j = t r_j + o_j: t e_r_j + |r_j| e_t + u |t r_j| (product) + u (|o_j| + |t r_j|) (sum):       e_p_j = u (4 t S_j + 4 |t r_j| + |o_j|).
        The cell index floor(p_j) and the fraction f_j = p_j - floor(p_j) are exact functions of the computed p_j: e_f_j = e_p_j.
    lerp(a, b, f) = f (b - a) + a on values of magnitude <= m: u |b - a| <= 2 u m for the difference, 2 u m for the product, u m for the sum:
        5 u m per level (3 u m fused); a level passes the errors of its operands on with weights (1 - f) + f = 1.  Three levels: 15 u m,
        rounded up to 16.  The trilinear interpolant is linear in each f_j with slope G_j:
            e_F  = 16 u max|corner| + sum_j |G_j| e_p_j.
        G_j is itself such a blend of corner differences (magnitude <= 2 max|corner|, at most three levels and one more difference: 24 u
        max|corner|) and moves with the OTHER fractions by mixed second differences, each at most 2 (max corner - min corner):
            e_G_j = 24 u max|corner| + 2 (max corner - min corner) sum_{i != j} e_p_i.
        Wb = the blend of the weights:  e_Wb = 16 u max w + (max w - min w) sum_j e_p_j.
    s = F0 / (F0 - F1), 0 < s <= 1: e_s = (|F0| e_F1 + |F1| e_F0) / (F0 - F1)^2 + 2 u (difference and quotient).
    depth = dt s + t0:        e_depth = dt e_s + 2 u |depth|    (fused: u t0 of t0 and u |depth| of the sum; the unfused count is twice that).
    weight = s (Wb1 - Wb0) + Wb0:  e_w = |Wb1 - Wb0| e_s + e_Wb0 + e_Wb1 + 3 u (|Wb0| + |Wb1|).
    g_j = s (G1_j - G0_j) + G0_j:  e_g_j = |G1_j - G0_j| e_s + e_G0_j + e_G1_j + 3 u (|G0_j| + |G1_j|).
    n = g / |g|: e_n_j = (e_g_j + sum_k e_g_k) / |g| + 4 u (three roundings of |g|^2, the root, the quotient); a normal whose |g| is within
        16 sum_k e_g_k of zero is not compared (cancellation: the fp32 blend may or may not vanish).
    C_RAY = 4: 2 for the unfused count where a bound above states the fused one (e_depth) and 2 for what first order leaves out (the bounds
    are evaluated at the reference's own F, G and s; products of two errors).  C_POS = 2 as in tsdf_ref.py.
Ambiguity, at every sample of a pixel up to and including its hit:
    |F| < C_POS e_F at an observed sample (the sign tests F_{k-1} > 0 >= F_k);
    p_j within C_POS e_p_j of an integer while the cells on the two sides of that face differ in observedness (two such axes at once: always);
    the same at either sample of the hit pair whatever the observedness (the gradient of a trilinear interpolant jumps across cell faces).
The reference skips samples outside the volume by a slab test of its own (widened by 1e-3 voxel and two samples: exact).
"""
import numpy as np

import tsdf_ref as R

U = 2.0 ** -24
C_POS = 2.0                  # decision tolerance = C_POS * rounding bound
C_RAY = 4.0                  # route constant of the depth / normal / weight bounds, from the derivation above
AMB_CAP = R.AMB_CAP          # ambiguous pixels: at most this share of the hit pixels in every case
# test-only knob: plausible kernel mistakes (tests/test_tsdf_raycast_ref_cpu.py asserts that compare rejects each on some case)
MISTAKES = ("back_face", "prev_unobserved", "corner_gt")

# the inputs of the suite: a pose that was never fused, rays sampled from 0.3 m to 3.6 m in steps of one voxel
HELD_OUT_POSE = R.look_at((0.12, -0.08, -0.05), (0.1, 0.0, 2.2))
T_MIN, T_MAX = 0.3, 3.6
N_STEPS = int(round((T_MAX - T_MIN) / R.VOXEL)) + 1
# (case of tsdf_ref.CASES, w_min): volumes whose observed region is ragged voxel by voxel ("gated", "weighted" above 0.25) sit at or beyond
# the ambiguity cap and are not compared; "t1", "gated", "weighted" have no voxel of weight 3
VALUE_CASES = [("t1", 1.0)] + [(n, w) for n in ("t3", "t8", "second", "inside", "holes", "odd") for w in (1.0, 3.0)] + [("weighted", 0.25)]
FULL_CASE = ("full", 1.0)
# image sizes (H, W) of the route suite's renders of the 9 x 17 x 68 slab of tsdf_ref.ROUTE_CASES (tests/test_gpu_recon3d_routes.py builds
# the views): 1, 2, 1 and 6 tiles of 16 x 16 pixels (the map edges), then 7, 8, 9 and 17 tiles -- fewer workgroups than the eight XCDs
# the kernel spreads them over, as many, one more, two rounds and one.  tests/test_tsdf_raycast_ref_cpu.py checks the ambiguous share of
# every one (a 40 x 40 render of nine tiles sits above the cap and was replaced by 33 x 40).
ROUTE_SIZES = [(1, 1), (15, 17), (16, 16), (17, 33), (15, 100), (20, 60), (33, 40), (10, 270)]


def ray_matrix(pose, K, origin, voxel):
    """M = [R K^-1 / voxel | (c - origin) / voxel - 0.5] in float64, rounded to fp32 [3,4] (what estdepth_amd.camera.tsdf_ray_matrix hands
    the kernel)"""
    pose, K = np.asarray(pose, np.float64).reshape(4, 4), np.asarray(K, np.float64).reshape(3, 3)
    A = (pose[:3, :3] @ np.linalg.inv(K)) / voxel
    o = (pose[:3, 3] - np.asarray(origin, np.float64)) / voxel - 0.5
    return np.concatenate([A, o[:, None]], 1).astype(np.float32)


def cell_observed(Wt, w_min, mistake=None):
    """[Z-1,Y-1,X-1] bool: all eight corner weights of the cell >= w_min (compared as stored fp32 values: exact)"""
    ok = np.asarray(Wt, np.float32) >= np.float32(w_min)
    if mistake == "corner_gt":                       # w > w_min: a corner of exactly w_min counts as unobserved
        ok = np.asarray(Wt, np.float32) > np.float32(w_min)
    return (ok[:-1, :-1, :-1] & ok[:-1, :-1, 1:] & ok[:-1, 1:, :-1] & ok[:-1, 1:, 1:]
            & ok[1:, :-1, :-1] & ok[1:, :-1, 1:] & ok[1:, 1:, :-1] & ok[1:, 1:, 1:])


def _lookup(cobs, ix, iy, iz):
    """observedness of the cells (ix, iy, iz) (integer arrays); cells outside the volume are unobserved"""
    nz, ny, nx = cobs.shape
    inr = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny) & (iz >= 0) & (iz < nz)
    out = np.zeros(ix.shape, dtype=bool)
    out[inr] = cobs[iz[inr], iy[inr], ix[inr]]
    return out


def _k_interval(r, o, dims, t_min, dt, n_steps, first=(0.0, 0.0, 0.0)):
    """per ray the sample indices [klo, khi] that can lie inside the volume (float64 slab test on the box widened by 1e-3 voxel and a
    relative margin, the interval by two samples); klo > khi: none"""
    n = r.shape[0]
    klo, khi = np.zeros(n), np.full(n, float(n_steps - 1))
    for j in range(3):
        eps = 1e-3 + 1e-5 * (abs(o[j]) + dims[j])
        lo, hi = first[j] - eps, first[j] + dims[j] - 1 + eps
        rj = r[:, j]
        zero = rj == 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t0, t1 = (lo - o[j]) / rj, (hi - o[j]) / rj
        ta, tb = np.minimum(t0, t1), np.maximum(t0, t1)
        inside = lo <= o[j] <= hi
        ta = np.where(zero, -np.inf if inside else np.inf, ta)
        tb = np.where(zero, np.inf if inside else -np.inf, tb)
        with np.errstate(invalid="ignore"):
            k0 = np.floor((ta - t_min) / dt * (1 - 1e-9) - 2)
            k1 = np.ceil((tb - t_min) / dt * (1 + 1e-9) + 2)
        klo = np.maximum(klo, np.nan_to_num(k0, nan=0.0, posinf=np.inf, neginf=-np.inf))
        khi = np.minimum(khi, np.nan_to_num(k1, nan=float(n_steps - 1), posinf=np.inf, neginf=-np.inf))
    return klo, khi


def _lerp(a, b, t):
    return a + t * (b - a)


def raycast(D, Wt, M, H, W, t_min, dt, n_steps, w_min, dtype=np.float64, rows=16, mistake=None, index_offset=None):
    """D, Wt [Z,Y,X] float32; M [3,4] float32; t_min, dt, w_min as the kernel receives them (rounded to fp32 here).  Returns a dict of [H,W]
    arrays: depth, weight, normal [H,W,3] (``dtype``), hit, amb, skip_normal (bool), tol_depth, tol_weight, tol_normal [H,W,3] (float64,
    absolute, to be scaled by C_RAY) and samples (int: samples evaluated up to the hit).  ``mistake``: one of MISTAKES, a deliberately
    wrong variant for the discrimination test.  ``index_offset`` = (x0, y0, z0): D, Wt are the brick of a larger volume that starts at
    that voxel, and M is the larger volume's matrix (positions stay in its voxel coordinates, so the fp32 arithmetic is the kernel's);
    everything outside the brick counts as unobserved, which is the larger volume's truth when its weights are zero there."""
    assert mistake is None or mistake in MISTAKES, mistake
    f = dtype
    off = np.zeros(3, np.int64) if index_offset is None else np.asarray(index_offset, np.int64)
    D, Wt = np.asarray(D, dtype=np.float32), np.asarray(Wt, dtype=np.float32)
    Z, Y, X = D.shape
    dims = np.array([X, Y, Z], dtype=np.float64)
    M32 = np.asarray(M, dtype=np.float32).reshape(3, 4)
    Mf, M64 = M32.astype(f), M32.astype(np.float64)
    tmin32, dt32 = np.float32(t_min), np.float32(dt)
    tmin64, dt64 = float(tmin32), float(dt32)
    cobs = cell_observed(Wt, w_min, mistake)
    o, o64 = Mf[:, 3], M64[:, 3]
    out = {"depth": np.zeros((H, W), f), "weight": np.zeros((H, W), f), "normal": np.zeros((H, W, 3), f), "hit": np.zeros((H, W), bool),
           "amb": np.zeros((H, W), bool), "skip_normal": np.zeros((H, W), bool), "tol_depth": np.zeros((H, W)), "tol_weight": np.zeros((H, W)),
           "tol_normal": np.zeros((H, W, 3)), "samples": np.zeros((H, W), np.int64)}
    for v0 in range(0, H, rows):
        v1 = min(H, v0 + rows)
        vv, uu = np.meshgrid(np.arange(v0, v1), np.arange(W), indexing="ij")
        vv, uu = vv.ravel(), uu.ravel()
        n = uu.size
        uf, vf = uu.astype(f), vv.astype(f)
        r = np.stack([Mf[j, 0] * uf + (Mf[j, 1] * vf + Mf[j, 2]) for j in range(3)], 1)                       # [n,3] in f
        r64 = r.astype(np.float64)
        S = np.stack([np.abs(M64[j, 0] * uu) + np.abs(M64[j, 1] * vv) + np.abs(M64[j, 2]) for j in range(3)], 1)
        klo, khi = _k_interval(r64, o64, dims, tmin64, dt64, n_steps, off.astype(np.float64))
        done = ~(klo <= khi)
        amb = np.zeros(n, bool)
        hit_b = np.zeros(n, bool)
        depth, weight, normal = np.zeros(n, f), np.zeros(n, f), np.zeros((n, 3), f)
        tol_d, tol_w, tol_n, skip_n = np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros(n, bool)
        samples = np.zeros(n, np.int64)
        # the previous sample of every ray of the block
        P = {"obs": np.zeros(n, bool), "F": np.zeros(n, f), "Wb": np.zeros(n, f), "G": np.zeros((n, 3), f), "eF": np.zeros(n),
             "eWb": np.zeros(n), "eG": np.zeros((n, 3)), "near": np.zeros(n, bool)}
        if done.all():
            k_first, k_last = 0, -1
        else:
            k_first, k_last = int(klo[~done].min()), int(khi[~done].max())
        for k in range(k_first, k_last + 1):
            idx = np.nonzero(~done & (klo <= k))[0]
            if idx.size == 0:
                if done.all():
                    break
                continue
            m = idx.size
            t = f(f(tmin32) + f(k) * f(dt32))
            t64 = float(t)
            t_prev = f(f(tmin32) + f(k - 1) * f(dt32))
            p = (o[None] + t * r[idx]).astype(f)
            p64 = p.astype(np.float64)
            fl = np.floor(p)
            ii = fl.astype(np.int64) - off[None]
            obs = _lookup(cobs, ii[:, 0], ii[:, 1], ii[:, 2])
            e_p = U * (4 * t64 * S[idx] + 4 * np.abs(t64 * r64[idx]) + np.abs(o64)[None])
            rnd = np.round(p64)
            near = np.abs(p64 - rnd) < C_POS * e_p                                                            # [m,3]
            near_any = near.any(1)
            amb_face = near.sum(1) >= 2
            for j in range(3):
                sel = np.nonzero(near[:, j])[0]
                if sel.size:
                    a, b = ii[sel].copy(), ii[sel].copy()
                    a[:, j] = rnd[sel, j].astype(np.int64) - off[j] - 1
                    b[:, j] = rnd[sel, j].astype(np.int64) - off[j]
                    amb_face[sel] |= _lookup(cobs, a[:, 0], a[:, 1], a[:, 2]) != _lookup(cobs, b[:, 0], b[:, 1], b[:, 2])
            F, Wb, G = np.zeros(m, f), np.zeros(m, f), np.zeros((m, 3), f)
            eF, eWb, eG = np.zeros(m), np.zeros(m), np.zeros((m, 3))
            sub = np.nonzero(obs)[0]
            if mistake == "prev_unobserved":         # F is interpolated in every cell of the volume, observed or not
                sub = np.nonzero(((ii >= 0) & (ii <= np.array([X - 2, Y - 2, Z - 2])[None])).all(1))[0]
            if sub.size:
                ix, iy, iz = ii[sub, 0], ii[sub, 1], ii[sub, 2]
                fx, fy, fz = ((p[sub] - fl[sub]).astype(f)).T
                c, w = {}, {}
                for dz in (0, 1):
                    for dy in (0, 1):
                        for dx in (0, 1):
                            c[dx, dy, dz] = D[iz + dz, iy + dy, ix + dx].astype(f)
                            w[dx, dy, dz] = Wt[iz + dz, iy + dy, ix + dx].astype(f)
                c00, c10 = _lerp(c[0, 0, 0], c[1, 0, 0], fx), _lerp(c[0, 1, 0], c[1, 1, 0], fx)
                c01, c11 = _lerp(c[0, 0, 1], c[1, 0, 1], fx), _lerp(c[0, 1, 1], c[1, 1, 1], fx)
                c0, c1 = _lerp(c00, c10, fy), _lerp(c01, c11, fy)
                Fs = _lerp(c0, c1, fz)
                gx = _lerp(_lerp(c[1, 0, 0] - c[0, 0, 0], c[1, 1, 0] - c[0, 1, 0], fy), _lerp(c[1, 0, 1] - c[0, 0, 1], c[1, 1, 1] - c[0, 1, 1], fy), fz)
                gy = _lerp(c10 - c00, c11 - c01, fz)
                gz = c1 - c0
                Wbs = _lerp(_lerp(_lerp(w[0, 0, 0], w[1, 0, 0], fx), _lerp(w[0, 1, 0], w[1, 1, 0], fx), fy),
                            _lerp(_lerp(w[0, 0, 1], w[1, 0, 1], fx), _lerp(w[0, 1, 1], w[1, 1, 1], fx), fy), fz)
                cs = np.stack([v.astype(np.float64) for v in c.values()])
                ws = np.stack([v.astype(np.float64) for v in w.values()])
                cmax, crange = np.abs(cs).max(0), cs.max(0) - cs.min(0)
                Gs = np.stack([gx, gy, gz], 1)
                eps = e_p[sub]
                tot = eps.sum(1)
                F[sub], Wb[sub], G[sub] = Fs, Wbs, Gs
                eF[sub] = 16 * U * cmax + (np.abs(Gs.astype(np.float64)) * eps).sum(1)
                eG[sub] = 24 * U * cmax[:, None] + 2 * crange[:, None] * (tot[:, None] - eps)
                eWb[sub] = 16 * U * ws.max(0) + (ws.max(0) - ws.min(0)) * tot
            samples[idx] += 1
            F64 = F.astype(np.float64)
            amb[idx] |= obs & (np.abs(F64) < C_POS * eF)
            amb[idx] |= amb_face
            Fp, Gp, Wbp = P["F"][idx], P["G"][idx], P["Wb"][idx]
            hit = obs & P["obs"][idx] & (Fp > 0) & (F <= 0)
            if mistake == "back_face":               # any sign change, the surface seen from behind included
                hit = obs & P["obs"][idx] & (((Fp > 0) & (F <= 0)) | ((Fp < 0) & (F >= 0)))
            if mistake == "prev_unobserved":         # ... and only sample k has to be observed
                hit = obs & (Fp > 0) & (F <= 0)
            if hit.any():
                h = np.nonzero(hit)[0]
                gi = idx[h]
                F0, F1 = Fp[h], F[h]
                s = F0 / (F0 - F1)
                dep = (t_prev + f(dt32) * s).astype(f)
                g = (Gp[h] + s[:, None] * (G[h] - Gp[h])).astype(f)
                ln = np.sqrt((g * g).sum(1))
                nrm = np.where(ln[:, None] > 0, g / np.where(ln > 0, ln, 1)[:, None], 0).astype(f)
                wgt = (Wbp[h] + s * (Wb[h] - Wbp[h])).astype(f)
                F0d, F1d, sd = F0.astype(np.float64), F1.astype(np.float64), s.astype(np.float64)
                e_s = (np.abs(F0d) * eF[h] + np.abs(F1d) * P["eF"][gi]) / (F0d - F1d) ** 2 + 2 * U
                G0d, G1d = Gp[h].astype(np.float64), G[h].astype(np.float64)
                e_g = np.abs(G1d - G0d) * e_s[:, None] + P["eG"][gi] + eG[h] + 3 * U * (np.abs(G0d) + np.abs(G1d))
                lnd = ln.astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    e_n = (e_g + e_g.sum(1, keepdims=True)) / lnd[:, None] + 4 * U
                W0d, W1d = Wbp[h].astype(np.float64), Wb[h].astype(np.float64)
                depth[gi], normal[gi], weight[gi] = dep, nrm, wgt
                tol_d[gi] = dt64 * e_s + 2 * U * np.abs(dep.astype(np.float64))
                tol_w[gi] = np.abs(W1d - W0d) * e_s + P["eWb"][gi] + eWb[h] + 3 * U * (np.abs(W0d) + np.abs(W1d))
                skip_n[gi] = lnd <= 16 * e_g.sum(1)
                tol_n[gi] = np.where(np.isfinite(e_n), e_n, 0.0)
                amb[gi] |= near_any[h] | P["near"][gi]
                hit_b[gi] = True
                done[gi] = True
            P["obs"][idx], P["F"][idx], P["Wb"][idx], P["G"][idx] = obs, F, Wb, G
            P["eF"][idx], P["eWb"][idx], P["eG"][idx], P["near"][idx] = eF, eWb, eG, near_any
            done |= khi <= k
        sl = (vv, uu)
        out["depth"][sl], out["weight"][sl], out["normal"][sl], out["hit"][sl], out["amb"][sl] = depth, weight, normal, hit_b, amb
        out["tol_depth"][sl], out["tol_weight"][sl], out["tol_normal"][sl], out["skip_normal"][sl], out["samples"][sl] = tol_d, tol_w, tol_n, skip_n, samples
    return out


def compare(got, ref, label=""):
    """THE comparison of the suite.  ``got``: dict(depth [H,W], normal [H,W,3], weight [H,W]) of fp32 arrays; ``ref`` from raycast(dtype=float64).
    Returns a dict of figures after asserting what the module docstring states."""
    gd, gn, gw = (np.asarray(got[k]) for k in ("depth", "normal", "weight"))
    assert gd.shape == ref["depth"].shape and gn.shape == ref["normal"].shape and gw.shape == ref["weight"].shape
    assert np.isfinite(gd).all() and np.isfinite(gn).all() and np.isfinite(gw).all(), "an output is not finite"
    hit, amb = ref["hit"], ref["amb"]
    n_hit, n_amb = int(hit.sum()), int(amb.sum())
    fig = {"hit": n_hit, "ambiguous": n_amb, "amb_share": n_amb / max(n_hit, 1)}
    assert n_amb <= AMB_CAP * n_hit, "%s: %d ambiguous pixels exceed %.2f of the %d hit pixels" % (label, n_amb, AMB_CAP, n_hit)
    keep = ~amb
    got_hit = gd != 0
    wrong = keep & (got_hit != hit)
    fig["hit_mismatch"] = int(wrong.sum())
    miss = keep & ~hit
    zero = (gd[miss] == 0).all() and (gw[miss] == 0).all() and (gn[miss] == 0).all()
    sel = keep & hit & got_hit
    for name, g, tol in (("depth", gd, ref["tol_depth"]), ("weight", gw, ref["tol_weight"]), ("normal", gn, ref["tol_normal"])):
        err = np.abs(g.astype(np.float64) - ref[name].astype(np.float64))
        s3 = sel & ~ref["skip_normal"] if name == "normal" else sel
        e, t = err[s3], tol[s3]
        ratio = e / np.maximum(t, 1e-300)
        fig[name + "_ratio"] = float(ratio.max()) if ratio.size else 0.0
        fig[name + "_err"] = float(e.max()) if e.size else 0.0
    print("tsdf_raycast compare %s: hit %d ambiguous %d (%.4f) hit/no-hit mismatches %d; max error / bound (bar %.1f): depth %.3f (%.3g m) "
          "normal %.3f (%.3g) weight %.3f (%.3g)" % (label, n_hit, n_amb, fig["amb_share"], fig["hit_mismatch"], C_RAY, fig["depth_ratio"],
                                                      fig["depth_err"], fig["normal_ratio"], fig["normal_err"], fig["weight_ratio"], fig["weight_err"]))
    assert not wrong.any(), "%s: hit / no-hit differs on %d unambiguous pixels, first at %s" % (label, fig["hit_mismatch"], np.argwhere(wrong)[0])
    assert zero, "%s: a pixel without a hit is not exactly zero" % label
    for name in ("depth", "normal", "weight"):
        assert fig[name + "_ratio"] <= C_RAY, "%s: %s error at %.3f of its bound (bar %.1f)" % (label, name, fig[name + "_ratio"], C_RAY)
    return fig


def backproject(depth, pose, K):
    """world points [H,W,3] float64 of a z-depth map seen from the camera-to-world ``pose`` (pixel centres on integers)"""
    H, W = depth.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(np.asarray(K, np.float64)).T
    return (rays * np.asarray(depth, np.float64)[..., None]) @ np.asarray(pose, np.float64)[:3, :3].T + np.asarray(pose, np.float64)[:3, 3]


def view(case, pose=None):
    """the arguments of one render of a tsdf_ref case: M from ``pose`` (default: the held-out pose), the case's image size and intrinsics"""
    H, W = case["depths"].shape[1:]
    pose = HELD_OUT_POSE if pose is None else pose
    return dict(M=ray_matrix(pose, case["K"], case["origin"], case["voxel"]), H=H, W=W, t_min=T_MIN, dt=case["voxel"], n_steps=N_STEPS, pose=pose)
