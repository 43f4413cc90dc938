"""float64 reference of the rigid-registration contract of the library (csrc/track/rigid_align.hip, include/estd_hip.h: estd_rigid_apply,
estd_rigid_system), in the style of tests/track_ref.py.  A plain helper module of the test suite (not a conftest); numpy only.

``apply`` evaluates T p (and R n) and ``evaluate`` the system, in float64 FROM THE fp32 VALUES THE KERNELS RECEIVE: the system's inputs are
the fp32 moved cloud, the index, the target and the normals, so every input is exact and only the kernel's own operations round.
``dtype=np.float32`` evaluates the same contract in numpy fp32 arithmetic (the CPU stand-in for the kernel; numpy has no fused
multiply-add, so every product rounds on its own).  With ``match=`` the decisions are TAKEN from a given match map and only the values are
computed: that is how the 29 sums of a device run are checked.  ``compare`` is THE comparison of the suite (GPU results and the stand-in
alike): ambiguous points <= AMB_CAP of the gated points (those whose index is in range); on every other point ``match`` exact and
    |residual - ref| <= C e_r;
wherever ``match`` is -1 the residual is exactly 0; sums[28] equals the number of matched points exactly and every other sum
    |sum_k - ref_k(given the match map)| <= C sum over the matched points of e_term_k;
``moved`` (and ``moved_normal``), when given, within C e_moved of T p.

Rounding bounds (first order, u = 2^-24; the counts are the unfused ones, a fused multiply-add rounds once where they count twice)
    moved_j = T_j0 x + T_j1 y + T_j2 z + T_j3, S_j = the sum of the absolute terms: three products and three additions in a chain, each
        addition's error at most u times the partial sum's magnitude <= S_j:        e_moved_j = 4 u S_j      (track_ref's e_a with exact p);
        the normal's row has no T_j3:                                               e_mn_j = 4 u S_j.
    e_j = q_j - m_j, both stored values:                                            e_e_j = u |e_j|.
    e2 = e_x^2 + e_y^2 + e_z^2:   e_e2 = sum_j 2 |e_j| e_e_j + 3 u e2              (track_ref's).
    c = n . s, S_c = sum_j |n_j s_j|, stored values:                                e_c = 3 u S_c.
    plane:  r = n . e, S_r = sum_j |n_j e_j|:  e_r = sum_j |n_j| e_e_j + 3 u S_r.
        w = q x n, S_w_x = |q_y n_z| + |q_z n_y| (and cyclic), stored values:       e_w_x = 2 u S_w_x.     J = (n, w): e_J = (0, 0, 0, e_w).
        terms, each ONE fp32 product: e(J_i J_j) = |J_i| e_J_j + |J_j| e_J_i + u |J_i J_j|; e(J_i r) = |J_i| e_r + |r| e_J_i + u |J_i r|;
        e(r^2) = 2 |r| e_r + u r^2.
    point:  residual = sqrt(e2):  e_res = e_e2 / (2 sqrt(e2)) + u sqrt(e2) (0 where e2 = 0: then e = 0 exactly);
        terms: 1, 0 and +-q_k are exact; q_y^2 + q_z^2: 3 u times the value; -(q_x q_y): u |q_x q_y|; e_k: e_e_k;
        (q x e)_x = q_y e_z - q_z e_y: |q_y| e_e_z + |q_z| e_e_y + 2 u (|q_y e_z| + |q_z e_y|) (and cyclic); e2: e_e2.
    The count is exact.  The float64 additions add <= 2^-53 n per term: n 2^-53 sum |term|.
    C = 2: for what first order leaves out, as track_ref's C_TRACK -- every count above is already the unfused one.
Decisions and their tolerances (C_POS = 2 as in track_ref.py).  The index gate compares integers and is exact.  A point that has reached
the decision in the reference is ambiguous when
    |e2 - dist_max^2| < C_POS e_e2 -- unless the gate is EXACT at the point: the numpy-fp32 evaluation reproduces the float64 values of e
        and e2 bit for bit.  Then every fp32 operation on the way was exact, any evaluation order, fused or not, gives those very values,
        and the gate compares two stored numbers (the case "tie": e2 == dist_max^2 passes the contract's <=);
    | c - cos_min | < C_POS e_c (| |c| - cos_min | with two_sided).

The scene is track_ref's: the plane z = 2.6 and the two spheres, here as a triangle mesh (the plane as two triangles, the spheres as
level-1 icospheres) and as samples of it with the faces' normals.  It fixes all six degrees of freedom:
tests/test_rigid_align_ref_cpu.py asserts that the eigenvalues of the reference's A / count lie within track_ref.COND_FIXTURE of each other.

``refine`` is the float64 reference REGISTRATION: brute-force correspondences (the nearest target point, or the closest point of the
nearest triangle), the same gates, the same systems, the same solve and the same stopping rule as estdepth_amd/registration.py.
"""
import functools

import numpy as np

import placement as PL
import track_ref as TR
from mesh_distance_ref import icosphere

U = 2.0 ** -24
C = 2.0                      # route constant of the value bounds, from the derivation above
C_POS = 2.0                  # decision tolerance = C_POS * rounding bound
AMB_CAP = 0.03               # ambiguous points: at most this share of the gated points in every case
N_SUMS = 29
PLANE, POINT = 0, 1
METRICS = {"plane": PLANE, "point": POINT}
DIST_MAX = 0.05              # the gate of the suite's cases: the bulk of the partners lies within 0.02, the planted outliers at 0.2
COS_MIN = 0.7
STEP_T, STEP_R = 1e-5, 1e-5  # registration.py's stopping rule (tracking.py's)
COND_MAX = 1e6
MISTAKES = ("cross_nxq", "gate_lt", "missing_wave", "point_sign")
TRIU = TR.TRIU
TWIST = TR.TWIST             # about 1 cm and 0.5 degrees


# ------------------------------------------------------------------------------------------------------------ the scene
@functools.lru_cache(maxsize=None)
def scene_mesh(level=1, place=None):
    """-> (xyz float32 [V,3], faces int32 [F,3]): the plane z = 2.6 over [-1.6, 1.6] x [-1.2, 1.2] as two triangles whose normals point
    to -z (towards the cameras), and the two spheres as icospheres of ``level``, outward.  ``place`` (placement.py): the float64 vertices
    moved there before the one rounding to fp32"""
    z = TR.PLANE_Z
    xyz = [np.array([(-1.6, -1.2, z), (1.6, -1.2, z), (1.6, 1.2, z), (-1.6, 1.2, z)], np.float64)]
    faces = [np.array([(0, 2, 1), (0, 3, 2)], np.int64)]
    n = 4
    for centre, radius in TR.SPHERES:
        v, f = icosphere(level, radius)
        xyz.append(v.astype(np.float64) + np.asarray(centre))
        faces.append(f.astype(np.int64) + n)
        n += v.shape[0]
    xyz = np.concatenate(xyz)
    if PL.key(place) is not None:
        xyz = PL.points(xyz, place)
    return xyz.astype(np.float32), np.concatenate(faces).astype(np.int32)


def subdivided(xyz, faces):
    """every triangle cut into four at its edges' midpoints, which stay ON the triangle: the same surface with other faces (and, sampled
    by area, other samples) -> (xyz float32, faces int32)"""
    xyz, faces = np.asarray(xyz, np.float64), np.asarray(faces, np.int64)
    pts, mid, out = [p for p in xyz], {}, []

    def m(i, j):
        k = (min(i, j), max(i, j))
        if k not in mid:
            pts.append(0.5 * (xyz[i] + xyz[j]))
            mid[k] = len(pts) - 1
        return mid[k]
    for a, b, c in faces.tolist():
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.asarray(pts).astype(np.float32), np.asarray(out, np.int32)


def face_normals(xyz, faces):
    """unit normals float64 [F,3] and areas [F] from the fp32 vertices"""
    t = np.asarray(xyz, np.float64)[np.asarray(faces, np.int64)]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ln = np.linalg.norm(n, axis=1)
    return n / ln[:, None], 0.5 * ln


def sample_scene(n, seed, place=None):
    """``n`` points spread by area over the scene's mesh -> (xyz float32 [n,3], normal float32 [n,3], face int64 [n]); ``place``: the
    float64 samples and normals of the unplaced scene moved there before the one rounding to fp32"""
    xyz, faces = scene_mesh()
    nrm, area = face_normals(xyz, faces)
    rng = np.random.RandomState(seed)
    f = rng.choice(faces.shape[0], size=n, p=area / area.sum())
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    t = xyz.astype(np.float64)[faces.astype(np.int64)[f]]
    p = t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])
    if PL.key(place) is not None:
        return PL.points(p, place).astype(np.float32), PL.vectors(nrm[f], place).astype(np.float32), f.astype(np.int64)
    return p.astype(np.float32), nrm[f].astype(np.float32), f.astype(np.int64)


def single_plane(n, seed):
    """``n`` points on the plane alone: three degrees of freedom are not fixed.  The normals carry 1e-4 of noise, as estimated normals
    do: A stays positive definite (the Cholesky factorisation goes through) with eigenvalues some 1e8 apart"""
    rng = np.random.RandomState(seed)
    p = np.stack([rng.uniform(-1.6, 1.6, n), rng.uniform(-1.2, 1.2, n), np.full(n, TR.PLANE_Z)], 1)
    nrm = np.array([0.0, 0.0, -1.0]) + 1e-4 * rng.randn(n, 3)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return p.astype(np.float32), nrm.astype(np.float32)


exp_se3 = TR.exp_se3
pose_error = TR.pose_error


def t12(T):
    """the 3 x 4 fp32 matrix estd_rigid_apply receives"""
    return np.ascontiguousarray(np.asarray(T, np.float64)[:3, :4].astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ the contract
def apply(T12, src, src_normal=None, dtype=np.float64):
    """-> dict(moved [n,3], tol_moved, moved_normal / tol_normal or None) from the fp32 matrix and points"""
    f = dtype
    T32 = np.asarray(T12, np.float32).reshape(3, 4)
    T, T64 = T32.astype(f), T32.astype(np.float64)
    p32 = np.asarray(src, np.float32)
    p, p64 = p32.astype(f), p32.astype(np.float64)
    moved = np.stack([T[j, 0] * p[:, 0] + (T[j, 1] * p[:, 1] + (T[j, 2] * p[:, 2] + T[j, 3])) for j in range(3)], 1)
    tol = np.stack([4 * U * (np.abs(T64[j, :3] * p64).sum(1) + abs(T64[j, 3])) for j in range(3)], 1)
    out = dict(moved=moved, tol_moved=tol, moved_normal=None, tol_normal=None)
    if src_normal is not None:
        s32 = np.asarray(src_normal, np.float32)
        s, s64 = s32.astype(f), s32.astype(np.float64)
        out["moved_normal"] = np.stack([T[j, 0] * s[:, 0] + (T[j, 1] * s[:, 1] + T[j, 2] * s[:, 2]) for j in range(3)], 1)
        out["tol_normal"] = np.stack([4 * U * np.abs(T64[j, :3] * s64).sum(1) for j in range(3)], 1)
    return out


def evaluate(c, dtype=np.float64, mistake=None, match=None, _exact=True):
    """``c``: dict(moved [N,3] f32, moved_normal [N,3] f32 or None, index int64 [N], target [Nt,3] f32, normal [Nn,3] f32 or None, by_index,
    metric ("plane" / "point"), dist_max, cos_min (None: no gate), two_sided) -- as the kernel receives them.  Returns a dict: match (int64
    [N], -1 = skipped), residual (``dtype``), gated, amb (bool), tol_r, terms [N,29] (``dtype``, zeros where skipped), tol_terms, sums
    (float64 [29]) and tol_sums.  ``mistake``: one of MISTAKES, a deliberately WRONG contract.  ``match``: take the decisions from this map."""
    assert mistake is None or mistake in MISTAKES, mistake
    f = dtype
    m32, q_all = np.asarray(c["moved"], np.float32), np.asarray(c["target"], np.float32)
    N, Nt = m32.shape[0], q_all.shape[0]
    n_all = np.asarray(c["normal"], np.float32) if c.get("normal") is not None else None
    Nn = n_all.shape[0] if n_all is not None else Nt
    metric = METRICS[c["metric"]]
    s32 = np.asarray(c["moved_normal"], np.float32) if c.get("moved_normal") is not None else None
    cos_min = c.get("cos_min")
    use_cos = s32 is not None and cos_min is not None and np.isfinite(cos_min)
    assert n_all is not None or not (use_cos or metric == PLANE)
    d2_32 = np.float32(c["dist_max"]) * np.float32(c["dist_max"])
    index = np.asarray(c["index"], np.int64)
    if match is None:
        gated = (index >= 0) & (index < Nn) & ((index < Nt) | (not c["by_index"]))
        k = np.where(gated, index, 0)
    else:
        match = np.asarray(match, np.int64)
        assert match.shape == (N,) and match.max(initial=-1) < Nn and match.min(initial=0) >= -1
        gated = match >= 0
        k = np.where(gated, match, 0)
    alive, amb = gated.copy(), np.zeros(N, bool)
    q32 = q_all[k] if c["by_index"] else q_all[:N]
    q32 = np.where(gated[:, None], q32, np.float32(0))
    mm32 = np.where(gated[:, None], m32, np.float32(0))
    n32 = n_all[k] if n_all is not None else np.zeros((N, 3), np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q, m, n = q32.astype(f), mm32.astype(f), n32.astype(f)
        q64, n64 = q32.astype(np.float64), n32.astype(np.float64)
        e = q - m
        e64 = e.astype(np.float64)
        e_e = U * np.abs(e64)
        e2 = e[:, 0] * e[:, 0] + (e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        e264 = e2.astype(np.float64)
        e_e2 = (2 * np.abs(e64) * e_e).sum(1) + 3 * U * e264
        if match is None:
            close = np.abs(e264 - float(d2_32)) < C_POS * e_e2
            if f is np.float64 and _exact and close.any():
                s = evaluate(c, np.float32, mistake, None, _exact=False)
                close &= ~((s["e2"].astype(np.float64) == e264) & (s["e"].astype(np.float64) == e64).all(1))
            amb |= alive & close
            alive &= (e2 < f(d2_32)) if mistake == "gate_lt" else (e2 <= f(d2_32))
            if use_cos:
                sn = np.where(gated[:, None], s32, np.float32(0))
                cc = n[:, 0] * sn[:, 0].astype(f) + (n[:, 1] * sn[:, 1].astype(f) + n[:, 2] * sn[:, 2].astype(f))
                e_c = 3 * U * np.abs(n64 * sn.astype(np.float64)).sum(1)
                cv = np.abs(cc) if c["two_sided"] else cc
                amb |= alive & (np.abs(cv.astype(np.float64) - float(np.float32(cos_min))) < C_POS * e_c)
                alive &= cv >= f(np.float32(cos_min))
        zero = np.zeros(N)
        if metric == PLANE:
            r = n[:, 0] * e[:, 0] + (n[:, 1] * e[:, 1] + n[:, 2] * e[:, 2])
            e_r = (np.abs(n64) * e_e).sum(1) + 3 * U * np.abs(n64 * e64).sum(1)
            w, e_w = [], []
            for a in range(3):
                i, j = (a + 1) % 3, (a + 2) % 3
                w.append(q[:, i] * n[:, j] - q[:, j] * n[:, i])
                e_w.append(2 * U * (np.abs(q64[:, i] * n64[:, j]) + np.abs(q64[:, j] * n64[:, i])))
            if mistake == "cross_nxq":
                w = [-t for t in w]
            J = [n[:, 0], n[:, 1], n[:, 2]] + w
            e_J = [zero, zero, zero] + e_w
            J64, r64 = [t.astype(np.float64) for t in J], r.astype(np.float64)
            terms = [(J[i] * J[j], np.abs(J64[i]) * e_J[j] + np.abs(J64[j]) * e_J[i] + U * np.abs(J64[i] * J64[j])) for i, j in TRIU]
            terms += [(J[i] * r, np.abs(J64[i]) * e_r + np.abs(r64) * e_J[i] + U * np.abs(J64[i] * r64)) for i in range(6)]
            terms += [(r * r, 2 * np.abs(r64) * e_r + U * r64 * r64)]
            res, tol_r = r, e_r
        else:
            sg = f(-1.0) if mistake == "point_sign" else f(1.0)
            one, nul = np.ones(N, f), np.zeros(N, f)
            qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
            ax, ay, az = np.abs(q64[:, 0]), np.abs(q64[:, 1]), np.abs(q64[:, 2])
            sq = lambda a, b: (a * a + b * b, 3 * U * (a * a + b * b).astype(np.float64))                       # noqa: E731
            pr = lambda a, b: (-(a * b), U * np.abs((a * b).astype(np.float64)))                                # noqa: E731
            terms = [(one, zero), (nul, zero), (nul, zero), (nul, zero), (sg * qz, zero), (-sg * qy, zero),
                     (one, zero), (nul, zero), (-sg * qz, zero), (nul, zero), (sg * qx, zero),
                     (one, zero), (sg * qy, zero), (-sg * qx, zero), (nul, zero),
                     sq(qy, qz), pr(qx, qy), pr(qx, qz), sq(qx, qz), pr(qy, qz), sq(qx, qy)]
            terms += [(e[:, a], e_e[:, a]) for a in range(3)]
            aq = (ax, ay, az)
            for a in range(3):
                i, j = (a + 1) % 3, (a + 2) % 3
                terms.append((sg * (q[:, i] * e[:, j] - q[:, j] * e[:, i]),
                              aq[i] * e_e[:, j] + aq[j] * e_e[:, i] + 2 * U * (np.abs(q64[:, i] * e64[:, j]) + np.abs(q64[:, j] * e64[:, i]))))
            terms += [(e2, e_e2)]
            res = np.sqrt(e2)
            root = np.sqrt(e264)
            tol_r = np.where(root > 0, e_e2 / np.maximum(2 * root, 1e-300), 0.0) + U * root
        terms += [(np.ones(N, f), zero)]
        val = np.stack([np.where(alive, t, f(0.0)) for t, _ in terms], 1)
        tol = np.stack([np.where(alive, t, 0.0) for _, t in terms], 1)
        res = np.where(alive, res, f(0.0))
    n_match = int(alive.sum())
    v64 = val.astype(np.float64)
    sums = v64.sum(0)
    tol_sums = tol.sum(0) + n_match * 2.0 ** -53 * np.abs(v64).sum(0)
    return {"match": np.where(alive, k, -1), "residual": res, "gated": gated, "amb": amb & gated, "tol_r": np.where(alive, tol_r, 0.0),
            "terms": val, "tol_terms": tol, "sums": sums, "tol_sums": tol_sums, "e2": e2, "e": e, "count": n_match}


def standin(c, mistake=None):
    """the numpy-fp32 stand-in for the two kernels on a case -> the dict ``compare`` takes.  ``mistake`` "missing_wave": the fourth wave
    of every 256-point workgroup never reaches the sums"""
    a = apply(c["T12"], c["src"], c["src_normal"], np.float32)
    s = evaluate(c, np.float32, None if mistake == "missing_wave" else mistake, _exact=False)
    sums = s["sums"]
    if mistake == "missing_wave":
        sums = s["terms"].astype(np.float64)[(np.arange(s["terms"].shape[0]) % 256) < 192].sum(0)
    return dict(moved=a["moved"], moved_normal=a["moved_normal"], residual=s["residual"].astype(np.float32), match=s["match"], sums=sums)


def compare(got, c, ref=None, label=""):
    """THE comparison of the suite.  ``got``: dict(residual f32 [N], match int64 [N], sums f64 [29], and optionally moved / moved_normal of
    the apply kernel on c["src"] / c["src_normal"] with c["T12"]); ``ref``: evaluate(c) (computed here when not given)."""
    ref = evaluate(c) if ref is None else ref
    res, mt, sums = np.asarray(got["residual"]), np.asarray(got["match"]).astype(np.int64), np.asarray(got["sums"], np.float64)
    N = ref["residual"].shape[0]
    assert res.shape == (N,) and mt.shape == (N,) and sums.shape == (N_SUMS,), (res.shape, mt.shape, sums.shape)
    fig = {"moved_ratio": 0.0}
    if got.get("moved") is not None:
        a = apply(c["T12"], c["src"], c["src_normal"])
        pairs = [(got["moved"], a["moved"], a["tol_moved"])]
        if a["moved_normal"] is not None:
            assert got.get("moved_normal") is not None, "%s: no moved normals came back" % label
            pairs.append((got["moved_normal"], a["moved_normal"], a["tol_normal"]))
        for g, want, tol in pairs:
            g = np.asarray(g, np.float64)
            assert g.shape == want.shape, (g.shape, want.shape)
            d = np.abs(g - want)
            fig["moved_ratio"] = max(fig["moved_ratio"], float(np.max(np.where(d == 0, 0.0, d / np.maximum(tol, 1e-300)), initial=0.0)))
    Nn = np.asarray(c["normal"]).shape[0] if c.get("normal") is not None else np.asarray(c["target"]).shape[0]
    gated, amb = ref["gated"], ref["amb"]
    n_gated, n_amb = int(gated.sum()), int(amb.sum())
    fig.update(gated=n_gated, ambiguous=n_amb, amb_share=n_amb / max(n_gated, 1), matched=int((mt >= 0).sum()))
    in_range = bool(((mt >= -1) & (mt < Nn)).all())
    finite = bool(np.isfinite(res).all()) and bool(np.isfinite(sums).all())
    keep = ~amb
    fig["match_mismatch"] = int((keep & (mt != ref["match"])).sum())
    skipped_zero = bool((res[mt < 0] == 0).all())
    both = keep & (mt >= 0) & (ref["match"] == mt)
    err = np.abs(res.astype(np.float64) - ref["residual"].astype(np.float64))[both]
    ratio = np.where(err == 0, 0.0, err / np.maximum(ref["tol_r"][both], 1e-300))
    fig["residual_ratio"] = float(ratio.max()) if ratio.size else 0.0
    fig["sum_ratio"], fig["count_exact"] = float("inf"), False
    if in_range and finite:
        given = evaluate(c, match=mt)
        fig["count_exact"] = bool(sums[28] == float((mt >= 0).sum()))
        d = np.abs(sums[:28] - given["sums"][:28])
        fig["sum_ratio"] = float(np.max(np.where(d == 0, 0.0, d / np.maximum(given["tol_sums"][:28], 1e-300))))
    print("rigid_align compare %s: gated %d ambiguous %d (%.4f) matched %d; match mismatches %d; max error / bound (bar %.1f): moved %.3g "
          "residual %.3g sums %.3g" % (label, n_gated, n_amb, fig["amb_share"], fig["matched"], fig["match_mismatch"], C, fig["moved_ratio"],
                                       fig["residual_ratio"], fig["sum_ratio"]))
    assert fig["moved_ratio"] <= C, "%s: a moved coordinate is at %.3f of its bound (bar %.1f)" % (label, fig["moved_ratio"], C)
    assert in_range, "%s: a match outside -1 .. Nn - 1" % label
    assert finite, "%s: an output is not finite" % label
    assert n_amb <= AMB_CAP * n_gated, "%s: %d ambiguous points exceed %.2f of the %d gated points" % (label, n_amb, AMB_CAP, n_gated)
    assert fig["match_mismatch"] == 0, "%s: match differs on %d unambiguous points" % (label, fig["match_mismatch"])
    assert skipped_zero, "%s: a skipped point's residual is not exactly zero" % label
    assert fig["residual_ratio"] <= C, "%s: residual error at %.3f of its bound (bar %.1f)" % (label, fig["residual_ratio"], C)
    assert fig["count_exact"], "%s: sums[28] = %r but %d points are matched" % (label, sums[28], fig["matched"])
    assert fig["sum_ratio"] <= C, "%s: a sum is at %.3f of its bound (bar %.1f)" % (label, fig["sum_ratio"], C)
    return fig


# ------------------------------------------------------------------------------------------------------------ Gauss-Newton, float64
def unpack(sums):
    return TR.unpack(sums)


def target_pivot(target):
    """registration.target_pivot in this module's words: the centre of the bounding box of the target's fp32 points (a cloud) or of the
    vertices its faces name (a mesh), (lo + hi) / 2 in float64 -> [3]"""
    xyz = np.asarray(target["xyz"], np.float32)
    if "faces" in target:
        xyz = xyz[np.unique(np.asarray(target["faces"], np.int64))]
    return 0.5 * (xyz.min(0).astype(np.float64) + xyz.max(0).astype(np.float64))


def pivoted(A, b, pivot):
    """(A, b) of twists about the world origin -> about ``pivot`` c: G = [[I, 0], [-[c]x, I]], A_c = G A G^T, b_c = G b (None: unchanged)"""
    if pivot is None:
        return A, b
    G = np.eye(6)
    G[3:, :3] = -TR.hat(np.asarray(pivot, np.float64).reshape(3))
    Ac = G @ A @ G.T
    return 0.5 * (Ac + Ac.T), G @ b


def pivot_step(xi, pivot):
    """C Exp(xi) C^-1 with C the translation by the pivot: the twist applied about the pivot (None: about the world origin)"""
    E = exp_se3(xi)
    if pivot is not None:
        c = np.asarray(pivot, np.float64).reshape(3)
        E[:3, 3] += c - E[:3, :3] @ c
    return E


def solve_step(A, b, count, min_count, cond_max=COND_MAX, pivot=None):
    """tracking.solve_step in this module's words -> (xi or None, reason); with ``pivot`` the tests and the solve are those of the
    system about it and xi is the twist about it"""
    if count < min_count:
        return None, "count"
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None, "cholesky"
    A, b = pivoted(A, b, pivot)
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None, "cholesky"
    ev = np.linalg.eigvalsh(A)
    if not ev[0] > 0 or ev[-1] > cond_max * ev[0]:
        return None, "condition"
    return np.linalg.solve(Lc.T, np.linalg.solve(Lc, b)), None


def closest_on_mesh(p, xyz, faces, chunk=2048):
    """brute force in float64: per point the closest point of the nearest triangle (Ericson 5.1.5) -> (closest [n,3], face [n], dist [n])"""
    p = np.asarray(p, np.float64)
    t = np.asarray(xyz, np.float64)[np.asarray(faces, np.int64)]
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    ab, ac = b - a, c - a
    out_p, out_f, out_d = [], [], []
    dot = lambda x, y: (x * y).sum(-1)                                                                        # noqa: E731
    for i in range(0, p.shape[0], chunk):
        q = p[i:i + chunk, None, :]
        ap, bp, cp = q - a, q - b, q - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(divide="ignore", invalid="ignore"):
            conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                     (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
            wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            den = 1.0 / (va + vb + vc)
            v = np.select(conds, [0 * d1, 1 + 0 * d1, d1 / (d1 - d3), 0 * d1, 0 * d1, 1 - wbc], vb * den)
            w = np.select(conds, [0 * d1, 0 * d1, 0 * d1, 1 + 0 * d1, d2 / (d2 - d6), wbc], vc * den)
        pt = a + v[..., None] * ab + w[..., None] * ac
        dd = ((q - pt) ** 2).sum(-1)
        f = np.argmin(dd, 1)
        r = np.arange(dd.shape[0])
        out_p.append(pt[r, f]); out_f.append(f); out_d.append(np.sqrt(dd[r, f]))
    return np.concatenate(out_p), np.concatenate(out_f), np.concatenate(out_d)


def nearest_point(p, target, chunk=1024):
    """brute force in float64 -> (index [n], dist [n]): every pair's |t|^2 - 2 p . t (one matrix product per chunk; its rounding, some
    1e-15 m2, is far below what separates two candidates anywhere but on a tie), the distance of the winner from the difference itself"""
    p, t = np.asarray(p, np.float64), np.asarray(target, np.float64)
    tt = (t * t).sum(1)
    idx = [np.argmin(tt[None] - 2.0 * (p[i:i + chunk] @ t.T), 1) for i in range(0, p.shape[0], chunk)]
    k = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    return k, np.sqrt(((p - t[k]) ** 2).sum(1))


def system64(src, T, target, metric, dist_max, src_normal=None, cos_min=None, two_sided=False):
    """one float64 system of the registration at the transform ``T``.  ``target``: dict(xyz, normal) (a cloud) or dict(xyz, faces) (a
    mesh).  Everything in float64 from the fp32 inputs (the moved cloud is NOT rounded to fp32: this is the reference of the method,
    the kernels' arithmetic has ``evaluate``) -> dict(A, b, count, rmse)"""
    T = np.asarray(T, np.float64)
    m = np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3]
    if "faces" in target:
        q, k, dist = closest_on_mesh(m, target["xyz"], target["faces"])
        n = face_normals(target["xyz"], target["faces"])[0][k]
    else:
        k, dist = nearest_point(m, target["xyz"])
        q = np.asarray(target["xyz"], np.float64)[k]
        n = np.asarray(target["normal"], np.float64)[k] if target.get("normal") is not None else None
    ok = dist <= float(np.float32(dist_max))
    if src_normal is not None and cos_min is not None:
        cc = (n * (np.asarray(src_normal, np.float64) @ T[:3, :3].T)).sum(1)
        ok &= (np.abs(cc) if two_sided else cc) >= cos_min
    q, e = q[ok], (q - m)[ok]
    if metric == "plane":
        n = n[ok]
        r = (n * e).sum(1)
        J = np.concatenate([n, np.cross(q, n)], 1)
        A, b, rr = J.T @ J, J.T @ r, float((r * r).sum())
    else:
        cnt = q.shape[0]
        Q = np.zeros((cnt, 3, 3))
        Q[:, 0, 1], Q[:, 0, 2], Q[:, 1, 0], Q[:, 1, 2], Q[:, 2, 0], Q[:, 2, 1] = -q[:, 2], q[:, 1], q[:, 2], -q[:, 0], -q[:, 1], q[:, 0]
        J = np.concatenate([np.broadcast_to(np.eye(3), (cnt, 3, 3)), -Q], 2)                 # [cnt,3,6]
        A, b, rr = np.einsum("nij,nik->jk", J, J), np.einsum("nij,ni->j", J, e), float((e * e).sum())
    count = int(ok.sum())
    return dict(A=A, b=b, count=count, rmse=float(np.sqrt(rr / count)) if count else 0.0)


def refine(src, target, init=None, metric="plane", dist_max=DIST_MAX, max_iter=30, min_count=100, pivot=None, **kw):
    """the float64 reference registration: registration.register's stages, solve and stopping rule -> dict(T, converged, reason, iterations,
    cond = the condition number of the first system that was tested).  ``pivot``: every system is solved about it and the step is the
    twist about it, as ``register`` does about ``target_pivot(target)``; None: about the world origin, the method before the pivot"""
    stages = [float(d) for d in (dist_max if isinstance(dist_max, (tuple, list)) else (dist_max,))]
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    out = dict(T=T, converged=False, reason="max_iter", iterations=0, cond=None)
    for d in stages:
        P, reason = T.copy(), "max_iter"
        for _ in range(max_iter):
            s = system64(src, P, target, metric, d, **kw)
            if out["cond"] is None and s["count"] >= min_count:
                out["cond"] = float(np.linalg.cond(pivoted(s["A"], s["b"], pivot)[0]))
            xi, why = solve_step(s["A"], s["b"], s["count"], min_count, pivot=pivot)
            if xi is None:
                return dict(T=T, converged=False, reason=why, iterations=out["iterations"], cond=out["cond"])
            P = pivot_step(xi, pivot) @ P
            out["iterations"] += 1
            if np.linalg.norm(xi[:3]) < STEP_T and np.linalg.norm(xi[3:]) < STEP_R:
                reason = "converged"
                break
        T = P
        out.update(T=T, converged=reason == "converged", reason=reason)
    return out


# ------------------------------------------------------------------------------------------------------------ the cases of the suite
ROUTE_SIZES = (1, 255, 256, 257, 64 * 256 + 1, 16641)


def make_case(N, metric="plane", normals=True, by_index=True, two_sided=False, seed=0, name="", place=None):
    """``N`` source points near ``N + 7`` samples of the scene: the partner of point i is index[i] (random; from N = 16 on one index is -1
    and one equals the number of targets).  The moved point lies about 6 mm off its partner, every tenth 0.2 m off (beyond DIST_MAX =
    0.05: the gate is far from both groups); the source normals are the partners' within a few degrees, every eighth negated (kept only
    by the two-sided gate) and every eleventh turned by about 70 degrees (kept by neither).  The system's inputs ``moved`` /
    ``moved_normal`` are the float64 T p, R n rounded to fp32.  ``place``: the same case with the scene built at that placement and the
    transform conjugated to it (the same motion of the scene)."""
    rng = np.random.RandomState(1000 + seed)
    Nt = N + 7
    q, nq, _ = sample_scene(Nt, seed, place)
    index = rng.randint(0, Nt, size=N).astype(np.int64)
    off = rng.randn(N, 3) * 0.0035
    off[5::10] += 0.2 * np.sign(rng.randn(N, 3)[5::10]) / np.sqrt(3.0)
    T = exp_se3(TWIST) if PL.key(place) is None else PL.conjugated(exp_se3(TWIST), place)
    T12 = t12(T)
    T64 = np.eye(4)
    T64[:3, :4] = T12.astype(np.float64)
    Ti = np.linalg.inv(T64)
    want = q[index].astype(np.float64) + off
    src = (want @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    sn = nq[index].astype(np.float64) + rng.randn(N, 3) * 0.03
    turn = np.cross(sn, rng.randn(N, 3))
    turn /= np.linalg.norm(turn, axis=1)[:, None]
    sn /= np.linalg.norm(sn, axis=1)[:, None]
    sn[7::11] = np.cos(1.2) * sn[7::11] + np.sin(1.2) * turn[7::11]
    sn[4::8] *= -1.0
    src_normal = (sn @ Ti[:3, :3].T).astype(np.float32) if normals else None
    if N >= 16:
        index[3], index[9] = -1, Nt
    a = apply(T12, src, src_normal)
    target = q
    if not by_index:
        target = np.where(((index >= 0) & (index < Nt))[:, None], q[np.clip(index, 0, Nt - 1)], np.float32(0)).astype(np.float32)
    return dict(name=name, N=N, T12=T12, src=src, src_normal=src_normal, moved=a["moved"].astype(np.float32),
                moved_normal=a["moved_normal"].astype(np.float32) if normals else None, index=index, target=np.ascontiguousarray(target),
                normal=nq, by_index=by_index, metric=metric, dist_max=DIST_MAX, cos_min=COS_MIN if normals else None, two_sided=two_sided)


def tie_case():
    """16 points whose partner lies at (0.25, 0, 0) + small integers / 64 from them, every value exact in fp32: point 5 sits at exactly
    dist_max = 0.25 (e2 == dist_max^2 passes the contract's <=), the others nearer or farther by a whole 1/64"""
    N = 16
    q = np.zeros((N, 3), np.float32)
    q[:, 0] = 1.0 + np.arange(N) / 4.0
    q[:, 2] = 2.0
    moved = q.copy()
    moved[:, 0] -= (0.25 + (np.arange(N) - 5) / 64.0).astype(np.float32)
    nrm = np.zeros((N, 3), np.float32)
    nrm[:, 0] = 1.0
    eye = t12(np.eye(4))
    return dict(name="tie", N=N, T12=eye, src=moved.copy(), src_normal=None, moved=moved, moved_normal=None, index=np.arange(N, dtype=np.int64),
                target=q, normal=nrm, by_index=True, metric="plane", dist_max=0.25, cos_min=None, two_sided=False)


# name: (N, metric, normals, by_index, two_sided)
CASES = {}
for _n in ROUTE_SIZES:
    CASES["plane-n%d" % _n] = (_n, "plane", True, True, False)
    CASES["point-n%d" % _n] = (_n, "point", False, True, False)
CASES.update({
    "plane-closest-n257": (257, "plane", True, False, False),
    "plane-two-sided-n257": (257, "plane", True, True, True),
    "plane-bare-n257": (257, "plane", False, True, False),
    "point-closest-normals-n257": (257, "point", True, False, True),
    "point-normals-n16641": (16641, "point", True, True, False),
    "plane-closest-two-sided-n16385": (16385, "plane", True, False, True),
    "cond-plane": (4000, "plane", False, True, False),
    "cond-point": (4000, "point", False, True, False),
})


@functools.lru_cache(maxsize=None)
def build_case(name, place=None):
    """the case ``name``; ``place``: the same case built at that placement (the cases of CASES only)"""
    if PL.key(place) is not None:
        n, metric, normals, by_index, two_sided = CASES[name]
        return make_case(n, metric, normals, by_index, two_sided, seed=len(name) + n % 97, name="%s@%s" % (name, PL.label(place)), place=PL.key(place))
    if name == "tie":
        return tie_case()
    if name == "none":                                      # every partner beyond the gate
        c = dict(make_case(300, seed=7, name=name))
        c["moved"] = (c["moved"] + np.float32(1.0)).astype(np.float32)
        return c
    n, metric, normals, by_index, two_sided = CASES[name]
    return make_case(n, metric, normals, by_index, two_sided, seed=len(name) + n % 97, name=name)


@functools.lru_cache(maxsize=None)
def reference(name, place=None):
    """the float64 evaluation of a case, computed once and shared"""
    return evaluate(build_case(name, place))


# the cases of the feature suite that are also built at placement.FAMILY_PLACES: the smallest size with more than one workgroup, both
# metrics and both ways of reading the target
PLACED_CASES = ("plane-n257", "point-n257", "plane-closest-n257")


@functools.lru_cache(maxsize=None)
def registration_fixture(scale=1.0, n=4000, seed=3, place=None):
    """``n`` samples of the scene's mesh moved by the INVERSE of Exp(scale * TWIST): registering them to the unmoved scene must give
    T_true = Exp(scale * TWIST) -> dict(src, src_normal, T_true, mesh = dict(xyz, faces), cloud = dict(xyz, normal): other samples).
    ``place`` (placement.py): the same scene and the same source built at that placement -- the float64 samples moved by the inverse
    twist and then to the placement, rounded to fp32 once -- with T_true conjugated, W Exp(scale * TWIST) W^-1, and ``centre``, the
    point the error of a transform is measured at"""
    place = PL.key(place)
    if place is not None:
        return _placed_registration_fixture(scale, n, seed, place)
    xyz, faces = scene_mesh()
    p, nrm, _ = sample_scene(n, seed)
    T = exp_se3(scale * TWIST)
    Ti = np.linalg.inv(T)
    src = (p.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    sn = (nrm.astype(np.float64) @ Ti[:3, :3].T).astype(np.float32)
    cq, cn, _ = sample_scene(4 * n, seed + 1)
    return dict(src=src, src_normal=sn, T_true=T, mesh=dict(xyz=xyz, faces=faces), cloud=dict(xyz=cq, normal=cn), centre=np.array(SCENE_CENTRE))


SCENE_CENTRE = (0.0, 0.0, 2.2)               # between the spheres and the plane: where a transform's error is measured in metres


def _placed_registration_fixture(scale, n, seed, place):
    xyz, faces = scene_mesh(place=place)
    base = scene_mesh()[0].astype(np.float64)[faces.astype(np.int64)]
    nrm, area = face_normals(scene_mesh()[0], faces)
    rng = np.random.RandomState(seed)                                                      # sample_scene's draws, kept in float64
    f = rng.choice(faces.shape[0], size=n, p=area / area.sum())
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    t = base[f]
    p = t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])
    T = exp_se3(scale * TWIST)
    Ti = np.linalg.inv(T)
    src = PL.points(p @ Ti[:3, :3].T + Ti[:3, 3], place).astype(np.float32)
    sn = PL.vectors(nrm[f] @ Ti[:3, :3].T, place).astype(np.float32)
    cq, cn, _ = sample_scene(4 * n, seed + 1, place)
    return dict(src=src, src_normal=sn, T_true=PL.conjugated(T, place), mesh=dict(xyz=xyz, faces=faces), cloud=dict(xyz=cq, normal=cn),
                centre=PL.points(np.array(SCENE_CENTRE), place))


def transform_error(T, T_true, centre):
    """(metres at ``centre``, radians): how far T moves the point ``centre`` from where T_true moves it, and the angle between the rotations.
    pose_error measures the translation at the world origin, where a rotation error of a placed scene is multiplied by its distance"""
    T, T_true, c = np.asarray(T, np.float64), np.asarray(T_true, np.float64), np.asarray(centre, np.float64)
    d = (T[:3, :3] @ c + T[:3, 3]) - (T_true[:3, :3] @ c + T_true[:3, 3])
    Rd = T[:3, :3] @ T_true[:3, :3].T
    return float(np.linalg.norm(d)), float(np.arccos(np.clip((np.trace(Rd) - 1.0) / 2.0, -1.0, 1.0)))
