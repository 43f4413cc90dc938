"""Reference of the global-registration contract of the library (csrc/register/global_register.hip; include/estd_hip.h: estd_cloud_spfh,
estd_cloud_fpfh, estd_feature_match, estd_ransac_pairs) and of estdepth_amd/registration.py's fpfh / match_features / ransac_pairs /
register_global.  A plain helper module of the test suite (not a conftest); numpy only, float64 and integers, no device.

``spfh``, ``fpfh`` and ``ransac`` repeat the header's operations one by one in float64 (numpy contracts nothing), so the device's hist,
pairs, desc, valid, count, status, T and the winner are compared for EQUALITY.  ``match`` forms the fp32 fma chain with
cloud_knn_ref.fma32 (an exact emulation of the fused multiply-add): equality again.  ``match_fast`` finds the same winners for large
inputs: candidates by a float64 matrix product, the exact chain on the eight best of them, the whole row again wherever the ninth is not
clearly behind.

``ssq``: the reference adds in the kernel's own order (64 lane chains, then the exclusive-or butterfly).  It is compared within
``ssq_bound``, a running error bound in the manner of tests/mesh_distance_ref.py: with u = 2^-53, S_i = |R_i0 p_0| + |R_i1 p_1| +
|R_i2 p_2| + |t_i|, the moved coordinate carries at most 4 u S_i, the difference e_i = m_i - q_i that plus u |e_i|, r2 at most
sum_i 2 |e_i| err(e_i) + 3 u r2, and the sum of n terms at most (n / 64 + 7) u ssq more (a chain of n / 64 additions and six butterfly
levels); two evaluations differ by at most twice that, and C_ROUTE = 2 is the project's route constant.

The fixture (``scene_mesh``): a floor and two walls, three boxes of pairwise different size and yaw and one sphere, 356 triangles, no
rigid symmetry -- unlike the plane and two spheres of tests/track_ref.py, where every point looks like its neighbour."""
import numpy as np

import mesh_distance_ref as MD
import mesh_sample_ref as MS
import rigid_align_ref as RA
from cloud_knn_ref import fma32, knn32

BINS = 33
U64 = 2.0 ** -53
C_ROUTE = 2.0
BASIN_T, BASIN_R = 0.098, np.radians(5.0)        # the start from which test_gpu_registration's x10 case shows the staged register converging
VOXEL = 0.07
HYPOTHESES = 16384
SCENE_CENTRE = np.array([1.2, 1.0, 0.5])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _bin11(v):
    return np.clip(np.floor(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9)), 0, 10).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ descriptors
def spfh(points, normal, index, count, oriented=True):
    """-> (hist int32 [n,33], pairs int32 [n])"""
    P, Nn = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(normal, np.float32).astype(np.float64).reshape(-1, 3)
    index, count = np.asarray(index, np.int64), np.asarray(count, np.int64)
    n, k = index.shape
    hist, pairs = np.zeros((n, BINS), np.int32), np.zeros(n, np.int32)
    if n == 0:
        return hist, pairs
    s = np.arange(n)[:, None]
    used = np.arange(k)[None] < np.clip(count, 0, k)[:, None]
    inr = (index >= 0) & (index < n)
    t = np.where(inr, index, 0)
    nt = Nn[t]
    ok = used & inr & (index != s) & ~(Nn == 0).all(1)[:, None] & ~(nt == 0).all(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = P[t] - P[:, None]
        ln = np.sqrt(_dot(d, d))
        ok &= ln != 0
        dn = d / ln[..., None]
        u = np.broadcast_to(Nn[:, None], dn.shape)
        phi = _dot(u, dn)
        v = _cross(dn, u)
        vl = np.sqrt(_dot(v, v))
        ok &= vl != 0
        v = v / vl[..., None]
        w = _cross(u, v)
        alpha, y, x = _dot(v, nt), _dot(w, nt), _dot(u, nt)
        if oriented:
            ba = _bin11((np.minimum(np.maximum(alpha, -1.0), 1.0) + 1.0) * 5.5)
            bf = _bin11((np.minimum(np.maximum(phi, -1.0), 1.0) + 1.0) * 5.5)
            q = np.abs(x) + np.abs(y)
            r = y / q
            pa = np.where(x >= 0, r, np.where(y >= 0, 2.0 - r, -2.0 - r))
            bt = np.where(q != 0, _bin11((pa + 2.0) * 2.75), 5)
        else:
            alpha, phi, y, x = np.abs(alpha), np.abs(phi), np.abs(y), np.abs(x)
            ba = _bin11(np.minimum(alpha, 1.0) * 11.0)
            bf = _bin11(np.minimum(phi, 1.0) * 11.0)
            q = x + y
            bt = np.where(q != 0, _bin11((y / q) * 11.0), 5)
    rows = np.broadcast_to(s, ok.shape)[ok]
    for off, b in ((0, ba), (11, bf), (22, bt)):
        np.add.at(hist, (rows, off + b[ok]), 1)
    return hist, ok.sum(1).astype(np.int32)


def fpfh(points, normal, index, count, hist, pairs):
    """-> (desc float32 [n,33], valid uint8 [n], invalid)"""
    P, Nn = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(normal, np.float32).reshape(-1, 3)
    index, count, hist, pairs = np.asarray(index, np.int64), np.asarray(count, np.int64), np.asarray(hist, np.int64), np.asarray(pairs, np.int64)
    n, k = index.shape
    i = np.arange(n)
    acc, m = np.zeros((n, BINS)), np.zeros(n, np.int64)
    c = np.clip(count, 0, k)
    for a in range(k):
        j = index[:, a]
        inr = (j >= 0) & (j < n)
        jj = np.where(inr, j, 0)
        d = P[jj] - P
        d2 = _dot(d, d)
        ok = (a < c) & inr & (j != i) & (pairs[jj] > 0) & (d2 > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            wj = 1.0 / (pairs[jj].astype(np.float64) * d2)
            acc = acc + np.where(ok[:, None], hist[jj].astype(np.float64) * wj[:, None], 0.0)
        m += ok
    with np.errstate(divide="ignore", invalid="ignore"):
        own = np.where(pairs[:, None] > 0, hist.astype(np.float64) / pairs[:, None].astype(np.float64), 0.0)
        F = own + np.where(m[:, None] > 0, acc / m[:, None].astype(np.float64), 0.0)
        desc = np.zeros((n, BINS), np.float32)
        for g in range(3):
            G = F[:, 11 * g:11 * g + 11]
            tot = G[:, 0].copy()
            for b in range(1, 11):
                tot = tot + G[:, b]
            desc[:, 11 * g:11 * g + 11] = np.where(tot[:, None] == 0, 0.0, G / tot[:, None]).astype(np.float32)
    valid = (~(Nn == 0).all(1) & (pairs >= 3)).astype(np.uint8)
    return desc, valid, int((valid == 0).sum())


def descriptors(points, normal, k, radius, oriented=True):
    """brute-force neighbours (cloud_knn_ref.knn32: estd_cloud_knn's lists to the bit), then spfh and fpfh -> dict"""
    _, index, count = knn32(points, points, k, radius)
    hist, pairs = spfh(points, normal, index, count, oriented)
    desc, valid, invalid = fpfh(points, normal, index, count, hist, pairs)
    return dict(index=index, count=count, hist=hist, pairs=pairs, desc=desc, valid=valid, invalid=invalid)


# ------------------------------------------------------------------------------------------------------------ matching
def d2_chain(a, b):
    """the header's fma chain over the last axis of two broadcastable fp32 arrays [..., 33] -> float32 [...]"""
    e = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float32)
    d2 = (e[..., 0] * e[..., 0]).astype(np.float32)
    for c in range(1, BINS):
        d2 = fma32(e[..., c], d2)
    return d2


def _pick(d2, cols):
    """best and second of one row's candidates: d2 [c] float32, cols [c] ascending indices"""
    if d2.shape[0] == 0:
        return -1, np.float32(np.inf), np.float32(np.inf)
    o = np.lexsort((cols, d2))
    return int(cols[o[0]]), d2[o[0]], (d2[o[1]] if o.shape[0] > 1 else np.float32(np.inf))


def match(a, b, a_valid=None, b_valid=None, chunk=32):
    """every row of a against every valid row of b, exactly -> (index int32 [m], d2 float32 [m], d2_second float32 [m])"""
    a, b = np.asarray(a, np.float32).reshape(-1, BINS), np.asarray(b, np.float32).reshape(-1, BINS)
    m = a.shape[0]
    cols = np.arange(b.shape[0]) if b_valid is None else np.nonzero(np.asarray(b_valid))[0]
    index, d2, second = np.full(m, -1, np.int32), np.full(m, np.inf, np.float32), np.full(m, np.inf, np.float32)
    for r0 in range(0, m, chunk):
        D = d2_chain(a[r0:r0 + chunk, None, :], b[None, cols, :]) if cols.shape[0] else np.zeros((min(chunk, m - r0), 0), np.float32)
        for r in range(D.shape[0]):
            if a_valid is None or a_valid[r0 + r]:
                index[r0 + r], d2[r0 + r], second[r0 + r] = _pick(D[r], cols)
    return index, d2, second


def match_fast(a, b, a_valid=None, b_valid=None, top=8):
    """the same result for large inputs (see the module docstring)"""
    a, b = np.asarray(a, np.float32).reshape(-1, BINS), np.asarray(b, np.float32).reshape(-1, BINS)
    m = a.shape[0]
    cols = np.arange(b.shape[0]) if b_valid is None else np.nonzero(np.asarray(b_valid))[0]
    if cols.shape[0] <= top + 1:
        return match(a, b, a_valid, b_valid)
    A, B = a.astype(np.float64), b[cols].astype(np.float64)
    D = (A * A).sum(1)[:, None] + (B * B).sum(1)[None] - 2.0 * (A @ B.T)
    part = np.argpartition(D, top, 1)[:, :top + 1]
    part = np.take_along_axis(part, np.argsort(np.take_along_axis(D, part, 1), 1), 1)        # ascending in the float64 distance
    near = np.sort(part[:, :top], 1)                                                          # ascending in the index, for the ties
    exact = d2_chain(a[:, None, :], b[cols[near]])
    ninth = np.take_along_axis(D, part[:, top:top + 1], 1)[:, 0]
    index, d2, second = np.full(m, -1, np.int32), np.full(m, np.inf, np.float32), np.full(m, np.inf, np.float32)
    for r in range(m):
        if a_valid is not None and not a_valid[r]:
            continue
        index[r], d2[r], second[r] = _pick(exact[r], cols[near[r]])
        if not ninth[r] > float(second[r]) * (1.0 + 1e-4) + 1e-9:                             # not clearly behind: the whole row, exactly
            index[r], d2[r], second[r] = _pick(d2_chain(a[r][None, :], b[cols]), cols)
    return index, d2, second


def mutual_pairs(a, b, a_valid=None, b_valid=None, fn=match_fast):
    """registration.match_features(mutual=True) -> (pairs int64 [C,2], d2 [C])"""
    ab, d2, _ = fn(a, b, a_valid, b_valid)
    ba, _, _ = fn(b, a, b_valid, a_valid)
    rows = np.nonzero((ab >= 0) & (ba[np.maximum(ab, 0)] == np.arange(ab.shape[0])))[0] if ba.shape[0] else np.zeros(0, np.int64)
    return np.stack([rows, ab[rows].astype(np.int64)], 1).astype(np.int64).reshape(-1, 2), d2[rows]


# ------------------------------------------------------------------------------------------------------------ hypotheses
def _frame(a, b, c):
    with np.errstate(divide="ignore", invalid="ignore"):
        ab = b - a
        l1 = np.sqrt(_dot(ab, ab))
        e1 = ab / l1[:, None]
        nrm = _cross(e1, c - a)
        l3 = np.sqrt(_dot(nrm, nrm))
        e3 = nrm / l3[:, None]
        e2 = _cross(e3, e1)
    return e1, e2, e3, (l1 != 0) & (l3 != 0)


def ransac(P, Q, hypotheses, seed, dist_max, edge_ratio, chunk=128):
    """-> dict(count int32 [H], status uint8 [H], ssq float64 [H], ssq_bound [H], T float64 [H,12], hypothesis, best_count)"""
    P, Q = np.asarray(P, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(Q, np.float32).astype(np.float64).reshape(-1, 3)
    C, H = P.shape[0], int(hypotheses)
    count, status, ssq = np.zeros(H, np.int32), np.zeros(H, np.uint8), np.zeros(H)
    bound, T = np.zeros(H), np.zeros((H, 12))
    out = dict(count=count, status=status, ssq=ssq, ssq_bound=bound, T=T, hypothesis=-1, best_count=0)
    if H == 0:
        return out
    if C == 0:
        status[:] = 1
        return out
    h = np.arange(H, dtype=np.uint64)
    c0, c1, c2 = [(MS.h64(seed, h, j) % np.uint64(C)).astype(np.int64) for j in range(3)]
    rep = (c0 == c1) | (c0 == c2) | (c1 == c2)
    pa, pb, pc, qa, qb, qc = P[c0], P[c1], P[c2], Q[c0], Q[c1], Q[c2]
    ln = lambda x, y: np.sqrt(_dot(y - x, y - x))                                            # noqa: E731
    er = float(edge_ratio)
    edges = np.zeros(H, bool)
    for (x, y), (s, t) in (((pa, pb), (qa, qb)), ((pb, pc), (qb, qc)), ((pc, pa), (qc, qa))):
        lp, lq = ln(x, y), ln(s, t)
        edges |= (lp < er * lq) | (lq < er * lp)
    e1p, e2p, e3p, okp = _frame(pa, pb, pc)
    e1q, e2q, e3q, okq = _frame(qa, qb, qc)
    with np.errstate(invalid="ignore"):
        R = (e1q[:, :, None] * e1p[:, None, :] + e2q[:, :, None] * e2p[:, None, :]) + e3q[:, :, None] * e3p[:, None, :]
        cp, cq = ((pa + pb) + pc) / 3.0, ((qa + qb) + qc) / 3.0
        t = cq - ((R[:, :, 0] * cp[:, None, 0] + R[:, :, 1] * cp[:, None, 1]) + R[:, :, 2] * cp[:, None, 2])
    degenerate = ~(okp & okq) | ~np.isfinite(R).all((1, 2)) | ~np.isfinite(t).all(1)
    status[:] = np.where(rep, 1, np.where(edges, 2, np.where(degenerate, 3, 0)))
    scored = np.nonzero(status == 0)[0]
    T[scored] = np.concatenate([R[scored], t[scored][:, :, None]], 2).reshape(-1, 12)
    d2max = float(dist_max) * float(dist_max)
    pad = (-C) % 64
    x = np.arange(64)
    for s0 in range(0, scored.shape[0], chunk):
        hs = scored[s0:s0 + chunk]
        Rh, th = R[hs][:, None], t[hs][:, None]                                                 # [c,1,3,3], [c,1,3]
        prod = Rh * P[None, :, None, :]                                                         # R_ij p_j
        mv = ((prod[..., 0] + prod[..., 1]) + prod[..., 2]) + th
        e = mv - Q[None]
        r2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        inl = r2 <= d2max
        count[hs] = inl.sum(1)
        S = np.abs(prod).sum(-1) + np.abs(th)
        err_e = 4 * U64 * S + U64 * np.abs(e)
        err = (2 * np.abs(e) * err_e).sum(-1) + 3 * U64 * r2
        lanes = np.pad(np.where(inl, r2, 0.0), ((0, 0), (0, pad))).reshape(hs.shape[0], -1, 64)
        acc = np.zeros((hs.shape[0], 64))
        for blk in range(lanes.shape[1]):
            acc = acc + lanes[:, blk]
        for k in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, x ^ k]
        ssq[hs] = acc[:, 0]
        bound[hs] = C_ROUTE * 2 * (np.where(inl, err, 0.0).sum(1) + (lanes.shape[1] + 7) * U64 * acc[:, 0])
    if scored.shape[0]:
        best = scored[np.lexsort((scored, -count[scored].astype(np.int64)))[0]]
        out.update(hypothesis=int(best), best_count=int(count[best]))
    return out


def winner_T(r):
    T = np.eye(4)
    if r["hypothesis"] >= 0:
        T[:3, :4] = r["T"][r["hypothesis"]].reshape(3, 4)
    return T


# ------------------------------------------------------------------------------------------------------------ the whole chain
def chain(src, src_normal, tgt, tgt_normal, voxel=VOXEL, k=32, hypotheses=HYPOTHESES, seed=0, edge_ratio=0.9, oriented=True, min_count=20):
    """registration.register_global(refine=None) on clouds that are thinned already -> dict(T_global, hypothesis, count, pairs, fitness, reason)"""
    fs = descriptors(src, src_normal, k, 5.0 * voxel, oriented)
    ft = descriptors(tgt, tgt_normal, k, 5.0 * voxel, oriented)
    pairs, _ = mutual_pairs(fs["desc"], ft["desc"], fs["valid"], ft["valid"])
    r = ransac(np.asarray(src, np.float32)[pairs[:, 0]], np.asarray(tgt, np.float32)[pairs[:, 1]], hypotheses, seed, 1.5 * voxel, edge_ratio)
    ok = r["best_count"] >= min_count
    return dict(T_global=winner_T(r) if ok else np.eye(4), hypothesis=r["hypothesis"], count=r["best_count"], pairs=int(pairs.shape[0]),
                fitness=r["best_count"] / max(1, pairs.shape[0]), reason="global" if ok else "inliers", match=pairs, ransac=r)


def staged(voxel=VOXEL):
    return (4.0 * voxel, 2.0 * voxel, voxel)


def refine(src, target, T, voxel=VOXEL, metric="plane"):
    """rigid_align_ref.refine from the global stage's transform, with register_global's default stages"""
    return RA.refine(src, target, init=T, metric=metric, dist_max=staged(voxel), pivot=RA.target_pivot(target))


# ------------------------------------------------------------------------------------------------------------ the fixture
BOXES = (((0.50, 0.35, 0.40), 20.0, (0.80, 0.70)), ((0.30, 0.60, 0.70), -35.0, (1.70, 1.30)), ((0.45, 0.25, 0.25), 60.0, (1.50, 0.50)))
SPHERE = ((0.60, 1.50, 0.30), 0.30)
ROOM = (2.4, 2.0, 1.2)


def _quad(a, b, c, d):
    return [a, b, c, d], [(0, 1, 2), (0, 2, 3)]


def scene_mesh():
    """-> (xyz float32 [V,3], faces int32 [F,3]): every triangle wound so that its normal points into the room / out of the object"""
    parts = []
    X, Y, Z = ROOM
    parts.append(_quad((0, 0, 0), (X, 0, 0), (X, Y, 0), (0, Y, 0)))                          # floor, +z
    parts.append(_quad((0, 0, 0), (0, Y, 0), (0, Y, Z), (0, 0, Z)))                          # wall x = 0, +x
    parts.append(_quad((0, 0, 0), (0, 0, Z), (X, 0, Z), (X, 0, 0)))                          # wall y = 0, +y
    for (sx, sy, sz), yaw, (cx, cy) in BOXES:
        c, s = np.cos(np.radians(yaw)), np.sin(np.radians(yaw))
        corner = lambda u, v, w: (cx + c * u * sx / 2 - s * v * sy / 2, cy + s * u * sx / 2 + c * v * sy / 2, w * sz)      # noqa: E731
        b = [corner(u, v, 0) for u, v in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        t = [corner(u, v, 1) for u, v in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        parts.append(_quad(t[0], t[1], t[2], t[3]))                                         # top
        for i in range(4):
            j = (i + 1) % 4
            parts.append(_quad(b[i], b[j], t[j], t[i]))                                     # sides, outwards
    sv, sf = MD.icosphere(2, SPHERE[1])
    sv = sv.astype(np.float64) + np.asarray(SPHERE[0])
    tri = sv[sf]
    out = _dot(_cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), tri.mean(1) - np.asarray(SPHERE[0])) > 0
    sf = np.where(out[:, None], sf, sf[:, ::-1])
    parts.append((list(sv), [tuple(f) for f in sf]))
    xyz, faces = [], []
    for v, f in parts:
        faces += [tuple(i + len(xyz) for i in t) for t in f]
        xyz += list(v)
    return np.asarray(xyz, np.float32), np.asarray(faces, np.int32)


def sample(n, seed):
    """``n`` points of the scene by area with their face normals (float64 draws, rounded once) -> (xyz [n,3] float64, normal [n,3] float64)"""
    xyz, faces = scene_mesh()
    nrm, area = RA.face_normals(xyz, faces)
    rng = np.random.RandomState(seed)
    f = rng.choice(faces.shape[0], size=n, p=area / area.sum())
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fold = u + v > 1
    u, v = np.where(fold, 1 - u, u), np.where(fold, 1 - v, v)
    t = xyz.astype(np.float64)[faces.astype(np.int64)][f]
    return t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0]), np.asarray(nrm, np.float64)[f]


def thin(points, normal, voxel):
    """voxel_downsample's rule in float64: the mean of each occupied cell (cells from the cloud's own minimum), unit normals"""
    p = np.asarray(points, np.float64)
    key = np.floor((p - p.min(0)) / voxel).astype(np.int64)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    out, nrm = np.zeros((cnt.shape[0], 3)), np.zeros((cnt.shape[0], 3))
    np.add.at(out, inv, p)
    np.add.at(nrm, inv, np.asarray(normal, np.float64))
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    return (out / cnt[:, None]).astype(np.float32), np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), 0.0).astype(np.float32)


def _axis_angle(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def motion(name):
    """T_true [4,4]: the source clouds are the scene moved by its inverse, so registering them to the scene must give it back"""
    T = np.eye(4)
    if name == "z90":
        T[:3, :3], T[:3, 3] = _axis_angle((0, 0, 1), 90.0), (1.0, 0.0, 0.0)
    elif name == "skew175":
        T[:3, :3], T[:3, 3] = _axis_angle((1, 2, 3), 175.0), np.array([2.0, -1.0, 2.0])
    else:
        rng = np.random.RandomState(int(name[4:]))
        T[:3, :3] = _axis_angle(rng.normal(size=3), rng.uniform(30.0, 180.0))
        T[:3, 3] = rng.uniform(-2.0, 2.0, size=3)
    return T


MOTIONS = ("z90", "skew175", "seed7")
_FIXTURE = {}


def fixture(name, voxel=VOXEL, raw=False):
    """-> dict(src, src_normal: the thinned source in its own frame; tgt, tgt_normal: the thinned target (other samples, the scene's frame);
    T_true; mesh; ``raw=True`` adds the samples before thinning, fp32).  Built once per motion."""
    key = (name, voxel)
    if key not in _FIXTURE:
        n = int(4.0 / (voxel * voxel) * 14.0)
        T = motion(name)
        Ti = np.linalg.inv(T)
        ps, ns = sample(n, 11)
        pt, nt = sample(n, 12)
        ps, ns = (ps @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32), (ns @ Ti[:3, :3].T).astype(np.float32)
        pt, nt = pt.astype(np.float32), nt.astype(np.float32)
        s, sn = thin(ps, ns, voxel)
        t, tn = thin(pt, nt, voxel)
        xyz, faces = scene_mesh()
        _FIXTURE[key] = dict(src=s, src_normal=sn, tgt=t, tgt_normal=tn, T_true=T, mesh=dict(xyz=xyz, faces=faces),
                             raw=dict(src=ps, src_normal=ns, tgt=pt, tgt_normal=nt))
    return _FIXTURE[key]


def faces_seen(xyz, faces, depths, poses, K, tol=0.02):
    """the triangles whose centroid some camera saw: it projects into the image and the depth map shows it there within ``tol`` metres"""
    c = xyz.astype(np.float64)[faces.astype(np.int64)].mean(1)
    seen = np.zeros(faces.shape[0], bool)
    for depth, pose in zip(depths, poses):
        H, W = depth.shape
        pc = (c - pose[:3, 3]) @ pose[:3, :3]                                                 # world -> camera
        z = pc[:, 2]
        uv = pc @ np.asarray(K, np.float64).T
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = np.rint(uv[:, 0] / z), np.rint(uv[:, 1] / z)
        ok = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
        seen |= ok & (np.abs(depth[vi, ui] - z) < tol)
    return seen


def room_before_the_cameras(tilt=35.0, centre=(0.0, 0.0, 1.75), cut=True):
    """the scene's mesh where tests/run_stream_ref.py's cameras (near the origin, looking along +z) see it from inside and obliquely, so
    that floor, walls and the sides of the boxes all show: turned about x by 180 + ``tilt`` degrees (a rotation: windings and normals
    stay), the middle of the room at ``centre`` -> (xyz float32 [V,3], faces int32 [F,3]).  ``cut``: the same surface in triangles of
    some 0.2 m (1 784 of them) instead of the 356"""
    xyz, faces = scene_mesh()
    for _ in range(4 if cut else 0):         # the large triangles of floor, walls and boxes cut (in their planes) to edges of some 0.2 m,
        area = RA.face_normals(xyz, faces)[1]                    # so that "the triangles a camera saw" follows the field of view
        big = area > 0.02
        if not big.any():
            break
        cut_xyz, cut = RA.subdivided(xyz, faces[big])
        xyz, faces = cut_xyz, np.concatenate([faces[~big], cut]).astype(np.int32)
    Rx = _axis_angle((1, 0, 0), 180.0 + tilt)
    p = (xyz.astype(np.float64) - np.array([ROOM[0] / 2, ROOM[1] / 2, ROOM[2] / 2])) @ Rx.T + np.asarray(centre, np.float64)
    return p.astype(np.float32), faces


def render_depth(xyz, faces, pose, K, H, W, chunk=4096, hit_faces=None):
    """z-depth maps [H,W] (pixel centres on integers, 0 where no triangle is hit) of a mesh from the camera-to-world ``pose``: every ray
    against every triangle (Moeller-Trumbore) in float64; the ray's camera-frame z is 1, so its parameter is the z-depth.
    ``hit_faces``: a bool array [F] in which the triangles that some pixel shows are marked"""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = ((np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T) @ pose[:3, :3].T).reshape(-1, 3)
    o = np.asarray(pose, np.float64)[:3, 3]
    tri = xyz.astype(np.float64)[faces.astype(np.int64)]
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    s = o - a                                                                                 # [F,3]
    sxe1 = np.cross(s, e1)
    out = np.zeros(rays.shape[0])
    for i in range(0, rays.shape[0], chunk):
        d = rays[i:i + chunk, None, :]                                                        # [c,1,3]
        pv = np.cross(d, e2[None])
        det = (pv * e1[None]).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            bu = (pv * s[None]).sum(-1) * inv
            bv = (d * sxe1[None]).sum(-1) * inv
            t = (e2 * sxe1).sum(-1)[None] * inv
        hit = (np.abs(det) > 1e-12) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0)
        tt = np.where(hit, t, np.inf)
        best = tt.min(1)
        out[i:i + chunk] = np.where(np.isfinite(best), best, 0.0)
        if hit_faces is not None:
            hit_faces[np.unique(tt.argmin(1)[np.isfinite(best)])] = True
    return out.reshape(H, W)


def error(T, T_true):
    """(metres at the scene's centre, radians): how far T puts the source's image of the scene's centre from where T_true puts it"""
    Ti = np.linalg.inv(np.asarray(T_true, np.float64))
    return RA.transform_error(T, T_true, Ti[:3, :3] @ SCENE_CENTRE + Ti[:3, 3])
