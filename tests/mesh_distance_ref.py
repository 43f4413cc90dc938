"""The point-to-triangle-mesh distance of include/estd_hip.h (estd_mesh_nearest; csrc/mesh/mesh_distance.hip) in numpy float64: the brute
force over all faces, a first-order fp32 rounding bound for the stated operation order, and the comparison the GPU tests hold the
kernels to.  Needs no device.

The pair.  ``closest64`` runs the header's tri_closest -- the region tests of Ericson 5.1.5 in the header's order -- in float64, on
every (query, face) pair at once.  Beside every value x it carries e(x), a bound of |the fp32 value - x| to first order in
u = 2^-24, by the usual running error analysis: the inputs are fp32 numbers, e = 0; a plain operation or a division z = x op y adds
u |z| to what it inherits, an fma z = x y + c likewise:
    e(x - y) = e(x) + e(y) + u |z|        e(x y) = |x| e(y) + |y| e(x) + u |z|        e(x y + c) = |x| e(y) + |y| e(x) + e(c) + u |z|
    e(x / y) = e(x) / |y| + |z| e(y) / |y| + u |z|
The region is the one the float64 values select.  Where fp32 selects another one, the pair sits within its rounding error of a region
boundary, and across every boundary the formulas of the two regions agree (v = d1 / (d1 - d3) is 0 where d1 = 0 and 1 where d3 = 0;
the interior's v = vb / (va + vb + vc) is d1 / (d1 - d3) and w is 0 where vc = 0, and so on round the triangle): a flipped test
changes (v, w) by no more than the errors already carried, to first order.  Underflow is left out: the cases stay far from it.
    d2 = fma(dx, dx, fma(dy, dy, dz dz)) with d = q - p gets e(d2) from the same rules;  dist = sqrt(d2), correctly rounded:
    e(dist) = e(d2) / (sqrt(d2 + e(d2)) + sqrt(d2)) + u dist            (the exact difference of the two roots, no linearisation at 0)
The minimum over the faces is 1-Lipschitz in each of them, so for the face f the device reports and the face g the reference finds
    | dist_device - dist64(g) | <= max(e(dist(f)), e(dist(g)))      and      dist64(f) - dist64(g) <= e(dist(f)) + e(dist(g)).
``compare`` allows C = 2 times these bounds, the project's usual constant.  A face index is accepted iff the float64 distance to THAT
face is within the allowance of the float64 minimum: two triangles that share the nearest edge are equidistant in exact arithmetic, the
index cannot be pinned further.  Found or not: r2 = fl(max_dist^2) is off by u/2 relative in the distance, so within the allowance
+ u max_dist of max_dist either answer is taken (and then checked as what it is); outside it the answer is pinned.  No query is left
out.  In EXACT_CASES every operation is exact in fp32 (dyadic coordinates, dyadic quotients): there the bits are pinned, the index too.

``nearest_planted`` is the float64 chain with one of MISTAKES planted, rounded to fp32 as a device result would be: the tests show
that ``compare`` rejects each of them.
"""
import numpy as np

U = 2.0 ** -24
C = 2.0                     # the allowance: C times the derived bound
MISTAKES = ("swapped_edge_region", "strict_radius", "largest_index_on_ties")


# ------------------------------------------------------------------------------------------------ values with their error bounds
def _v(x):
    return (np.asarray(x, np.float64), 0.0)


def _sub(x, y):
    z = x[0] - y[0]
    return z, x[1] + y[1] + U * np.abs(z)


def _add(x, y):
    z = x[0] + y[0]
    return z, x[1] + y[1] + U * np.abs(z)


def _mul(x, y):
    z = x[0] * y[0]
    return z, np.abs(x[0]) * y[1] + np.abs(y[0]) * x[1] + U * np.abs(z)


def _fma(x, y, c):
    z = x[0] * y[0] + c[0]
    return z, np.abs(x[0]) * y[1] + np.abs(y[0]) * x[1] + c[1] + U * np.abs(z)


def _neg(x):
    return -x[0], x[1]


def _div(x, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        z = x[0] / y[0]
        return z, x[1] / np.abs(y[0]) + np.abs(z) * y[1] / np.abs(y[0]) + U * np.abs(z)


def _dot(x, y):
    return _fma(x[0], y[0], _fma(x[1], y[1], _mul(x[2], y[2])))


def _pick(conds, choices, default):
    val = np.select(conds, [np.broadcast_to(c[0], conds[0].shape) for c in choices], default[0])
    err = np.select(conds, [np.broadcast_to(c[1], conds[0].shape) for c in choices], default[1])
    return val, err


def closest64(q, a, b, c, mistake=None):
    """tri_closest on broadcastable arrays [..., 3] -> dict(v, w, p [..., 3], d2, dist, e_d2, e_dist, region)"""
    q, a, b, c = (np.asarray(x, np.float64) for x in (q, a, b, c))
    comp = lambda x: [_v(x[..., j]) for j in range(3)]
    Q, A, B, Cc = comp(q), comp(a), comp(b), comp(c)
    vsub = lambda x, y: [_sub(x[j], y[j]) for j in range(3)]
    ab, ac, ap, bp, cp = vsub(B, A), vsub(Cc, A), vsub(Q, A), vsub(Q, B), vsub(Q, Cc)
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = _fma(d1, d4, _neg(_mul(d3, d2))), _fma(d5, d2, _neg(_mul(d1, d6))), _fma(d3, d6, _neg(_mul(d5, d4)))
    e43, e56 = _sub(d4, d3), _sub(d5, d6)
    shape = np.broadcast(d1[0], vc[0]).shape
    full = lambda m: np.broadcast_to(m, shape)
    rA = full((d1[0] <= 0) & (d2[0] <= 0))
    rB = full((d3[0] >= 0) & (d4[0] <= d3[0])) & ~rA
    rAB = full((vc[0] <= 0) & (d1[0] >= 0) & (d3[0] <= 0)) & ~(rA | rB)
    rC = full((d6[0] >= 0) & (d5[0] <= d6[0])) & ~(rA | rB | rAB)
    rAC = full((vb[0] <= 0) & (d2[0] >= 0) & (d6[0] <= 0)) & ~(rA | rB | rAB | rC)
    rBC = full((va[0] <= 0) & (e43[0] >= 0) & (e56[0] >= 0)) & ~(rA | rB | rAB | rC | rAC)
    if mistake == "swapped_edge_region":          # the edge AC's quotient where the edge AB's belongs, and the other way round
        rAB, rAC = rAC, rAB
    zero, one = (np.zeros(shape), 0.0), (np.ones(shape), 0.0)
    v_ab = _div(d1, _sub(d1, d3))
    w_ac = _div(d2, _sub(d2, d6))
    w_bc = _div(e43, _add(e43, e56))
    v_bc = _sub(one, w_bc)
    denom = _div(one, _add(_add(va, vb), vc))
    v_in, w_in = _mul(vb, denom), _mul(vc, denom)
    conds = [rA, rB, rAB, rC, rAC, rBC]
    v = _pick(conds, [zero, one, v_ab, zero, zero, v_bc], v_in)
    w = _pick(conds, [zero, zero, zero, one, w_ac, w_bc], w_in)
    p = [_fma(w, ac[j], _fma(v, ab[j], A[j])) for j in range(3)]
    d = [_sub(Q[j], p[j]) for j in range(3)]
    dd = _fma(d[0], d[0], _fma(d[1], d[1], _mul(d[2], d[2])))
    dist = np.sqrt(dd[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.sqrt(dd[0] + dd[1]) + dist
        e_dist = np.where(den > 0, dd[1] / den, 0.0) + U * dist
    region = np.select(conds, [0, 1, 2, 3, 4, 5], 6)
    return dict(v=v[0], w=w[0], p=np.stack([x[0] for x in p], -1), d2=dd[0], dist=dist, e_d2=dd[1], e_dist=e_dist, region=region)


# ------------------------------------------------------------------------------------------------ the mesh
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def valid_faces(xyz, faces):
    """the header's validity, bit for bit: indices in range, finite vertices, and the fp32 normal not zero -- each component two
    products rounded to fp32 and their difference (formed in float64 from fp32 operands: it is 0 there iff it is 0 exactly), n . n by
    the header's fma nesting"""
    xyz, faces = np.asarray(xyz, np.float32), np.asarray(faces, np.int64)
    V = xyz.shape[0]
    ok = ((faces >= 0) & (faces < V)).all(1) if faces.size else np.zeros(0, bool)
    tri = xyz[np.where(ok[:, None], faces, 0)].astype(np.float64) if V else np.zeros((faces.shape[0], 3, 3))
    ok = ok & np.isfinite(tri).all((1, 2))
    tri = np.where(ok[:, None, None], tri, 0.0)
    ab, ac = f32(tri[:, 1] - tri[:, 0]).astype(np.float64), f32(tri[:, 2] - tri[:, 0]).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        fma = lambda x, y, z: f32(x * y + z).astype(np.float64)
        mul = lambda x, y: f32(x * y).astype(np.float64)
        nx = f32(mul(ab[:, 1], ac[:, 2]) - mul(ab[:, 2], ac[:, 1])).astype(np.float64)
        ny = f32(mul(ab[:, 2], ac[:, 0]) - mul(ab[:, 0], ac[:, 2])).astype(np.float64)
        nz = f32(mul(ab[:, 0], ac[:, 1]) - mul(ab[:, 1], ac[:, 0])).astype(np.float64)
        nn = fma(nx, nx, fma(ny, ny, mul(nz, nz)))
    return ok & ~(nn == 0)


def brute_force(q, xyz, faces, mistake=None, chunk=64):
    """every query against every face -> dict(dist [M,F] (inf for an invalid face), e_dist [M,F], valid [F])"""
    q, xyz, faces = np.asarray(q, np.float32), np.asarray(xyz, np.float32), np.asarray(faces, np.int64)
    valid = valid_faces(xyz, faces)
    M, F = q.shape[0], faces.shape[0]
    dist, e = np.full((M, F), np.inf), np.zeros((M, F))
    keep = np.nonzero(valid)[0]
    if keep.size and M:
        tri = xyz[faces[keep]].astype(np.float64)
        for i in range(0, M, chunk):
            r = closest64(q[i:i + chunk, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], mistake)
            dist[i:i + chunk, keep], e[i:i + chunk, keep] = r["dist"], r["e_dist"]
    return dict(dist=dist, e_dist=e, valid=valid)


def nearest64(q, xyz, faces, bf=None):
    """-> (dmin [M] float64 (inf without a valid face), face [M]: the smallest index attaining it (-1 without), the brute force)"""
    bf = brute_force(q, xyz, faces) if bf is None else bf
    D = bf["dist"]
    if D.shape[1] == 0:
        return np.full(D.shape[0], np.inf), np.full(D.shape[0], -1, np.int64), bf
    face = np.argmin(D, 1)
    dmin = D[np.arange(D.shape[0]), face]
    return dmin, np.where(np.isfinite(dmin), face, -1), bf


def nearest_planted(q, xyz, faces, max_dist, mistake=None):
    """the float64 chain rounded to fp32 as a device result, with one of MISTAKES planted -> the dict ``compare`` takes"""
    assert mistake is None or mistake in MISTAKES, mistake
    bf = brute_force(q, xyz, faces, mistake if mistake == "swapped_edge_region" else None)
    D = bf["dist"]
    M, F = D.shape
    face, dist = np.full(M, -1, np.int32), np.full(M, np.float32(max_dist), np.float32)
    if F:
        d32 = D.astype(np.float32)
        best = d32.min(1)
        for i in range(M):
            ties = np.nonzero(d32[i] == best[i])[0]
            f = ties[-1] if mistake == "largest_index_on_ties" else ties[0]
            found = best[i] < np.float32(max_dist) if mistake == "strict_radius" else best[i] <= np.float32(max_dist)
            if np.isfinite(best[i]) and found:
                face[i], dist[i] = f, best[i]
    return dict(dist=dist, face=face, invalid=int((~bf["valid"]).sum()))


def compare(got, case, label="", bf=None):
    """``got``: dict(dist [M] float32, face [M], invalid, optionally bary [M,2], closest [M,3]); ``case``: dict(q, xyz, faces, max_dist)
    -> the figures: the largest share of the allowance used by a distance and by a face, the queries found.  Raises AssertionError."""
    q, xyz, faces, max_dist = np.asarray(case["q"], np.float32), np.asarray(case["xyz"], np.float32), np.asarray(case["faces"], np.int64), float(case["max_dist"])
    dmin, ref_face, bf = nearest64(q, xyz, faces, bf)
    D, E, valid = bf["dist"], bf["e_dist"], bf["valid"]
    M = q.shape[0]
    dist, face = np.asarray(got["dist"]), np.asarray(got["face"]).astype(np.int64)
    assert dist.shape == (M,) and face.shape == (M,) and dist.dtype == np.float32, (label, dist.shape, face.shape, dist.dtype)
    assert int(got["invalid"]) == int((~valid).sum()), "%s: %d invalid faces reported, %d expected" % (label, int(got["invalid"]), int((~valid).sum()))
    md32 = float(np.float32(max_dist))
    worst_d = worst_f = 0.0
    found = 0
    for i in range(M):
        f, g = int(face[i]), int(ref_face[i])
        assert f == -1 or (0 <= f < faces.shape[0] and valid[f]), "%s: query %d reports face %d, which is not a valid face" % (label, i, f)
        e_g = E[i, g] if g >= 0 else 0.0
        allow = C * (max(e_g, E[i, f]) if f >= 0 else e_g)
        margin = allow + U * md32
        if dmin[i] > md32 + margin:
            assert f == -1, "%s: query %d found face %d at %.9g, the nearest is %.9g > max_dist %.9g" % (label, i, f, dist[i], dmin[i], md32)
        elif dmin[i] < md32 - margin:
            assert f >= 0, "%s: query %d found nothing, face %d is at %.9g <= max_dist %.9g" % (label, i, g, dmin[i], md32)
        if f == -1:
            assert dist[i] == np.float32(max_dist), "%s: query %d found nothing but reports %.9g, not max_dist" % (label, i, dist[i])
            for k, n in (("bary", 2), ("closest", 3)):
                assert got.get(k) is None or not np.asarray(got[k])[i].any(), "%s: query %d found nothing but %s is not zero" % (label, i, k)
            continue
        found += 1
        err = abs(float(dist[i]) - dmin[i])
        assert err <= allow, "%s: query %d: dist %.9g, reference %.9g: off by %.3g, allowed %.3g" % (label, i, dist[i], dmin[i], err, allow)
        gap, allow_f = D[i, f] - dmin[i], C * (E[i, f] + e_g)
        assert gap <= allow_f, "%s: query %d: face %d is %.3g further than face %d, allowed %.3g" % (label, i, f, gap, g, allow_f)
        if allow > 0:
            worst_d = max(worst_d, err / allow)
        if allow_f > 0:
            worst_f = max(worst_f, gap / allow_f)
        a, b, c = (xyz[faces[f, j]].astype(np.float64) for j in range(3))
        scale = 4.0 * U * (np.abs(a) + np.abs(b - a) + np.abs(c - a)).max()
        if got.get("bary") is not None and got.get("closest") is not None:
            v, w = (float(x) for x in np.asarray(got["bary"])[i])
            p = a + v * (b - a) + w * (c - a)
            assert -4 * U <= v and -4 * U <= w and v + w <= 1 + 8 * U, "%s: query %d: bary (%r, %r) leaves the triangle" % (label, i, v, w)
            assert np.abs(p - np.asarray(got["closest"])[i]).max() <= scale, "%s: query %d: closest is not the point of its bary" % (label, i)
        if got.get("closest") is not None:
            back = np.linalg.norm(q[i].astype(np.float64) - np.asarray(got["closest"])[i].astype(np.float64))
            assert abs(back - float(dist[i])) <= allow + 2 * scale, "%s: query %d: closest is %.9g away, dist says %.9g" % (label, i, back, dist[i])
    return dict(dist=worst_d, face=worst_f, found=found, queries=M, invalid=int((~valid).sum()))


# ------------------------------------------------------------------------------------------------ meshes
def icosphere(level=2, radius=1.0):
    """-> (xyz float32 [V,3] on the sphere, faces int32 [F,3]), F = 20 x 4^level"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(np.float32), np.asarray(f, np.int32)


def unit_cube():
    """the surface of [0, 1]^3 as 12 triangles"""
    xyz = np.asarray([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return xyz, np.asarray([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)


def square(edge=1.0):
    """[0, edge]^2 in the plane z = 0 as two triangles"""
    return np.asarray([(0, 0, 0), (edge, 0, 0), (edge, edge, 0), (0, edge, 0)], np.float32), np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)


def soup(n, rng, size=0.08, lo=0.0, hi=1.0):
    """n separate random triangles of about ``size`` in [lo, hi]^3"""
    centre = rng.uniform(lo, hi, (n, 1, 3))
    xyz = (centre + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    return xyz, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


# ------------------------------------------------------------------------------------------------ cases
# the right triangle a = (0,0,0), b = (4,0,0), c = (0,4,0) and one query in each of Ericson's seven regions; every fp32 operation of
# tri_closest is exact on them (small integers, quotients 1/2, 1/4 and 1/16 x small integers): the bits are pinned
RIGHT = (np.asarray([(0, 0, 0), (4, 0, 0), (0, 4, 0)], np.float32), np.asarray([(0, 1, 2)], np.int32))
SEVEN = {  # region: (query, (v, w), closest, d2)
    "A": ((-1, -2, 2), (0, 0), (0, 0, 0), 9.0),
    "B": ((6, -1, 0), (1, 0), (4, 0, 0), 5.0),
    "C": ((-1, 7, 2), (0, 1), (0, 4, 0), 14.0),
    "AB": ((1, -3, 0), (0.25, 0), (1, 0, 0), 9.0),
    "AC": ((-2, 2, 1), (0, 0.5), (0, 2, 0), 5.0),
    "BC": ((3, 3, 1), (0.5, 0.5), (2, 2, 0), 3.0),
    "interior": ((1, 2, -3), (0.25, 0.5), (1, 2, 0), 9.0),
}


def exact_case(name):
    """-> (case dict, expected dict(dist float32 [M], face [M], bary [M,2], closest [M,3])), all bits pinned"""
    if name == "seven":
        keys = list(SEVEN)
        q = np.asarray([SEVEN[k][0] for k in keys], np.float32)
        want = dict(dist=np.sqrt(np.asarray([SEVEN[k][3] for k in keys], np.float32)), face=np.zeros(len(keys), np.int32),
                    bary=np.asarray([SEVEN[k][1] for k in keys], np.float32), closest=np.asarray([SEVEN[k][2] for k in keys], np.float32))
        return dict(q=q, xyz=RIGHT[0], faces=RIGHT[1], max_dist=8.0), want
    if name == "tie":
        # two triangles in the planes z = 0 and z = 2 with the same footprint, the query midway: the smaller index wins, also when it comes last
        xyz = np.asarray([(0, 0, 2), (4, 0, 2), (0, 4, 2), (0, 0, 0), (4, 0, 0), (0, 4, 0)], np.float32)
        faces = np.asarray([(0, 1, 2), (3, 4, 5)], np.int32)
        q = np.asarray([(1, 1, 1), (1, 2, 1.5)], np.float32)
        want = dict(dist=np.asarray([1, 0.5], np.float32), face=np.asarray([0, 0], np.int32), bary=np.asarray([(0.25, 0.25), (0.25, 0.5)], np.float32),
                    closest=np.asarray([(1, 1, 2), (1, 2, 2)], np.float32))
        return dict(q=q, xyz=xyz, faces=faces, max_dist=4.0), want
    if name == "radius":
        # at exactly max_dist: found; one fp32 step beyond: not found
        q = np.asarray([(1, 1, 3), (1, 1, np.nextafter(np.float32(3), np.float32(4))), (1, 1, -3)], np.float32)
        want = dict(dist=np.asarray([3, 3, 3], np.float32), face=np.asarray([0, -1, 0], np.int32),
                    bary=np.asarray([(0.25, 0.25), (0, 0), (0.25, 0.25)], np.float32), closest=np.asarray([(1, 1, 0), (0, 0, 0), (1, 1, 0)], np.float32))
        return dict(q=q, xyz=RIGHT[0], faces=RIGHT[1], max_dist=3.0), want
    raise KeyError(name)


def check_exact(got, want, label=""):
    """the pinned bits of an EXACT_CASES case: dist, face, and bary / closest where ``got`` has them"""
    bits = lambda x: np.ascontiguousarray(np.asarray(x, np.float32) + np.float32(0)).view(np.uint32)       # -0 counts as 0
    assert np.array_equal(np.asarray(got["face"]).astype(np.int64), want["face"].astype(np.int64)), "%s: faces %r, expected %r" % (label, got["face"], want["face"])
    for k in ("dist", "bary", "closest"):
        if got.get(k) is not None:
            assert np.array_equal(bits(got[k]), bits(want[k])), "%s: %s %r, expected %r" % (label, k, got[k], want[k])


EXACT_CASES = ("seven", "tie", "radius")
SIZES_M = (1, 63, 64, 65, 257)
SIZES_F = (1, 2, 63, 65, 1000)
CASES = ["rand_m%d_f%d" % (m, f) for m in SIZES_M for f in SIZES_F] + ["outside", "walls", "icosphere", "cube", "invalid_mix", "invalid_only", "m0"]


def walls(rng, small=300):
    """two wall-sized triangles (a 4 x 3 wall) and ``small`` triangles of a few centimetres in front of it"""
    wall = np.asarray([(0, 0, 0), (4, 0, 0), (4, 3, 0), (0, 3, 0)], np.float32)
    xyz, faces = soup(small, rng, size=0.04, lo=0.2, hi=2.5)
    return np.concatenate([wall, xyz]), np.concatenate([np.asarray([(0, 1, 2), (0, 2, 3)], np.int32), faces + 4])


PLACED_CASE = "rand_m65_f65"  # the case that is also built at placement.FAMILY_PLACES: the smallest with more than a wave of queries and of faces


def build_case(name, place=None):
    """-> dict(q float32 [M,3], xyz float32 [V,3], faces int32 [F,3], max_dist); a function of the name alone.  ``place`` (placement.py;
    the rand_ cases): the draws of the unplaced case kept in float64, moved to the placement and rounded to fp32 once"""
    import placement as PL
    rng = np.random.default_rng(abs(hash_name(name)))
    if PL.key(place) is not None:
        m, f = (int(x[1:]) for x in name.split("_")[1:])
        xyz = (rng.uniform(0.0, 1.0, (f, 1, 3)) + rng.uniform(-0.08, 0.08, (f, 3, 3))).reshape(-1, 3)              # soup's draws
        q = rng.uniform(-0.2, 1.2, (m, 3))
        return dict(q=PL.points(q, place).astype(np.float32), xyz=PL.points(xyz, place).astype(np.float32),
                    faces=np.arange(3 * f, dtype=np.int32).reshape(f, 3), max_dist=0.5)
    if name.startswith("rand_"):
        m, f = (int(x[1:]) for x in name.split("_")[1:])
        xyz, faces = soup(f, rng)
        return dict(q=rng.uniform(-0.2, 1.2, (m, 3)).astype(np.float32), xyz=xyz, faces=faces, max_dist=0.5)
    if name == "outside":                        # every query outside the grid's box, some beyond max_dist
        xyz, faces = soup(200, rng)
        q = rng.uniform(-1, 1, (130, 3))
        q = (q / np.abs(q).max(1, keepdims=True) * rng.uniform(1.3, 4.0, (130, 1)) + 0.5).astype(np.float32)
        return dict(q=q, xyz=xyz, faces=faces, max_dist=2.5)
    if name == "walls":
        xyz, faces = walls(rng)
        return dict(q=rng.uniform((-0.5, -0.5, -1), (4.5, 3.5, 3), (257, 3)).astype(np.float32), xyz=xyz, faces=faces, max_dist=1.0)
    if name == "icosphere":                      # shared edges and vertices: ties in exact arithmetic
        xyz, faces = icosphere(2)
        q = rng.normal(size=(200, 3))
        q = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.2, 1.8, (200, 1))).astype(np.float32)
        return dict(q=q, xyz=xyz, faces=faces, max_dist=1.0)
    if name == "cube":
        xyz, faces = unit_cube()
        return dict(q=rng.uniform(-0.5, 1.5, (150, 3)).astype(np.float32), xyz=xyz, faces=faces, max_dist=2.0)
    if name == "invalid_mix":                    # indices at -1, V, 2^31 - 1 and -2^31, a NaN and an infinite vertex, faces without area
        xyz, faces = soup(40, rng)
        V = xyz.shape[0]
        xyz = np.concatenate([xyz, np.asarray([(np.nan, 0, 0), (0, np.inf, 0), (0.5, 0.5, 0.5)], np.float32)])
        bad = np.asarray([(-1, 0, 1), (0, V + 3, 1), (0, 1, 2 ** 31 - 1), (-2 ** 31, 1, 2), (0, 1, V), (3, V + 1, 5), (7, 7, 8), (9, 10, 9), (4, 4, 4),
                          (0, V + 2, V + 2)], np.int64).astype(np.int32)
        faces = np.concatenate([faces[:20], bad, faces[20:]])
        return dict(q=rng.uniform(-0.2, 1.2, (65, 3)).astype(np.float32), xyz=xyz, faces=faces, max_dist=0.5)
    if name == "invalid_only":
        xyz = np.asarray([(0, 0, 0), (1, 0, 0), (2, 0, 0), (np.nan, 1, 1)], np.float32)
        faces = np.asarray([(0, 1, 2), (0, 1, 3), (0, 1, 4), (1, 1, 2)], np.int32)
        return dict(q=rng.uniform(-1, 1, (65, 3)).astype(np.float32), xyz=xyz, faces=faces, max_dist=0.5)
    if name == "m0":
        xyz, faces = soup(10, rng)
        return dict(q=np.zeros((0, 3), np.float32), xyz=xyz, faces=faces, max_dist=0.5)
    raise KeyError(name)


def hash_name(name):
    """a seed from a name that does not change between runs (hash() of a str does)"""
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xffffffff
    return h
