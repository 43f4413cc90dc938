"""Reference of the mesh-sampling contract of the library (csrc/mesh/mesh_sample.hip, include/estd_hip.h: estd_mesh_face_area, the glue,
estd_mesh_sample) and of ``fusion3d.mesh_area`` / ``sample_mesh``.  A plain helper module of the test suite (not a conftest); numpy only.

What is exact and what has a bound (``compare`` is THE comparison of the suite; ROUTE = 2 is the route constant of the mesh kernels: the
device is held to 2 x a derived first-order bound, and every bound below comes from the expressions, none from a measurement).

area.  e = 2^-53.  The vertices are fp32, exact in float64.  Each of e1 = b - a, e2 = c - a is one rounding; a component of the cross
  product, nx = e1y e2z - e1z e2y, carries the two edge roundings, one per product and one for the difference: |dnx| <= 4 e mx with
  mx = |e1y e2z| + |e1z e2y| (likewise my, mz; cancellation makes this an absolute bound, not a relative one).  len = sqrt(nx^2 + ny^2 +
  nz^2): d len <= |dn| <= 4 e |m| (Cauchy-Schwarz), plus three roundings in the squares and the sum (3 e of the radicand = 1.5 e of len)
  and the square root (taken as 1 e, correctly rounded or not): |d len| <= e (4 |m| + 2.5 len); the halving is exact, so
  ``area_bound = 0.5 e (4 |m| + 2.5 len)``.  For a well-shaped triangle |m| ~ len, i.e. about 6.5 ulp of the result.  Where |m| = 0
  (repeated indices; collinear points along an axis) the bound is 0 and the area must be +0 exactly.
face_normal.  n / len in float64, rounded once to fp32: per component 2^-24 (a half ulp of a value <= 1) + e (4 mx / len + |nx| / len *
  (4 |m| / len + 2.5) + 1) <= ``normal_bound = 2^-24 + e (8 |m| / len + 3.5)``.  A normal is LEFT OUT only where the area lies within ROUTE
  x its bound of zero without being bound to be zero (0 < len <= ROUTE x len's bound): its direction is rounding noise there.  compare
  caps that share at 3 %; no case of CASES leaves one out in the reference itself (test_mesh_sample_ref_cpu.py).
face.  Checked GIVEN THE DEVICE'S OWN area, as tracking's sums are checked given the device's match map: the reference quantises those
  bits with the power of two of the contract, forms cum, w and every t_i in integers (all below 2^62: int64 is exact) and must get face[i]
  exactly, for every sample.  Nothing is left out.
bary.  Exact.  iu, iv are 24-bit integers from the integer mixer; the fold happens in integers (iu + iv > 2^24 <=> u + v > 1, and
  2^24 - iu is 1 - u without a rounding: a multiple of 2^-24 not above 1 has at most 24 significant bits); u = iu 2^-24 is an exact fp32
  product.  After the fold iu + iv <= 2^24, so u, v >= 0 and u + v <= 1 exactly.
xyz / attrs.  p = fma(v, c - a, fma(u, b - a, a)) in fp32, u32 = 2^-24: four roundings, |dp| <= u32 (u |b - a| + v |c - a| + |inner| + |p|)
  with inner = a + u (b - a): ``point_bound``, evaluated on the float64 values.  The reference p is the float64 value of a + u (b - a) +
  v (c - a); its own error (2^-53) is 2^-29 of the bound.
normal (per sample) = face_normal[face[i]]: exact, given the device's own face normals.

``MISTAKES`` is a test-only knob: plausible kernel mistakes; test_mesh_sample_ref_cpu.py asserts that compare rejects each."""
import functools
import math

import numpy as np

ROUTE = 2.0
E64 = 2.0 ** -53
U32 = 2.0 ** -24
MIN_STRATUM = 1 << 20
LEFT_OUT_CAP = 0.03
MISTAKES = ("lower_bound", "no_fold", "swap_bc", "no_jitter", "unhalved")

M1, M2 = np.uint64(0xbf58476d1ce4e5b9), np.uint64(0x94d049bb133111eb)
G1, G2 = np.uint64(0x9e3779b97f4a7c15), np.uint64(0xd1b54a32d192ed03)


def mix64(z):
    """the finaliser of SplitMix64 on a uint64 array (numpy's uint64 arithmetic wraps modulo 2^64)"""
    z = z ^ (z >> np.uint64(30))
    z = z * M1
    z = z ^ (z >> np.uint64(27))
    z = z * M2
    return z ^ (z >> np.uint64(31))


def h64(seed, i, stream):
    """seed: an integer (taken modulo 2^64), i: uint64 array, stream: 0, 1 or 2 -> uint64 array"""
    i = np.asarray(i, np.uint64)
    with np.errstate(over="ignore"):
        return mix64(mix64(np.uint64(int(seed) & 0xffffffffffffffff) + (i + np.uint64(1)) * G1) + np.uint64(stream + 1) * G2)


def h64_int(seed, i, stream):
    """the same in Python integers, one sample (the CPU suite holds the two against each other)"""
    K = (1 << 64) - 1

    def mix(z):
        z ^= z >> 30
        z = z * 0xbf58476d1ce4e5b9 & K
        z ^= z >> 27
        z = z * 0x94d049bb133111eb & K
        return z ^ (z >> 31)
    return mix((mix(((seed & K) + (i + 1) * 0x9e3779b97f4a7c15) & K) + (stream + 1) * 0xd1b54a32d192ed03) & K)


def face_area(xyz, faces, mistake=None):
    """-> dict(area [F] float64, normal [F,3] float32, invalid, area_bound [F], normal_bound [F], left_out [F] bool), in the
    header's order of operations (numpy does not contract)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = xyz.shape[0], faces.shape[0]
    ok = ((faces >= 0) & (faces < V)).all(1) if F else np.zeros(0, bool)
    safe = np.where(ok[:, None], faces, 0)
    p = xyz.astype(np.float64) if V else np.zeros((1, 3))
    a, b, c = p[safe[:, 0]], p[safe[:, 1]], p[safe[:, 2]]
    e1, e2 = b - a, c - a
    t1 = np.stack([e1[:, 1] * e2[:, 2], e1[:, 2] * e2[:, 0], e1[:, 0] * e2[:, 1]], 1)
    t2 = np.stack([e1[:, 2] * e2[:, 1], e1[:, 0] * e2[:, 2], e1[:, 1] * e2[:, 0]], 1)
    n = t1 - t2
    m = np.sqrt(((np.abs(t1) + np.abs(t2)) ** 2).sum(1))
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ln = np.where(ok, ln, 0.0)
    m = np.where(ok, m, 0.0)
    area = ln if mistake == "unhalved" else 0.5 * ln
    with np.errstate(invalid="ignore", divide="ignore"):
        normal = np.where((ln > 0)[:, None], n / ln[:, None], 0.0).astype(np.float32)
        len_bound = E64 * (4.0 * m + 2.5 * ln)
        normal_bound = np.where(ln > 0, U32 + E64 * (8.0 * m / ln + 3.5), 0.0)
    left_out = (ln > 0) & (ln <= ROUTE * len_bound)
    return dict(area=area, normal=normal, invalid=int((~ok).sum()), area_bound=0.5 * len_bound, normal_bound=normal_bound, left_out=left_out)


def scale_exponent(n_faces, area_max):
    """e of the contract's glue: the areas are multiplied by 2^e before the floor"""
    if n_faces <= 0 or not area_max > 0:
        return 0
    return min(1000, 62 - (int(n_faces) - 1).bit_length() - math.frexp(float(area_max))[1])


def quantise(area):
    """area [F] float64 -> (q [F] int64, e)"""
    area = np.asarray(area, np.float64)
    e = scale_exponent(area.shape[0], float(area.max()) if area.size else 0.0)
    return np.floor(np.ldexp(area, e)).astype(np.int64), e


def stratum(total, n):
    """w = total // n, or a RuntimeError as the host layers raise it"""
    if total <= 0:
        raise RuntimeError("mesh_sample: the mesh has no area")
    w = int(total) // int(n)
    if w < MIN_STRATUM:
        raise RuntimeError("mesh_sample: strata of %d units" % w)
    return w


def choose(area, n, seed, first=0, count=None, mistake=None, w=None):
    """the triangles of the samples first .. first + count - 1 of ``n`` (count: default all) given the bits of ``area`` ->
    dict(face int32, t int64, w, total, q).  ``w``: a stratum narrower than total // n, as the C entry point takes one (n w <= total)"""
    q, _ = quantise(area)
    cum = np.cumsum(q)
    total = int(cum[-1]) if cum.size else 0
    w = stratum(total, n) if w is None else int(w)
    assert total < 1 << 62 and n * w <= total
    i = np.arange(first, first + (n - first if count is None else count), dtype=np.int64)
    jitter = (h64(seed, i, 0) % np.uint64(w)).astype(np.int64) if mistake != "no_jitter" else np.zeros_like(i)
    t = i * w + jitter
    face = np.searchsorted(cum, t, side="left" if mistake == "lower_bound" else "right")
    return dict(face=np.minimum(face, cum.size - 1).astype(np.int32), t=t, w=w, total=total, q=q)


def bary(seed, i, mistake=None):
    """-> (bary [n,2] float32, the integers [n,2])"""
    iu = (h64(seed, i, 1) >> np.uint64(40)).astype(np.int64)
    iv = (h64(seed, i, 2) >> np.uint64(40)).astype(np.int64)
    fold = (iu + iv > 1 << 24) & (mistake != "no_fold")
    iu, iv = np.where(fold, (1 << 24) - iu, iu), np.where(fold, (1 << 24) - iv, iv)
    ints = np.stack([iu, iv], 1)
    return (ints.astype(np.float32) * np.float32(U32)).astype(np.float32), ints


def interpolate(rows, faces, face, uv, mistake=None):
    """rows [V,C] fp32, the chosen triangles and the barycentric pairs -> (values [n,C] float64, point_bound [n,C])"""
    rows = np.asarray(rows, np.float32).astype(np.float64)
    tri = np.asarray(faces, np.int64)[np.asarray(face, np.int64)]
    a, b, c = rows[tri[:, 0]], rows[tri[:, 2 if mistake == "swap_bc" else 1]], rows[tri[:, 1 if mistake == "swap_bc" else 2]]
    u, v = uv[:, :1].astype(np.float64), uv[:, 1:].astype(np.float64)
    inner = a + u * (b - a)
    p = inner + v * (c - a)
    return p, U32 * (u * np.abs(b - a) + v * np.abs(c - a) + np.abs(inner) + np.abs(p))


def sample(xyz, faces, attrs, n, seed, area=None, first=0, count=None, mistake=None, w=None):
    """The whole operator in float64 / integers.  ``area``: the bits to choose from (default the reference's own) ->
    dict(xyz, face, bary, normal, attrs (or None), xyz_bound, attrs_bound, area, invalid, w, total)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    fa = face_area(xyz, faces, mistake)
    if area is None:
        area = fa["area"]
    if faces.shape[0] == 0 or n == 0:
        z = np.zeros
        return dict(xyz=z((0, 3)), face=z(0, np.int32), bary=z((0, 2), np.float32), normal=z((0, 3), np.float32),
                    attrs=None if attrs is None else z((0, np.asarray(attrs).shape[1])), xyz_bound=z((0, 3)), attrs_bound=None,
                    area=fa["area"], invalid=fa["invalid"], w=0, total=0, fa=fa)
    ch = choose(area, n, seed, first, count, mistake, w)
    i = np.arange(first, first + ch["face"].shape[0], dtype=np.int64)
    uv, _ = bary(seed, i, mistake)
    p, pb = interpolate(xyz, faces, ch["face"], uv, mistake)
    at = ab = None
    if attrs is not None:
        at, ab = interpolate(attrs, faces, ch["face"], uv, mistake)
    return dict(xyz=p, face=ch["face"], bary=uv, normal=fa["normal"][ch["face"]], attrs=at, xyz_bound=pb, attrs_bound=ab, area=fa["area"],
                invalid=fa["invalid"], w=ch["w"], total=ch["total"], fa=fa)


def n_for_density(density, total):
    """N of ``sample_mesh(density=)``: ceil(density x total area)"""
    return int(math.ceil(float(density) * float(total)))


def _worst(diff, bound):
    """the largest |diff| / bound; a bound of 0 demands equality"""
    diff, bound = np.abs(np.asarray(diff, np.float64)), np.asarray(bound, np.float64)
    assert (diff[bound == 0] == 0).all(), "a value that is bound to be exact differs"
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, diff / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def compare(got, xyz, faces, attrs, n, seed, what="", first=0, w=None):
    """``got``: dict(xyz, face, bary, normal, attrs, area, invalid[, face_normal]) of numpy arrays, the operator's outputs for the mesh
    (xyz, faces, attrs), ``n`` samples and ``seed`` (``first``: got holds the rows from that sample on; ``w``: as in ``choose``) -> the largest fractions of the
    bounds seen; AssertionError where a bound times ROUTE or an exact value is missed"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = faces.shape[0]
    fa = face_area(xyz, faces)
    assert int(got["invalid"]) == fa["invalid"], "%s: invalid = %d, the reference has %d" % (what, int(got["invalid"]), fa["invalid"])
    area = np.asarray(got["area"])
    assert area.dtype == np.float64 and area.shape == (F,), "%s: area is %s %s" % (what, area.dtype, area.shape)
    assert not np.signbit(area).any() and np.isfinite(area).all(), "%s: an area is negative or not finite" % what
    fig = dict(area=_worst(area - fa["area"], fa["area_bound"]), faces=F, invalid=fa["invalid"], left_out=0)
    assert fig["area"] <= ROUTE, "%s: area off by %.3g of its bound" % (what, fig["area"])
    if got.get("face_normal") is not None:
        fn = np.asarray(got["face_normal"])
        assert fn.dtype == np.float32 and fn.shape == (F, 3), "%s: face_normal is %s %s" % (what, fn.dtype, fn.shape)
        keep = ~fa["left_out"]
        fig["left_out"] = int((~keep).sum())
        assert fig["left_out"] <= LEFT_OUT_CAP * F, "%s: %d of %d normals left out" % (what, fig["left_out"], F)
        fig["face_normal"] = _worst((fn.astype(np.float64) - fa["normal"].astype(np.float64))[keep], np.repeat(fa["normal_bound"][keep, None], 3, 1))
        assert fig["face_normal"] <= ROUTE, "%s: a face normal is off by %.3g of its bound" % (what, fig["face_normal"])
    count = np.asarray(got["face"]).shape[0]
    ref = sample(xyz, faces, attrs, n, seed, area=area, first=first, count=count if F and n else None, w=w)
    for k, dt, cols in (("face", np.int32, None), ("bary", np.float32, 2), ("xyz", np.float32, 3), ("normal", np.float32, 3)):
        a = np.asarray(got[k])
        want = (ref["face"].shape[0],) + ((cols,) if cols else ())
        assert a.dtype == dt and a.shape == want, "%s: %s is %s %s, expected %s %s" % (what, k, a.dtype, a.shape, np.dtype(dt), want)
    bad = np.nonzero(np.asarray(got["face"]) != ref["face"])[0]
    assert bad.size == 0, "%s: face differs at %d of %d samples, first at %d: %d for %d" % (
        what, bad.size, ref["face"].shape[0], bad[0], got["face"][bad[0]], ref["face"][bad[0]])
    assert np.array_equal(np.asarray(got["bary"]), ref["bary"]), "%s: bary differs" % what
    fig["xyz"] = _worst(np.asarray(got["xyz"], np.float64) - ref["xyz"], ref["xyz_bound"])
    assert fig["xyz"] <= ROUTE, "%s: a position is off by %.3g of its bound" % (what, fig["xyz"])
    if attrs is None:
        assert got.get("attrs") is None, "%s: attributes out of nowhere" % what
    else:
        a = np.asarray(got["attrs"])
        assert a.dtype == np.float32 and a.shape == ref["attrs"].shape, "%s: attrs is %s %s" % (what, a.dtype, a.shape)
        fig["attrs"] = _worst(a.astype(np.float64) - ref["attrs"], ref["attrs_bound"])
        assert fig["attrs"] <= ROUTE, "%s: an attribute is off by %.3g of its bound" % (what, fig["attrs"])
    if got.get("face_normal") is not None and ref["face"].size:
        assert np.array_equal(np.asarray(got["normal"]), np.asarray(got["face_normal"])[ref["face"]]), "%s: normal is not the triangle's" % what
    fig["samples"] = int(ref["face"].shape[0])
    return fig


# ------------------------------------------------------------------------------------------------ meshes
def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """-> (xyz [V,3] float32, faces [F,3] int32, F = 20 x 4^level), counter-clockwise seen from outside"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [tuple(np.asarray(p, np.float64) / np.linalg.norm(p)) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = (np.asarray(v[i]) + np.asarray(v[j])) / 2.0
                v.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    xyz = (np.asarray(v, np.float64) * radius + np.asarray(centre, np.float64)).astype(np.float32)
    return xyz, np.asarray(f, np.int32)


def random_mesh(F, seed, spread=1.0, offset=0.0):
    """F triangles over 40 + F // 2 shared vertices"""
    rng = np.random.default_rng(seed)
    V = 40 + F // 2
    xyz = (rng.uniform(-spread, spread, (V, 3)) + offset).astype(np.float32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    return xyz, faces


def _areas_mesh():
    """40 right triangles in a row whose areas run from 1 to 10^-6"""
    xyz, faces = [], []
    for k in range(40):
        s = 10.0 ** (-3.0 * k / 39.0)
        xyz += [(2.0 * k, 0.0, 0.5), (2.0 * k + s, 0.0, 0.5), (2.0 * k, 2.0 * s, 0.5 + s)]
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    return np.asarray(xyz, np.float32), np.asarray(faces, np.int32)


def _zero_area_mesh():
    """zero-area triangles -- repeated indices and collinear points along an axis -- first, last and in runs among 20 proper ones"""
    xyz, faces = random_mesh(20, 5)
    V = xyz.shape[0]
    xyz = np.concatenate([xyz, np.asarray([(5, 3, 7), (6, 3, 7), (9, 3, 7), (5, 3, 9.5), (5, 3, -2)], np.float32)])
    rep = [(1, 1, 2), (3, 4, 3), (6, 6, 6), (7, 8, 8)]
    col = [(V, V + 1, V + 2), (V + 2, V, V + 1), (V, V + 3, V + 4)]
    z = [np.asarray(t, np.int32)[None] for t in rep + col]
    parts = [z[0], z[4], faces[:7], z[1], z[5], z[2], faces[7:8], z[6], faces[8:], z[3], z[4]]
    return xyz, np.concatenate(parts)


def _out_of_range_mesh():
    xyz, faces = random_mesh(20, 6)
    V = xyz.shape[0]
    faces = faces.copy()
    faces[0, 0], faces[3, 1], faces[4, 2], faces[11, 0], faces[19, 2] = -1, V, -1, V, V
    faces[12] = (-1, V, 2 ** 31 - 1)
    return xyz, faces


def _sphere_pair():
    """two icospheres, 5120 + 1280 triangles, with their vertex normals as attributes"""
    x1, f1 = icosphere(4, 0.55, (0.1, 0.05, 2.0))
    x2, f2 = icosphere(3, 0.3, (-0.9, 0.4, 1.7))
    n1 = (x1.astype(np.float64) - (0.1, 0.05, 2.0)) / 0.55
    n2 = (x2.astype(np.float64) - (-0.9, 0.4, 1.7)) / 0.3
    return np.concatenate([x1, x2]), np.concatenate([f1, f2 + x1.shape[0]]).astype(np.int32), np.concatenate([n1, n2]).astype(np.float32)


def tie_case():
    """A target that hits a prefix sum exactly, the one place where an upper and a lower bound differ: triangle 0 has no area, triangle 1
    has 2^60 units, the stratum is the narrowest allowed and the seed is the first whose jitter of sample 0 is 0, so t_0 = 0 = cum[0]
    -> (xyz, faces, n, seed, w)"""
    xyz = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32)
    faces = np.asarray([(0, 0, 1), (0, 1, 2)], np.int32)
    seeds = np.arange(1 << 23, dtype=np.uint64)
    with np.errstate(over="ignore"):
        hit = np.nonzero(mix64(mix64(seeds + G1) + G2) % np.uint64(MIN_STRATUM) == 0)[0]
    return xyz, faces, 64, int(hit[0]), MIN_STRATUM


def _attrs(V, C, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (V, C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def build_case(name):
    """-> (xyz [V,3] float32, faces [F,3] int32, attrs [V,C] float32 or None, n, seed); the arrays are shared: leave them unchanged"""
    one = (np.asarray([(0.25, -1, 2), (1.5, 0.5, 2.25), (-0.5, 1, 3)], np.float32), np.asarray([(0, 1, 2)], np.int32))
    m65 = random_mesh(65, 1)
    if name == "one":
        out = one + (None, 1, 0)
    elif name == "one-257":
        out = one + (None, 257, 0)
    elif name == "f65-n64":
        out = m65 + (None, 64, 0)
    elif name == "f65-n1000":
        out = m65 + (None, 1000, 0)
    elif name == "f65-n1000-seed":
        out = m65 + (None, 1000, (1 << 63) + 12345)
    elif name == "areas-1e6":
        out = _areas_mesh() + (None, 3000, 3)
    elif name == "zero-area":
        out = _zero_area_mesh() + (None, 300, 0)
    elif name == "out-of-range":
        out = _out_of_range_mesh() + (None, 200, 0)
    elif name == "no-faces":
        out = (m65[0], np.zeros((0, 3), np.int32), None, 10, 0)
    elif name == "no-samples":
        out = m65 + (_attrs(m65[0].shape[0], 3, 2), 0, 0)
    elif name in ("attrs-1", "attrs-3", "attrs-6"):
        out = m65 + (_attrs(m65[0].shape[0], int(name[-1]), 4), 300, 7)
    elif name == "far":
        out = random_mesh(65, 8, spread=2.0, offset=1000.0) + (None, 500, 0)
    elif name == "spheres":
        x, f, nrm = _sphere_pair()
        out = (x, f, nrm, 50000, 11)
    else:
        raise KeyError(name)
    return out


PLACED_CASE = "attrs-3"      # the case that is also built at placement.FAMILY_PLACES: the 65-face mesh with attributes, 300 samples


def placed_case(place):
    """PLACED_CASE built at a placement (placement.py): random_mesh's draws kept in float64, moved there and rounded to fp32 once (as
    "far" does with its 1000 m along every axis); faces, attributes, n and seed are the unplaced case's"""
    import placement as PL
    xyz0, faces, attrs, n, seed = build_case(PLACED_CASE)
    V = xyz0.shape[0]
    xyz = np.random.default_rng(1).uniform(-1.0, 1.0, (V, 3))                                   # random_mesh(65, 1)'s first draw
    assert np.array_equal(xyz.astype(np.float32), xyz0)
    return PL.points(xyz, place).astype(np.float32), faces, attrs, n, seed


CASES = ("one", "one-257", "f65-n64", "f65-n1000", "f65-n1000-seed", "areas-1e6", "zero-area", "out-of-range", "no-faces", "no-samples",
         "attrs-1", "attrs-3", "attrs-6", "far", "spheres")


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference's own result of a case (shared: leave it unchanged)"""
    xyz, faces, attrs, n, seed = build_case(name)
    return sample(xyz, faces, attrs, n, seed)


def as_got(ref):
    """a reference result in the form compare takes the device's"""
    return dict(xyz=ref["xyz"].astype(np.float32), face=ref["face"], bary=ref["bary"], normal=ref["normal"],
                attrs=None if ref["attrs"] is None else ref["attrs"].astype(np.float32), area=ref["area"], invalid=ref["invalid"],
                face_normal=ref["fa"]["normal"])


# ------------------------------------------------------------------------------------------------ the analytic scene as a coarse mesh
def scene_mesh(depths, poses, K, level=2, facing=0.3):
    """A coarse ground-truth mesh of the observed part of track_ref's three-body scene, as a decimated scan would describe it: the plane
    z = 2.6 as TWO triangles over the bounding rectangle of the plane points the frames ``depths`` [T,H,W] at ``poses`` see, each sphere as
    the triangles of a level-``level`` icosphere that face the first camera (cosine above ``facing``) -> (xyz [V,3] float32, faces [F,3]
    int32), without unused vertices"""
    import run_stream_ref as RS
    import track_ref as T
    pts = np.concatenate([RS.backproject(d, P, K) for d, P in zip(depths, poses)])
    on_plane = pts[np.abs(pts[:, 2] - T.PLANE_Z) < 2e-3]                      # millimetre storage: within 0.5 mm
    (x0, y0), (x1, y1) = on_plane[:, :2].min(0), on_plane[:, :2].max(0)
    xyz = [np.asarray([(x0, y0, T.PLANE_Z), (x1, y0, T.PLANE_Z), (x1, y1, T.PLANE_Z), (x0, y1, T.PLANE_Z)])]
    faces = [np.asarray([(0, 2, 1), (0, 3, 2)])]                              # seen from z < 2.6
    cam = np.asarray(poses[0], np.float64)[:3, 3]
    n_v = 4
    for centre, radius in T.SPHERES:
        v, f = icosphere(level, radius, centre)
        mid = v.astype(np.float64)[f].mean(1)
        out = (mid - np.asarray(centre)) / np.linalg.norm(mid - np.asarray(centre), axis=1, keepdims=True)
        to_cam = (cam - mid) / np.linalg.norm(cam - mid, axis=1, keepdims=True)
        f = f[(out * to_cam).sum(1) > facing]
        used = np.unique(f)
        xyz.append(v[used].astype(np.float64))
        faces.append(np.searchsorted(used, f) + n_v)
        n_v += used.shape[0]
    return np.concatenate(xyz).astype(np.float32), np.concatenate(faces).astype(np.int32)


def nearest_brute(query, target, chunk=512):
    """[M,3], [N,3] float64 -> [M] the distance to the nearest target, by brute force"""
    query, target = np.asarray(query, np.float64), np.asarray(target, np.float64)
    out = np.empty(query.shape[0])
    t2 = (target ** 2).sum(1)
    for i in range(0, query.shape[0], chunk):
        q = query[i:i + chunk]
        d2 = (q ** 2).sum(1)[:, None] - 2.0 * q @ target.T + t2[None]
        j = d2.argmin(1)
        out[i:i + chunk] = np.linalg.norm(q - target[j], axis=1)
    return out


def cloud_scores(pred, gt, threshold=0.05, max_dist=1.0):
    """compare_clouds' figures in float64 by brute force -> dict(accuracy, completeness, precision, recall, fscore)"""
    a, c = np.minimum(nearest_brute(pred, gt), max_dist), np.minimum(nearest_brute(gt, pred), max_dist)
    P, R = float((a < np.float32(threshold)).mean()), float((c < np.float32(threshold)).mean())
    return dict(accuracy=float(a.mean()), completeness=float(c.mean()), precision=P, recall=R, fscore=2 * P * R / (P + R) if P + R > 0 else 0.0)
