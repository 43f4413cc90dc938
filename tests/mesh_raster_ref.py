"""The mesh rasteriser's contract (include/estd_hip.h: estd_mesh_raster, estd_mesh_raster_resolve; csrc/mesh/mesh_raster.hip) in numpy
float64: triangles looped over their pixels, every operation one IEEE float64 operation in the order the header states (numpy's
elementwise products, sums and quotients are single rounded operations, never fused).  Nothing here is a bound: ``compare`` asks for
EQUALITY TO THE BIT of depth, face, bary, facing and invalid.

``raster`` sweeps the whole image for every triangle (the contract as written); ``box=True`` sweeps what the kernel sweeps (the bounding
box of the projections with a one-pixel margin when all three q_z > z_near, the whole image otherwise, nothing when det is 0 or not
finite) -- the skip the contract allows, used for the large cases, where the full sweep would take minutes.

``variant`` breaks the contract on purpose, one rule at a time, for tests/test_mesh_raster_ref_cpu.py: the comparison has to reject
each.  ``visible_points`` is the float64 visibility test of estdepth_amd.fusion3d.visible_points."""
import numpy as np

ALL_ONES = np.uint64(0xffffffffffffffff)
VARIANTS = ("strict-edges", "one-winding", "swapped-bary", "half-pixel", "largest-id")


# ------------------------------------------------------------------------------------------------- cameras and shapes
def intrinsics(H, W, f=None):
    f = float(f if f is not None else 0.8 * max(H, W))
    return np.asarray([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], np.float64)


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """camera-to-world pose [4,4] float64: x right, y down, z forward"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def raster_matrix(pose, K):
    """M = K [R^T | -R^T c] in float64 -> [12] (estdepth_amd.camera.mesh_raster_matrix forms the same)"""
    pose, K = np.asarray(pose, np.float64), np.asarray(K, np.float64)
    Rt = pose[:3, :3].T
    return (K @ np.concatenate([Rt, -(Rt @ pose[:3, 3])[:, None]], 1)).reshape(-1)


def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """-> (xyz float32 [V,3], faces int32 [20 * 4^level, 3]), counter-clockwise seen from outside"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return (np.asarray(v) * radius + np.asarray(centre, np.float64)).astype(np.float32), np.asarray(f, np.int32)


# ------------------------------------------------------------------------------------------------- the contract
def project(mat, xyz):
    """q_j = ((M_j0 x + M_j1 y) + M_j2 z) + M_j3 per vertex, widened to float64 -> [V,3]"""
    M = np.asarray(mat, np.float64).reshape(3, 4)
    p = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((M[j, 0] * p[:, 0] + M[j, 1] * p[:, 1]) + M[j, 2] * p[:, 2]) + M[j, 3] for j in range(3)], 1)


def _cross(a, b):
    return np.asarray([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def setup(q0, q1, q2):
    with np.errstate(all="ignore"):
        n = [_cross(q1, q2), _cross(q2, q0), _cross(q0, q1)]
        det = (n[0][0] * q0[0] + n[0][1] * q0[1]) + n[0][2] * q0[2]
    return n, det


def _edges(n, U, V, variant=None):
    """-> (E [3], S, covered) on the pixel arrays U, V"""
    with np.errstate(all="ignore"):
        E = [(n[k][0] * U + n[k][1] * V) + n[k][2] for k in range(3)]
        S = (E[0] + E[1]) + E[2]
        if variant == "strict-edges":
            pos, neg = (E[0] > 0) & (E[1] > 0) & (E[2] > 0) & (S > 0), (E[0] < 0) & (E[1] < 0) & (E[2] < 0) & (S < 0)
        else:
            pos, neg = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0) & (S > 0), (E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0) & (S < 0)
        if variant == "one-winding":
            neg = np.zeros_like(neg)
    return E, S, pos | neg


def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1)


def _pixels(H, W, variant):
    V, U = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return (U + 0.5, V + 0.5) if variant == "half-pixel" else (U, V)


def _box(q, det, H, W, z_near):
    """the rows and columns the kernel sweeps for this triangle -> (r0, r1, u0, u1) inclusive, or None"""
    if not np.isfinite(det) or det == 0:
        return None
    zn = float(np.float32(z_near))
    if not all(q[i][2] > zn for i in range(3)):
        return 0, H - 1, 0, W - 1
    with np.errstate(all="ignore"):
        x, y = [q[i][0] / q[i][2] for i in range(3)], [q[i][1] / q[i][2] for i in range(3)]
    lo_x, hi_x = max(np.floor(min(x)) - 1.0, 0.0), min(np.ceil(max(x)) + 1.0, W - 1.0)
    lo_y, hi_y = max(np.floor(min(y)) - 1.0, 0.0), min(np.ceil(max(y)) + 1.0, H - 1.0)
    if not (lo_x <= hi_x and lo_y <= hi_y):
        return None
    return int(lo_y), int(hi_y), int(lo_x), int(hi_x)


def merge(keys, xyz, faces, mat, z_near, first=0, count=None, box=False, variant=None):
    """estd_mesh_raster: the triangles first .. first + count - 1 merged into ``keys`` uint64 [H,W] in place -> this range's invalid count"""
    H, W = keys.shape
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    n_v = np.asarray(xyz).reshape(-1, 3).shape[0]
    count = faces.shape[0] - first if count is None else count
    q = project(mat, xyz)
    ok = valid_faces(faces, n_v)
    U, V = _pixels(H, W, variant)
    zn = np.float32(z_near)
    for f in range(first, first + count):
        if not ok[f]:
            continue
        tri = [q[faces[f, i]] for i in range(3)]
        n, det = setup(*tri)
        sl = (slice(None), slice(None))
        if box:
            b = _box(tri, det, H, W, z_near)
            if b is None:
                continue
            sl = (slice(b[0], b[1] + 1), slice(b[2], b[3] + 1))
        _, S, cover = _edges(n, U[sl], V[sl], variant)
        if not cover.any():
            continue
        with np.errstate(all="ignore"):
            d = (det / S).astype(np.float32)
        hit = cover & np.isfinite(d) & (d > zn)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        if variant == "largest-id":                                        # among equal depths the LARGEST index wins
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0xffffffff - f)
        keys[sl] = np.minimum(keys[sl], np.where(hit, key, ALL_ONES))
    return int((~ok[first:first + count]).sum())


def resolve(keys, xyz, faces, mat, variant=None):
    """estd_mesh_raster_resolve -> dict(depth, face, bary, facing)"""
    H, W = keys.shape
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    q = project(mat, xyz)
    depth, face = np.zeros((H, W), np.float32), np.full((H, W), -1, np.int32)
    bary, facing = np.zeros((H, W, 2), np.float32), np.zeros((H, W), np.int32)
    U, V = _pixels(H, W, variant)
    won = keys != ALL_ONES
    ids = (keys & np.uint64(0xffffffff)).astype(np.int64)
    if variant == "largest-id":
        ids = 0xffffffff - ids
    for f in np.unique(ids[won]):
        px = won & (ids == f)
        n, _ = setup(*[q[faces[f, i]] for i in range(3)])
        E, S, _ = _edges(n, U[px], V[px])
        with np.errstate(all="ignore"):
            b1, b2 = (E[1] / S).astype(np.float32), (E[2] / S).astype(np.float32)
        depth[px] = (keys[px] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        face[px] = f
        bary[px] = np.stack([b2, b1] if variant == "swapped-bary" else [b1, b2], 1)
        facing[px] = np.where(S < 0, 1, np.where(S > 0, -1, 0))
    return dict(depth=depth, face=face, bary=bary, facing=facing)


def raster(xyz, faces, mat, H, W, z_near, box=False, variant=None, ranges=None):
    """the operator: ``ranges`` [(first, count), ...] splits the mesh over several merges into one key buffer"""
    keys = np.full((H, W), ALL_ONES, np.uint64)
    n_f = np.asarray(faces).reshape(-1, 3).shape[0]
    invalid = sum(merge(keys, xyz, faces, mat, z_near, a, c, box, variant) for a, c in (ranges or [(0, n_f)]))
    return dict(resolve(keys, xyz, faces, mat, variant), invalid=invalid, keys=keys)


def points_of(out, xyz, faces):
    """the 3D point of every covered pixel from face and bary: a + b1 (b - a) + b2 (c - a), float64 -> ([n,3], mask)"""
    m = out["face"] >= 0
    tri = np.asarray(xyz, np.float64)[np.asarray(faces)[out["face"][m]]]
    b = out["bary"][m].astype(np.float64)
    return tri[:, 0] + b[:, :1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:] * (tri[:, 2] - tri[:, 0]), m


def compare(got, want, what=""):
    """equality to the bit of every map and of the invalid count; ``got`` / ``want``: dicts of numpy arrays -> dict(covered, faces seen)"""
    for k, bits in (("depth", np.uint32), ("face", None), ("bary", np.uint32), ("facing", None)):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s is %s %s, expected %s %s" % (what, k, a.dtype, a.shape, b.dtype, b.shape)
        if bits is not None:
            a, b = a.view(bits), b.view(bits)
        bad = a != b
        assert not bad.any(), "%s: %s differs in %d of %d values, first at %s" % (what, k, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
    assert int(got["invalid"]) == int(want["invalid"]), "%s: invalid %d, expected %d" % (what, int(got["invalid"]), int(want["invalid"]))
    return dict(covered=int((want["face"] >= 0).sum()), seen=int(np.unique(want["face"][want["face"] >= 0]).size))


# ------------------------------------------------------------------------------------------------- visibility
def visible_points(points, depth_maps, mats, tol, z_near=1e-3, depth_max=None):
    """in how many of the views a point is seen -> int32 [N].  Per view: q = M (p, 1) in the contract's order, c = q_z, the nearest pixel
    (rint(q_x / c), rint(q_y / c)); seen iff the pixel lies inside the image, c > z_near, c <= depth_max (when given), the rendered
    depth there is positive and c <= depth + tol."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    views = np.zeros(pts.shape[0], np.int32)
    for depth, mat in zip(depth_maps, mats):
        depth = np.asarray(depth, np.float32)
        H, W = depth.shape
        q = project(mat, pts)
        c = q[:, 2]
        with np.errstate(all="ignore"):
            u, v = np.rint(q[:, 0] / c), np.rint(q[:, 1] / c)
        ok = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (c > float(z_near))
        if depth_max is not None:
            ok &= c <= float(depth_max)
        ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
        d = depth[vi, ui].astype(np.float64)
        views += (ok & (d > 0) & (c <= d + float(tol))).astype(np.int32)
    return views


# ------------------------------------------------------------------------------------------------- the cases
def _cam(H, W, eye=(0, 0, 0), target=(0, 0, 1), f=None):
    return raster_matrix(look_at(eye, target), intrinsics(H, W, f))


def _f32(a):
    return np.asarray(a, np.float32).reshape(-1, 3)


def _i32(a):
    return np.asarray(a, np.int32).reshape(-1, 3)


def _one_triangle(H, W):
    # a triangle that covers most of the image and leaves its corners free, slanted in depth
    return _f32([(-0.9, -0.7, 1.5), (1.0, -0.5, 2.5), (-0.2, 0.9, 2.0)]), _i32([(0, 1, 2)]), _cam(H, W), H, W, 1e-3


def _square(H, W, z=2.0, half=4.0, flip=False):
    xyz = _f32([(-half, -half, z), (half, -half, z), (half, half, z), (-half, half, z)])
    faces = _i32([(0, 2, 1), (0, 3, 2)] if flip else [(0, 1, 2), (0, 2, 3)])
    return xyz, faces, _cam(H, W), H, W, 1e-3


def _coincident(n=4096):
    xyz, _, mat, H, W, zn = _one_triangle(4, 4)
    return xyz, _i32([(0, 1, 2)] * n), mat, H, W, zn


def _stacked(n=4096):
    """the same triangle at n depths 1.5 + 1e-3 k, in a shuffled order: the nearest is face 2731, not face 0"""
    rng = np.random.RandomState(5)
    order = rng.permutation(n)
    base = np.asarray([(-3.0, -3.0, 0.0), (3.0, -2.0, 0.0), (0.0, 3.0, 0.0)])
    xyz = np.concatenate([base + (0, 0, 1.5 + 1e-3 * k) for k in order])
    return _f32(xyz), _i32(np.arange(3 * n)), _cam(4, 4), 4, 4, 1e-3


def _subpixel(n=1000):
    rng = np.random.RandomState(7)
    H, W = 24, 32
    c = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), rng.uniform(1.5, 3.0, n)], 1)
    xyz = (c[:, None, :] + rng.uniform(-0.02, 0.02, (n, 3, 3))).reshape(-1, 3)      # about 0.3 pixel across
    return _f32(xyz), _i32(np.arange(3 * n)), _cam(H, W), H, W, 1e-3


def _interpenetrating():
    xyz = _f32([(-1, -1, 1.5), (1, -1, 2.5), (0, 1, 2.0), (-1, -1, 2.5), (1, -1, 1.5), (0, 1, 2.0), (-1, 0.2, 1.2), (1, 0.2, 1.2), (0, -0.3, 3.0)])
    return xyz, _i32([(0, 1, 2), (3, 4, 5), (6, 7, 8)]), _cam(33, 41), 33, 41, 1e-3


def _floor():
    """y points down: a floor 1 m under the camera, from 5 m behind it to 20 m in front"""
    xyz = _f32([(-30, 1, -5), (30, 1, -5), (0, 1, 20)])
    return xyz, _i32([(0, 1, 2)]), _cam(30, 40), 30, 40, 0.25


def _behind():
    xyz = _f32([(-1, -1, -2), (1, -1, -2), (0, 1, -3)])
    return xyz, _i32([(0, 1, 2)]), _cam(16, 16), 16, 16, 1e-3


def _back_faces():
    a = _square(20, 28, z=2.0, half=0.6, flip=True)
    b = _square(20, 28, z=3.0, half=1.5)
    return _f32(np.concatenate([a[0], b[0]])), _i32(np.concatenate([a[1], b[1] + 4])), a[2], 20, 28, 1e-3


def _degenerate():
    """zero-area faces (a repeated index, a repeated position, three positions on a line whose projections are exact) and faces with a NaN
    or infinite vertex: first, last and in runs between the triangles that draw"""
    nan, inf = float("nan"), float("inf")
    xyz = _f32([(-1, -1, 2), (1, -1, 2), (0, 1, 2), (-1, -1, 2), (0, 0, 4), (1, 1, 4), (2, 2, 4), (nan, 0, 2), (0, inf, 2), (0, 0, -inf),
                (-1.5, 1, 3), (1.5, 1, 3), (0, -1.5, 3)])
    bad = [(0, 0, 1), (0, 3, 1), (4, 5, 6), (7, 1, 2), (0, 8, 2), (0, 1, 9), (2, 2, 2)]
    faces = bad[:3] + [(0, 1, 2)] + bad[3:] + bad + [(10, 11, 12)] + bad[::-1]
    # a camera with integer entries: q is exact, so the collinear face has n = 0 exactly
    M = np.asarray([[8, 0, 10, 0], [0, 8, 8, 0], [0, 0, 1, 0]], np.float64).reshape(-1)
    return xyz, _i32(faces), M, 17, 21, 1e-3


def _out_of_range():
    xyz, faces, mat, H, W, zn = _interpenetrating()
    V = xyz.shape[0]
    extra = [(-1, 0, 1), (0, V, 1), (0, 1, 2 ** 31 - 1), (-2 ** 31, 0, 1), (V, V, V)]
    return xyz, _i32(extra[:2] + [tuple(faces[0])] + extra[2:4] + [tuple(f) for f in faces[1:]] + extra[4:]), mat, H, W, zn


def _no_faces():
    xyz, _, mat, H, W, zn = _one_triangle(9, 7)
    return xyz, np.zeros((0, 3), np.int32), mat, H, W, zn


def _no_vertices(n_faces):
    return np.zeros((0, 3), np.float32), _i32([(0, 1, 2)] * n_faces), _cam(9, 7), 9, 7, 1e-3


def _icospheres(pose):
    a, fa = icosphere(4, 0.8, (0.3, 0.0, 3.0))
    b, fb = icosphere(3, 0.5, (-0.6, 0.2, 2.4))
    eye = [(0.0, 0.0, 0.0), (1.5, -0.8, 0.6)][pose]
    H, W = 120, 160
    mat = raster_matrix(look_at(eye, (0.0, 0.0, 2.8)), intrinsics(H, W))
    return _f32(np.concatenate([a, b])), _i32(np.concatenate([fa, fb + a.shape[0]])), mat, H, W, 1e-3


CASES = {
    "tri-1x1": lambda: _one_triangle(1, 1), "tri-8x8": lambda: _one_triangle(8, 8), "tri-9x7": lambda: _one_triangle(9, 7),
    "tri-65x33": lambda: _one_triangle(33, 65), "square-64x48": lambda: _square(48, 64), "coincident-4096": _coincident,
    "stacked-4096": _stacked, "subpixel-1000": _subpixel, "interpenetrating": _interpenetrating, "floor": _floor, "behind": _behind,
    "back-faces": _back_faces, "degenerate": _degenerate, "out-of-range": _out_of_range, "no-faces": _no_faces,
    "no-vertices": lambda: _no_vertices(5), "nothing": lambda: _no_vertices(0), "icospheres-pose0": lambda: _icospheres(0),
    "icospheres-pose1": lambda: _icospheres(1),
}
BOXED = ("icospheres-pose0", "icospheres-pose1", "subpixel-1000")          # swept as the kernel sweeps them (see the module's docstring)
_WANT = {}


def build_case(name):
    """-> (xyz float32 [V,3], faces int32 [F,3], mat float64 [12], H, W, z_near)"""
    return CASES[name]()


def placed_case(place):
    """"interpenetrating" -- three triangles that cross, so the nearest face changes within a pixel row -- built at a placement
    (placement.py): the float64 vertices and the camera moved there, the vertices rounded to fp32 once, the matrix formed in float64 from
    the placed pose.  The projection of the contract is float64 from the fp32 vertices, so the reference stays exact; what the placement
    adds is the cancellation of M_j3 against coordinates of hundreds of metres"""
    import placement as PL
    H, W = 33, 41
    xyz = np.asarray([(-1, -1, 1.5), (1, -1, 2.5), (0, 1, 2.0), (-1, -1, 2.5), (1, -1, 1.5), (0, 1, 2.0), (-1, 0.2, 1.2), (1, 0.2, 1.2), (0, -0.3, 3.0)], np.float64)
    mat = raster_matrix(PL.pose(look_at((0, 0, 0), (0, 0, 1)), place), intrinsics(H, W))
    return PL.points(xyz, place).astype(np.float32), _i32([(0, 1, 2), (3, 4, 5), (6, 7, 8)]), mat, H, W, 1e-3


def expected(name):
    """the reference's maps of a case, computed once and shared (do not modify)"""
    if name not in _WANT:
        _WANT[name] = raster(*build_case(name), box=name in BOXED)
    return _WANT[name]
