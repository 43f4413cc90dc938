"""CPU: the reference of the mesh rasteriser (tests/mesh_raster_ref.py) against geometry that needs no rasteriser to state -- planes and
a sphere with analytic depths, exact coverage counts, the tie and order rules, triangles behind and under the camera -- so that the
device's equality with the reference (tests/test_gpu_mesh_raster_routes.py) means equality with the contract.  The comparison itself is
tested too: it has to reject each of five deliberately broken rasterisers."""
import numpy as np
import pytest

import mesh_raster_ref as R


def _square_on_pixels(order=(0, 1), flip=False):
    """a fronto-parallel square at z = 2 whose corners project onto the pixel centres (4, 3) and (20, 19) of a 24 x 28 image"""
    H, W, f, z = 24, 28, 16.0, 2.0
    K = np.asarray([[f, 0, 12.0], [0, f, 11.0], [0, 0, 1]])
    x0, x1, y0, y1 = ((4 - 12) * z / f, (20 - 12) * z / f, (3 - 11) * z / f, (19 - 11) * z / f)        # -1, 1, -1, 1: exact
    xyz = np.asarray([(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)], np.float32)
    tris = [(0, 2, 1), (0, 3, 2)] if flip else [(0, 1, 2), (0, 2, 3)]
    return xyz, np.asarray([tris[i] for i in order], np.int32), R.raster_matrix(np.eye(4), K), H, W


def test_a_square_on_pixel_centres_is_covered_exactly_once():
    xyz, faces, mat, H, W = _square_on_pixels()
    out = R.raster(xyz, faces, mat, H, W, 1e-3)
    inside = np.zeros((H, W), bool)
    inside[3:20, 4:21] = True                                       # the border pixels have E = 0: they belong to the square
    assert np.array_equal(out["face"] >= 0, inside)
    assert np.all(out["depth"][inside] == np.float32(2.0)) and np.all(out["depth"][~inside] == 0)
    # each triangle alone covers its half and the diagonal; together the diagonal (E = 0 exactly for both) goes to face 0
    alone = [R.raster(xyz, faces[i:i + 1], mat, H, W, 1e-3)["face"] >= 0 for i in range(2)]
    assert np.array_equal(alone[0] | alone[1], inside)
    both = alone[0] & alone[1]
    rows, cols = np.nonzero(both)
    assert both.sum() == 17 and np.array_equal(rows - 3, cols - 4)
    assert np.all(out["face"][both] == 0)
    swapped = R.raster(xyz, faces[::-1].copy(), mat, H, W, 1e-3)
    assert np.all(swapped["face"][both] == 0) and np.array_equal(swapped["depth"].view(np.uint32), out["depth"].view(np.uint32))
    assert np.all(out["facing"][inside] == -1)                      # 0 1 2 runs clockwise on a screen whose y points down
    assert np.all(R.raster(*_square_on_pixels(flip=True), 1e-3)["facing"][inside] == 1)


def _plane_depth(n, p0, pose, K, H, W):
    """z-depth of the plane n . (x - p0) = 0 along every pixel's ray, float64"""
    V, U = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([U, V, np.ones_like(U)], -1) @ np.linalg.inv(K).T @ pose[:3, :3].T      # world direction per unit z-depth
    return ((np.asarray(p0) - pose[:3, 3]) @ n) / (rays @ n)


def test_a_slanted_plane_has_the_analytic_depth():
    H, W = 30, 40
    K, pose = R.intrinsics(H, W), R.look_at((0.2, -0.1, 0.0), (0.0, 0.1, 2.0))
    n = np.asarray([0.3, -0.2, 1.0])
    n /= np.linalg.norm(n)
    p0 = np.asarray([0.0, 0.0, 2.5])
    a, b = np.cross(n, (0, 1, 0)), None
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    xyz = np.asarray([p0 - 9 * a - 9 * b, p0 + 9 * a - 9 * b, p0 + 9 * a + 9 * b, p0 - 9 * a + 9 * b], np.float32)
    out = R.raster(xyz, np.asarray([(0, 1, 2), (0, 2, 3)], np.int32), R.raster_matrix(pose, K), H, W, 1e-3)
    assert np.all(out["face"] >= 0)
    # the plane through the ROUNDED corners: refit it, so that only the rasteriser's float64 arithmetic and one fp32 rounding remain
    c = xyz.astype(np.float64)
    n32 = np.cross(c[1] - c[0], c[2] - c[0])
    want = _plane_depth(n32 / np.linalg.norm(n32), c[0], pose, K, H, W)
    assert np.abs(out["depth"] - want).max() <= 2.0 ** -23 * want.max()          # half an ulp of fp32 and then some
    pts, m = R.points_of(out, xyz, [(0, 1, 2), (0, 2, 3)])
    q = R.project(R.raster_matrix(pose, K), pts.astype(np.float32))
    V, U = np.nonzero(m)
    assert np.abs(q[:, 0] / q[:, 2] - U).max() < 1e-3 and np.abs(q[:, 1] / q[:, 2] - V).max() < 1e-3      # bary puts the point on the pixel's ray


def test_an_icosphere_against_the_analytic_sphere():
    """A level-2 icosphere (320 triangles) of radius r inscribed in the sphere: its longest edge e is that of the level-0 edge's middle
    pieces, e <= 2 r sin(theta / 2) with theta = 63.435 / 4 degrees; a chord of length e lies at most the sagitta s = r (1 - cos(asin(e /
    (sqrt(3) r)))) inside the sphere at a triangle's centre (circumradius e / sqrt(3) for the worst, equilateral, case).  Along a ray
    that meets the sphere at an angle a from its normal the depth error is at most s / cos(a); the test keeps cos(a) >= 0.5."""
    r, centre = 0.5, np.asarray([0.1, -0.05, 2.0])
    xyz, faces = R.icosphere(2, r, centre)
    H, W = 48, 64
    K = R.intrinsics(H, W)
    out = R.raster(xyz, faces, R.raster_matrix(np.eye(4), K), H, W, 1e-3, box=True)
    e = np.linalg.norm(xyz[faces[:, 0]].astype(np.float64) - xyz[faces[:, 1]], axis=1).max()
    sag = r * (1.0 - np.cos(np.arcsin(min(1.0, e / (3 ** 0.5 * r)))))
    V, U = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([U, V, np.ones_like(U)], -1) @ np.linalg.inv(K).T
    bq, cq = d @ centre, centre @ centre - r * r
    aq = (d * d).sum(-1)
    disc = bq * bq - aq * cq
    hit = disc > 0
    t = np.where(hit, (bq - np.sqrt(np.where(hit, disc, 0))) / aq, 0)              # z-depth of the near intersection
    normal = (d * t[..., None] - centre) / r
    cos_a = -(normal * d).sum(-1) / np.sqrt(aq)
    steep = hit & (cos_a >= 0.5)
    assert steep.sum() > 300 and np.all(out["face"][steep] >= 0)
    err = out["depth"][steep] - t[steep]
    assert err.min() >= -1e-6 and err.max() <= sag / 0.5 + 1e-6, (err.min(), err.max(), sag)
    assert np.all(out["face"][~hit] == -1) and np.all(out["facing"][out["face"] >= 0] == 1)      # inscribed; outward = counter-clockwise


def test_no_hole_along_a_shared_edge_under_1000_subpixel_shifts():
    """two triangles sharing an edge, in either face order and with either winding: the quadrilateral's interior is covered whatever the
    sub-pixel position of the edge"""
    rng = np.random.RandomState(11)
    H, W = 12, 14
    K = R.intrinsics(H, W, 10.0)
    mat = R.raster_matrix(np.eye(4), K)
    base = np.asarray([(-1.0, -0.9, 2.0), (1.1, -0.7, 2.3), (0.9, 1.0, 2.1), (-0.8, 0.8, 1.9)])
    for i in range(1000):
        xyz = (base + np.concatenate([rng.uniform(-0.2, 0.2, 2), [0]])).astype(np.float32)
        tris = [[(0, 1, 2), (0, 2, 3)], [(0, 2, 3), (0, 1, 2)], [(0, 2, 1), (0, 2, 3)], [(2, 1, 0), (3, 2, 0)]][i % 4]
        out = R.raster(xyz, np.asarray(tris, np.int32), mat, H, W, 1e-3)
        # inside the quadrilateral by exact-enough float64 half-plane tests on the rounded corners, with a margin that keeps off its border
        q = R.project(mat, xyz)
        p = q[:, :2] / q[:, 2:]
        V, U = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        inside = np.ones((H, W), bool)
        for a, b in ((0, 1), (1, 2), (2, 3), (3, 0)):
            inside &= ((p[b, 0] - p[a, 0]) * (V - p[a, 1]) - (p[b, 1] - p[a, 1]) * (U - p[a, 0])) > 1e-9
        assert inside.sum() > 20 and np.all(out["face"][inside] >= 0), i


def test_a_tie_goes_to_the_smallest_face_and_a_permutation_maps_the_ids():
    xyz, faces, mat, H, W, zn = R.build_case("coincident-4096")
    out = R.raster(xyz, faces[:64], mat, H, W, zn)
    assert (out["face"] >= 0).any() and np.all(out["face"][out["face"] >= 0] == 0)
    xyz, faces, mat, H, W, zn = R.build_case("interpenetrating")
    a = R.raster(xyz, faces, mat, H, W, zn)
    perm = np.asarray([2, 0, 1])
    b = R.raster(xyz, faces[perm], mat, H, W, zn)
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
    m = a["face"] >= 0
    assert len(np.unique(a["face"][m])) == 3 and np.array_equal(perm[b["face"][m]], a["face"][m])


def test_a_floor_under_and_behind_the_camera():
    xyz, faces, mat, H, W, zn = R.build_case("floor")
    out = R.raster(xyz, faces, mat, H, W, zn)
    m = out["face"] >= 0
    assert m.any() and out["depth"][m].min() > np.float32(zn)
    # the floor y = 1 (y points down) through pixel row v: depth = f / (v - cy); rows at and above the horizon see nothing
    K = R.intrinsics(H, W)
    rows = np.arange(H)
    want = np.where(rows > K[1, 2], K[1, 1] / np.maximum(rows - K[1, 2], 1e-9), 0)
    mid = W // 2
    for v in rows:
        if want[v] > 0 and want[v] < 19:
            assert m[v, mid] and abs(out["depth"][v, mid] - want[v]) < 1e-5 * want[v], v
        if want[v] == 0:
            assert not m[v].any(), v
    assert R.raster(*R.build_case("behind"))["face"].max() == -1
    assert R.raster(*R.build_case("behind"), box=True)["face"].max() == -1


def test_faces_that_draw_nothing():
    xyz, faces, mat, H, W, zn = R.build_case("degenerate")
    out = R.raster(xyz, faces, mat, H, W, zn)
    drawn = np.unique(out["face"][out["face"] >= 0])
    assert list(drawn) == [3, 15] and out["invalid"] == 0          # the two real triangles; NaN and flat faces are valid and cover nothing
    xyz, faces, mat, H, W, zn = R.build_case("out-of-range")
    out = R.raster(xyz, faces, mat, H, W, zn)
    assert out["invalid"] == 5 and set(np.unique(out["face"])) <= {-1, 2, 5, 6}
    for name in ("no-faces", "no-vertices", "nothing"):
        out = R.raster(*R.build_case(name))
        assert out["face"].max() == -1 and out["depth"].max() == 0 and out["invalid"] == (5 if name == "no-vertices" else 0)


@pytest.mark.parametrize("name", ["interpenetrating", "out-of-range", "degenerate", "floor", "back-faces", "tri-9x7"])
def test_split_ranges_and_the_box_give_the_same_bits(name):
    case = R.build_case(name)
    whole = R.raster(*case)
    F = case[1].shape[0]
    for ranges in ([(0, F // 2), (F // 2, F - F // 2)], [(F // 2, F - F // 2), (0, F // 2)], [(i, 1) for i in range(F)][::-1]):
        R.compare(R.raster(*case, ranges=ranges), whole, "%s in %d ranges" % (name, len(ranges)))
    R.compare(R.raster(*case, box=True), whole, name + " boxed")


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_the_comparison_rejects_a_broken_rasteriser(variant):
    """each variant differs from the contract on at least one of these cases, and compare says so"""
    caught = 0
    for name, case in (("square", _square_on_pixels()[:5] + (1e-3,)), ("back-faces", R.build_case("back-faces")),
                       ("coincident", R.build_case("coincident-4096")[:1] + (R.build_case("coincident-4096")[1][:8],) + R.build_case("coincident-4096")[2:]),
                       ("tri-9x7", R.build_case("tri-9x7"))):
        want = R.raster(*case)
        R.compare(R.raster(*case), want, name)
        try:
            R.compare(R.raster(*case, variant=variant), want, name)
        except AssertionError:
            caught += 1
    assert caught >= 1, variant


def test_visible_points():
    """a wall at z = 2 seen from the origin; tol = 0.05"""
    H, W = 24, 32
    K = R.intrinsics(H, W)
    mat = R.raster_matrix(np.eye(4), K)
    xyz, faces = np.asarray([(-1, -1, 2), (1, -1, 2), (1, 1, 2), (-1, 1, 2)], np.float32), np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)
    depth = R.raster(xyz, faces, mat, H, W, 1e-3)["depth"]
    tol = 0.05
    pts = np.asarray([(0.1, 0.1, 2.0 + 2 * tol), (0.1, 0.1, 2.0), (0.1, 0.1, 2.0 + 0.9 * tol), (5.0, 0.0, 2.0), (0.1, 0.1, -1.0), (0.0, 0.0, 1.0),
                      (1.3, 0.0, 2.0)], np.float32)
    # behind the wall; on it; hidden by less than tol; outside the image; behind the camera; in front of the wall; beside the wall (no depth)
    assert list(R.visible_points(pts, [depth], [mat], tol)) == [0, 1, 1, 0, 0, 1, 0]
    assert list(R.visible_points(pts, [depth, depth], [mat, mat], tol)) == [0, 2, 2, 0, 0, 2, 0]
    assert list(R.visible_points(pts, [depth], [mat], tol, depth_max=1.5)) == [0, 0, 0, 0, 0, 1, 0]
    assert list(R.visible_points(pts, [depth], [mat], tol, z_near=1.5)) == [0, 1, 1, 0, 0, 0, 0]
