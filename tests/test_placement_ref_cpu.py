"""Where the scene lies must not decide a pose solve: the float64 references of registration (tests/rigid_align_ref.py ``refine``) and of
tracking (tests/track_ref.py ``refine_stopped``) at the placements of tests/placement.py -- the scene, its cameras and its source cloud built
d in {0, 8, 64, 512} metres from the world origin along (1, -1, 1/2), and once at 64 m in a world that is also turned about no axis -- and
the host side of estdepth_amd/tracking.py driven by the reference.  No device is needed.

The kernels' Jacobian rows (n, q x n) pivot on the world origin, so the 6 x 6 system couples rotation and translation through |q| and its
condition grows with the square of the scene's distance.  Solved about the world origin the references REFUSE the scene from some tens of
metres on ("condition", COND_MAX = 1e6); solved about a pivot at the scene -- the centre of the target's box, the model camera's centre --
their verdict, their iteration count and the condition of the system are those of the scene at the origin.

Measured with the references (this file prints every figure, pytest -s):
    registration, n = 2000, identity start, cond(A_c) of the first system about the box centre / cond(A) about the world origin
        cloud, plane   d = 0: 49.4 / 76     8: 49.4 / 8.6e5    64: 49.4 / 3.4e9 (refused)   64 turned: 50.5 / 1.8e9   512: 49.4 / 1.4e13
        cloud, point       3.52 / 117         3.52 / 5.8e4        3.52 / 1.8e8 (refused)        2.49 / 2.0e8             3.52 / 6.9e11
        mesh, plane        50.2 / 77          50.2 / 8.7e5        50.2 / 3.4e9 (refused)        51.1 / 1.8e9             50.3 / 1.4e13
        mesh, point        3.53 / 117         3.53 / 5.8e4        3.53 / 1.7e8 (refused)        2.47 / 2.0e8             3.53 / 6.9e11
      the plane metric converges in 4 (cloud) and 3 (mesh) iterations at every placement, 0.19 mm and 1.6e-4 rad off the truth against the
      cloud; the point metric runs to max_iter (30) at every placement but one: against the cloud at 512 m the 30th step is the first below
      the stopping rule (at the origin it is the 33rd).  Nearest-neighbour partners flicker until they settle, and WHEN they settle hangs
      on the last bits of the inputs, which at 512 m are 6e-5 m apart, above STEP_T.  At 512 m the point metric is therefore held to "not
      refused"; every other verdict is held to that at the origin, reason and iteration count.
    tracking, 120 x 160, about the model camera's centre / about the world origin
        cond 152.2 at every placement / 164, 2.5e6 (refused from 8 m on), 9.7e9, 4.9e9, 3.9e13; converged in 3 iterations at every placement
    COND_FACTOR: a translated scene keeps cond(A_c) within 1.05 of the origin's (measured 1.002; the emulation of the kernels' arithmetic
    gave 1.04 at 512 m); the turned scene within 1.5 (measured 1.43: the box whose centre is the pivot is the box of the turned scene).
"""
import numpy as np
import pytest

import placement as PL
import rigid_align_ref as R
import track_ref as T

N = 2000
COND_FACTOR, COND_FACTOR_TURNED = 1.05, 1.5
PLACED = [k for k in PL.PLACES if k != "d0"]


def _within(c, c0, factor):
    return c0 / factor <= c <= c0 * factor


@pytest.fixture(scope="module")
def at_origin():
    """the references at d = 0, once"""
    fx = R.registration_fixture(1.0, N, 3)
    out = {(kind, metric): R.refine(fx["src"], fx[kind], metric=metric, pivot=R.target_pivot(fx[kind])) for kind in ("cloud", "mesh") for metric in ("plane", "point")}
    cf = T.convergence_fixture((120, 160))
    out["track"] = T.refine_stopped(cf["depth"], cf["K"], cf["guess"], cf["model"], pivot=cf["model"]["pose"][:3, 3])
    return out


def test_the_placements_are_built_not_shifted():
    W = PL.matrix(PL.PLACES["d64-rotated"])
    assert np.abs(W[:3, :3] @ W[:3, :3].T - np.eye(3)).max() < 1e-15 and np.abs(np.abs(W[:3, :3]) - 0.5).max() < 0.45      # no entry near 0 or 1
    assert np.array_equal(PL.matrix((512, False))[:3, 3], [512.0, -512.0, 256.0]) and PL.key((0, False)) is None
    fx0, fx = R.registration_fixture(1.0, N, 3), R.registration_fixture(1.0, N, 3, (64, True))
    assert fx["src"].dtype == np.float32 and fx["cloud"]["xyz"].dtype == np.float32 and fx["mesh"]["xyz"].dtype == np.float32
    # the placed fixture is the unplaced one seen from the placed world: the same shape to the placed coordinates' rounding
    back = (fx["src"].astype(np.float64) - W[:3, 3]) @ W[:3, :3]
    assert np.abs(back - fx0["src"]).max() < 4 * 2.0 ** -24 * 128
    assert np.abs(fx["T_true"] @ W - W @ fx0["T_true"]).max() < 1e-12
    assert np.array_equal(R.registration_fixture(1.0, N, 3, (0, False))["src"], fx0["src"])
    cf0, cf = T.convergence_fixture((120, 160)), T.convergence_fixture((120, 160), (64, True))
    assert np.array_equal(cf["depth"], cf0["depth"]) and np.abs(cf["pose"] - W @ cf0["pose"]).max() == 0
    assert np.abs(cf["model"]["normal"].astype(np.float64) - cf0["model"]["normal"].astype(np.float64) @ W[:3, :3].T).max() < 2.0 ** -23


@pytest.mark.parametrize("metric", ["plane", "point"])
@pytest.mark.parametrize("kind", ["cloud", "mesh"])
@pytest.mark.parametrize("where", PLACED)
def test_the_reference_registration_gives_the_origins_verdict(where, kind, metric, at_origin):
    place = PL.PLACES[where]
    fx, base = R.registration_fixture(1.0, N, 3, place), at_origin[(kind, metric)]
    pivot = R.target_pivot(fx[kind])
    out = R.refine(fx["src"], fx[kind], metric=metric, pivot=pivot)
    et, er = R.transform_error(out["T"], fx["T_true"], fx["centre"])
    print("PLACEMENT-REF register %s %s %s: cond(A_c) %.4g (origin %.4g) %s after %d iterations (origin: %s after %d); %.3g m %.3g rad off at the centre"
          % (where, kind, metric, out["cond"], base["cond"], out["reason"], out["iterations"], base["reason"], base["iterations"], et, er))
    assert _within(out["cond"], base["cond"], COND_FACTOR_TURNED if place[1] else COND_FACTOR)
    if metric == "point" and place[0] >= 512:
        assert out["reason"] in ("converged", "max_iter")             # see the module docstring: the inputs' spacing is above STEP_T
    else:
        assert (out["converged"], out["reason"], out["iterations"]) == (base["converged"], base["reason"], base["iterations"])
    if metric == "plane":
        assert out["converged"]
        e0 = R.transform_error(np.eye(4), fx["T_true"], fx["centre"])
        assert et < 0.1 * e0[0] and er < 0.1 * e0[1]


@pytest.mark.parametrize("metric", ["plane", "point"])
@pytest.mark.parametrize("kind", ["cloud", "mesh"])
def test_about_the_world_origin_the_registration_is_refused_at_64_m(kind, metric):
    """the defect, pinned in the reference: the method before the pivot refuses a scene 64 m out for its condition, and returns the start"""
    fx = R.registration_fixture(1.0, N, 3, PL.PLACES["d64"])
    out = R.refine(fx["src"], fx[kind], metric=metric)
    assert not out["converged"] and out["reason"] == "condition" and out["iterations"] == 0 and np.array_equal(out["T"], np.eye(4))
    assert out["cond"] > R.COND_MAX


@pytest.mark.parametrize("where", PLACED)
def test_the_reference_tracking_gives_the_origins_verdict(where, at_origin):
    place = PL.PLACES[where]
    cf, base = T.convergence_fixture((120, 160), place), at_origin["track"]
    out = T.refine_stopped(cf["depth"], cf["K"], cf["guess"], cf["model"], pivot=cf["model"]["pose"][:3, 3])
    et, er = T.pose_error_at(out["pose"], cf["pose"], cf["centre"])
    print("PLACEMENT-REF track %s: cond(A_c) %.4g (origin %.4g) %s after %d iterations; %.3g m %.3g rad off at the centre"
          % (where, out["cond"], base["cond"], out["reason"], out["iterations"], et, er))
    assert base["converged"] and (out["converged"], out["reason"], out["iterations"]) == (True, "converged", base["iterations"])
    assert _within(out["cond"], base["cond"], COND_FACTOR)          # the camera's centre turns with the world: no wider factor is needed
    e0 = T.pose_error_at(cf["guess"], cf["pose"], cf["centre"])
    assert et < 0.1 * e0[0] and er < 0.1 * e0[1]


def test_about_the_world_origin_the_tracking_is_refused_at_64_m():
    cf = T.convergence_fixture((120, 160), PL.PLACES["d64"])
    out = T.refine_stopped(cf["depth"], cf["K"], cf["guess"], cf["model"])
    assert out["reason"] == "condition" and out["iterations"] == 0 and np.array_equal(out["pose"], cf["guess"]) and out["cond"] > 1e6


def test_the_host_layer_solves_about_the_pivot():
    """estdepth_amd.tracking.gauss_newton on the reference's systems at 64 m: refused about the world origin, and about the pivot the very
    iteration of the reference; the pivoted system is the system of the recentred Jacobian rows"""
    from estdepth_amd import tracking
    cf = T.convergence_fixture((120, 160), PL.PLACES["d64-rotated"])
    system = lambda P: T.step(cf["depth"], cf["K"], P, cf["model"])                                             # noqa: E731
    pivot = cf["model"]["pose"][:3, 3]
    plain = tracking.gauss_newton(system, cf["guess"])
    assert plain["reason"] == "condition" and not plain["converged"] and np.array_equal(plain["pose"], cf["guess"])
    out = tracking.gauss_newton(system, cf["guess"], pivot=pivot)
    ref = T.refine_stopped(cf["depth"], cf["K"], cf["guess"], cf["model"], pivot=pivot)
    assert out["converged"] and out["reason"] == "converged" and out["iterations"] == ref["iterations"]
    assert np.abs(out["pose"] - ref["pose"]).max() < 1e-9
    # A_c = G A G^T is the sum of the outer products of the rows (n, (p - c) x n): from the reference's own rows
    s = system(cf["guess"])
    J = s["J"][s["match"] >= 0]
    Jc = np.concatenate([J[:, :3], J[:, 3:] - np.cross(pivot, J[:, :3])], 1)
    Ac, bc = tracking.pivoted(s["A"], s["b"], pivot)
    assert np.abs(Ac - Jc.T @ Jc).max() <= 1e-6 * np.abs(Ac).max() and np.array_equal(Ac, Ac.T)
    assert np.abs(bc - Jc.T @ s["residual"][s["match"] >= 0]).max() <= 1e-6 * np.abs(bc).max()
    assert tracking.pivoted(s["A"], s["b"], None)[0] is s["A"]
    # the step is the twist about the pivot: the pivot itself moves by the twist's translation part alone (to first order)
    xi = 1e-6 * np.array([1.0, -2.0, 0.5, 0.3, 0.7, -1.1])
    E = tracking.pivot_step(xi, pivot)
    assert np.abs(E[:3, :3] @ pivot + E[:3, 3] - pivot - xi[:3]).max() < 1e-11
    assert np.abs(E - R.pivot_step(xi, pivot)).max() == 0 and np.abs(E - T.pivot_step(xi, pivot)).max() == 0
    assert np.array_equal(tracking.pivot_step(xi, None), tracking.exp_se3(xi))


@pytest.mark.parametrize("where", ["d0", "d64", "d64-rotated"])
def test_a_degenerate_target_is_refused_about_any_pivot(where):
    """a plane alone leaves three motions free wherever the twist pivots; so do too few partners and a system that is not positive definite"""
    from estdepth_amd import tracking
    place = PL.PLACES[where]
    p, n = R.single_plane(500, 1)
    p = PL.points(p.astype(np.float64), place).astype(np.float32)
    n = PL.vectors(n.astype(np.float64), place).astype(np.float32)
    target = dict(xyz=p, normal=n)
    for pivot in (R.target_pivot(target), R.target_pivot(target) + np.array([0.7, -0.4, 1.1])):
        out = R.refine(p, target, metric="plane", pivot=pivot)
        assert not out["converged"] and out["reason"] == "condition" and np.array_equal(out["T"], np.eye(4)) and out["cond"] > R.COND_MAX
    fx = R.registration_fixture(1.0, 1000, 3, place)
    out = R.refine(fx["src"][:50], fx["mesh"], metric="plane", min_count=100, pivot=R.target_pivot(fx["mesh"]))
    assert out["reason"] == "count" and np.array_equal(out["T"], np.eye(4))
    # the host layer on a fronto-parallel plane seen by the tracking reference, and its three refusals about a pivot
    cf = T.convergence_fixture((120, 160), place)
    pivot = cf["model"]["pose"][:3, 3]
    system = lambda P: T.step(cf["depth"], cf["K"], P, cf["model"])                                             # noqa: E731
    few = tracking.gauss_newton(system, cf["guess"], min_count=10 ** 6, pivot=pivot)
    assert few["reason"] == "count" and np.array_equal(few["pose"], cf["guess"])
    s = T.step(cf["depth"], cf["K"], cf["guess"], cf["model"])
    flat = s["J"][s["match"] >= 0]
    flat = flat[np.abs(flat[:, :3] @ PL.vectors(np.array([0.0, 0.0, -1.0]), place)) > 0.999999]                 # the rows of the plane's pixels alone
    assert flat.shape[0] > 1000
    A = flat.T @ flat
    assert tracking.solve_step(A, np.ones(6), flat.shape[0], 100, pivot=pivot)[1] in ("cholesky", "condition")
    A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1e-7])
    assert tracking.solve_step(A, np.ones(6), 1000, 100, pivot=pivot)[1] == "condition"
    assert tracking.solve_step(-A, np.ones(6), 1000, 100, pivot=pivot)[1] == "cholesky"
    assert tracking.solve_step(A * np.nan, np.ones(6), 1000, 100, pivot=pivot)[1] == "cholesky"
    assert tracking.solve_step(A, np.ones(6), 10, 100, pivot=pivot)[1] == "count"


# ------------------------------------------------------------------------------------------------------------ the placed cases of the families
@pytest.mark.parametrize("where", list(PL.FAMILY_PLACES))
@pytest.mark.parametrize("name", R.PLACED_CASES)
def test_the_rigid_align_stand_in_stays_under_the_cap_when_placed(name, where):
    """the condition of the placed GPU cases (tests/test_gpu_registration.py): the reference ALONE, through its numpy-fp32 stand-in, keeps the
    ambiguous share under AMB_CAP and every bound of ``compare`` at 64 m and at 512 m"""
    c = R.build_case(name, PL.FAMILY_PLACES[where])
    fig = R.compare(R.standin(c), c, R.reference(name, PL.FAMILY_PLACES[where]), c["name"] + " stand-in")
    assert fig["amb_share"] <= R.AMB_CAP and fig["matched"] >= 0.6 * fig["gated"]
    assert np.abs(c["target"]).max() > PL.FAMILY_PLACES[where][0] / 2


@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_the_track_stand_in_under_the_cap_out_to_128_m(d):
    """frame_align's pixel decision -- which model pixel a point falls into -- is taken from a projection formed in fp32 world coordinates,
    so the share of pixels within the rounding of a pixel edge grows with the distance: 0.015 at 64 m, 0.029 at 128 m, 0.056 at 256 m,
    0.111 at 512 m of the 120 x 160 case.  The cap is a condition, so the family's placed cases are at 64 m and 128 m (T.PLACED_AT), the
    largest power of two under it; beyond, the reference alone already breaks the cap, whatever the kernel does"""
    c = T.build_case(T.PLACED_CASE, (d, False))
    ref = T.reference(T.PLACED_CASE, (d, False))
    share = ref["amb"].sum() / max(ref["valid"].sum(), 1)
    print("PLACEMENT-REF frame_align %s: ambiguous share %.4f (cap %.2f)" % (c["name"], share, T.AMB_CAP))
    assert (share <= T.AMB_CAP) == (d <= max(T.PLACED_AT))
    if d in T.PLACED_AT:
        s = T.evaluate(c, np.float32)
        fig = T.compare(dict(residual=s["residual"], match=s["match"], sums=s["sums"]), c, ref, c["name"] + " stand-in")
        assert fig["matched"] >= 0.7 * fig["valid"]


def _integrated(place, dtype):
    import tsdf_ref as V
    c = V.build_case(V.PLACED_CASE, place)
    mats = V.tsdf_matrices64(c["poses"], c["K"], c["origin"], c["voxel"])
    Z0 = np.zeros(c["dims"], np.float32)
    return c, Z0, V.integrate(Z0, Z0, mats, c["depths"], c["confs"], dtype=dtype, **c["params"])


@pytest.mark.parametrize("where", list(PL.FAMILY_PLACES))
def test_the_tsdf_stand_ins_stay_under_the_cap_when_placed(where):
    """integrate and ray-cast of the smallest case with the cameras and the volume's corner 64 m and 512 m out: the matrices are formed in
    float64 relative to the corner, so the references' ambiguous shares stay where they are at the origin (integrate 0.0009 there, 0.0010
    and 0.0009 placed; ray-cast 0.0028 there, 0.0010 and 0.0011 placed; cap 0.03) and the numpy-fp32 stand-ins pass both comparisons"""
    import tsdf_raycast_ref as RR
    import tsdf_ref as V
    place = PL.FAMILY_PLACES[where]
    c, Z0, ref = _integrated(place, np.float64)
    got = _integrated(place, np.float32)[2]
    fig = V.compare(got["D"], got["Wt"], ref, D_before=Z0, W_before=Z0)
    base = V.build_case(V.PLACED_CASE)
    assert fig["amb_share"] <= V.AMB_CAP and fig["updated"] > 1000
    assert all(float(np.float32(v)) == v for v in c["origin"]) and np.abs(np.asarray(c["origin"]) - np.asarray(base["origin"]) - PL.offset(place[0])).max() < 2e-5
    assert np.array_equal(c["depths"], base["depths"]) and np.abs(c["poses"][:, :3, 3] - base["poses"][:, :3, 3] - PL.offset(place[0])).max() < 1e-12
    pose = PL.pose(RR.HELD_OUT_POSE, place)
    v = RR.view(c, pose)
    args = (got["D"], got["Wt"], v["M"], v["H"], v["W"], RR.T_MIN, v["dt"], v["n_steps"], 1.0)
    ray = RR.compare(RR.raycast(*args, dtype=np.float32), RR.raycast(*args), c["name"])
    print("PLACEMENT-REF tsdf %s: ambiguous share integrate %.4f, ray-cast %.4f" % (c["name"], fig["amb_share"], ray["amb_share"]))
    assert ray["amb_share"] <= RR.AMB_CAP and ray["hit"] > 1000


@pytest.mark.parametrize("where", ["d64", "d64-rotated", "d512"])
def test_the_other_families_references_accept_their_stand_ins_when_placed(where):
    """cloud_nearest, mesh_nearest and mesh_sample have no ambiguity cap (mesh_sample's is the share of face normals left out): their
    numpy stand-ins pass the unchanged comparisons on the placed cases; the rasteriser and the simplifier are compared to the bit, and
    their references see what they see at the origin"""
    import cloud_metrics_ref as C
    import mesh_distance_ref as MD
    import mesh_raster_ref as MR
    import mesh_sample_ref as MS
    import mesh_simplify_ref as SI
    place = PL.PLACES[where]
    c = C.build_case(C.PLACED_CASE, place)
    d, i = C.nearest32(c["query"], c["target"], c["max_dist"])
    assert C.compare(d, i, c["query"], c["target"], c["max_dist"], C.nearest64(c["query"], c["target"])[0], c["name"])["found"] >= 1
    if not place[1]:
        m = MD.build_case(MD.PLACED_CASE, place)
        fig = MD.compare(MD.nearest_planted(m["q"], m["xyz"], m["faces"], m["max_dist"]), m, "%s@%s" % (MD.PLACED_CASE, where))
        assert fig["found"] > 30
    host = MS.placed_case(place)
    fig = MS.compare(MS.as_got(MS.sample(*host)), *host, "%s@%s" % (MS.PLACED_CASE, where))
    assert fig["left_out"] <= MS.LEFT_OUT_CAP * fig["faces"] and fig["samples"] == host[3]
    flat, placed = MR.expected("interpenetrating"), MR.raster(*MR.placed_case(place))
    assert abs(int((placed["face"] >= 0).sum()) - int((flat["face"] >= 0).sum())) <= 2 and (placed["face"] != flat["face"]).mean() < 0.02
    both = (placed["face"] >= 0) & (flat["face"] >= 0)
    assert np.abs(placed["depth"][both].astype(np.float64) - flat["depth"][both]).max() < 64 * 2.0 ** -24 * max(place[0], 1)
    xyz, faces = SI.patch(SI.PLACED_FACES, place=place)
    stats = SI.simplify(xyz, faces, 0.1)["stats"]
    assert 10 < stats["vertices"] < 40 and stats["faces"] > 10 and stats["invalid"] == 0
