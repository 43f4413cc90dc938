"""estdepth_amd/registration.py and estdepth_amd/tracking.py on the device with the scene AWAY from the world origin: the placements of
tests/placement.py -- d in {0, 8, 64, 512} metres along (1, -1, 1/2), and at 64 m once more in a world that is also turned about no axis.
Every scene is built in float64 at its placement and rounded to fp32 once.  tests/test_placement_ref_cpu.py holds the float64 references to
the same placements; about the world origin they refuse the scene at 64 m for its condition, which is what ``register``, ``refine_pose``
and ``TSDFVolume.track`` did before they solved about a pivot.

    register            registration_fixture(1.0, n = 2000): plane metric against the 8 000-point cloud (the bar below), against the mesh
                        and the point metric against the cloud (verdict and figures)
    TSDFVolume.track,   the frame and the guess of track_ref.convergence_fixture((120, 160)) against a 128^3 volume fused from eight views
    refine_pose         of the scene at 3 cm, its model rendered once at the guess; refine_pose also against the fixture's analytic model

The bar: ``converged`` at 0, 8, 64 m and in the turned world (at 512 m the reason may be "max_iter": the fp32 coordinates are 6e-5 m apart
there, above STEP_T = 1e-5 m, so a step need never fall under the stopping rule; the reason is recorded), and at EVERY placement the error of
the returned transform at the scene's centre in metres and its rotation error are at most MARGIN = 1.25 times the error of the float64
reference on the same inputs (run_stream_ref's semantic bar).  The reference of tracking iterates on the device's own rendered maps, as in
tests/test_gpu_track.py.  Against the fixture's ANALYTIC model the reference's own error is the rounding of its fp32 matrices (1e-8 m and no
measurable angle at the origin), which bounds nothing; there the verdict is asserted and the pose must come ten times closer to the truth.
``compare_meshes(align=...)`` at 64 m reports the alignment block it reports at the origin: the same verdict, and the aligned accuracy back
within the repeatability of the unmoved prediction's (the rule of tests/test_gpu_registration.py).

Every figure is printed on a PLACEMENT line (pytest -s); a device run's are in profiles/placement_gpu_tests.txt."""
import numpy as np
import pytest
import torch

from estdepth_amd import registration, tracking

import placement as PL
import rigid_align_ref as R
import track_ref as T
import tsdf_ref as V

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 1.25                # run_stream_ref.MARGIN, the project's semantic bar
N = 2000
HW = (120, 160)
DIMS = (128, 128, 128)       # 3.84 m at 3 cm about the scene's centre: the turned scene fits as well as the upright one
STAGED = (0.4, 0.2, 0.1)
WHERE = list(PL.PLACES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _target(fx, kind):
    return {k: _dev(v) for k, v in fx[kind].items()}


def _x(got, ref):
    return got / ref if ref > 0 else float("inf") if got > 0 else 0.0


def _cond(A, b, pivot):
    return float(np.linalg.cond(tracking.pivoted(A, b, pivot)[0]))


# ------------------------------------------------------------------------------------------------------------ registration
@pytest.mark.parametrize("where", WHERE)
def test_register_is_as_good_as_its_reference_wherever_the_scene_lies(where):
    place = PL.PLACES[where]
    fx = R.registration_fixture(1.0, N, 3, place)
    src, tgt = _dev(fx["src"]), _target(fx, "cloud")
    pivot = registration.target_pivot(tgt, R.DIST_MAX)
    assert np.array_equal(pivot, R.target_pivot(fx["cloud"]))                      # the same pivot to the bit: reference and product are one method
    ref = R.refine(fx["src"], fx["cloud"], metric="plane", pivot=pivot)
    out = registration.register(src, tgt, metric="plane", dist_max=R.DIST_MAX)
    first = registration.rigid_system(src, np.eye(4), tgt, metric="plane", dist_max=R.DIST_MAX)
    cond, cond0 = _cond(first["A"], first["b"], pivot), float(np.linalg.cond(first["A"]))
    tr, ar = R.transform_error(ref["T"], fx["T_true"], fx["centre"])
    td, ad = R.transform_error(out["T"], fx["T_true"], fx["centre"])
    print("PLACEMENT register cloud plane %s: %s after %d iterations (reference %s after %d); cond(A_c) %.4g (reference %.4g; about the world origin %.3g); "
          "at the centre %.4g m %.4g rad off (reference %.4g m %.4g rad: x%.3f x%.3f); rmse %.3g count %d"
          % (where, out["reason"], out["iterations"], ref["reason"], ref["iterations"], cond, ref["cond"], cond0, td, ad, tr, ar, _x(td, tr), _x(ad, ar),
             out["rmse"], out["count"]))
    assert ref["converged"] and out["reason"] not in registration.REFUSALS
    if place[0] < 512:
        assert out["converged"] and out["reason"] == "converged"
    else:
        assert out["reason"] in ("converged", "max_iter")
    assert td <= MARGIN * tr and ad <= MARGIN * ar
    assert cond <= 1.05 * ref["cond"] and cond < 1e3                                 # the fp32 products of the kernel leave the pivoted system what it is


@pytest.mark.parametrize("kind,metric", [("mesh", "plane"), ("cloud", "point")])
@pytest.mark.parametrize("where", WHERE)
def test_register_is_not_refused_on_the_other_routes(where, kind, metric):
    """the mesh target (the reference lands on the truth to 1e-9 m at the origin: the source ARE samples of the mesh, so its error bounds
    nothing: there the verdict, and the result ten times closer than the start) and the point metric (which runs to max_iter in the reference
    too and is still 3.8 mm off when it stops: there MARGIN times the reference's error, as for the plane metric against the cloud)"""
    place = PL.PLACES[where]
    fx = R.registration_fixture(1.0, N, 3, place)
    ref = R.refine(fx["src"], fx[kind], metric=metric, pivot=R.target_pivot(fx[kind]))
    out = registration.register(_dev(fx["src"]), _target(fx, kind), metric=metric, dist_max=R.DIST_MAX)
    t0, a0 = R.transform_error(np.eye(4), fx["T_true"], fx["centre"])
    tr, ar = R.transform_error(ref["T"], fx["T_true"], fx["centre"])
    td, ad = R.transform_error(out["T"], fx["T_true"], fx["centre"])
    print("PLACEMENT register %s %s %s: %s after %d iterations (reference %s after %d); at the centre %.4g m %.4g rad off (reference %.4g m %.4g rad; start %.4g m "
          "%.4g rad)" % (kind, metric, where, out["reason"], out["iterations"], ref["reason"], ref["iterations"], td, ad, tr, ar, t0, a0))
    assert out["reason"] not in registration.REFUSALS and ref["reason"] not in registration.REFUSALS
    if metric == "plane" and place[0] < 512:
        assert out["converged"] and ref["converged"]
    if metric == "plane":
        assert td <= 0.1 * t0 and ad <= 0.1 * a0
    else:
        assert td <= MARGIN * tr and ad <= MARGIN * ar and td < t0 and ad < a0


def _aligned_scores(place):
    from estdepth_amd.cloud_metrics import compare_meshes
    fx = R.registration_fixture(1.0, N, 3, place)
    gt = _target(fx, "mesh")
    fine_xyz, fine_faces = R.subdivided(*R.scene_mesh())                               # the same surface with other faces, as in test_gpu_registration.py
    Ti = np.linalg.inv(R.exp_se3(R.TWIST))
    pred = dict(xyz=_dev(PL.points(fine_xyz.astype(np.float64), place).astype(np.float32)), faces=_dev(fine_faces))
    moved = dict(xyz=_dev(PL.points(fine_xyz.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], place).astype(np.float32)), faces=pred["faces"])
    base = compare_meshes(pred, gt, 1000.0)
    repeat = max(abs(compare_meshes(pred, gt, 1000.0, seed=s)["accuracy"] - base["accuracy"]) for s in (1, 2, 3))
    plain = compare_meshes(moved, gt, 1000.0)
    got = compare_meshes(moved, gt, 1000.0, align=dict(metric="plane", dist_max=STAGED))
    td, ad = R.transform_error(np.asarray(got["alignment"]["T"]).reshape(4, 4), fx["T_true"], fx["centre"])
    return dict(base=base, repeat=repeat, plain=plain, got=got, err=(td, ad))


def test_compare_meshes_aligns_at_64_m_as_at_the_origin():
    s0, s64 = _aligned_scores(None), _aligned_scores(PL.PLACES["d64"])
    for where, s in (("d0", s0), ("d64", s64)):
        al = s["got"]["alignment"]
        print("PLACEMENT compare_meshes %s: %s after %d iterations, overlap %.3f rmse %.3g; accuracy unmoved %.6f (repeatability %.3g), offset %.6f, aligned %.6f; "
              "T off by %.3g m %.3g rad at the centre" % (where, al["reason"], al["iterations"], al["overlap"], al["rmse"], s["base"]["accuracy"], s["repeat"],
                                                         s["plain"]["accuracy"], s["got"]["accuracy"], s["err"][0], s["err"][1]))
        assert sorted(al) == ["T", "converged", "correction", "iterations", "overlap", "reason", "rmse"]
        assert al["converged"] and al["reason"] == "converged"
        assert s["plain"]["accuracy"] > s["base"]["accuracy"] + s["repeat"]
        assert abs(s["got"]["accuracy"] - s["base"]["accuracy"]) <= s["repeat"]
    a0, a64 = s0["got"]["alignment"], s64["got"]["alignment"]
    assert (a64["converged"], a64["reason"]) == (a0["converged"], a0["reason"])


# ------------------------------------------------------------------------------------------------------------ tracking
_VIEWS = {}


def _views():
    """the eight views of tests/test_gpu_track.py's volume: depth maps do not change when the world moves with its cameras"""
    if not _VIEWS:
        K = V.intrinsics(*HW)
        poses = V.scene_poses(8, seed=2)
        _VIEWS.update(K=K, poses=poses, depths=np.stack([T.scene_maps(P, K, *HW)[0] for P in poses]).astype(np.float32))
    return _VIEWS


def _fused(place):
    from estdepth_amd.fusion3d import TSDFVolume
    v, cf = _views(), T.convergence_fixture(HW, place)
    half = 0.5 * V.VOXEL * np.array(DIMS[::-1], np.float64)
    vol = TSDFVolume(DIMS, V.VOXEL, tuple(cf["centre"] - half), device=DEV)
    vol.integrate(_dev(v["depths"]), torch.from_numpy(PL.pose(v["poses"], place)), torch.from_numpy(v["K"]))
    assert np.abs(vol.centre - cf["centre"]).max() <= 2.0 ** -23 * max(np.abs(cf["centre"]).max(), 1.0)      # the origin is an fp32 value
    return vol, cf


@pytest.mark.parametrize("where", WHERE)
def test_track_is_as_good_as_its_reference_wherever_the_scene_lies(where):
    place = PL.PLACES[where]
    vol, cf = _fused(place)
    K, Kt, depth, guess = cf["K"], torch.from_numpy(cf["K"]), _dev(cf["depth"]), cf["guess"]
    t0, a0 = T.pose_error_at(guess, cf["pose"], cf["centre"])
    out = vol.track(depth, torch.from_numpy(guess), Kt)
    maps = vol.render(torch.from_numpy(guess), Kt, HW)
    model_dev = dict(depth=maps["depth"], normal=maps["normal"], pose=torch.from_numpy(guess), K=Kt)
    model = dict(depth=maps["depth"].cpu().numpy(), normal=maps["normal"].cpu().numpy(), pose=guess, K=K)
    first = tracking.align_step(depth, Kt, torch.from_numpy(guess), model_dev, dist_max=vol.trunc, z_near=vol.z_near)
    for label, got, pivot in (("TSDFVolume.track", out, vol.centre),
                              ("refine_pose", tracking.refine_pose(depth, Kt, torch.from_numpy(guess), model_dev, dist_max=vol.trunc, z_near=vol.z_near), guess[:3, 3])):
        P_ref, _ = T.refine(cf["depth"], K, guess, model, iters=10, pivot=pivot, dist_max=vol.trunc, z_near=vol.z_near)
        tr, ar = T.pose_error_at(P_ref, cf["pose"], cf["centre"])
        td, ad = T.pose_error_at(got["pose"].numpy(), cf["pose"], cf["centre"])
        print("PLACEMENT %s %s: %s after %d iterations; cond(A_c) %.4g (about the world origin %.3g); at the centre %.4g m %.4g rad off (reference, 10 iterations: "
              "%.4g m %.4g rad: x%.3f x%.3f; guess %.4g m %.4g rad); rmse %.3g -> %.3g, count %d"
              % (label, where, got["reason"], got["iterations"], _cond(first["A"], first["b"], pivot), float(np.linalg.cond(first["A"])), td, ad, tr, ar, _x(td, tr),
                 _x(ad, ar), t0, a0, got["trace"][0]["rmse"], got["trace"][-1]["rmse"], got["trace"][0]["count"]))
        assert got["reason"] not in registration.REFUSALS
        if place[0] < 512:
            assert got["converged"] and got["reason"] == "converged"
        else:
            assert got["reason"] in ("converged", "max_iter")
        assert td <= MARGIN * tr and ad <= MARGIN * ar
        assert td < t0 and ad < a0 and _cond(first["A"], first["b"], pivot) < 1e3
    assert out["matched_share"] > 0.8


@pytest.mark.parametrize("where", WHERE)
def test_refine_pose_on_the_analytic_model(where):
    """the convergence fixture as it stands: the model maps are the analytic scene's at the true pose.  The pivot is refine_pose's own, the
    model camera's centre."""
    place = PL.PLACES[where]
    cf = T.convergence_fixture(HW, place)
    Kt, guess = torch.from_numpy(cf["K"]), torch.from_numpy(cf["guess"])
    model = dict(depth=_dev(cf["model"]["depth"]), normal=_dev(cf["model"]["normal"]), pose=torch.from_numpy(cf["model"]["pose"]), K=Kt)
    pivot = cf["model"]["pose"][:3, 3]
    ref = T.refine_stopped(cf["depth"], cf["K"], cf["guess"], cf["model"], pivot=pivot)
    out = tracking.refine_pose(_dev(cf["depth"]), Kt, guess, model, dist_max=T.DIST_MAX)
    first = tracking.align_step(_dev(cf["depth"]), Kt, guess, model, dist_max=T.DIST_MAX)
    t0, a0 = T.pose_error_at(cf["guess"], cf["pose"], cf["centre"])
    tr, ar = T.pose_error_at(ref["pose"], cf["pose"], cf["centre"])
    td, ad = T.pose_error_at(out["pose"].numpy(), cf["pose"], cf["centre"])
    cond = _cond(first["A"], first["b"], pivot)
    print("PLACEMENT refine_pose analytic %s: %s after %d iterations (reference %s after %d); cond(A_c) %.4g (reference %.4g; about the world origin %.3g); at the "
          "centre %.4g m %.4g rad off (reference %.4g m %.4g rad; guess %.4g m %.4g rad)"
          % (where, out["reason"], out["iterations"], ref["reason"], ref["iterations"], cond, ref["cond"], float(np.linalg.cond(first["A"])), td, ad, tr, ar, t0, a0))
    assert ref["converged"] and out["reason"] not in registration.REFUSALS
    if place[0] < 512:
        assert out["converged"] and out["reason"] == "converged"
    assert td <= 0.1 * t0 and ad <= 0.1 * a0
    assert cond <= 1.05 * ref["cond"]
