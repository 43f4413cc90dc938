"""estdepth_amd/registration.py on the device against the float64 reference registration of tests/rigid_align_ref.py (``refine``: brute-force
correspondences, the same gates, the same solve and the same stopping rule).

The convergence fixture: 4 000 samples of the scene's mesh (the plane and two spheres of tests/track_ref.py as 162 triangles) moved by the
inverse of Exp(TWIST) -- about 1 cm and 0.5 degrees -- and once by ten times that with the staged dist_max (0.4, 0.2, 0.1).  ``register``
against the ``TriangleGrid`` of the unmoved mesh (plane metric) and against 16 000 other samples of it through a ``PointGrid`` (both
metrics) must land where the reference lands.  The allowed gap is measured, not chosen: the device may be off the TRUE transform by
2 x the reference's own error plus the stopping step (1e-5 m, 1e-5 rad) -- the factor 2 because the partners may differ on ambiguous
points.  The figures are printed (REGISTRATION lines; recorded in profiles/rigid_align_gpu_tests.txt and DESIGN 3.16).

Refusals return the guess unchanged: a single plane ("condition"), fewer than min_count partners ("count").  ``rigid_system`` twice gives
the same 29 doubles bit for bit under both bindings.  ``compare_meshes(align=...)`` on a prediction offset by the small twist brings the
accuracy back to the unmoved prediction's figure within the sampled scores' own repeatability, MEASURED here as the largest change of
that figure over three other sampling seeds; without ``align`` the result has today's keys and bits.

Away from the origin: the 257-point cases of both metrics and of both ways to read the target, built 64 m and 512 m out (tests/placement.py),
through ``rigid_align_ref.compare`` unchanged -- the bounds scale with the coordinates, the ambiguous share stays under its cap (the
reference alone: tests/test_placement_ref_cpu.py).  The pose solves at those placements: tests/test_gpu_placement.py."""
import numpy as np
import pytest
import torch

from estdepth_amd import registration

import placement as PL
import rigid_align_ref as R
from test_gpu_recon3d_routes import _dev, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STAGED = (0.4, 0.2, 0.1)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _target(fx, kind):
    if kind == "mesh":
        return dict(xyz=_dev(fx["mesh"]["xyz"]), faces=_dev(fx["mesh"]["faces"]))
    return dict(xyz=_dev(fx["cloud"]["xyz"]), normal=_dev(fx["cloud"]["normal"]))


@pytest.mark.parametrize("kind,metric,scale", [("mesh", "plane", 1.0), ("cloud", "plane", 1.0), ("cloud", "point", 1.0), ("mesh", "plane", 10.0)])
def test_register_lands_where_the_reference_lands(kind, metric, scale):
    fx = R.registration_fixture(scale)
    dist = STAGED if scale > 1 else R.DIST_MAX
    ref = R.refine(fx["src"], fx[kind], metric=metric, dist_max=dist, pivot=R.target_pivot(fx[kind]))
    out = registration.register(_dev(fx["src"]), _target(fx, kind), metric=metric, dist_max=dist)
    t0, a0 = R.pose_error(np.eye(4), fx["T_true"])
    tr, ar = R.pose_error(ref["T"], fx["T_true"])
    td, ad = R.pose_error(out["T"], fx["T_true"])
    print("REGISTRATION %s %s x%g: start %.3f mm %.4f deg; reference %.3g mm %.3g deg (%s, %d iterations); device %.3g mm %.3g deg (%s, %d iterations), "
          "rmse %.3g count %d overlap %.3f" % (kind, metric, scale, 1e3 * t0, np.degrees(a0), 1e3 * tr, np.degrees(ar), ref["reason"], ref["iterations"],
                                              1e3 * td, np.degrees(ad), out["reason"], out["iterations"], out["rmse"], out["count"], out["overlap"]))
    assert out["T"].shape == (4, 4) and out["T"].dtype == np.float64
    assert out["converged"] == ref["converged"] and out["reason"] == ref["reason"]
    assert td <= 2 * tr + R.STEP_T and ad <= 2 * ar + R.STEP_R
    assert len(out["trace"]) >= out["iterations"] >= 1 and out["count"] == out["trace"][-1]["count"] and 0 < out["overlap"] <= 1
    tc, ac = R.pose_error(out["T"], np.eye(4))
    assert abs(out["correction"][0] - tc) < 1e-12 and abs(out["correction"][1] - ac) < 1e-7
    if metric == "plane":
        assert out["converged"]


def test_a_single_plane_is_refused_for_its_condition():
    p, n = R.single_plane(2000, 1)
    guess = R.exp_se3(0.2 * R.TWIST)
    out = registration.register(_dev(p), dict(xyz=_dev(p), normal=_dev(n)), init=guess, metric="plane", dist_max=R.DIST_MAX)
    ref = R.refine(p, dict(xyz=p, normal=n), init=guess, metric="plane", dist_max=R.DIST_MAX, pivot=R.target_pivot(dict(xyz=p)))
    assert ref["reason"] == "condition"
    assert not out["converged"] and out["reason"] == "condition" and out["iterations"] == 0
    assert np.array_equal(out["T"], guess) and out["correction"] == (0.0, 0.0)


def test_too_few_partners_are_refused_for_their_count():
    fx = R.registration_fixture(1.0)
    guess = R.exp_se3(0.1 * R.TWIST)
    out = registration.register(_dev(fx["src"][:60]), _target(fx, "mesh"), init=guess, metric="plane", dist_max=R.DIST_MAX, min_count=100)
    assert not out["converged"] and out["reason"] == "count" and np.array_equal(out["T"], guess) and out["count"] <= 60
    # a stage that starves after one that went through: the transform of the accepted stage comes back
    # (every one of the 4 000 points has a partner within DIST_MAX, but not every one within a nanometre)
    full = registration.register(_dev(fx["src"]), _target(fx, "mesh"), metric="plane", dist_max=(R.DIST_MAX, 1e-9), min_count=4000)
    first = registration.register(_dev(fx["src"]), _target(fx, "mesh"), metric="plane", dist_max=R.DIST_MAX, min_count=4000)
    assert full["reason"] == "count" and not full["converged"] and first["converged"] and np.array_equal(full["T"], first["T"])


@pytest.mark.parametrize("where", list(PL.FAMILY_PLACES))
@pytest.mark.parametrize("name", R.PLACED_CASES)
def test_the_kernels_meet_their_bounds_away_from_the_origin(name, where):
    from estdepth_amd import ops
    place = PL.FAMILY_PLACES[where]
    c, ref = R.build_case(name, place), R.reference(name, place)
    opt = lambda a: _dev(a) if a is not None else None                                                            # noqa: E731
    moved, mn = ops.rigid_apply(_dev(c["src"]), opt(c["src_normal"]), torch.from_numpy(c["T12"]))
    res, mt, sums = ops.rigid_system(_dev(c["moved"]), opt(c["moved_normal"]), _dev(c["index"]), _dev(c["target"]), _dev(c["normal"]), c["by_index"],
                                     c["metric"], c["dist_max"], c["cos_min"], c["two_sided"])
    got = dict(moved=moved.cpu().numpy(), moved_normal=mn.cpu().numpy() if mn is not None else None, residual=res.cpu().numpy(),
               match=mt.cpu().numpy(), sums=sums.cpu().numpy())
    fig = R.compare(got, c, ref, c["name"])
    assert fig["matched"] >= 0.6 * fig["gated"] and float(np.abs(c["target"]).max()) > place[0] / 2
    print("PLACEMENT rigid_align %s: moved %.3f residual %.3f sums %.3f of the bound, ambiguous share %.4f, matched %d"
          % (c["name"], fig["moved_ratio"], fig["residual_ratio"], fig["sum_ratio"], fig["amb_share"], fig["matched"]))


@pytest.mark.parametrize("kind,metric", [("mesh", "plane"), ("cloud", "point")])
def test_rigid_system_is_repeatable_under_both_bindings(kind, metric):
    fx = R.registration_fixture(1.0)
    src, sn, tgt = _dev(fx["src"]), _dev(fx["src_normal"]), _target(fx, kind)
    T = R.exp_se3(0.5 * R.TWIST)
    run = lambda: registration.rigid_system(src, T, tgt, metric=metric, dist_max=R.DIST_MAX, src_normal=sn, cos_min=0.5)      # noqa: E731
    a, b = under("torch", run), under("torch", run)
    c, d = under("ctypes", run), under("ctypes", run)
    for other in (b, c, d):
        assert a["sums"].tobytes() == other["sums"].tobytes()
        assert torch.equal(a["match"], other["match"]) and torch.equal(a["residual"].view(torch.int32), other["residual"].view(torch.int32))
    assert a["sums"].shape == (29,) and a["count"] == int(a["sums"][28]) == int((a["match"] >= 0).sum()) > 3000
    assert sorted(a) == ["A", "b", "count", "match", "overlap", "residual", "rmse", "sums"] and a["overlap"] == a["count"] / 4000
    assert np.array_equal(a["A"], a["A"].T) and a["A"].shape == (6, 6) and a["b"].shape == (6,)


def test_compare_meshes_with_align_undoes_a_rigid_offset():
    from estdepth_amd.cloud_metrics import compare_meshes
    fx = R.registration_fixture(1.0)
    assert list(fx["mesh"]) == ["xyz", "faces"]
    gt = dict(xyz=_dev(fx["mesh"]["xyz"]), faces=_dev(fx["mesh"]["faces"]))
    # the prediction: the SAME surface with other faces (every triangle cut into four in its own plane), hence other samples.  ICP
    # minimises the misfit of two surfaces; only where they coincide at the true pose is the true pose its minimum, and only then can
    # the aligned score be held to the unmoved one's repeatability (against a finer sphere the minimum sits 0.5 mm off, in float64 too)
    fine = R.subdivided(*fx["mesh"].values())
    Ti = np.linalg.inv(fx["T_true"])
    pred = dict(xyz=_dev(fine[0]), faces=_dev(fine[1]))
    moved = dict(xyz=_dev((fine[0].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)), faces=pred["faces"])
    density = 1000.0
    base = compare_meshes(pred, gt, density)
    seeds = [compare_meshes(pred, gt, density, seed=s)["accuracy"] for s in (1, 2, 3)]
    repeat = max(abs(v - base["accuracy"]) for v in seeds)
    plain = compare_meshes(moved, gt, density)
    again = compare_meshes(moved, gt, density)
    got = compare_meshes(moved, gt, density, align=dict(metric="plane", dist_max=STAGED))
    al = got["alignment"]
    T = np.asarray(al["T"]).reshape(4, 4)
    td, ad = R.pose_error(T, fx["T_true"])
    print("REGISTRATION compare_meshes: accuracy unmoved %.6f (other seeds %s: repeatability %.3g), offset %.6f, aligned %.6f; T off by %.3g mm %.3g deg; %s"
          % (base["accuracy"], ["%.6f" % v for v in seeds], repeat, plain["accuracy"], got["accuracy"], 1e3 * td, np.degrees(ad),
             {k: v for k, v in al.items() if k != "T"}))
    assert "alignment" not in plain and sorted(plain) == sorted(base) and plain == again                 # today's keys and bits
    assert sorted(set(got) - set(plain)) == ["alignment"]
    assert sorted(al) == ["T", "converged", "correction", "iterations", "overlap", "reason", "rmse"] and al["converged"] and len(al["T"]) == 16
    assert plain["accuracy"] > base["accuracy"] + repeat                                                  # the offset shows in the score
    assert abs(got["accuracy"] - base["accuracy"]) <= repeat
    # not converged: reported, and the unmoved prediction is scored
    stuck = compare_meshes(moved, gt, density, align=dict(metric="plane", dist_max=0.1, max_iter=1))
    assert not stuck["alignment"]["converged"] and stuck["alignment"]["reason"] == "max_iter"
    assert {k: v for k, v in stuck.items() if k != "alignment"} == plain
