"""CPU checks of the rigid registration (csrc/track/rigid_align.hip) that need no device: the float64 reference of tests/rigid_align_ref.py
against its numpy-fp32 stand-in on every case of the suite (the comparison the GPU tests use), the deliberate mistakes -- each must be
rejected --, the conditioning of the scene, the ambiguous shares, the linearisation behind both metrics and the reference registration.

Figures of the stand-in (printed per case): moved coordinates at most 0.78 of their bound, residuals 0.63, sums 0.51; no ambiguous point in
any case (the gate radius 0.05 lies between the bulk of the partners, within 0.02, and the planted outliers at 0.2; the cosine threshold
0.7 between the three groups of normals at about 1, -1 and 0.36)."""
import numpy as np
import pytest

import rigid_align_ref as R
import track_ref as TR

ALL = sorted(R.CASES) + ["tie", "none"]


@pytest.mark.parametrize("name", ALL)
def test_standin_against_reference(name):
    c = R.build_case(name)
    fig = R.compare(R.standin(c), c, R.reference(name), name)
    assert fig["amb_share"] <= R.AMB_CAP                      # the condition of the suite, asserted on the stand-in's cases
    if name == "none":
        assert fig["matched"] == 0
    elif name == "tie":
        assert fig["matched"] == 6 and R.reference(name)["match"][5] == 5
    else:
        assert fig["matched"] >= 1


def test_the_gates_cut_where_the_cases_say():
    """with normals: about a tenth lost to the distance gate, the turned normals to the cosine gate, the negated ones unless two-sided"""
    one, two = R.reference("plane-n16641"), R.reference("plane-closest-two-sided-n16385")
    bare = R.reference("point-n16641")
    share = lambda r: r["count"] / r["gated"].sum()                                                            # noqa: E731
    print("rigid_align matched shares: no normals %.3f, one-sided %.3f, two-sided %.3f" % (share(bare), share(one), share(two)))
    assert 0.85 < share(bare) < 0.95 and share(one) < share(two) - 0.05 < share(bare) - 0.05
    c = R.build_case("plane-n16641")
    assert c["index"][3] == -1 and c["index"][9] == c["target"].shape[0]
    assert one["match"][3] == -1 and one["match"][9] == -1 and not one["gated"][3] and not one["gated"][9]


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_the_comparison_rejects_each_mistake(mistake):
    name = {"gate_lt": "tie", "point_sign": "point-n257"}.get(mistake, "plane-n257")
    c = R.build_case(name)
    with pytest.raises(AssertionError):
        R.compare(R.standin(c, mistake), c, R.reference(name), "%s (%s)" % (name, mistake))


@pytest.mark.parametrize("name", ["cond-plane", "cond-point"])
def test_the_scene_fixes_all_six_degrees_of_freedom(name):
    r = R.reference(name)
    A = R.unpack(r["sums"])[0]
    ev = np.linalg.eigvalsh(A / r["count"])
    print("rigid_align %s: eigenvalues of A / count %s, ratio %.1f" % (name, np.array2string(ev, precision=4), ev[-1] / ev[0]))
    assert ev[0] > 0 and ev[-1] <= TR.COND_FIXTURE * ev[0]


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_the_system_is_the_gradient_of_the_left_update(metric):
    """b = sum J^T r must be minus half the derivative of sum |r|^2 along T <- Exp(xi) T at xi = 0: finite differences of the reference's
    own sum of squares, the partners held fixed"""
    c = dict(R.build_case("cond-%s" % metric))
    base = R.evaluate(c)
    b = base["sums"][21:27]
    T0 = np.eye(4)
    T0[:3, :4] = c["T12"].astype(np.float64)
    h, grad = 1e-4, np.zeros(6)
    for k in range(6):
        rr = []
        for s in (+h, -h):
            xi = np.zeros(6)
            xi[k] = s
            T = R.exp_se3(xi) @ T0
            moved = c["src"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            q = c["target"][np.where(base["match"] >= 0, base["match"], 0)].astype(np.float64)
            e = (q - moved)[base["match"] >= 0]
            if metric == "plane":
                n = c["normal"][base["match"][base["match"] >= 0]].astype(np.float64)
                rr.append(float(((n * e).sum(1) ** 2).sum()))
            else:
                rr.append(float((e * e).sum()))
        grad[k] = (rr[0] - rr[1]) / (2 * h)
    rel = np.abs(-0.5 * grad - b).max() / np.abs(b).max()
    print("rigid_align finite differences (%s): %.4f of the largest |b_i|" % (metric, rel))
    assert rel < 0.02                                       # J is taken at the partner q, not at the moved point: a first-order difference


@pytest.mark.parametrize("target,metric", [("mesh", "plane"), ("cloud", "plane")])
def test_the_reference_registration_converges(target, metric):
    fx = R.registration_fixture(1.0, n=1000)
    out = R.refine(fx["src"], fx[target], metric=metric, dist_max=R.DIST_MAX)
    t0, a0 = R.pose_error(np.eye(4), fx["T_true"])
    t1, a1 = R.pose_error(out["T"], fx["T_true"])
    print("rigid_align reference registration (%s, %s): %.2f mm %.3f deg -> %.3g mm %.3g deg in %d iterations (%s)"
          % (target, metric, 1e3 * t0, np.degrees(a0), 1e3 * t1, np.degrees(a1), out["iterations"], out["reason"]))
    assert t1 < 0.1 * t0 and a1 < 0.1 * a0


def test_the_reference_registration_refuses_a_single_plane_and_a_starved_system():
    p, n = R.single_plane(500, 1)
    out = R.refine(p, dict(xyz=p, normal=n), metric="plane")
    assert not out["converged"] and out["reason"] == "condition" and np.array_equal(out["T"], np.eye(4))
    fx = R.registration_fixture(1.0, n=1000)
    out = R.refine(fx["src"][:50], fx["mesh"], metric="plane", min_count=100)
    assert not out["converged"] and out["reason"] == "count" and np.array_equal(out["T"], np.eye(4))
