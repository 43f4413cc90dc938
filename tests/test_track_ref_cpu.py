"""CPU checks of the frame-to-model alignment (csrc/track/frame_align.hip) that need no device: the float64 reference of tests/track_ref.py
against its numpy-fp32 stand-in on every case of the GPU suites, the wrong contracts it must reject, closed forms, the update convention,
the host side of estdepth_amd/tracking.py driven by the reference, the C ABI's argument checks and the descriptor's layout.

Figures of the numpy-fp32 stand-in against the reference (printed per case, pytest -s): ambiguous share of the valid pixels 0 - 0.0009 (cap
0.03); largest residual error 0.03 - 0.39 of the unscaled bound, largest error of a sum 0.01 - 0.90 of its bound (bar C_TRACK = 2; the 0.90
is the one-pixel map).  The convergence fixture: eigenvalues of A / count 0.0063 .. 1.03 (ratio 164, bar COND_FIXTURE = 1000); from a guess off
by 9.8 mm and 0.50 degrees the float64 reference is within 1e-8 m and 1e-8 rad after 10 iterations (bar: a tenth of the perturbation)."""
import ctypes

import numpy as np
import pytest
import torch

from estdepth_amd import tracking  # noqa: F401 -- the feature under test: without it this module does not import

import track_ref as T
import tsdf_ref as R
from helpers import check_desc_layout

ALL_CASES = list(T.CASES) + ["tie", "full"]


def _got(s):
    return dict(residual=s["residual"], match=s["match"], sums=s["sums"])


@pytest.fixture(scope="module")
def lib():
    from estdepth_amd import _native, build
    build.build()
    return _native.lib()


# ------------------------------------------------------------------------------------------------------------ reference and stand-in
@pytest.mark.parametrize("name", ALL_CASES)
def test_stand_in_meets_the_comparison(name):
    """numpy fp32 (no fused multiply-add) against the float64 reference under THE comparison, the ambiguous share <= 0.03 included"""
    c, ref = T.build_case(name), T.reference(name)
    s = T.evaluate(c, np.float32)
    fig = T.compare(_got(s), c, ref, name + " stand-in")
    if name == "away":
        assert fig["matched"] == 0 and (s["sums"] == 0).all() and (s["match"] == -1).all()
    elif name == "tie":
        assert fig["matched"] == 1 and ref["match"][8, 8] == 8 * 16 + 8 and not ref["amb"].any()
    else:
        assert fig["matched"] >= max(1, 0.7 * fig["valid"])


def test_route_sizes_are_the_raycast_suites():
    import tsdf_raycast_ref as RR
    assert set(T.ROUTE_SIZES) <= set(RR.ROUTE_SIZES)
    assert np.array_equal(T.HELD_OUT_POSE, RR.HELD_OUT_POSE)
    assert T.C_TRACK <= RR.C_RAY and T.C_POS == R.C_POS


@pytest.mark.parametrize("mistake", T.MISTAKES)
def test_each_mistake_is_rejected(mistake):
    name = "tie" if mistake == "gate_lt" else "mid-model90"
    c, ref = T.build_case(name), T.reference(name)
    for dtype in (np.float64, np.float32):
        with pytest.raises(AssertionError):
            T.compare(_got(T.evaluate(c, dtype, mistake=mistake)), c, ref, "%s %s" % (name, mistake))
    T.compare(_got(T.evaluate(c, np.float64)), c, ref, name)                 # the contract itself passes


def test_sums_are_checked_given_the_match_map():
    """a wrong decision on an ambiguous pixel changes the device's sums; the sums check follows the device's decisions"""
    c, ref = T.build_case("mid"), T.reference("mid")
    s = T.evaluate(c, np.float32)
    mt = s["match"].copy()
    v, u = np.argwhere(mt >= 0)[100]
    mt[v, u] = -1                                                             # one matched pixel dropped from the map but kept in the sums
    with pytest.raises(AssertionError):
        T.compare(dict(residual=np.where(mt >= 0, s["residual"], 0), match=mt, sums=s["sums"]), c, ref, "dropped pixel")
    given = T.evaluate(c, np.float32, match=mt)                               # sums formed from the changed map agree with it
    assert given["count"] == ref["count"] - 1 or given["count"] == s["count"] - 1
    bad = ref["amb"].copy()
    ref2 = dict(ref, amb=bad | (np.arange(mt.size).reshape(mt.shape) == v * mt.shape[1] + u))
    T.compare(dict(residual=np.where(mt >= 0, s["residual"], 0), match=mt, sums=given["sums"]), c, ref2, "dropped ambiguous pixel")


# ------------------------------------------------------------------------------------------------------------ closed forms
def _plane_case(delta, hw=(24, 32), tilt=None):
    H, W = hw
    K = R.intrinsics(H, W)
    P = np.eye(4) if tilt is None else R.look_at((0.3, -0.2, 0.0), (0.0, 0.0, 2.6))
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = (np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T) @ P[:3, :3].T
    depth = ((2.6 - P[2, 3]) / rays[..., 2]).astype(np.float32)
    normal = np.zeros((H, W, 3), np.float32)
    normal[..., 2] = -1.0
    guess = P.copy()
    guess[2, 3] += delta
    return dict(depth=depth, conf=None, conf_min=0.0, m_depth=depth.copy(), m_normal=normal, K=K, K_m=K, pose=P, guess=guess, model_pose=P,
                mats=T.matrices64(guess, K, P, K), dist_max=T.DIST_MAX, z_near=T.Z_NEAR)


@pytest.mark.parametrize("tilt", [None, True], ids=["fronto", "tilted"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_identical_pose_on_a_plane_gives_zero(dtype, tilt):
    """the same pose and the same map on both sides: p and q are the same expression of the same numbers, so r = 0 and b = 0 EXACTLY"""
    c = _plane_case(0.0, tilt=tilt)
    s = T.evaluate(c, dtype)
    assert s["count"] == c["depth"].size and (s["match"].reshape(-1) == np.arange(c["depth"].size)).all()
    assert (s["residual"] == 0).all() and (s["sums"][21:28] == 0).all() and s["sums"][28] == c["depth"].size


def test_shift_along_the_normal_of_a_fronto_parallel_plane():
    """the guess delta behind the true pose along the plane's normal: r = delta on every matched pixel, and one solve returns it"""
    delta = 0.02
    c = _plane_case(delta)
    s = T.evaluate(c)
    assert s["count"] > 0.8 * c["depth"].size
    hit = s["match"] >= 0
    assert np.abs(s["residual"][hit] - delta).max() < 1e-6                   # the maps and matrices are fp32 values: 2.6 is not exact
    A, b, rr, n = T.unpack(s["sums"])
    assert abs(np.sqrt(rr / n) - delta) < 1e-6
    # a plane alone leaves three motions free (A is singular): the minimum-norm solution is the shift and nothing else
    xi = np.linalg.lstsq(A, b, rcond=1e-9)[0]
    assert np.abs(xi - np.array([0, 0, -delta, 0, 0, 0])).max() < 1e-5
    moved = T.exp_se3(xi) @ c["guess"]
    assert np.abs(moved - c["pose"]).max() < 1e-5
    from estdepth_amd import tracking
    assert tracking.solve_step(A, b, n, 1)[0] is None                        # and refine_pose refuses it


def test_update_convention_against_finite_differences():
    """d/d eps sum r^2 (Exp(eps e_i) P) at 0 = -2 b_i: the sign of r, the order (t, omega), p x n and the LEFT update in world axes.  The
    cost is only piecewise smooth (a pixel changes its model pixel as the pose moves), so the central difference at eps = 1e-4 carries a
    few per cent of noise: bar 5 % of the largest |2 b_i|; the same derivative under the RIGHT update misses that bar (the axes differ by
    the camera's rotation), as does the one with the twist's halves exchanged."""
    fx = T.convergence_fixture()
    cost = lambda P: T.step(fx["depth"], fx["K"], P, fx["model"])["sums"][27]                    # noqa: E731
    b = T.step(fx["depth"], fx["K"], fx["guess"], fx["model"])["b"]
    eps = 1e-4

    def gradient(move):
        g = []
        for i in range(6):
            xi = np.zeros(6)
            xi[i] = eps
            g.append((cost(move(T.exp_se3(xi))) - cost(move(T.exp_se3(-xi)))) / (2 * eps))
        return np.array(g)
    scale = np.abs(2 * b).max()
    left = np.abs(gradient(lambda E: E @ fx["guess"]) + 2 * b).max() / scale
    right = np.abs(gradient(lambda E: fx["guess"] @ E) + 2 * b).max() / scale
    print("frame_align finite differences: left update %.4f of the largest |2 b_i|, right update %.4f" % (left, right))
    assert left <= 0.05 < right
    assert np.abs(gradient(lambda E: E @ fx["guess"]) + 2 * np.concatenate([b[3:], b[:3]])).max() / scale > 0.05


def test_exp_is_a_rigid_motion_and_the_host_layer_agrees():
    from estdepth_amd import tracking
    for xi in (T.TWIST, 30 * T.TWIST, np.array([0.1, 0.2, -0.3, 0, 0, 0]), np.array([0, 0, 0, 1e-9, 0, -2e-9]), np.zeros(6)):
        E = T.exp_se3(xi)
        assert np.abs(E[:3, :3] @ E[:3, :3].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(E[:3, :3]) - 1) < 1e-14
        assert np.abs(tracking.exp_se3(xi) - E).max() < 1e-15
        assert np.abs(T.exp_se3(-np.asarray(xi)) @ E - np.eye(4)).max() < 1e-14
    # first order: Exp(xi) p = p + t + omega x p
    xi = 1e-6 * np.array([1.0, -2.0, 0.5, 0.3, 0.7, -1.1])
    p = np.array([0.4, -0.3, 2.0])
    assert np.abs((T.exp_se3(xi) @ np.append(p, 1))[:3] - (p + xi[:3] + np.cross(xi[3:], p))).max() < 1e-11


def test_matrices_of_the_host_layer():
    from estdepth_amd import camera
    c = T.build_case("mid-model90")
    got = camera.frame_align_matrices(*(torch.from_numpy(np.ascontiguousarray(c[k])) for k in ("guess", "K", "model_pose", "K_m")))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 12) and not got.is_cuda
    want = c["mats"].reshape(3, 12).astype(np.float64)
    assert np.abs(got.numpy().astype(np.float64) - want).max() <= 2.0 ** -22 * np.abs(want).max()
    # L takes a pixel at its depth to the world point, Fm takes it to the model's pixel, Bm back
    L, Fm, Bm = (m.astype(np.float64) for m in c["mats"])
    x = L @ np.array([40.0 * 2.0, 30.0 * 2.0, 2.0, 1.0])
    pc = c["guess"] @ np.append(np.linalg.inv(c["K"]) @ np.array([40.0, 30.0, 1.0]) * 2.0, 1.0)
    assert np.abs(x - pc[:3]).max() < 1e-5
    a = Fm @ np.append(x, 1.0)
    back = Bm @ np.array([a[0], a[1], a[2], 1.0])
    assert np.abs(back - x).max() < 1e-4


# ------------------------------------------------------------------------------------------------------------ convergence, float64 only
def test_the_fixture_constrains_all_six_motions():
    fx = T.convergence_fixture()
    s = T.step(fx["depth"], fx["K"], fx["guess"], fx["model"])
    ev = np.linalg.eigvalsh(s["A"] / s["count"])
    print("frame_align fixture: eigenvalues of A / count %s, ratio %.1f" % (np.array2string(ev, precision=4), ev[-1] / ev[0]))
    assert ev[0] > 0 and ev[-1] <= T.COND_FIXTURE * ev[0]
    # the plane and ONE sphere: the rotation about the plane's normal through the sphere's centre is free
    keep = T.SPHERES
    try:
        T.SPHERES = keep[:1]
        depth, normal = T.scene_maps(fx["pose"], fx["K"], *fx["depth"].shape)
    finally:
        T.SPHERES = keep
    model = dict(depth=depth.astype(np.float32), normal=normal.astype(np.float32), pose=fx["pose"], K=fx["K"])
    one = T.step(depth.astype(np.float32), fx["K"], fx["pose"], model)
    ev1 = np.linalg.eigvalsh(one["A"] / one["count"])
    assert ev1[0] < 1e-6 * ev1[-1]


def test_reference_converges_from_the_perturbed_guess():
    fx = T.convergence_fixture()
    t0, a0 = T.pose_error(fx["guess"], fx["pose"])
    assert 0.008 < t0 < 0.012 and np.radians(0.4) < a0 < np.radians(0.6)
    P, trace = T.refine(fx["depth"], fx["K"], fx["guess"], fx["model"], iters=10)
    t1, a1 = T.pose_error(P, fx["pose"])
    print("frame_align convergence: %.2f mm %.3f deg -> %.3g mm %.3g deg; rmse %s" % (1e3 * t0, np.degrees(a0), 1e3 * t1, np.degrees(a1),
                                                                                     " ".join("%.2e" % r for r in trace)))
    assert t1 <= t0 / 10 and a1 <= a0 / 10
    assert trace[-1] < trace[0]


# ------------------------------------------------------------------------------------------------------------ tracking.py on the reference
def _system(fx, **kw):
    return lambda P: T.step(fx["depth"], fx["K"], P, fx["model"], **kw)


def test_gauss_newton_of_the_host_layer_on_the_reference():
    from estdepth_amd import tracking
    fx = T.convergence_fixture()
    out = tracking.gauss_newton(_system(fx), fx["guess"], max_iter=10, min_count=100)
    assert out["converged"] and out["reason"] == "converged" and 2 <= out["iterations"] <= 10 and len(out["trace"]) == out["iterations"]
    P, _ = T.refine(fx["depth"], fx["K"], fx["guess"], fx["model"], iters=out["iterations"])
    assert np.abs(out["pose"] - P).max() < 1e-12
    t0, a0 = T.pose_error(fx["guess"], fx["pose"])
    assert abs(out["correction"][0] - t0) < 1e-4 and abs(out["correction"][1] - a0) < 1e-4
    assert out["trace"][0]["count"] > 10000 and out["trace"][-1]["rmse"] < out["trace"][0]["rmse"]
    short = tracking.gauss_newton(_system(fx), fx["guess"], max_iter=2)
    assert not short["converged"] and short["reason"] == "max_iter" and short["iterations"] == 2
    assert T.pose_error(short["pose"], fx["pose"])[0] < t0
    zero = tracking.gauss_newton(_system(fx), fx["guess"], max_iter=0)
    assert zero["iterations"] == 0 and len(zero["trace"]) == 1 and np.array_equal(zero["pose"], fx["guess"]) and zero["correction"] == (0.0, 0.0)


def test_refusals_return_the_guess_unchanged():
    from estdepth_amd import tracking
    fx = T.convergence_fixture()
    few = tracking.gauss_newton(_system(fx), fx["guess"], min_count=10 ** 6)
    assert not few["converged"] and few["reason"] == "count" and np.array_equal(few["pose"], fx["guess"]) and few["iterations"] == 0
    away = tracking.gauss_newton(_system(fx), fx["guess"] @ np.diag([-1.0, 1.0, -1.0, 1.0]), min_count=1)
    assert away["reason"] == "count" and away["trace"][0]["count"] == 0
    c = _plane_case(0.01)                                                      # a plane alone: three motions are free
    plane = dict(depth=c["depth"], K=c["K"], model=dict(depth=c["m_depth"], normal=c["m_normal"], pose=c["pose"], K=c["K"]))
    flat = tracking.gauss_newton(_system(plane), c["guess"], min_count=10)
    assert not flat["converged"] and flat["reason"] in ("cholesky", "condition") and np.array_equal(flat["pose"], c["guess"])
    A = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1e-7])
    assert tracking.solve_step(A, np.ones(6), 1000, 100)[1] == "condition"
    assert tracking.solve_step(-A, np.ones(6), 1000, 100)[1] == "cholesky"
    assert tracking.solve_step(A * np.nan, np.ones(6), 1000, 100)[1] == "cholesky"
    xi, why = tracking.solve_step(np.diag([1.0, 2, 3, 4, 5, 6]), np.arange(1.0, 7.0), 1000, 100)
    assert why is None and np.allclose(xi, 1.0)
    # a step refused in the middle of the iteration also returns the first guess
    calls = []

    def second_fails(P):
        calls.append(1)
        s = T.step(fx["depth"], fx["K"], P, fx["model"])
        return s if len(calls) == 1 else dict(s, count=0)
    mid = tracking.gauss_newton(second_fails, fx["guess"])
    assert mid["reason"] == "count" and mid["iterations"] == 1 and np.array_equal(mid["pose"], fx["guess"]) and len(mid["trace"]) == 2


def test_host_layer_checks_its_inputs_without_a_device():
    from estdepth_amd import tracking
    d = torch.zeros(4, 4)
    model = dict(depth=d, normal=torch.zeros(4, 4, 3), pose=torch.eye(4), K=torch.eye(3))
    for args in ((d, torch.eye(3), torch.eye(4), model), (np.zeros((4, 4)), torch.eye(3), torch.eye(4), model)):
        with pytest.raises(RuntimeError):
            tracking.align_step(*args)                                         # CPU tensors / arrays: there is no CPU path
    with pytest.raises(RuntimeError):
        tracking.refine_pose(d, torch.eye(3), torch.full((4, 4), float("nan")), model)
    with pytest.raises(RuntimeError):
        tracking.refine_pose(d, torch.eye(3), torch.eye(4), model, max_iter=-1)


# ------------------------------------------------------------------------------------------------------------ the C ABI without a device
def _desc(**kw):
    from estdepth_amd import _native
    d = _native.FrameAlignDesc()
    d.H, d.W, d.Hm, d.Wm = 4, 6, 5, 7
    d.dist_max, d.z_near, d.conf_min = 0.1, 1e-3, 0.0
    for k in ("depth", "m_depth", "m_normal", "residual", "match", "sums", "partials"):
        setattr(d, k, 0x1000)                                                  # never dereferenced: every call below returns before a launch
    d.conf = None
    for i in range(12):
        d.L[i] = d.Fm[i] = d.Bm[i] = 1.0
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


BAD = [dict(depth=None), dict(m_depth=None), dict(m_normal=None), dict(residual=None), dict(match=None), dict(sums=None), dict(partials=None),
       dict(H=0), dict(W=-1), dict(Hm=0), dict(Wm=0),
       dict(dist_max=0.0), dict(dist_max=-0.1), dict(dist_max=float("nan")), dict(dist_max=float("inf")), dict(dist_max=1e30), dict(dist_max=1e-30),
       dict(z_near=-1e-3), dict(z_near=float("nan")), dict(z_near=float("inf")),
       dict(L=(3, float("nan"))), dict(Fm=(0, float("inf"))), dict(Bm=(11, float("-inf")))]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_malformed_descriptors_are_argument_errors(lib, bad):
    assert lib.estd_frame_align(ctypes.byref(_desc(**bad)), None) == -1


def test_null_descriptor_and_sizes_beyond_2_31(lib):
    assert lib.estd_frame_align(None, None) == -1
    assert lib.estd_frame_align(ctypes.byref(_desc(H=65536, W=32768)), None) == -3
    assert lib.estd_frame_align(ctypes.byref(_desc(Hm=32768, Wm=65536)), None) == -3
    assert lib.estd_frame_align(ctypes.byref(_desc(H=65536, W=32768, dist_max=0.0)), None) == -1          # argument errors come first
    assert lib.estd_frame_align_partials(1, 1) == 29 * 8
    assert lib.estd_frame_align_partials(16, 16) == 29 * 8 and lib.estd_frame_align_partials(17, 33) == 6 * 29 * 8
    assert lib.estd_frame_align_partials(480, 640) == 1200 * 29 * 8
    assert lib.estd_frame_align_partials(0, 5) == 0 and lib.estd_frame_align_partials(65536, 32768) == 0


def test_descriptor_layout(lib, tmp_path):
    """sizeof / offsetof of estd_frame_align_desc as the C compiler sees it == the ctypes mirror; ESTD_FRAME_ALIGN_SUMS == the bindings'"""
    from estdepth_amd import _native, ops
    out = check_desc_layout(tmp_path, "estd_frame_align_desc", _native.FrameAlignDesc, macros=["ESTD_FRAME_ALIGN_SUMS"])
    assert out[-1] == ops.FRAME_ALIGN_SUMS == T.N_SUMS == 29
