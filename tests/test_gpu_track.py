"""csrc/track/frame_align.hip and estdepth_amd/tracking.py on the device against the float64 reference of tests/track_ref.py: the 120 x 160 and
480 x 640 value cases (holes, a confidence gate, a model map of another size and pose) under both bindings, identical bits across calls and
bindings, a guess that matches nothing, malformed arguments under both bindings, align_step through the host layer's own matrices, and the
semantic test: TSDFVolume.track on a held-out frame of the three-body scene with a perturbed guess.

Bar (track_ref.compare): ambiguous pixels <= 3 % of the valid pixels; on all others match is exact, skipped pixels are exactly 0 / -1, the
residual is within C_TRACK = 2 times its first-order bound, and each of the 29 sums within C_TRACK times the summed per-term bounds of the
reference's evaluation GIVEN the device's match map.  Semantic: from a guess off by 9.8 mm and 0.50 degrees the device's final pose error is
<= 1.25 x the error the float64 reference reaches from the same rendered maps (translation and angle each) and below the perturbation;
fusing the refined frame renders closer to the analytic scene at the true pose than fusing the perturbed one (median and 95th percentile
of |depth - analytic| in voxels over the frame's own pixels).  The figures of a device run (this file prints them, pytest -s):
profiles/track_gpu_tests.txt.

Away from the origin: the 120 x 160 case built 64 m and 128 m out (tests/placement.py; track_ref.PLACED_AT), through ``track_ref.compare``
unchanged.  Not 512 m: the model pixel a point falls into is decided from a projection in fp32 world coordinates, and beyond 128 m the
reference alone has more than 3 % of the pixels within the rounding of a pixel edge (0.056 at 256 m, 0.111 at 512 m;
tests/test_placement_ref_cpu.py measures it).  The pose solve itself is tested out to 512 m in tests/test_gpu_placement.py."""
import numpy as np
import pytest
import torch

from estdepth_amd import tracking  # noqa: F401 -- the feature under test: without it this module does not import

import track_ref as T
import tsdf_ref as R
from helpers import _binding

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 1.25                # the semantic bar of the colour test (tsdf_color_ref.MEDIAN_FACTOR)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(c):
    from estdepth_amd import ops
    conf = _dev(c["conf"]) if c["conf"] is not None else None
    mats = torch.from_numpy(np.ascontiguousarray(c["mats"].reshape(3, 12)))
    out = ops.frame_align(_dev(c["depth"]), conf, _dev(c["m_depth"]), _dev(c["m_normal"]), mats, c["dist_max"], c["z_near"], c["conf_min"])
    torch.cuda.synchronize()
    return dict(zip(("residual", "match", "sums"), (t.cpu().numpy() for t in out)))


VALUE_CASES = ["mid", "mid-conf", "mid-model90"]


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", VALUE_CASES)
def test_against_reference(name, binding, monkeypatch):
    _binding(monkeypatch, binding)
    c = T.build_case(name)
    fig = T.compare(_run(c), c, T.reference(name), "%s %s" % (name, binding))
    assert fig["matched"] > 10000
    print("TRACK-RATIO %s %s residual %.3f sums %.3f amb %.4f" % (name, binding, fig["residual_ratio"], fig["sum_ratio"], fig["amb_share"]))


@pytest.mark.parametrize("d", T.PLACED_AT)
def test_against_reference_away_from_the_origin(d):
    c, ref = T.build_case(T.PLACED_CASE, (d, False)), T.reference(T.PLACED_CASE, (d, False))
    fig = T.compare(_run(c), c, ref, c["name"])
    assert fig["matched"] > 10000 and float(np.abs(c["mats"][0][:, 3]).max()) > d / 2
    print("PLACEMENT frame_align %s: residual %.3f sums %.3f of the bound, ambiguous share %.4f, matched %d"
          % (c["name"], fig["residual_ratio"], fig["sum_ratio"], fig["amb_share"], fig["matched"]))


def test_full_size():
    """480 x 640: 1200 workgroups, more partials than one pass of the reduction's 64 lanes"""
    c = T.build_case("full")
    fig = T.compare(_run(c), c, T.reference("full"), "full")
    assert fig["matched"] > 200000
    print("TRACK-RATIO full residual %.3f sums %.3f amb %.4f" % (fig["residual_ratio"], fig["sum_ratio"], fig["amb_share"]))


def test_calls_and_bindings_give_identical_bits(monkeypatch):
    c = T.build_case("mid-conf")
    runs = []
    for binding in ("torch", "torch", "ctypes"):
        _binding(monkeypatch, binding)
        runs.append(_run(c))
    for other in runs[1:]:
        assert np.array_equal(runs[0]["residual"].view(np.uint32), other["residual"].view(np.uint32))
        assert np.array_equal(runs[0]["match"], other["match"])
        assert np.array_equal(runs[0]["sums"].view(np.uint64), other["sums"].view(np.uint64))
    assert runs[0]["match"].dtype == np.int32 and runs[0]["sums"].dtype == np.float64 and runs[0]["sums"].shape == (29,)


def test_the_tie_passes_the_gate():
    """e2 == dist_max^2 exactly at one pixel of an all-exact case: the contract's <= matches it"""
    c = T.build_case("tie")
    got = _run(c)
    T.compare(got, c, T.reference("tie"), "tie")
    assert got["match"][8, 8] == 8 * 16 + 8 and (got["match"] >= 0).sum() == 1 and got["residual"][8, 8] == np.float32(-0.25)
    assert got["sums"][28] == 1.0 and got["sums"][27] == 0.0625


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_invalid_depths_and_a_guess_that_matches_nothing(binding, monkeypatch):
    _binding(monkeypatch, binding)
    c = T.build_case("mid")
    for fill in (0.0, np.nan, np.inf, -1.0, T.Z_NEAR):
        got = _run(dict(c, depth=np.full_like(c["depth"], fill)))
        assert (got["match"] == -1).all() and (got["residual"] == 0).all() and (got["sums"] == 0).all(), fill
    got = _run(dict(c, m_depth=np.zeros_like(c["m_depth"])))                      # a model without a single hit
    assert (got["match"] == -1).all() and (got["sums"] == 0).all()
    got = _run(dict(c, conf=np.zeros_like(c["depth"]), conf_min=0.5))            # every pixel gated out
    assert (got["match"] == -1).all() and (got["sums"] == 0).all()
    away = T.build_case("away")
    got = _run(away)
    assert (got["match"] == -1).all() and (got["residual"].view(np.uint32) == 0).all() and (got["sums"].view(np.uint64) == 0).all()


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_arguments_raise_before_launch(binding, monkeypatch):
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    d = torch.full((6, 8), 2.0, device=DEV)
    md, mn = torch.full((5, 7), 2.0, device=DEV), torch.zeros(5, 7, 3, device=DEV)
    mats = torch.from_numpy(np.ascontiguousarray(T.build_case("r16x16")["mats"].reshape(3, 12)))
    good = dict(depth=d, conf=None, m_depth=md, m_normal=mn, mats=mats, dist_max=0.1, z_near=1e-3, conf_min=0.0)

    def run(**kw):
        a = dict(good, **kw)
        return ops.frame_align(a["depth"], a["conf"], a["m_depth"], a["m_normal"], a["mats"], a["dist_max"], a["z_near"], a["conf_min"])
    nan_mats = mats.clone()
    nan_mats[2, 5] = float("nan")
    for bad in (dict(depth=d.double()), dict(depth=d.cpu()), dict(depth=torch.zeros(6, 16, device=DEV)[:, ::2]), dict(depth=torch.zeros(2, 6, 8, device=DEV)),
                dict(depth=torch.zeros(0, 8, device=DEV)), dict(conf=torch.zeros(6, 9, device=DEV)), dict(conf=d.cpu()), dict(conf=d.double()),
                dict(m_depth=md.cpu()), dict(m_depth=md.double()), dict(m_depth=torch.zeros(2, 5, 7, device=DEV)),
                dict(m_normal=torch.zeros(5, 7, device=DEV)), dict(m_normal=torch.zeros(5, 8, 3, device=DEV)), dict(m_normal=mn.cpu()),
                dict(mats=mats.to(DEV)), dict(mats=mats[:2]), dict(mats=mats.double()), dict(mats=nan_mats),
                dict(dist_max=0.0), dict(dist_max=-1.0), dict(dist_max=float("nan")), dict(dist_max=float("inf")), dict(dist_max=1e30),
                dict(dist_max=1e-30), dict(z_near=-1e-3), dict(z_near=float("nan")), dict(conf_min=float("nan"))):
        with pytest.raises(RuntimeError):
            run(**bad)
    res, mt, sums = run()                                                        # a well-formed call still works
    torch.cuda.synchronize()
    assert tuple(res.shape) == (6, 8) and mt.dtype == torch.int32 and tuple(sums.shape) == (29,) and sums.dtype == torch.float64


def test_align_step_through_the_host_layer():
    """tracking.align_step forms its own matrices (camera.frame_align_matrices): the reference evaluated from THOSE matrices"""
    from estdepth_amd import camera, tracking
    c = T.build_case("mid-model90")
    tt = {k: torch.from_numpy(np.ascontiguousarray(c[k])) for k in ("guess", "K", "model_pose", "K_m")}
    mats = camera.frame_align_matrices(tt["guess"], tt["K"], tt["model_pose"], tt["K_m"]).numpy().reshape(3, 3, 4)
    c2 = dict(c, mats=mats)
    model = dict(depth=_dev(c["m_depth"]), normal=_dev(c["m_normal"]), pose=tt["model_pose"], K=tt["K_m"])
    s = tracking.align_step(_dev(c["depth"])[None], tt["K"], tt["guess"], model, dist_max=c["dist_max"], z_near=c["z_near"])
    ref = T.reference("mid-model90") if np.array_equal(mats, c["mats"]) else T.evaluate(c2)
    fig = T.compare(dict(residual=s["residual"].cpu().numpy(), match=s["match"].cpu().numpy(), sums=s["sums"]), c2, ref, "align_step")
    A, b, rr, n = T.unpack(s["sums"])
    assert np.array_equal(s["A"], A) and np.array_equal(s["A"], s["A"].T) and np.array_equal(s["b"], b) and s["count"] == n == fig["matched"]
    assert s["rmse"] == np.sqrt(rr / n) and 0.001 < s["rmse"] < 0.02
    for bad in (dict(model=dict(model, normal=None)), dict(conf=torch.zeros(3, 3, device=DEV)), dict(dist_max=0.0), dict(z_near=-1.0)):
        kw = dict(dict(model=model, dist_max=0.1), **bad)
        with pytest.raises(RuntimeError):
            tracking.align_step(_dev(c["depth"]), tt["K"], tt["guess"], kw.pop("model"), **kw)
    with pytest.raises(RuntimeError):
        tracking.align_step(_dev(c["depth"]), tt["K"], torch.full((4, 4), float("inf")), model)


# ------------------------------------------------------------------------------------------------------------ the semantic test
DIMS, ORIGIN, HW = (96, 128, 128), (-1.92, -1.92, 0.2), (120, 160)


@pytest.fixture(scope="module")
def fused():
    """eight views of the three-body scene (the poses of tsdf_ref's t8 case) fused at 3 cm -> (volume tensor, K, analytic frame)"""
    from estdepth_amd.fusion3d import TSDFVolume
    H, W = HW
    K = R.intrinsics(H, W)
    poses = R.scene_poses(8, seed=2)
    depths = np.stack([T.scene_maps(P, K, H, W)[0] for P in poses]).astype(np.float32)
    vol = TSDFVolume(DIMS, R.VOXEL, ORIGIN, device=DEV)
    vol.integrate(_dev(depths), torch.from_numpy(poses), torch.from_numpy(K))
    torch.cuda.synchronize()
    frame = T.scene_maps(T.HELD_OUT_POSE, K, H, W)[0]
    return vol, K, frame


def _copy(vol):
    from estdepth_amd.fusion3d import TSDFVolume
    out = TSDFVolume(DIMS, R.VOXEL, ORIGIN, device=DEV)
    out.volume.copy_(vol.volume)
    return out


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_track_recovers_a_perturbed_pose(fused, binding, monkeypatch):
    _binding(monkeypatch, binding)
    vol, K, frame = fused
    H, W = HW
    depth, Kt = _dev(frame.astype(np.float32)), torch.from_numpy(K)
    guess = T.perturbed(T.HELD_OUT_POSE)
    t0, a0 = T.pose_error(guess, T.HELD_OUT_POSE)
    out = vol.track(depth, torch.from_numpy(guess), Kt)
    assert out["reason"] in ("converged", "max_iter"), out["reason"]
    td, ad = T.pose_error(out["pose"].numpy(), T.HELD_OUT_POSE)
    # the float64 reference from the same rendered maps, ten iterations
    maps = vol.render(torch.from_numpy(guess), Kt, (H, W))
    model = dict(depth=maps["depth"].cpu().numpy(), normal=maps["normal"].cpu().numpy(), pose=guess, K=K)
    P_ref, trace = T.refine(frame.astype(np.float32), K, guess, model, iters=10, pivot=vol.centre, dist_max=vol.trunc, z_near=vol.z_near)
    tr, ar = T.pose_error(P_ref, T.HELD_OUT_POSE)
    print("TRACK-SEMANTIC %s: guess off by %.2f mm %.3f deg; device %.3f mm %.4f deg after %d iterations (%s), reference %.3f mm %.4f deg; rmse %.2f -> "
          "%.2f mm, matched share %.3f, correction %.2f mm %.3f deg" % (binding, 1e3 * t0, np.degrees(a0), 1e3 * td, np.degrees(ad), out["iterations"], out["reason"],
                                                                        1e3 * tr, np.degrees(ar), 1e3 * out["trace"][0]["rmse"], 1e3 * out["trace"][-1]["rmse"],
                                                                        out["matched_share"], 1e3 * out["correction"][0], np.degrees(out["correction"][1])))
    assert td <= MARGIN * tr and ad <= MARGIN * ar
    assert td < t0 and ad < a0
    assert out["matched_share"] > 0.8 and out["trace"][-1]["rmse"] < out["trace"][0]["rmse"]
    chk = vol.check_frame(depth, out["pose"], Kt)
    bad = vol.check_frame(depth, torch.from_numpy(guess), Kt)
    assert tuple(chk["residual"].shape) == (H, W) and chk["rmse"] < bad["rmse"] and chk["matched_share"] > 0.8
    assert abs(bad["rmse"] - out["trace"][0]["rmse"]) < 1e-12 and bad["count"] == out["trace"][0]["count"]


def test_fusing_the_refined_frame_renders_closer(fused):
    vol, K, frame = fused
    H, W = HW
    depth, Kt = _dev(frame.astype(np.float32)), torch.from_numpy(K)
    guess = torch.from_numpy(T.perturbed(T.HELD_OUT_POSE))
    refined = vol.track(depth, guess, Kt)["pose"]
    fig = {}
    for label, pose in (("refined", refined), ("perturbed", guess)):
        v = _copy(vol)
        v.integrate(depth[None], pose[None], Kt)
        got = v.render(torch.from_numpy(T.HELD_OUT_POSE), Kt, (H, W), depth_min=0.3, depth_max=3.6)["depth"].cpu().numpy()
        hit = (got > 0) & (frame > 0)
        err = np.abs(got.astype(np.float64) - frame)[hit] / R.VOXEL
        fig[label] = (float(np.median(err)), float(np.percentile(err, 95)), int(hit.sum()))
    print("TRACK-SEMANTIC fusion: |depth - analytic| at the true pose in voxels, median / p95: refined frame %.4f / %.4f (%d pixels), perturbed frame "
          "%.4f / %.4f (%d pixels)" % (fig["refined"] + fig["perturbed"]))
    assert fig["refined"][2] > 10000
    assert fig["refined"][0] < fig["perturbed"][0] and fig["refined"][1] < fig["perturbed"][1]


def test_track_refuses_when_nothing_matches(fused):
    vol, K, frame = fused
    depth, Kt = _dev(frame.astype(np.float32)), torch.from_numpy(K)
    away = torch.from_numpy(T.HELD_OUT_POSE @ np.diag([-1.0, 1.0, -1.0, 1.0]))
    out = vol.track(depth, away, Kt)
    assert not out["converged"] and out["reason"] == "count" and torch.equal(out["pose"], away) and out["iterations"] == 0
    chk = vol.check_frame(depth, away, Kt)
    assert chk["count"] == 0 and chk["rmse"] == 0.0 and bool((chk["match"] == -1).all())
    with pytest.raises(RuntimeError):
        vol.track(depth.cpu(), away, Kt)
    with pytest.raises(RuntimeError):
        vol.track(depth, away[:3], Kt)
