"""csrc/tsdf_raycast.hip on the device against the float64 reference of tests/tsdf_raycast_ref.py.  Every volume is fused on the device by the
existing integrate, copied back, rendered on the device, and the reference is evaluated on the copied-back volume: the cases of
tsdf_raycast_ref.VALUE_CASES under both bindings from a held-out and from a fused pose, the 640 x 480 render of the 256^3 volume, holes, an
empty volume, cameras inside and beside the volume, the front-face rule, identical bits across calls and across a pose stack, the geometry
against the analytic scene, malformed arguments under both bindings and the end-to-end path JointStream(graph=True) -> integrate_outputs ->
render.

Bar (tsdf_raycast_ref.compare): ambiguous pixels <= 3 % of the hit pixels; on all others hit / no-hit agrees exactly, no-hit pixels are exactly
zero, and depth, normal and weight are within C_RAY = 4 times their first-order bounds.  Geometry: |depth - analytic| <= 0.1 voxel in the
median and 0.5 voxel at the 95th percentile of the hit pixels.
Figures of the CPU stand-ins (the numpy-fp32 evaluation and the kernel's source compiled for the host): largest depth error 0.38 of the unscaled
bound (bar 4), normals 0.04, weights 0.13; ambiguous share 0.0008 - 0.0045 (cap 0.03).  The figures of a device run are not recorded yet: this
file prints them per case (pytest -s)."""
import numpy as np
import pytest
import torch

import placement as PL
import tsdf_ref as R
import tsdf_raycast_ref as RR
from helpers import _binding

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_FUSED = {}
_REFS = {}


def _fused(name, place=None):
    """(case, TSDFVolume fused on the device by integrate, D, Wt copied back), once per case"""
    name = name if PL.key(place) is None else "%s@%s" % (name, PL.label(place))
    if name not in _FUSED:
        from estdepth_amd.fusion3d import TSDFVolume
        case = R.build_case(name.split("@")[0], place)
        p = case["params"]
        vol = TSDFVolume(case["dims"], case["voxel"], case["origin"], trunc=p["trunc"], w_max=p["w_max"], z_near=p["z_near"], device=DEV)
        depths = torch.from_numpy(case["depths"]).to(DEV)
        confs = torch.from_numpy(case["confs"]).to(DEV) if case["confs"] is not None else None
        for _ in range(case["calls"]):
            vol.integrate(depths, torch.from_numpy(case["poses"]), torch.from_numpy(case["K"]), conf=confs, conf_min=p["conf_min"], weighted=p["weighted"])
        torch.cuda.synchronize()
        v = vol.volume.cpu().numpy()
        _FUSED[name] = (case, vol, v[0], v[1])
    return _FUSED[name]


def _n_steps(vol, case, pose, depth_min=RR.T_MIN, depth_max=RR.T_MAX):
    """samples per ray of the render below, as TSDFVolume.render derives them from the depth range"""
    from estdepth_amd.fusion3d import render_plan
    H, W = case["depths"].shape[1:]
    return render_plan(vol.dims, vol.voxel_size, vol.origin, vol.z_near, torch.from_numpy(np.asarray(pose)), torch.from_numpy(case["K"]), (H, W),
                       depth_min, depth_max)[4][0]


def _render(vol, case, pose, w_min, depth_min=RR.T_MIN, depth_max=RR.T_MAX):
    H, W = case["depths"].shape[1:]
    out = vol.render(torch.from_numpy(np.asarray(pose)), torch.from_numpy(case["K"]), (H, W), depth_min=depth_min, depth_max=depth_max, w_min=w_min)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _reference(case, D, Wt, pose, w_min, t_min=RR.T_MIN, n_steps=None):
    from estdepth_amd import camera
    v = RR.view(case, pose)
    M = camera.tsdf_ray_matrix(torch.from_numpy(np.asarray(v["pose"])), torch.from_numpy(case["K"]), case["origin"], case["voxel"]).numpy().reshape(3, 4)
    assert np.array_equal(M, v["M"]) or np.abs(M.astype(np.float64) - v["M"]).max() <= 2.0 ** -23 * np.abs(v["M"]).max()
    return RR.raycast(D, Wt, M, v["H"], v["W"], t_min, v["dt"], n_steps or _n_steps(_FUSED[case["name"]][1], case, pose, t_min, RR.T_MAX), w_min)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("which", ["held_out", "fused"])
@pytest.mark.parametrize("name,w_min", RR.VALUE_CASES)
def test_render_against_reference(name, w_min, which, binding, monkeypatch):
    """every case of the table, from a pose that was never fused and from a fused one, under both bindings"""
    _binding(monkeypatch, binding)
    case, vol, D, Wt = _fused(name)
    pose = RR.HELD_OUT_POSE if which == "held_out" else case["poses"][-1]
    got = _render(vol, case, pose, w_min)
    if (name, w_min, which) not in _REFS:                            # the same device volume under both bindings: one reference
        _REFS[name, w_min, which] = _reference(case, D, Wt, pose, w_min)
    fig = RR.compare(got, _REFS[name, w_min, which], "%s w_min %g %s %s" % (name, w_min, which, binding))
    assert fig["hit"] > 1000


@pytest.mark.parametrize("where", list(PL.FAMILY_PLACES))
def test_render_away_from_the_origin(where):
    """the smallest case fused and rendered 64 m and 512 m out (tests/placement.py): the pixel-to-ray matrix is formed in float64 relative
    to the volume's corner, so the rays are those at the origin; the comparison and its cap are unchanged"""
    place = PL.FAMILY_PLACES[where]
    case, vol, D, Wt = _fused(R.PLACED_CASE, place)
    pose = PL.pose(RR.HELD_OUT_POSE, place)
    fig = RR.compare(_render(vol, case, pose, 1.0), _reference(case, D, Wt, pose, 1.0), case["name"])
    assert fig["hit"] > 1000
    print("PLACEMENT tsdf_raycast %s: ambiguous share %.4f, hit %d" % (case["name"], fig["amb_share"], fig["hit"]))
    _FUSED.pop(case["name"])


def test_render_full_size():
    """640 x 480 out of the 256^3 volume"""
    name, w_min = RR.FULL_CASE
    case, vol, D, Wt = _fused(name)
    got = _render(vol, case, RR.HELD_OUT_POSE, w_min)
    fig = RR.compare(got, _reference(case, D, Wt, RR.HELD_OUT_POSE, w_min), "full")
    assert fig["hit"] > 100000
    _FUSED.pop(name)


def test_ragged_volumes_run_clean():
    """"gated" and "weighted" at w_min 1: ragged observed regions, beyond the ambiguity cap, so no value comparison: outputs finite, hit /
    no-hit and zeros as the reference has them outside its ambiguous pixels"""
    for name in ("gated", "weighted"):
        case, vol, D, Wt = _fused(name)
        got = _render(vol, case, RR.HELD_OUT_POSE, 1.0)
        ref = _reference(case, D, Wt, RR.HELD_OUT_POSE, 1.0)
        assert all(np.isfinite(v).all() for v in got.values())
        keep = ~ref["amb"]
        assert np.array_equal((got["depth"] != 0)[keep], ref["hit"][keep])
        miss = got["depth"] == 0
        assert (got["weight"][miss] == 0).all() and (got["normal"][miss] == 0).all()


def test_holes_leave_unobserved_pixels_empty():
    """NaN / inf / 0 depths left unobserved regions inside the view: fewer hits than the same scene without holes, none invented"""
    case, vol, D, Wt = _fused("holes")
    got = _render(vol, case, RR.HELD_OUT_POSE, 1.0)
    full = _render(_fused("t3")[1], _fused("t3")[0], RR.HELD_OUT_POSE, 1.0)
    n_holes, n_full = int((got["depth"] > 0).sum()), int((full["depth"] > 0).sum())
    assert 1000 < n_holes < n_full - 500


def test_empty_volume_and_missing_frustum():
    """"away": nothing was fused -> zero hits, all outputs exactly zero; a camera that looks away from a filled volume: the same"""
    case, vol, D, Wt = _fused("away")
    assert Wt.max() == 0
    got = _render(vol, case, RR.HELD_OUT_POSE, 1.0)
    assert all((v == 0).all() for v in got.values())
    case, vol, D, Wt = _fused("t3")
    flip = np.diag([-1.0, 1.0, -1.0, 1.0])
    pose = RR.HELD_OUT_POSE @ flip                                   # half a turn about y: the frustum misses the volume
    got = _render(vol, case, pose, 1.0)
    assert all((v == 0).all() for v in got.values())
    RR.compare(got, _reference(case, D, Wt, pose, 1.0), "t3 looking away")
    beside = R.look_at((30.0, 0.0, 0.0), (30.0, 0.0, 5.0))          # parallel to the volume, 30 m to its side
    got = _render(vol, case, beside, 1.0)
    assert all((v == 0).all() for v in got.values())


def test_front_face_rule():
    """t_min behind the sphere's front and the plane: rays that start inside the band behind a surface or beyond it do not hit it"""
    case, vol, D, Wt = _fused("t3")
    got = _render(vol, case, RR.HELD_OUT_POSE, 1.0, depth_min=1.7)
    fig = RR.compare(got, _reference(case, D, Wt, RR.HELD_OUT_POSE, 1.0, t_min=1.7), "t3 from t_min 1.7")
    assert fig["hit"] > 1000 and (got["depth"][got["depth"] > 0] > 1.7).all()
    front = _render(vol, case, RR.HELD_OUT_POSE, 1.0)["depth"]
    inside_sphere = (front > 0) & (front < 1.6)                      # pixels whose surface lies in front of t_min: the sphere is not hit from inside
    assert inside_sphere.sum() > 1000 and not ((got["depth"] > 0) & (got["depth"] < 2.3) & inside_sphere).any()
    # behind the plane (z-depth 2.61 .. 2.69 in this camera), inside its band: no front face anywhere; no hit pixels, so no share to cap
    got = _render(vol, case, RR.HELD_OUT_POSE, 1.0, depth_min=2.72)
    ref = _reference(case, D, Wt, RR.HELD_OUT_POSE, 1.0, t_min=2.72)
    assert ref["hit"].sum() == 0 and (got["depth"][~ref["amb"]] == 0).all() and (got["depth"] > 0).sum() <= ref["amb"].sum()


def test_calls_and_stacks_give_identical_bits():
    case, vol, D, Wt = _fused("t3")
    a = _render(vol, case, RR.HELD_OUT_POSE, 1.0)
    b = _render(vol, case, RR.HELD_OUT_POSE, 1.0)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    poses = np.stack([RR.HELD_OUT_POSE, case["poses"][0], case["poses"][2]])
    stack = _render(vol, case, poses, 1.0)
    assert stack["depth"].shape == (3,) + a["depth"].shape and stack["normal"].shape == (3,) + a["normal"].shape
    for i in range(3):
        one = _render(vol, case, poses[i], 1.0)
        for k in one:
            assert np.array_equal(one[k].view(np.uint32), stack[k][i].view(np.uint32)), (k, i)
    # the default range (z_near .. past the volume, one voxel per step) finds the same surface
    H, W = case["depths"].shape[1:]
    dflt = vol.render(torch.from_numpy(RR.HELD_OUT_POSE), torch.from_numpy(case["K"]), (H, W))["depth"].cpu().numpy()
    both = (dflt > 0) & (a["depth"] > 0)
    assert both.sum() > 0.98 * (a["depth"] > 0).sum() and np.median(np.abs(dflt - a["depth"])[both]) < 0.1 * case["voxel"]


@pytest.mark.parametrize("name", ["t3", "t8", "full"])
def test_geometry_against_the_analytic_scene(name):
    """independent of the reference's arithmetic: the rendered depth at the held-out pose against the analytic plane-plus-sphere scene"""
    case, vol, D, Wt = _fused(name)
    got = _render(vol, case, RR.HELD_OUT_POSE, 1.0)
    H, W = got["depth"].shape
    ana = R.raycast_scene(RR.HELD_OUT_POSE, case["K"], H, W)
    hit = (got["depth"] > 0) & (ana > 0)
    assert hit.sum() > 10000
    err = np.abs(got["depth"].astype(np.float64) - ana)[hit] / case["voxel"]
    med, p95 = float(np.median(err)), float(np.percentile(err, 95))
    print("tsdf_raycast geometry %s: %d hit pixels, |depth - analytic| median %.4f voxel, p95 %.4f voxel, max %.2f voxel" % (name, hit.sum(), med, p95, err.max()))
    assert med <= 0.1 and p95 <= 0.5
    # the normals of the plane's pixels point back at the cameras (-z)
    on_plane = hit & (np.abs(RR.backproject(got["depth"], RR.HELD_OUT_POSE, case["K"])[..., 2] - 2.6) < case["voxel"])
    assert on_plane.sum() > 1000 and (got["normal"][on_plane, 2] < -0.9).mean() > 0.95
    if name == "full":
        _FUSED.pop(name)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_arguments_raise_before_launch(binding, monkeypatch):
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    vol = torch.zeros(2, 8, 8, 8, device=DEV)
    mat = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]).reshape(12)
    good = dict(volume=vol, mat=mat, H=6, W=8, t_min=0.0, dt=0.5, n_steps=8, w_min=1.0)

    def cast(**kw):
        a = dict(good, **kw)
        return ops.tsdf_raycast(a["volume"], a["mat"], a["H"], a["W"], a["t_min"], a["dt"], a["n_steps"], a["w_min"])
    cast()
    for bad in (dict(volume=vol.double()), dict(volume=vol.cpu()), dict(volume=torch.zeros(2, 8, 8, 16, device=DEV)[..., ::2]),
                dict(volume=torch.zeros(2, 8, 8, 10, device=DEV)), dict(volume=torch.zeros(8, 8, 8, device=DEV)), dict(volume=torch.zeros(3, 8, 8, 8, device=DEV)),
                dict(mat=mat.to(DEV)), dict(mat=mat[:9]), dict(mat=mat.double()), dict(mat=torch.full((12,), float("nan"))),
                dict(H=0), dict(W=-1), dict(n_steps=0), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("inf")), dict(t_min=-0.1), dict(t_min=float("nan")),
                dict(w_min=float("nan"))):
        with pytest.raises(RuntimeError):
            cast(**bad)
    d, n, w = cast()                                                 # a well-formed call still works
    torch.cuda.synchronize()
    assert tuple(d.shape) == (6, 8) and tuple(n.shape) == (6, 8, 3) and tuple(w.shape) == (6, 8) and float(d.abs().sum()) == 0.0


def test_end_to_end_joint_stream():
    """plumbing, not values: JointStream(graph=True) over a short synthetic sequence, integrate_outputs per clip, then render at every target
    pose: some pixels hit, every output is finite, no-hit pixels are exactly zero, render == ops.tsdf_raycast with camera.tsdf_ray_matrix on the
    same volume bit for bit, and a second identical run gives the same bits"""
    from estdepth_amd import DepthNetHybrid, camera, ops, synth
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume, render_plan
    from estdepth_amd.streaming import JointStream
    torch.backends.cudnn.allow_tf32 = False
    H, W, n_frames, seq = 128, 160, 8, 5
    m = DepthNetHybrid(ndepths=64, depth_min=0.1, depth_max=10.0, resnet=18, IF_EST_transformer=True).eval()
    synth.fill_state_dict(m, seed=3, head_gain=1.0)
    m = m.to(DEV)
    imgs = synth.smooth_images(n_frames, H, W, seed=9)[0].to(DEV)
    poses = torch.from_numpy(np.stack([synth.camera_pose(v) for v in range(n_frames)])).float()
    K = torch.from_numpy(synth.intrinsics(H, W)).float()
    dims, vox = (64, 64, 64), 0.08
    origin = frustum_volume(poses[1], K, (H, W), 0.1, 5.0, dims, vox)
    runs = []
    for run in range(2):
        stream = JointStream(m, seq_len=seq, graph=True)
        vol = TSDFVolume(dims, vox, origin, device=DEV)
        targets = []
        for start in range(0, n_frames - seq + 1, stream.stride):
            sl = slice(start, start + seq)
            outputs, _, _ = stream.push_clip(imgs[sl], poses[sl].to(DEV), K.to(DEV))
            vol.integrate_outputs(outputs, poses[sl][None], K[None])
            targets += list(range(start + 1, start + seq - 1))
        maps = vol.render(poses[targets], K, (H, W))
        torch.cuda.synchronize()
        assert maps["depth"].shape == (len(targets), H, W)
        hits = 0
        for i, t in enumerate(targets):
            d, n, w = maps["depth"][i], maps["normal"][i], maps["weight"][i]
            assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(n).all()) and bool(torch.isfinite(w).all())
            miss = d == 0
            assert float(w[miss].abs().sum()) == 0.0 and float(n[miss].abs().sum()) == 0.0 and bool((d >= 0).all())
            hits += int((~miss).sum())
            mats, hw, t_min, dt, n_steps, _ = render_plan(vol.dims, vol.voxel_size, vol.origin, vol.z_near, poses[t], K, (H, W))
            assert torch.equal(mats, camera.tsdf_ray_matrix(poses[t], K, vol.origin, vol.voxel_size))
            direct = ops.tsdf_raycast(vol.volume, mats[0].contiguous(), H, W, t_min, dt, n_steps[0], 1.0)
            for a, b in zip((d, n, w), direct):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert hits > 0
        runs.append(maps)
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), k
