"""The colour path of the TSDF volume on the device (csrc/tsdf.hip tsdf_integrate_kernel<*, true> and tsdf_edge_colors_kernel,
csrc/tsdf_raycast.hip tsdf_raycast_kernel<*, true>) against the float64 references of tests/tsdf_color_ref.py, under both bindings.

Bars: D and Wt bit-identical to the call without colour; |C - C_ref| <= C_COLOR 2^-24 A_c on unambiguous updated voxels (ambiguous share <=
3 %); voxels the reference leaves alone keep their bits in all five planes; edge colours within C_EXTRACT 2^-24 (|C0| + |C1|); render colour
within C_RAY of its first-order bound; the median colour error at the extracted points <= 1.25 x the float64 reference's own median.
The figures of a device run are kept in profiles/tsdf_color_gpu_tests.txt."""
import numpy as np
import pytest
import torch

import tsdf_color_ref as CR
import tsdf_raycast_ref as RR
import tsdf_ref as R
from helpers import _binding

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_CACHE = {}


def _volume(case, color=True, D0=None, C0=None):
    from estdepth_amd.fusion3d import TSDFVolume
    p = case["params"]
    vol = TSDFVolume(case["dims"], case["voxel"], case["origin"], trunc=p["trunc"], w_max=p["w_max"], z_near=p["z_near"], device=DEV, color=color)
    if D0 is not None:
        vol.volume[0].copy_(torch.from_numpy(D0).to(DEV))
    if C0 is not None:
        vol.color.copy_(torch.from_numpy(C0).to(DEV))
    return vol


def _integrate(vol, fx, frames=None):
    """-> (D, Wt, C or None) copied back"""
    case = fx["case"]
    p = case["params"]
    sl = slice(None) if frames is None else frames
    depths = torch.from_numpy(case["depths"][sl]).to(DEV)
    confs = torch.from_numpy(case["confs"][sl]).to(DEV) if case["confs"] is not None else None
    images = torch.from_numpy(fx["images"][sl]).to(DEV) if vol.color is not None else None
    vol.integrate(depths, torch.from_numpy(case["poses"][sl]), torch.from_numpy(case["K"]), conf=confs, conf_min=p["conf_min"], weighted=p["weighted"],
                  images=images)
    torch.cuda.synchronize()
    v = vol.volume.cpu().numpy()
    return v[0], v[1], (vol.color.cpu().numpy() if vol.color is not None else None)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _check_case(name, normalised):
    fx = CR.fixture(name, normalised)
    case = fx["case"]
    D0, W0, C0, ref = fx["D0"], fx["W0"], fx["C0"], fx["ref"]
    vol, plain = _volume(case, True, D0, C0), _volume(case, False, D0)
    for call in range(case["calls"]):
        if call:                                                  # the second call of "second": the reference starts from the device's planes
            key = (name, normalised, call)
            if key not in _CACHE or not all(_same_bits(a, b) for a, b in zip(_CACHE[key][0], (D0, W0, C0))):
                _CACHE[key] = ((D0, W0, C0), CR.integrate(D0, W0, C0, fx["mats"], case["depths"], fx["images"], case["confs"], **case["params"]))
            ref = _CACHE[key][1]
        gD, gW, gC = _integrate(vol, fx)
        pD, pW, _ = _integrate(plain, fx)
        assert _same_bits(gD, pD) and _same_bits(gW, pW), "D / Wt differ from the call without colour"
        fig = CR.compare(gC, ref, C_before=C0)
        still = ~ref["amb"] & ~ref["updated"]
        assert _same_bits(gD[still], D0[still]) and _same_bits(gW[still], W0[still]), "an untouched voxel's D or Wt changed"
        assert fig["updated"] > 1000
        D0, W0, C0 = gD, gW, gC
    return D0, W0, C0


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", CR.CASES)
def test_integrate_color_against_reference(name, binding, monkeypatch):
    """every case under both bindings on planes pre-filled with a sentinel pattern: D / Wt bit-identical to tsdf_integrate_, colour within the
    bound, untouched voxels keep their bits in all five planes"""
    _binding(monkeypatch, binding)
    out = _check_case(name, False)
    if name == "second":
        assert out[1].max() == 4.0


def test_bindings_give_the_same_bits(monkeypatch):
    """ctypes == torch, bit for bit in all five planes, on an unweighted and a weighted case"""
    for name in ("t3", "weighted"):
        fx = CR.fixture(name)
        planes = []
        for binding in ("torch", "ctypes"):
            _binding(monkeypatch, binding)
            planes.append(_integrate(_volume(fx["case"], True, fx["D0"], fx["C0"]), fx))
        assert all(_same_bits(a, b) for a, b in zip(*planes)), name


def test_untouched_voxels_keep_a_non_zero_weight():
    """all five planes pre-filled, the weight plane with small integers: which voxels a call updates depends on the maps alone, so the voxels
    the reference leaves alone keep their bits in every plane, the weight included, and D / Wt equal the call without colour"""
    fx = CR.fixture("t3")
    case, ref = fx["case"], fx["ref"]
    W0 = np.random.RandomState(13).randint(0, 3, size=case["dims"]).astype(np.float32)
    vol, plain = _volume(case, True, fx["D0"], fx["C0"]), _volume(case, False, fx["D0"])
    for v in (vol, plain):
        v.volume[1].copy_(torch.from_numpy(W0).to(DEV))
    gD, gW, gC = _integrate(vol, fx)
    pD, pW, _ = _integrate(plain, fx)
    assert _same_bits(gD, pD) and _same_bits(gW, pW)
    still, moved = ~ref["amb"] & ~ref["updated"], ~ref["amb"] & ref["updated"]
    assert _same_bits(gW[still], W0[still]) and _same_bits(gD[still], fx["D0"][still]) and _same_bits(gC[:, still], fx["C0"][:, still])
    assert (gW[moved] > W0[moved]).all() and np.isfinite(gC).all()


@pytest.mark.parametrize("name", CR.NORMALISED)
def test_normalised_images(name):
    _check_case(name, True)


def test_one_call_versus_three_and_nine_frames_split():
    """one T = 3 call == three T = 1 calls, and nine frames through TSDFVolume.integrate == a call of eight and a call of one, bit for bit in
    all five planes"""
    fx = CR.fixture("t3")
    one = _integrate(_volume(fx["case"]), fx)
    vol = _volume(fx["case"])
    for t in range(3):
        three = _integrate(vol, fx, frames=slice(t, t + 1))
    assert all(_same_bits(a, b) for a, b in zip(one, three))
    fx8 = CR.fixture("t8")
    case = fx8["case"]
    nine = dict(fx8, case=dict(case, depths=np.concatenate([case["depths"], case["depths"][:1]]), poses=np.concatenate([case["poses"], case["poses"][:1]])),
                images=np.concatenate([fx8["images"], fx8["images"][:1]]))
    whole = _integrate(_volume(case), nine)
    vol = _volume(case)
    _integrate(vol, nine, frames=slice(0, 8))
    split = _integrate(vol, nine, frames=slice(8, 9))
    assert vol.frames == 9 and whole[1].max() == 9.0
    assert all(_same_bits(a, b) for a, b in zip(whole, split))


def _sorted_points(pts):
    order = torch.argsort(pts["edge"])
    return {k: v[order].cpu().numpy() for k, v in pts.items() if k != "count"}


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_extract_points_color(binding, monkeypatch):
    """extract_points()["color"] against the edge reference on the device's own planes; the other keys bit-identical to a colourless volume
    fed the same depths; the median colour error at the points against the analytic texture under 1.25 x the reference's own"""
    _binding(monkeypatch, binding)
    from estdepth_amd import ops
    for name in ("t3", "weighted"):
        fx = CR.fixture(name)
        case = fx["case"]
        vol, plain = _volume(case), _volume(case, False)
        gD, gW, gC = _integrate(vol, fx)
        _integrate(plain, fx)
        w_min = 1.0 if name == "t3" else 0.25
        pts, base = vol.extract_points(w_min=w_min), plain.extract_points(w_min=w_min)
        assert "color" not in base and set(pts) == set(base) | {"color"} and pts["count"] == base["count"] > 1000
        got, want = _sorted_points(pts), _sorted_points(base)
        for k in want:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        assert got["color"].shape == (pts["count"], 3)
        CR.compare_edge_colors(got["color"], got["edge"], gD, gC)
        med, p95 = CR.median_error(got["xyz"], got["color"])
        ref_med, ref_p95 = _CACHE.setdefault(("median", name), CR.reference_median(CR.integrate(
            np.zeros_like(gD), np.zeros_like(gW), np.zeros_like(gC), fx["mats"], case["depths"], fx["images"], case["confs"], **case["params"]), case, w_min))
        print("colour at the points, %s: median %.3f (reference %.3f, bar %.3f), 95th percentile %.2f (reference %.2f) of 255"
              % (name, med, ref_med, CR.MEDIAN_FACTOR * ref_med, p95, ref_p95))
        assert med <= CR.MEDIAN_FACTOR * ref_med
    # ids outside the volume (or whose far end is) give zeros; no record: an empty result
    Z, Y, X = case["dims"]
    n = Z * Y * X
    edge = torch.tensor([-1, 3 * n, 3 * (X - 1), 3 * (n - 1) + 2, 3 * (n - 1) + 1, int(got["edge"][0])], device=DEV)
    col = ops.tsdf_edge_colors(vol.volume, vol.color, edge).cpu().numpy()
    assert (col[:5] == 0).all() and _same_bits(col[5], got["color"][0])
    assert tuple(ops.tsdf_edge_colors(vol.volume, vol.color, edge[:0]).shape) == (0, 3)
    vol.reset()
    assert float(vol.color.abs().sum()) == 0 and vol.extract_points()["color"].shape == (0, 3)


def _render(vol, case, pose, w_min):
    H, W = case["depths"].shape[1:]
    out = vol.render(torch.from_numpy(np.asarray(pose)), torch.from_numpy(case["K"]), (H, W), depth_min=RR.T_MIN, depth_max=RR.T_MAX, w_min=w_min)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", ["t3", "odd"])
def test_render_color(name, binding, monkeypatch):
    """render() at the held-out pose: depth / normal / weight bit-identical to the colourless render, colour against the reference, no-hit
    pixels exactly zero"""
    from estdepth_amd import camera
    from estdepth_amd.fusion3d import render_plan
    _binding(monkeypatch, binding)
    fx = CR.fixture(name)
    case = fx["case"]
    vol, plain = _volume(case), _volume(case, False)
    gD, gW, gC = _integrate(vol, fx)
    _integrate(plain, fx)
    got, base = _render(vol, case, RR.HELD_OUT_POSE, 1.0), _render(plain, case, RR.HELD_OUT_POSE, 1.0)
    assert set(got) == set(base) | {"color"}
    for k in base:
        assert _same_bits(got[k], base[k]), k
    if ("render", name) not in _CACHE:
        view = RR.view(case)
        pose, K = torch.from_numpy(RR.HELD_OUT_POSE), torch.from_numpy(case["K"])
        view["M"] = camera.tsdf_ray_matrix(pose, K, case["origin"], case["voxel"]).numpy().reshape(3, 4)
        view["n_steps"] = render_plan(vol.dims, vol.voxel_size, vol.origin, vol.z_near, pose, K, (view["H"], view["W"]), RR.T_MIN, RR.T_MAX)[4][0]
        _CACHE["render", name] = (gD, gW, gC), CR.render_colors(gD, gW, gC, view, 1.0)
    planes, ref = _CACHE["render", name]
    assert all(_same_bits(a, b) for a, b in zip(planes, (gD, gW, gC)))
    RR.compare(got, ref["ray"], "%s %s" % (name, binding))
    fig = CR.compare_render(got["color"], ref, "%s %s" % (name, binding))
    assert fig["hit"] > 5000
    assert (got["color"][got["depth"] == 0] == 0).all()
    stack = vol.render(torch.from_numpy(np.stack([RR.HELD_OUT_POSE, case["poses"][0]])), torch.from_numpy(case["K"]), got["depth"].shape,
                       depth_min=RR.T_MIN, depth_max=RR.T_MAX)
    assert tuple(stack["color"].shape) == (2,) + got["color"].shape and _same_bits(stack["color"][0].cpu().numpy(), got["color"])


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_arguments_raise_before_launch(binding, monkeypatch):
    from estdepth_amd import ops
    from estdepth_amd.fusion3d import TSDFVolume
    _binding(monkeypatch, binding)
    vol, col = torch.zeros(2, 8, 8, 8, device=DEV), torch.zeros(3, 8, 8, 8, device=DEV)
    d, im = [torch.ones(6, 8, device=DEV)], [torch.ones(3, 6, 8, device=DEV)]
    m = torch.zeros(1, 12)

    def integ(volume=vol, color=col, depths=d, images=im, mats=m):
        ops.tsdf_integrate_color_(volume, color, depths, [], images, mats, 0.1, 1e-3, 0.0, False, 64.0)
    integ()                                                                           # the well-formed call passes
    for bad in (dict(color=torch.zeros(2, 8, 8, 8, device=DEV)), dict(color=torch.zeros(3, 8, 8, 4, device=DEV)), dict(color=col.cpu()), dict(color=col.double()),
                dict(color=torch.zeros(3, 8, 8, 16, device=DEV)[..., ::2]), dict(images=[]), dict(images=im * 2), dict(images=[torch.ones(3, 6, 8)]),
                dict(images=[torch.ones(3, 6, 9, device=DEV)]), dict(images=[torch.ones(1, 6, 8, device=DEV)]), dict(images=[torch.ones(3, 6, 8, device=DEV).half()]),
                dict(volume=vol.cpu()), dict(depths=d * 9, images=im * 9, mats=torch.zeros(9, 12))):
        with pytest.raises(RuntimeError):
            integ(**bad)
    edge = torch.zeros(4, dtype=torch.int64, device=DEV)
    ops.tsdf_edge_colors(vol, col, edge)
    for bad in (dict(color=col[:2]), dict(color=col.cpu()), dict(edge=edge.int()), dict(edge=edge.cpu()), dict(edge=edge[None]), dict(volume=vol.double())):
        a = dict(dict(volume=vol, color=col, edge=edge), **bad)
        with pytest.raises(RuntimeError):
            ops.tsdf_edge_colors(a["volume"], a["color"], a["edge"])
    mat = torch.tensor([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    ops.tsdf_raycast_color(vol, col, mat, 4, 4, 0.0, 1.0, 4, 1.0)
    for bad in (dict(color=col[:2]), dict(color=col.cpu()), dict(color=torch.zeros(3, 8, 4, 8, device=DEV)), dict(mat=mat[:11]), dict(H=0), dict(n_steps=0),
                dict(dt=0.0)):
        a = dict(dict(color=col, mat=mat, H=4, n_steps=4, dt=1.0), **bad)
        with pytest.raises(RuntimeError):
            ops.tsdf_raycast_color(vol, a["color"], a["mat"], a["H"], 4, 0.0, a["dt"], a["n_steps"], 1.0)
    # the volume class: images are required by a colour volume and an error for any other
    poses, K = torch.eye(4)[None], torch.eye(3)
    cv = TSDFVolume((8, 8, 8), 0.1, (0, 0, 0), device=DEV, color=True)
    pv = TSDFVolume((8, 8, 8), 0.1, (0, 0, 0), device=DEV)
    with pytest.raises(RuntimeError):
        cv.integrate(d[0][None], poses, K)
    with pytest.raises(RuntimeError):
        pv.integrate(d[0][None], poses, K, images=im[0][None])
    with pytest.raises(RuntimeError):
        cv.integrate(d[0][None], poses, K, images=im[0][None].cpu())
    with pytest.raises(RuntimeError):
        cv.integrate(d[0][None], poses, K, images=torch.ones(1, 3, 6, 10, device=DEV))
    torch.cuda.synchronize()
    assert cv.frames == 0 and float(cv.color.abs().sum()) == 0 and float(cv.volume.abs().sum()) == 0


def test_end_to_end_joint_stream_color(tmp_path):
    """JointStream over a short synthetic sequence with the clips' own images passed through integrate_outputs: the planes equal a colourless
    volume's where they overlap, the coloured PLY holds extract_points' vertices and its RGB bytes round-trip"""
    from estdepth_amd import DepthNetHybrid, synth
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    from estdepth_amd.streaming import JointStream
    torch.backends.cudnn.allow_tf32 = False
    H, W, n_frames, seq = 128, 160, 5, 5
    m = DepthNetHybrid(ndepths=64, depth_min=0.1, depth_max=10.0, resnet=18, IF_EST_transformer=True).eval()
    synth.fill_state_dict(m, seed=3, head_gain=1.0)
    m = m.to(DEV)
    imgs = synth.smooth_images(n_frames, H, W, seed=9)[0].to(DEV)
    poses = torch.from_numpy(np.stack([synth.camera_pose(v) for v in range(n_frames)])).float()
    K = torch.from_numpy(synth.intrinsics(H, W)).float()
    dims, vox = (64, 64, 64), 0.08
    origin = frustum_volume(poses[1], K, (H, W), 0.1, 5.0, dims, vox)
    stream = JointStream(m, seq_len=seq, graph=True)
    vol, plain = TSDFVolume(dims, vox, origin, device=DEV, color=True), TSDFVolume(dims, vox, origin, device=DEV)
    outputs, _, _ = stream.push_clip(imgs, poses.to(DEV), K.to(DEV))
    with pytest.raises(RuntimeError):
        vol.integrate_outputs(outputs, poses[None], K[None], imgs=imgs[None, :, :, ::2, ::2])
    vol.integrate_outputs(outputs, poses[None], K[None], imgs=imgs[None])
    plain.integrate_outputs(outputs, poses[None], K[None])
    torch.cuda.synchronize()
    assert vol.frames == seq - 2 and torch.equal(vol.volume.view(torch.int32), plain.volume.view(torch.int32))
    seen = vol.volume[1] > 0
    assert int(seen.sum()) > 1000 and float(vol.color[:, ~seen].abs().sum()) == 0
    lo, hi = float(imgs[1:seq - 1].min()), float(imgs[1:seq - 1].max())
    assert float(vol.color[:, seen].min()) >= lo - 1e-4 and float(vol.color[:, seen].max()) <= hi + 1e-4          # an average of image values
    scale, offset = 200.0 / max(hi - lo, 1e-6), -lo * 200.0 / max(hi - lo, 1e-6) + 20.0
    path = tmp_path / "scene.ply"
    n = vol.save_ply(str(path), color_scale=scale, color_offset=offset)
    pts = vol.extract_points()
    assert n == pts["count"] > 100
    head, body = path.read_bytes().split(b"end_header\n", 1)
    assert b"element vertex %d\n" % n in head and b"property uchar blue" in head and len(body) == 27 * n
    rec = np.frombuffer(body, dtype=[("v", "<f4", (6,)), ("c", "u1", (3,))])
    order = torch.argsort(pts["edge"])
    want = np.clip(np.rint(pts["color"][order].cpu().numpy().astype(np.float64) * scale + offset), 0, 255).astype(np.uint8)
    assert np.array_equal(rec["c"], want) and want.min() >= 19 and want.max() <= 221 and want.std() > 0
    assert np.array_equal(rec["v"][:, :3], pts["xyz"][order].cpu().numpy())
