"""csrc/tsdf.hip on the device against the float64 reference of tests/tsdf_ref.py: estd_tsdf_integrate over the cases of tsdf_ref.CASES,
untouched voxels, one call versus three, estd_tsdf_extract_points, malformed arguments under both bindings, and the end-to-end path
JointStream(graph=True) -> TSDFVolume.integrate_outputs.

Bar (tsdf_ref.compare): ambiguous voxels <= 3 % of the updated ones; on all others Wt exact (unweighted) and |D - D_ref| <= 5 * 2^-24 * A.
Measured on an MI355X (profiles/tsdf_gpu_tests.txt): largest |D - D_ref| / (2^-24 A) over every case 1.024 (case "second", first call);
ambiguous share at most 0.0202 (case "full"; the small cases 0.0009 - 0.0060); one T = 3 call and three T = 1 calls came out BIT-IDENTICAL;
extraction: positions at most 1.49, weights 0.71, normals 0.37 in units of 2^-24 of their magnitudes (bound 8)."""
import numpy as np
import pytest
import torch

import placement as PL
import tsdf_ref as R
from helpers import _binding

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _volume(case, fill=None):
    from estdepth_amd.fusion3d import TSDFVolume
    p = case["params"]
    vol = TSDFVolume(case["dims"], case["voxel"], case["origin"], trunc=p["trunc"], w_max=p["w_max"], z_near=p["z_near"], device=DEV)
    if fill is not None:
        vol.volume[0].copy_(torch.from_numpy(fill).to(DEV))
    return vol


def _integrate(vol, case, frames=None):
    p = case["params"]
    sl = slice(None) if frames is None else frames
    depths = torch.from_numpy(case["depths"][sl]).to(DEV)
    confs = torch.from_numpy(case["confs"][sl]).to(DEV) if case["confs"] is not None else None
    vol.integrate(depths, torch.from_numpy(case["poses"][sl]), torch.from_numpy(case["K"]), conf=confs, conf_min=p["conf_min"],
                  weighted=p["weighted"])
    torch.cuda.synchronize()
    v = vol.volume.cpu().numpy()
    return v[0], v[1]


def _mats(case):
    from estdepth_amd import camera
    return camera.tsdf_matrices(torch.from_numpy(case["poses"]), torch.from_numpy(case["K"]), case["origin"], case["voxel"]).numpy().reshape(-1, 3, 4)


def _sentinel(dims):
    """a pattern of D values at Wt = 0 that no update produces by accident"""
    rng = np.random.RandomState(11)
    return rng.uniform(-0.9, 0.9, size=dims).astype(np.float32)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", [n for n in sorted(R.CASES) if n != "full"])
def test_integrate_against_reference(name, binding, monkeypatch):
    """every small case under both bindings, on a volume pre-filled with a sentinel pattern at Wt = 0: values within the bar, voxels the
    reference leaves alone keep the pattern bit for bit"""
    _binding(monkeypatch, binding)
    case = R.build_case(name)
    D0, W0 = _sentinel(case["dims"]), np.zeros(case["dims"], np.float32)
    vol = _volume(case, fill=D0)
    mats = _mats(case)
    for _ in range(case["calls"]):
        gD, gW = _integrate(vol, case)
        ref = R.integrate(D0, W0, mats, case["depths"], case["confs"], **case["params"])
        fig = R.compare(gD, gW, ref, weighted=case["params"]["weighted"], D_before=D0, W_before=W0)
        assert fig["updated"] == 0 if name == "away" else fig["updated"] > 1000
        D0, W0 = gD, gW
    if name == "second":
        assert gW.max() == 4.0


@pytest.mark.parametrize("where", list(PL.FAMILY_PLACES))
def test_integrate_away_from_the_origin(where):
    """the smallest case with its cameras and the volume's corner 64 m and 512 m out (tests/placement.py): the host forms the voxel-to-pixel
    matrices in float64 relative to the volume's corner, so the kernel sees the numbers it sees at the origin to their last bits or so;
    the comparison and its cap are unchanged (the reference alone: tests/test_placement_ref_cpu.py)"""
    case = R.build_case(R.PLACED_CASE, PL.FAMILY_PLACES[where])
    assert min(abs(v) for v in case["origin"]) > PL.FAMILY_PLACES[where][0] / 4
    D0, W0 = _sentinel(case["dims"]), np.zeros(case["dims"], np.float32)
    vol = _volume(case, fill=D0)
    gD, gW = _integrate(vol, case)
    ref = R.integrate(D0, W0, _mats(case), case["depths"], case["confs"], **case["params"])
    fig = R.compare(gD, gW, ref, D_before=D0, W_before=W0)
    assert fig["updated"] > 1000
    print("PLACEMENT tsdf_integrate %s: ambiguous share %.4f, updated %d" % (case["name"], fig["amb_share"], fig["updated"]))
    ref = R.extract(gD, gW, 1.0, case["voxel"], case["origin"])               # the points of the same volume: positions 64 m and 512 m out
    got = _points(vol.extract_points(w_min=1.0))
    assert np.array_equal(np.sort(got["edge"]), ref["edge"]) and len(ref["edge"]) > 1000
    R.compare_points(got, ref)


def test_integrate_full_size():
    """640 x 480 maps into a 256^3 volume"""
    case = R.build_case("full")
    vol = _volume(case)
    gD, gW = _integrate(vol, case)
    Z0 = np.zeros(case["dims"], np.float32)
    ref = R.integrate(Z0, Z0, _mats(case), case["depths"], None, **case["params"])
    R.compare(gD, gW, ref, D_before=Z0, W_before=Z0)


def test_one_call_versus_three():
    """one T = 3 call and three T = 1 calls both meet the bar; they are expected to be bit-identical, and on an MI355X they are"""
    case = R.build_case("t3")
    one = _integrate(_volume(case), case)
    vol = _volume(case)
    for t in range(3):
        three = _integrate(vol, case, frames=slice(t, t + 1))
    Z0 = np.zeros(case["dims"], np.float32)
    ref = R.integrate(Z0, Z0, _mats(case), case["depths"], None, **case["params"])
    R.compare(*one, ref)
    R.compare(*three, ref)
    same = np.array_equal(one[0].view(np.uint32), three[0].view(np.uint32)) and np.array_equal(one[1], three[1])
    print("one T=3 call vs three T=1 calls bit-identical:", same)
    assert same


def test_more_than_eight_frames_split_in_order():
    """11 frames = one call of 8 + one of 3 == the reference fed frame by frame"""
    case = R.build_case("t8")
    depths = np.concatenate([case["depths"], case["depths"][:3]])
    poses = np.concatenate([case["poses"], case["poses"][:3]])
    big = dict(case, depths=depths, poses=poses)
    gD, gW = _integrate(_volume(big), big)
    Z0 = np.zeros(case["dims"], np.float32)
    ref = R.integrate(Z0, Z0, _mats(big), depths, None, **case["params"])
    R.compare(gD, gW, ref)
    assert gW.max() == 11.0


def _points(pts):
    return {k: pts[k].cpu().numpy() for k in ("edge", "xyz", "normal", "weight")}


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_extraction_against_reference(binding, monkeypatch):
    _binding(monkeypatch, binding)
    case = R.build_case("t3")
    vol = _volume(case)
    gD, gW = _integrate(vol, case)
    for w_min in (1.0, 3.0):
        ref = R.extract(gD, gW, w_min, case["voxel"], case["origin"])
        pts = vol.extract_points(w_min=w_min)
        assert pts["count"] == len(ref["edge"]) > 1000
        got = _points(pts)
        assert np.array_equal(np.sort(got["edge"]), ref["edge"])
        R.compare_points(got, ref)
        # towards the free space the cameras saw: on the plane z = 2.6 the normals point back at the cameras (-z)
        on_plane = np.abs(got["xyz"][:, 2] - 2.6) < case["voxel"]
        assert on_plane.sum() > 100 and (got["normal"][on_plane, 2] < -0.5).mean() > 0.95
    # too small a capacity: the full count comes back, exactly `capacity` records are written, each one a reference crossing
    ref = R.extract(gD, gW, 1.0, case["voxel"], case["origin"])
    cap = len(ref["edge"]) // 3
    pts = vol.extract_points(w_min=1.0, capacity=cap)
    assert pts["count"] == len(ref["edge"]) and pts["edge"].shape[0] == cap
    R.compare_points(_points(pts), ref)
    # an empty volume has no crossing
    vol.reset()
    assert vol.extract_points()["count"] == 0 and vol.fused_voxels() == 0


def test_extraction_on_sphere_volume_with_borders(tmp_path):
    """an analytic volume whose surface runs into the border and into unobserved voxels (one-sided differences); PLY written"""
    from estdepth_amd.fusion3d import TSDFVolume
    n, vox = 40, 0.05
    c = (np.arange(n) + 0.5) * vox
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    sdf = np.sqrt((x - 1.0) ** 2 + (y - 0.9) ** 2 + (z - 0.2) ** 2) - 0.7
    D = np.clip(sdf / 0.2, -1, 1).astype(np.float32)
    W = np.where((np.abs(sdf) < 0.15) & (x + y < 2.6), 2.0, 0.0).astype(np.float32)
    vol = TSDFVolume((n, n, n), vox, (0.0, 0.0, 0.0), device=DEV)
    vol.volume.copy_(torch.from_numpy(np.stack([D, W])).to(DEV))
    ref = R.extract(D, W, 1.0, vox, (0.0, 0.0, 0.0))
    pts = vol.extract_points()
    assert pts["count"] == len(ref["edge"]) > 500
    R.compare_points(_points(pts), ref)
    path = tmp_path / "cloud.ply"
    assert vol.save_ply(str(path)) == pts["count"]
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    assert b"element vertex %d" % pts["count"] in head and len(body) == 24 * pts["count"]


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_arguments_raise_before_launch(binding, monkeypatch):
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    vol = torch.zeros(2, 8, 8, 8, device=DEV)
    d = [torch.ones(6, 8, device=DEV)]
    m = torch.zeros(1, 12)
    org = torch.zeros(3)

    def integ(volume=vol, depths=d, confs=(), mats=m, weighted=False):
        ops.tsdf_integrate_(volume, depths, list(confs), mats, 0.1, 1e-3, 0.0, weighted, 64.0)
    integ()                                                                           # the well-formed call passes
    for bad in (dict(volume=vol.double()), dict(volume=vol.cpu()), dict(volume=torch.zeros(2, 8, 8, 16, device=DEV)[..., ::2]),
                dict(depths=[], mats=torch.zeros(0, 12)), dict(volume=torch.zeros(2, 8, 8, 10, device=DEV)),
                dict(depths=d * 9, mats=torch.zeros(9, 12)), dict(confs=[torch.ones(6, 9, device=DEV)]), dict(confs=[torch.ones(6, 8)]),
                dict(depths=[torch.ones(6, 8, device=DEV).half()]), dict(mats=torch.zeros(1, 12, device=DEV)), dict(mats=torch.zeros(2, 12)),
                dict(weighted=True), dict(volume=torch.zeros(8, 8, 8, device=DEV))):
        with pytest.raises(RuntimeError):
            integ(**bad)
    for bad in (dict(volume=vol.cpu()), dict(volume=torch.zeros(2, 8, 8, 10, device=DEV)), dict(capacity=-1), dict(origin=torch.zeros(2)),
                dict(volume=vol.double())):
        kw = dict(dict(volume=vol, capacity=0, origin=org), **bad)
        with pytest.raises(RuntimeError):
            ops.tsdf_extract_points(kw["volume"], 0.1, kw["origin"], 1.0, kw["capacity"])
    torch.cuda.synchronize()
    assert float(vol.abs().sum()) >= 0


def test_t9_at_the_c_level():
    import ctypes
    from estdepth_amd import _native
    vol = torch.zeros(2, 8, 8, 8, device=DEV)
    depth = torch.ones(6, 8, device=DEV)
    d = _native.TsdfIntegrateDesc()
    d.Z = d.Y = d.X = 8
    d.H, d.W, d.T = 6, 8, 9
    d.trunc, d.w_max = 0.1, 64.0
    d.tsdf, d.weight = vol.data_ptr(), vol.data_ptr() + 4 * 512
    for t in range(8):
        d.depth[t] = depth.data_ptr()
    assert _native.lib().estd_tsdf_integrate(ctypes.byref(d), None) == -1
    d.T = 0
    assert _native.lib().estd_tsdf_integrate(ctypes.byref(d), None) == -1


def test_end_to_end_joint_stream():
    """JointStream(graph=True) over a short synthetic sequence, integrate_outputs per clip on the graph's static output buffers: the volume
    equals the reference integration of the same device depth maps, and a second identical run gives the same bits"""
    from estdepth_amd import DepthNetHybrid, synth
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    from estdepth_amd.streaming import JointStream
    torch.backends.cudnn.allow_tf32 = False
    H, W, n_frames, seq = 128, 160, 8, 5
    m = DepthNetHybrid(ndepths=64, depth_min=0.1, depth_max=10.0, resnet=18, IF_EST_transformer=True).eval()
    synth.fill_state_dict(m, seed=3, head_gain=1.0)
    m = m.to(DEV)
    imgs = synth.smooth_images(n_frames, H, W, seed=9)[0].to(DEV)
    poses = torch.from_numpy(np.stack([synth.camera_pose(v) for v in range(n_frames)])).float()
    K = torch.from_numpy(synth.intrinsics(H, W)).float()
    dims, vox, conf_min = (64, 64, 64), 0.08, 0.0
    origin = frustum_volume(poses[1], K, (H, W), 0.1, 5.0, dims, vox)
    volumes = []
    for run in range(2):
        stream = JointStream(m, seq_len=seq, graph=True)
        vol = TSDFVolume(dims, vox, origin, device=DEV)
        D0, W0 = np.zeros(dims, np.float32), np.zeros(dims, np.float32)
        for start in range(0, n_frames - seq + 1, stream.stride):
            sl = slice(start, start + seq)
            outputs, _, _ = stream.push_clip(imgs[sl], poses[sl].to(DEV), K.to(DEV))
            vol.integrate_outputs(outputs, poses[sl][None], K[None], conf_min=conf_min)
            if run == 0:
                depths = np.stack([outputs[("depth", t, 0)][0, 0].cpu().numpy() for t in range(seq - 2)])
                confs = np.stack([outputs[("fused_prob", t)][0, 0].cpu().numpy() for t in range(seq - 2)])
                case = dict(poses=poses[sl][1:seq - 1].double().numpy(), K=K.double().numpy(), origin=origin, voxel=vox)
                ref = R.integrate(D0, W0, _mats(case), depths, confs, trunc=vol.trunc, z_near=vol.z_near, conf_min=conf_min, w_max=vol.w_max)
                torch.cuda.synchronize()
                g = vol.volume.cpu().numpy()
                R.compare(g[0], g[1], ref, D_before=D0, W_before=W0)
                D0, W0 = g[0], g[1]
        assert vol.frames == 2 * (seq - 2)
        torch.cuda.synchronize()
        volumes.append(vol.volume.clone())
    assert volumes[0][1].max() > 0
    assert torch.equal(volumes[0].view(torch.int32), volumes[1].view(torch.int32))
