"""csrc/depth_consistency.hip on the device against the float64 reference of tests/consistency_ref.py: every case of consistency_ref.CASES under
both bindings through consistency.check_views, the 480 x 640 check against 4 sources, identical bits across calls, invalid and out-of-image
inputs, malformed arguments under both bindings, filter_window against per-frame check_views, the filter's job on corrupted maps and the
end-to-end path ConsistencyWindow -> TSDFVolume.integrate_filtered -> render.

Bar (consistency_ref.compare): ambiguous pixels <= 3 % of the valid target pixels; on all others views and visible are exact, invalid pixels
are exactly zero, and depth and rel_err are within C_CONS = 2 times their first-order bounds.  The filter: no corrupted pixel of the middle
frame kept at min_views = 2, at least 90 % of the uncorrupted pixels that have views >= 2 on the clean maps kept (the float64 reference: 0 of
945 and 96.3 %).  Geometry of the filtered volume: |depth - analytic| <= 0.1 voxel in the median and 0.5 voxel at the 95th percentile of the
hit pixels (the bars of test_gpu_tsdf_raycast.py).
Figures of the numpy-fp32 stand-in: largest depth error 0.23 of the unscaled bound, rel_err 0.25 (bar 2); ambiguous share 0.0002 - 0.0028.  The
figures of the device run (this file prints them per case, pytest -s): profiles/consistency_gpu_tests.txt."""
import numpy as np
import pytest
import torch

import consistency_ref as C
import tsdf_ref as R
from helpers import _binding

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("views", "visible", "depth", "rel_err")
_REFS = {}


def _tensors(c):
    return (torch.from_numpy(c["target"]).to(DEV), torch.from_numpy(c["pose_t"]), torch.from_numpy(c["K_t"]),
            torch.from_numpy(c["sources"]).to(DEV), torch.from_numpy(c["poses_s"]), torch.from_numpy(c["K_s"]))


def _check(c, **kw):
    from estdepth_amd import consistency
    d, P, K, src, Ps, Ks = _tensors(c)
    out = consistency.check_views(d, P, K, src, Ps, Ks, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _reference(name):
    """the float64 evaluation from the matrices the kernel receives (camera.consistency_matrices), once per case"""
    if name not in _REFS:
        from estdepth_amd import camera
        c = C.build_case(name)
        _, P, K, _, Ps, Ks = _tensors(c)
        mats = camera.consistency_matrices(P, K, Ps, Ks).numpy().reshape(-1, 2, 3, 4)
        assert np.abs(mats.astype(np.float64) - c["mats"]).max() <= 2.0 ** -22 * np.abs(c["mats"]).max()
        _REFS[name] = C.reference(name) if np.array_equal(mats, c["mats"]) else C.evaluate(c["target"], c["sources"], mats)
    return _REFS[name]


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_check_against_reference(name, binding, monkeypatch):
    _binding(monkeypatch, binding)
    fig = C.compare(_check(C.build_case(name)), _reference(name), "%s %s" % (name, binding))
    assert fig["valid"] > 500 and 0.5 < fig["consistent_share"] < 0.99


def test_full_size():
    """480 x 640 against 4 sources"""
    fig = C.compare(_check(C.build_case("full")), _reference("full"), "full")
    assert fig["valid"] > 300000
    _REFS.pop("full")


def test_calls_give_identical_bits():
    c = C.build_case("s8")
    a, b = _check(c), _check(c)
    for k in NAMES:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_invalid_target_and_source_looking_away():
    c = dict(C.build_case("s4"))
    for fill in (0.0, np.nan, np.inf, -1.0, C.Z_NEAR):
        got = _check(dict(c, target=np.full_like(c["target"], fill)))
        assert all((got[k] == 0).all() for k in NAMES), fill
    flip = np.diag([-1.0, 1.0, -1.0, 1.0])                          # half a turn about y: every source looks away from the scene
    got = _check(dict(c, poses_s=np.stack([P @ flip for P in c["poses_s"]])))
    valid = C.depth_valid(c["target"])
    assert all(np.isfinite(got[k]).all() for k in NAMES)
    assert (got["visible"] == 0).all() and (got["views"] == 0).all() and (got["rel_err"] == 0).all()
    assert np.array_equal(got["depth"], np.where(valid, c["target"], np.float32(0)))
    # sources without a single valid depth: the same
    got = _check(dict(c, sources=np.zeros_like(c["sources"])))
    assert (got["visible"] == 0).all() and np.array_equal(got["depth"], np.where(valid, c["target"], np.float32(0)))


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_arguments_raise_before_launch(binding, monkeypatch):
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    t = torch.full((6, 8), 2.0, device=DEV)
    eye = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]).reshape(12)
    mats = torch.stack([torch.stack([eye, eye])] * 2).contiguous()
    good = dict(target=t, sources=[t, t.clone()], mats=mats, px_max=1.0, rel_max=0.01, z_near=1e-3)

    def run(**kw):
        a = dict(good, **kw)
        return ops.depth_consistency(a["target"], a["sources"], a["mats"], a["px_max"], a["rel_max"], a["z_near"])
    nan_mats = mats.clone()
    nan_mats[1, 1, 3] = float("nan")
    for bad in (dict(target=t.double()), dict(target=t.cpu()), dict(target=torch.zeros(6, 16, device=DEV)[:, ::2]), dict(target=torch.zeros(2, 6, 8, device=DEV)),
                dict(target=torch.zeros(1, 8, device=DEV), sources=[torch.zeros(1, 8, device=DEV)] * 2),
                dict(sources=[]), dict(sources=[t] * 9, mats=torch.stack([torch.stack([eye, eye])] * 9).contiguous()), dict(sources=[t, t.cpu()]),
                dict(sources=[t, torch.zeros(6, 9, device=DEV)]), dict(sources=[t, t.double()]), dict(sources=[t]),
                dict(mats=mats.to(DEV)), dict(mats=mats[:1]), dict(mats=mats.double()), dict(mats=nan_mats),
                dict(px_max=0.0), dict(px_max=-1.0), dict(px_max=float("nan")), dict(px_max=float("inf")),
                dict(rel_max=0.0), dict(rel_max=float("nan")), dict(rel_max=float("inf")), dict(z_near=-1e-3), dict(z_near=float("nan"))):
        with pytest.raises(RuntimeError):
            run(**bad)
    views, visible, depth, rel_err = run()                           # a well-formed call still works: identity matrices, identical maps
    torch.cuda.synchronize()
    assert all(tuple(x.shape) == (6, 8) for x in (views, visible, depth, rel_err))
    assert bool((views == 2).all()) and bool((visible == 2).all()) and bool((depth == 2).all()) and bool((rel_err == 0).all())


def test_filter_window_equals_per_frame_checks():
    from estdepth_amd import consistency
    c = C.build_case("s4")
    depths, poses, K = torch.from_numpy(c["depths"]).to(DEV), torch.from_numpy(c["poses"]), torch.from_numpy(c["K_t"])
    out = consistency.filter_window(depths, poses, K, radius=2, min_views=2)
    T = depths.shape[0]
    assert tuple(out["depth"].shape) == tuple(depths.shape) and out["mask"].dtype == torch.bool
    for t in range(T):
        nb = C.window_sources(t, T, 2)
        one = consistency.check_views(depths[t], poses[t], K, depths[nb], poses[nb])
        for k in NAMES:
            assert torch.equal(out[k][t].view(torch.int32), one[k].view(torch.int32)), (t, k)
        assert torch.equal(out["mask"][t], one["views"] >= 2)


def test_filter_drops_outliers_and_keeps_the_rest():
    """5 noise-free frames, 5 % of each map's pixels off by a factor in [0.6, 0.85] u [1.2, 1.5]"""
    from estdepth_amd import consistency
    st = C.corrupted_stack(5, (120, 160))
    poses, K = torch.from_numpy(st["poses"]), torch.from_numpy(st["K"])
    got = consistency.filter_window(torch.from_numpy(st["depths"]).to(DEV), poses, K, radius=2, min_views=2)
    clean = consistency.filter_window(torch.from_numpy(st["clean"]).to(DEV), poses, K, radius=2, min_views=2)
    kept, bad = got["mask"][2].cpu().numpy(), st["bad"][2]
    base = ~bad & clean["mask"][2].cpu().numpy()
    retained = (kept & base).sum() / base.sum()
    print("depth_consistency filter: %d corrupted pixels of the middle frame, %d kept; %.4f of the %d clean consistent pixels retained"
          % (bad.sum(), (kept & bad).sum(), retained, base.sum()))
    assert bad.sum() > 800 and base.sum() > 10000
    assert not (kept & bad).any()
    assert retained >= 0.9


def test_end_to_end_filtered_fusion():
    """ConsistencyWindow -> integrate_filtered on the corrupted maps beside plain integrate of the same maps"""
    from estdepth_amd import camera, consistency, ops
    from estdepth_amd.fusion3d import TSDFVolume
    st = C.corrupted_stack(5, (120, 160))
    H, W = st["depths"].shape[1:]
    dims, origin, vox = (96, 128, 128), (-1.92, -1.92, 0.2), R.VOXEL
    depths, poses, K = torch.from_numpy(st["depths"]).to(DEV), torch.from_numpy(st["poses"]), torch.from_numpy(st["K"])
    filtered, plain, direct = (TSDFVolume(dims, vox, origin, device=DEV) for _ in range(3))
    win = consistency.ConsistencyWindow(radius=2, min_views=2)
    order = []
    for t in range(depths.shape[0]):
        rec = win.push(depths[t], poses[t], K)
        if rec is not None:
            order.append(rec["frame_index"])
            filtered.integrate_filtered(rec)
    for rec in win.flush():
        order.append(rec["frame_index"])
        filtered.integrate_filtered(rec)
    assert order == list(range(5)) and filtered.frames == 5
    s = win.summary()
    print("depth_consistency end to end: summary %s" % s)
    assert 0.5 < s["kept_share"] < 0.98 and 0.5 < s["consistent_share"] < 0.98
    # plain fusion is what it was: integrate == the operator called directly on the same inputs, bit for bit
    plain.integrate(depths, poses, K)
    mats = camera.tsdf_matrices(poses, K, direct.origin, vox)
    ops.tsdf_integrate_(direct.volume, [depths[t].contiguous() for t in range(5)], [], mats.contiguous(), direct.trunc, direct.z_near, 0.0, False, direct.w_max)
    torch.cuda.synchronize()
    assert torch.equal(plain.volume.view(torch.int32), direct.volume.view(torch.int32))
    # the outliers carved voxels the filtered run never touched
    assert plain.fused_voxels() > filtered.fused_voxels() > 0
    # the filtered volume at the middle pose against the analytic scene
    got = filtered.render(poses[2], K, (H, W), depth_min=0.3, depth_max=3.6)["depth"].cpu().numpy()
    ana = R.raycast_scene(st["poses"][2], st["K"], H, W)
    hit = (got > 0) & (ana > 0)
    err = np.abs(got.astype(np.float64) - ana)[hit] / vox
    med, p95 = float(np.median(err)), float(np.percentile(err, 95))
    raw = plain.render(poses[2], K, (H, W), depth_min=0.3, depth_max=3.6)["depth"].cpu().numpy()
    both = (raw > 0) & (ana > 0)
    err_raw = np.abs(raw.astype(np.float64) - ana)[both] / vox
    print("depth_consistency end to end: filtered volume %d voxels, %d hit pixels, |depth - analytic| median %.4f voxel, p95 %.4f voxel; plain volume %d "
          "voxels, %d hit pixels, median %.4f, p95 %.4f" % (filtered.fused_voxels(), hit.sum(), med, p95, plain.fused_voxels(), both.sum(),
                                                        float(np.median(err_raw)), float(np.percentile(err_raw, 95))))
    assert hit.sum() > 10000
    assert med <= 0.1 and p95 <= 0.5
    # with a network confidence the views mask the depth and the confidence gates as in integrate
    gated = TSDFVolume(dims, vox, origin, device=DEV)
    conf = torch.full((H, W), 0.5, device=DEV)
    rec = dict(consistency.check_views(depths[2], poses[2], K, depths[[0, 1, 3, 4]], poses[[0, 1, 3, 4]]), pose=poses[2], K=K, conf=conf)
    gated.integrate_filtered(rec, min_views=2, conf_min=0.6)
    assert gated.fused_voxels() == 0
    gated.integrate_filtered(rec, min_views=2, conf_min=0.4)
    same = TSDFVolume(dims, vox, origin, device=DEV)
    same.integrate_filtered(dict(rec, conf=None), min_views=2)
    assert gated.fused_voxels() > 0 and torch.equal(gated.volume.view(torch.int32), same.volume.view(torch.int32))
