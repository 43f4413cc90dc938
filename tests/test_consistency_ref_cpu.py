"""CPU-only checks of the cross-view consistency reference (tests/consistency_ref.py) and of everything in the feature that needs no device:
the ambiguous share and the numpy-fp32 stand-in of every case of the GPU suite, closed forms, the silhouette and occlusion behaviour, wrong
kernels that the comparison rejects, camera.consistency_matrices, the host layer's argument checks, ConsistencyWindow with the kernel call
replaced by the reference, the ESTD_ERR_* returns of estd_depth_consistency and the descriptor's layout against gcc."""
import ctypes
import math

import numpy as np
import pytest
import torch

import consistency_ref as C
import tsdf_ref as R
from helpers import check_desc_layout


def _dilate(mask, r):
    for _ in range(r):
        mask = C._window3(mask, np.any, False)
    return mask


# ------------------------------------------------------------------------------------------------------------ the cases of the GPU suite
@pytest.mark.parametrize("name", list(C.CASES) + ["full"])
def test_ambiguous_share_and_fp32_evaluation(name):
    """the share of ambiguous pixels stays under the cap, both outcomes occur, and the numpy-fp32 evaluation passes THE comparison"""
    c, ref = C.build_case(name), C.reference(name)
    got = C.evaluate(c["target"], c["sources"], c["mats"], dtype=np.float32)
    fig = C.compare(got, ref, name + " numpy-fp32")
    S = c["sources"].shape[0]
    seen = ref["visible"][ref["valid"]] > 0
    assert fig["valid"] > 0.8 * c["target"].size * (0.75 if name == "s4" else 1.0)
    assert 0.5 < fig["consistent_share"] < 0.99, "the noise must produce both outcomes"
    assert (ref["views"][ref["valid"]][seen] == 0).any() and (ref["views"] == S).any()
    if name == "s4":                                                 # the holes: invalid in the target, and skipped taps in the sources
        assert not ref["valid"][10:30, 20:60].any() and not ref["valid"][50:70, 80:120].any()
        assert not ref["valid"][90:110, 30:70].any() and not ref["valid"][40:45, 5:15].any()
        assert (ref["visible"][ref["valid"]] < S).mean() > 0.1
    if name == "kdiff":
        assert not np.array_equal(c["K_s"][0], c["K_t"]) and not np.array_equal(c["K_s"][0], c["K_s"][1])


# ------------------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("S", C.ROUTE_SOURCES)
@pytest.mark.parametrize("hw", C.ROUTE_SIZES)
def test_route_cases_ambiguous_share_and_fp32_evaluation(hw, S):
    """the small maps of tests/test_gpu_recon3d_routes.py (the edges of the 16 x 16 tiles, 1 and 8 sources): the same two properties"""
    import test_gpu_recon3d_routes as G
    assert (hw in G.CONS_SIZES) and len(G.CONS_SIZES) == 4
    c = C.make_case(hw, S, seed=S + hw[0], name="route")
    ref = C.evaluate(c["target"], c["sources"], c["mats"])
    fig = C.compare(C.evaluate(c["target"], c["sources"], c["mats"], dtype=np.float32), ref, "route %dx%d S%d" % (hw + (S,)))
    assert fig["amb_share"] <= C.AMB_CAP and fig["valid"] >= 4


def test_identical_pose_and_maps():
    """a source at the target's own pose with the target's own map: the round trip ends where it started"""
    H, W, S = 60, 80, 3
    P, K = R.scene_poses(3, seed=4)[1], R.intrinsics(H, W)
    d = C.noisy(R.raycast_scene(P, K, H, W), np.random.RandomState(0))
    mats = C.matrices64(P, K, np.stack([P] * S), K)
    for dtype in (np.float64, np.float32):
        out = C.evaluate(d, np.stack([d] * S), mats, dtype=dtype)
        inner = np.zeros((H, W), bool)
        inner[1:-1, 1:-1] = True
        assert out["valid"].all()
        assert (out["views"][inner] == S).all() and (out["visible"][inner] == S).all()
        assert np.abs(out["depth"].astype(np.float64) - d)[inner].max() <= 1e-5 * d.max()
        assert out["rel_err"][inner].max() <= 1e-5


def test_scaled_source_agrees_nowhere():
    """plane only (sphere radius 0): a source whose depths are 5 % off is seen everywhere it was seen before and agrees nowhere"""
    H, W = 60, 80
    poses, K = R.scene_poses(3, seed=5), R.intrinsics(H, W)
    maps = np.stack([R.raycast_scene(P, K, H, W, radius=0.0) for P in poses]).astype(np.float32)
    assert np.allclose(maps, maps[0], rtol=0.05) and (maps > 0).all()
    mats = C.matrices64(poses[1], K, poses[[0]], K)
    good = C.evaluate(maps[1], maps[[0]], mats)
    off = C.evaluate(maps[1], (maps[[0]].astype(np.float64) * 1.05).astype(np.float32), mats)
    assert (good["views"] == good["visible"]).all() and good["visible"].sum() > 0.9 * H * W
    assert (off["views"] == 0).all()
    assert np.array_equal(off["visible"], good["visible"])
    assert np.array_equal(off["depth"], maps[1].astype(np.float64)) and (off["rel_err"] == 0).all()


def test_noise_free_scene_is_consistent_off_the_silhouette():
    """without noise every source that sees a pixel agrees with it, except in the band beside the sphere's silhouette where a neighbour
    sees the other surface: at most f b (1 / z_sphere - 1 / z_plane) pixels wide, plus the bilinear footprint"""
    hw, S = (60, 80), 2
    c = C.make_case(hw, S, noise=0.0, seed=2)
    ref = C.evaluate(c["target"], c["sources"], c["mats"])
    t = c["target"].astype(np.float64)
    sil = (C._window3(t, np.max, -np.inf) - C._window3(t, np.min, np.inf)) > 0.05
    base = max(np.linalg.norm(P[:3, 3] - c["pose_t"][:3, 3]) for P in c["poses_s"])
    band = int(math.ceil(c["K_t"][0, 0] * base * (1 / 1.45 - 1 / 2.6))) + 2
    off = ~_dilate(sil, band)
    assert sil.sum() > 100 and off.sum() > 0.4 * t.size
    assert (ref["views"][off] == ref["visible"][off]).all()
    assert (ref["views"] != ref["visible"]).any(), "the band beside the silhouette holds the pixels a neighbour sees differently"


def test_occluded_pixels_are_visible_but_not_consistent():
    """a source far to the side: the plane pixels whose line of sight from that source passes through the sphere are visible (the source
    has a depth there: the sphere's) and not consistent; plane pixels whose line of sight clears the sphere agree"""
    H, W = 120, 160
    K = R.intrinsics(H, W)
    Pt, Ps = R.look_at((0, 0, 0), (0.1, 0.05, 2.2)), R.look_at((1.0, 0, 0), (0.1, 0.05, 2.2))
    dt, dsrc = (R.raycast_scene(P, K, H, W).astype(np.float32) for P in (Pt, Ps))
    ref = C.evaluate(dt, dsrc[None], C.matrices64(Pt, K, Ps[None], K))
    X = R_backproject(dt, Pt, K)
    on_plane = np.abs(X[..., 2] - 2.6) < 1e-4
    eye, centre, radius = Ps[:3, 3], np.array([0.1, 0.05, 2.0]), 0.55
    ray = X - eye
    length = np.linalg.norm(ray, axis=-1)
    ray = ray / length[..., None]
    along = np.clip(((centre - eye) * ray).sum(-1), 0, length)
    dist = np.linalg.norm(eye + ray * along[..., None] - centre, axis=-1)
    occluded, free = on_plane & (dist < 0.9 * radius), on_plane & (dist > 1.1 * radius)
    assert occluded.sum() > 1000 and free.sum() > 5000
    assert (ref["visible"][occluded] == 1).all() and (ref["views"][occluded] == 0).all()
    seen = free & (ref["visible"] == 1)
    assert seen.sum() > 5000 and (ref["views"][seen] == 1).all()
    assert np.array_equal(ref["depth"][occluded], dt.astype(np.float64)[occluded]), "nothing agrees: the target's own depth"


def R_backproject(depth, pose, K):
    H, W = depth.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T
    return (rays * depth.astype(np.float64)[..., None]) @ pose[:3, :3].T + pose[:3, 3]


# ------------------------------------------------------------------------------------------------------------ the comparison itself
def test_comparison_rejects_a_wrong_kernel():
    """nearest-neighbour sampling instead of the bilinear blend, F and B exchanged, and >= where the contract has > in the validity of a
    depth (target pixels and taps that are exactly z_near: exact comparisons, so no ambiguity shields them)"""
    c, ref = C.build_case("s2"), C.reference("s2")
    for variant in ("nearest", "swap"):
        with pytest.raises(AssertionError):
            C.compare(C.evaluate(c["target"], c["sources"], c["mats"], dtype=np.float32, variant=variant), ref, "s2 " + variant)
    target, sources = c["target"].copy(), c["sources"].copy()
    target[20:24, 30:40] = np.float32(C.Z_NEAR)
    sources[:, 40:44, 30:40] = np.float32(C.Z_NEAR)
    ref = C.evaluate(target, sources, c["mats"])
    assert not ref["valid"][20:24, 30:40].any()
    C.compare(C.evaluate(target, sources, c["mats"], dtype=np.float32), ref, "s2 with depths at z_near")
    with pytest.raises(AssertionError):
        C.compare(C.evaluate(target, sources, c["mats"], dtype=np.float32, variant="ge"), ref, "s2 ge")
    # a result that is right except for the average of one pixel
    got = {k: np.asarray(v, np.float32).copy() for k, v in C.evaluate(c["target"], c["sources"], c["mats"], dtype=np.float32).items() if k in ("views", "visible", "depth", "rel_err")}
    y, x = np.argwhere(C.reference("s2")["valid"] & ~C.reference("s2")["amb"] & (C.reference("s2")["views"] == 2))[0]
    got["depth"][y, x] *= np.float32(1 + 1e-5)
    with pytest.raises(AssertionError):
        C.compare(got, C.reference("s2"), "s2 one pixel off")


# ------------------------------------------------------------------------------------------------------------ matrices
def test_consistency_matrices_match_the_reference_and_invert_each_other():
    from estdepth_amd import camera
    for name in ("s8", "kdiff"):
        c = C.build_case(name)
        M = camera.consistency_matrices(torch.from_numpy(c["pose_t"]), torch.from_numpy(c["K_t"]), torch.from_numpy(c["poses_s"]), torch.from_numpy(c["K_s"]))
        assert M.dtype == torch.float32 and tuple(M.shape) == (c["sources"].shape[0], 2, 12) and not M.is_cuda
        M = M.numpy().reshape(-1, 2, 3, 4)
        assert np.abs(M.astype(np.float64) - c["mats"]).max() <= 2.0 ** -22 * np.abs(c["mats"]).max()
        rng = np.random.RandomState(1)
        for s in range(M.shape[0]):
            F, B = M[s, 0].astype(np.float64), M[s, 1].astype(np.float64)
            u, v, d = rng.uniform(0, 150, 50), rng.uniform(0, 110, 50), rng.uniform(0.5, 4.0, 50)
            p = F[:, :3] @ (np.stack([u, v, np.ones(50)]) * d) + F[:, 3:]
            q = B[:, :3] @ (np.stack([p[0] / p[2], p[1] / p[2], np.ones(50)]) * p[2]) + B[:, 3:]
            np.testing.assert_allclose(np.stack([q[0] / q[2], q[1] / q[2], q[2]]), np.stack([u, v, d]), rtol=0, atol=2e-3)
    one = camera.consistency_matrices(torch.from_numpy(c["pose_t"]), torch.from_numpy(c["K_t"]), torch.from_numpy(c["poses_s"]), torch.from_numpy(c["K_s"][0]))
    assert tuple(one.shape) == (2, 2, 12) and torch.equal(one[0], torch.from_numpy(M[0].reshape(2, 12)))
    with pytest.raises(RuntimeError, match="K_s"):
        camera.consistency_matrices(torch.eye(4), torch.eye(3), torch.eye(4).repeat(3, 1, 1), torch.eye(3).repeat(2, 1, 1))


# ------------------------------------------------------------------------------------------------------------ host layer without a device
def _fake_kernel(calls=None):
    """ops.depth_consistency with the numpy-fp32 reference behind it (CPU tensors in and out)"""
    def run(target, sources, mats, px_max, rel_max, z_near):
        if calls is not None:
            calls.append(len(sources))
        out = C.evaluate(target.numpy(), np.stack([s.numpy() for s in sources]), mats.numpy().reshape(-1, 2, 3, 4), px_max, rel_max, z_near, dtype=np.float32)
        return tuple(torch.from_numpy(np.ascontiguousarray(out[k], dtype=np.float32)) for k in ("views", "visible", "depth", "rel_err"))
    return run


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_ops_argument_checks_without_device(binding, monkeypatch):
    from estdepth_amd import ops
    ops.T()
    monkeypatch.setattr(ops, "BINDING", binding)
    t, mats = torch.ones(6, 8), torch.zeros(2, 2, 12)
    with pytest.raises(RuntimeError):                               # CPU tensors: there is no CPU path
        ops.depth_consistency(t, [t, t], mats, 1.0, 0.01, 1e-3)
    if binding == "ctypes":
        with pytest.raises(RuntimeError, match="ROCm device"):
            ops.depth_consistency(t, [t, t], mats, 1.0, 0.01, 1e-3)
        with pytest.raises(RuntimeError, match="must be a tensor"):
            ops.depth_consistency(None, [t], mats, 1.0, 0.01, 1e-3)


def test_check_views_and_filter_window_argument_checks(monkeypatch):
    from estdepth_amd import consistency, ops
    monkeypatch.setattr(ops, "depth_consistency", _fake_kernel())
    c = C.build_case("tiny")
    d, P, K = torch.from_numpy(c["target"]), torch.from_numpy(c["pose_t"]), torch.from_numpy(c["K_t"])
    src, Ps = torch.from_numpy(c["sources"]), torch.from_numpy(c["poses_s"])
    out = consistency.check_views(d, P, K, src, Ps)
    assert sorted(out) == ["depth", "rel_err", "views", "visible"] and all(tuple(v.shape) == tuple(d.shape) for v in out.values())
    C.compare({k: v.numpy() for k, v in out.items()}, C.reference("tiny"), "tiny through check_views")
    for bad, msg in ((dict(src_depths=src[:0], src_poses=Ps[:0]), "sources"), (dict(src_depths=torch.cat([src, src[:1]]), src_poses=torch.cat([Ps, Ps[:1]])), "sources"),
                     (dict(src_depths=src[:, :-1]), "source 0"), (dict(src_poses=Ps[:3]), "src_poses"), (dict(pose=P[:3]), "pose"), (dict(K=K[:2]), "pose"),
                     (dict(src_K=torch.eye(3).repeat(3, 1, 1)), "src_K"), (dict(px_max=0.0), "px_max"), (dict(px_max=float("nan")), "px_max"),
                     (dict(rel_max=-1.0), "rel_max"), (dict(rel_max=float("inf")), "rel_max"), (dict(z_near=-1e-3), "z_near"),
                     (dict(depth=torch.ones(4)), "depth"), (dict(pose=P * float("nan")), "not finite")):
        a = dict(dict(depth=d, pose=P, K=K, src_depths=src, src_poses=Ps), **bad)
        with pytest.raises(RuntimeError, match=msg):
            consistency.check_views(**a)
    stack, poses = torch.from_numpy(c["depths"]), torch.from_numpy(c["poses"])
    for bad, msg in ((dict(depths=stack[0]), "depths"), (dict(depths=stack[:1], poses=poses[:1]), "two frames"), (dict(poses=poses[:-1]), "poses"),
                     (dict(K=torch.eye(3).repeat(2, 1, 1)), "K must"), (dict(radius=0), "radius"), (dict(min_views=0), "min_views"),
                     (dict(px_max=-1.0), "px_max")):
        a = dict(dict(depths=stack, poses=poses, K=K), **bad)
        with pytest.raises(RuntimeError, match=msg):
            consistency.filter_window(**a)
    for bad in (dict(radius=0), dict(radius=5), dict(min_views=0), dict(rel_max=0.0)):
        with pytest.raises(RuntimeError):
            consistency.ConsistencyWindow(**bad)


def test_neighbours():
    from estdepth_amd import consistency
    assert consistency.neighbours(0, 6, 2) == [1, 2] and consistency.neighbours(3, 6, 2) == [1, 2, 4, 5] and consistency.neighbours(5, 6, 2) == [3, 4]
    assert consistency.neighbours(6, 13, 6) == [2, 3, 4, 5, 7, 8, 9, 10], "capped at 8, the nearest first"
    assert consistency.neighbours(3, 6, 2) == C.window_sources(3, 6, 2)


def test_consistency_window_order_latency_flush_and_summary(monkeypatch):
    """the kernel call replaced by the reference: frames come back in order, ``radius`` pushes late, checked against the right neighbours;
    flush() hands out the rest; the record carries what the caller gave; summary() equals the totals computed by hand; filter_window
    gives the same maps"""
    from estdepth_amd import consistency, ops
    calls = []
    monkeypatch.setattr(ops, "depth_consistency", _fake_kernel(calls))
    T, radius, min_views = 6, 2, 2
    c = C.make_case((24, 32), T - 1, seed=6)
    depths, poses, K = c["depths"], c["poses"], c["K_t"]
    win = consistency.ConsistencyWindow(radius=radius, min_views=min_views)
    records = []
    for t in range(T):
        pushed = torch.from_numpy(depths[t].copy())
        rec = win.push(pushed, torch.from_numpy(poses[t]), torch.from_numpy(K), conf=("conf", t), extra=("frame", t))
        pushed.fill_(123.0)                                          # the caller's buffer is overwritten by the next forward: the window cloned it
        assert (rec is None) == (t < radius), t
        if rec is not None:
            assert rec["frame_index"] == t - radius
            records.append(rec)
    assert win.summary()["frames"] == T - radius
    records += list(win.flush())
    assert list(win.flush()) == [] and win.frames == []
    assert [r["frame_index"] for r in records] == list(range(T))
    assert calls == [2, 3, 4, 4, 3, 2]
    tot = dict(valid=0, views=0.0, visible=0.0, agree=0, rel=0.0, kept=0)
    for t, rec in enumerate(records):
        nb = C.window_sources(t, T, radius)
        want = C.evaluate(depths[t], depths[nb], C.matrices64(poses[t], K, poses[nb], K), dtype=np.float32)
        for k in ("views", "visible", "depth", "rel_err"):
            assert np.array_equal(rec[k].numpy(), want[k]), (t, k)
        assert rec["conf"] == ("conf", t) and rec["extra"] == ("frame", t) and rec["min_views"] == min_views
        assert np.array_equal(rec["pose"].numpy(), poses[t]) and np.array_equal(rec["K"].numpy(), K)
        tot["valid"] += int(want["valid"].sum())
        tot["views"] += float(want["views"].sum())
        tot["visible"] += float(want["visible"].sum())
        tot["agree"] += int((want["views"] > 0).sum())
        tot["rel"] += float(want["rel_err"].astype(np.float64).sum())
        tot["kept"] += int((want["views"] >= min_views).sum())
    s = win.summary()
    assert s["frames"] == T and s["valid_pixels"] == tot["valid"]
    assert s["consistent_share"] == pytest.approx(tot["views"] / tot["visible"], rel=1e-12)
    assert s["rel_err"] == pytest.approx(tot["rel"] / tot["agree"], rel=1e-9)
    assert s["kept_share"] == pytest.approx(tot["kept"] / tot["valid"], rel=1e-12)
    assert 0 < s["kept_share"] < 1 and 0 < s["consistent_share"] < 1
    out = consistency.filter_window(torch.from_numpy(depths), torch.from_numpy(poses), torch.from_numpy(K), radius=radius, min_views=min_views)
    assert tuple(out["depth"].shape) == depths.shape and out["mask"].dtype == torch.bool
    for t, rec in enumerate(records):
        for k in ("views", "visible", "depth", "rel_err"):
            assert torch.equal(out[k][t], rec[k]), (t, k)
        assert torch.equal(out["mask"][t], rec["views"] >= min_views)
    # a stream of one frame has nothing to check against: it comes back unfiltered, with no view
    lone = consistency.ConsistencyWindow(radius=1)
    assert lone.push(torch.from_numpy(depths[0]), torch.from_numpy(poses[0]), torch.from_numpy(K)) is None
    (rec,) = list(lone.flush())
    assert float(rec["views"].sum()) == 0 and np.array_equal(rec["depth"].numpy(), np.where(C.depth_valid(depths[0]), depths[0], 0))


# ------------------------------------------------------------------------------------------------------------ the entry point
def _desc(**kw):
    from estdepth_amd import _native
    d = _native.DepthConsistencyDesc()
    d.H, d.W, d.S = 6, 8, 2
    d.px_max, d.rel_max, d.z_near = 1.0, 0.01, 1e-3
    d.target = d.views = d.visible = d.depth = d.rel_err = 0x1000   # never dereferenced: every descriptor below fails validation
    for s in range(8):
        d.source[s] = 0x1000
    for k, v in kw.items():
        if k == "mat":
            d.mats[v[0]][v[1]][v[2]] = v[3]
        elif k == "source":
            d.source[v] = None
        else:
            setattr(d, k, v)
    return d


def test_entry_point_validates_without_gpu():
    """every malformed descriptor: ESTD_ERR_ARG (-1) before any launch; beyond the launch grid: ESTD_ERR_UNSUPPORTED (-3)"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    assert lib.estd_depth_consistency(None, None) == -1
    assert lib.estd_depth_consistency(ctypes.byref(_native.DepthConsistencyDesc()), None) == -1
    for bad in (dict(target=None), dict(views=None), dict(visible=None), dict(depth=None), dict(rel_err=None), dict(source=0), dict(source=1),
                dict(S=0), dict(S=9), dict(S=-1), dict(H=0), dict(W=0), dict(H=-4), dict(H=1), dict(W=1),
                dict(px_max=0.0), dict(px_max=-1.0), dict(px_max=float("nan")), dict(px_max=float("inf")), dict(px_max=1e30), dict(px_max=1e-30),
                dict(rel_max=0.0), dict(rel_max=-0.01), dict(rel_max=float("nan")), dict(rel_max=float("inf")),
                dict(z_near=-1e-3), dict(z_near=float("nan")), dict(z_near=float("inf")),
                dict(mat=(1, 0, 5, float("nan"))), dict(mat=(0, 1, 11, float("inf")))):
        assert lib.estd_depth_consistency(ctypes.byref(_desc(**bad)), None) == -1, bad
    assert lib.estd_depth_consistency(ctypes.byref(_desc(H=65536, W=32768)), None) == -3
    # what lies beyond S is not looked at
    assert lib.estd_depth_consistency(ctypes.byref(_desc(H=65536, W=32768, source=5, mat=(7, 1, 0, float("nan")))), None) == -3


def test_desc_struct_layout(tmp_path):
    """sizeof / offsetof of estd_depth_consistency_desc as the C compiler sees it == the ctypes mirror"""
    from estdepth_amd import _native, ops
    out = check_desc_layout(tmp_path, "estd_depth_consistency_desc", _native.DepthConsistencyDesc, macros=["ESTD_CONSISTENCY_MAX_SOURCES"])
    assert out[-1] == ops.CONSISTENCY_MAX_SOURCES == 8
