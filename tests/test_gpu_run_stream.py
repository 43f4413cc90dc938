"""tools/run_stream.py end to end on the device, driven in-process through run(parse([...])) with --depth-source gt on the analytic
three-body scene of tests/run_stream_ref.py (10 frames at 640 x 480, 8 targets, a 96 x 128 x 128 volume at 3 cm): which frame is the target and
which pose goes with it, the intrinsics at another --image-size, fusion behind the consistency window and its flush, tracking from the second
fused target on, the second volume of --score-3d, the renders of --render-fused -- and, with the real network on a small configuration, that
no flag changes what another one writes.

Bars.  The fused volume against tsdf_ref.integrate of the very maps, poses and intrinsics the tool was fed (tsdf_ref.compare: C_INTEGRATE,
AMB_CAP); bit-identity where two paths must compute the same thing (a second run, --score-3d's two volumes at the native size, the
filtered volume against one built from the library by hand, the fused depth maps against the test's own render); MARGIN = 1.25, the
project's semantic bar, ALWAYS on the float64 chain evaluated on the same inputs: the distance of the device's cloud to the analytic
surface (median, 95th percentile) <= MARGIN x the float64 chain's; orderings (filtered below unfiltered, tracked below untracked) as strict
inequalities -- tests/test_run_stream_cpu.py shows each holds by a factor of 2 in the fp32 stand-ins.  The figures of a device run (this
file prints them, pytest -s): profiles/run_stream_gpu_tests.txt -- largest |D - D_ref| / (2^-24 A) 0.95 at the native and 1.12 at half size (bar 5),
ambiguous shares 0.0217 and 0.0108 (cap 0.03); device / float64 distances 1.000 (cap 1.25); filtered / unfiltered p95 0.037; tracked /
untracked median 0.11 and p95 0.41, on the filtered records 0.13 and 0.45; every drifted frame from 9.85 mm / 0.50 degrees to at most
1.1 mm (4.5 mm on the first filtered record after the drift sets in); 9 tests in 14 s."""
import os
import shutil
import time

import numpy as np
import pytest
import torch

import cloud_metrics_ref as C
import run_stream_ref as S
import track_ref as T
import tsdf_raycast_ref as RC
import tsdf_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOOL = S.load_tool()
MARGIN = S.MARGIN
HW = (S.IMAGE_SIZE[1], S.IMAGE_SIZE[0])
TARGETS = S.targets_of(S.N_FRAMES)
SEED = 5


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.time()
    yield
    print("RUN-STREAM time %s %.1f s" % (request.node.name, time.time() - t0))


def _run(scene_dir, out, *flags, size=S.IMAGE_SIZE):
    """one run of the tool on a stored scene -> (report, state)"""
    argv = ["--scene-dir", str(scene_dir), "--frame-interval", "1", "--out", str(out), "--depth-source", "gt",
            "--image-size", str(size[0]), str(size[1])] + S.VOLUME_ARGS + [str(f) for f in flags]
    report, state = TOOL.run(TOOL.parse(argv))
    torch.cuda.synchronize()
    return report, state


def _volume(state):
    v = state.volume.volume.cpu().numpy()
    return v[0], v[1]


def _cloud(path):
    from estdepth_amd.fusion3d import read_ply
    return read_ply(str(path))["xyz"]


def _stem(name):
    return os.path.splitext(os.path.basename(str(name)))[0]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ scenes and shared runs
@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_clean")
    sc = S.write_scene(d, S.N_FRAMES, seed=SEED)
    return dict(dir=d, scene=sc, read=S.read_back(d))


@pytest.fixture(scope="module")
def corrupted(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_corrupt")
    sc = S.write_scene(d, S.N_FRAMES, corrupt=0.05, seed=SEED)
    return dict(dir=d, scene=sc, read=S.read_back(d))


@pytest.fixture(scope="module")
def drifted(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_drift")
    sc = S.write_scene(d, S.N_FRAMES, drift_from=4, seed=SEED)
    return dict(dir=d, scene=sc, read=S.read_back(d))


@pytest.fixture(scope="module")
def native_ref(clean):
    """the float64 chain at the native size, on what the tool is fed: computed once, shared, left unchanged"""
    rb = clean["read"]
    origin = S.volume_origin(rb["poses"][0], rb["K"], HW)
    ref, pts = S.fuse64(rb["depths"][TARGETS], rb["poses"][TARGETS], rb["K"], origin)
    return dict(origin=origin, ref=ref, pts=pts, dist=S.distance_figures(pts["xyz"]))


@pytest.fixture(scope="module")
def native_run(clean, tmp_path_factory):
    """--fuse at the native size: (report, state, out directory, PLY path, volume D, volume W)"""
    out = tmp_path_factory.mktemp("native")
    report, state = _run(clean["dir"], out, "--fuse", out / "scene.ply")
    D, W = _volume(state)
    return dict(report=report, state=state, out=out, ply=out / "scene.ply", D=D, W=W)


# ------------------------------------------------------------------------------------------------------------ 1. fusion, native size
def test_fusion_at_the_native_size(clean, native_ref, native_run, tmp_path):
    rb, report, state = clean["read"], native_run["report"], native_run["state"]
    assert report["frames"] == S.N_FRAMES and report["windows"] == len(TARGETS) and report["predictions_resized_to_gt_grid"] == 0
    assert tuple(state.volume.origin.tolist()) == native_ref["origin"] and state.volume.frames == len(TARGETS)
    assert state.volume_gt is None and state.geo is None
    # which frame was fused with which pose
    assert [_stem(n) for n, _ in state.fused] == [_stem(rb["names"][t]) for t in TARGETS]
    for (_, pose), t in zip(state.fused, TARGETS):
        assert np.array_equal(pose.numpy(), rb["poses"][t].astype(np.float64))
    Z0 = np.zeros(S.DIMS, np.float32)
    fig = R.compare(native_run["D"], native_run["W"], native_ref["ref"], D_before=Z0, W_before=Z0)
    print("RUN-STREAM fusion native: updated %d ambiguous share %.4f (cap %.2f) max |dD| / bound %.3f (bar %.1f)"
          % (fig["updated"], fig["amb_share"], R.AMB_CAP, fig["max_ratio"], R.C_INTEGRATE))
    assert fig["updated"] > 200000
    # the dumps are the targets' own maps, in the stream's layout; the depth errors against the ground truth vanish
    for t in TARGETS:
        d = np.load(native_run["out"] / "refined_depth" / (_stem(rb["names"][t]) + ".npy"))
        assert d.dtype == np.float16 and d.shape == (1,) + HW and np.array_equal(d[0], np.float16(rb["depths"][t]))
        p = np.load(native_run["out"] / "refined_prob" / (_stem(rb["names"][t]) + ".npy"))
        assert p.shape == HW and (p == 1).all()
    assert report["errors"]["l1"] == 0 and report["errors"]["rmse"] == 0 and report["errors"]["ratio_threshold_1.25"] == 1
    # the cloud
    xyz = _cloud(native_run["ply"])
    own = R.extract(native_run["D"], native_run["W"], 1.0, S.VOXEL, native_ref["origin"])      # the crossings of the device's own volume
    assert xyz.shape[0] == report["points"] == len(own["edge"])
    med, p95 = S.distance_figures(xyz)
    med64, p9564 = native_ref["dist"]
    print("RUN-STREAM fusion native: %d points, distance to the analytic surface in voxels: device median %.4f p95 %.4f, float64 chain median %.4f "
          "p95 %.4f, device / float64 %.3f %.3f (cap %.2f)" % (xyz.shape[0], med, p95, med64, p9564, med / med64, p95 / p9564, MARGIN))
    assert med <= MARGIN * med64 and p95 <= MARGIN * p9564
    # a second run gives the same bytes
    report2, _ = _run(clean["dir"], tmp_path, "--fuse", tmp_path / "scene.ply")
    assert (tmp_path / "scene.ply").read_bytes() == native_run["ply"].read_bytes() and report2["points"] == report["points"]
    assert report2["fused_voxels"] == report["fused_voxels"] == int((native_run["W"] > 0).sum())


# ------------------------------------------------------------------------------------------------------------ 2. half size
def test_fusion_at_half_size(clean, native_ref, native_run, tmp_path):
    """--image-size 320 240: the maps and intrinsics the tool used are the nearest-neighbour maps at 240 x 320 and scaled_intrinsics((320, 240));
    the reference project's principal-point scaling (a quarter pixel off the pixel-centre convention) is common to both sides"""
    size, hw = (320, 240), (240, 320)
    rb = clean["read"]
    K = S.reader_intrinsics(size).astype(np.float32)
    report, state = _run(clean["dir"], tmp_path, "--fuse", tmp_path / "scene.ply", size=size)
    assert report["predictions_resized_to_gt_grid"] == len(TARGETS) and report["windows"] == len(TARGETS)
    origin = S.volume_origin(rb["poses"][0], K, hw)
    assert tuple(state.volume.origin.tolist()) == origin
    maps = S.resample(rb["depths"][TARGETS], hw)
    d = np.load(tmp_path / "refined_depth" / (_stem(rb["names"][TARGETS[0]]) + ".npy"))
    assert d.shape == (1,) + hw and np.array_equal(d[0], np.float16(maps[0]))
    ref, pts = S.fuse64(maps, rb["poses"][TARGETS], K, origin)
    D, W = _volume(state)
    Z0 = np.zeros(S.DIMS, np.float32)
    fig = R.compare(D, W, ref, D_before=Z0, W_before=Z0)
    xyz = _cloud(tmp_path / "scene.ply")
    assert xyz.shape[0] == report["points"] == len(R.extract(D, W, 1.0, S.VOXEL, origin)["edge"])
    med, p95 = S.distance_figures(xyz)
    med64, p9564 = S.distance_figures(pts["xyz"])
    print("RUN-STREAM fusion half size: updated %d ambiguous share %.4f (cap %.2f) max |dD| / bound %.3f (bar %.1f); %d points, distance in voxels: "
          "device median %.4f p95 %.4f, float64 chain median %.4f p95 %.4f, device / float64 %.3f %.3f (cap %.2f); the native run: median %.4f p95 %.4f"
          % ((fig["updated"], fig["amb_share"], R.AMB_CAP, fig["max_ratio"], R.C_INTEGRATE, xyz.shape[0], med, p95, med64, p9564, med / med64,
              p95 / p9564, MARGIN) + S.distance_figures(_cloud(native_run["ply"]))))
    assert fig["updated"] > 200000
    assert med <= MARGIN * med64 and p95 <= MARGIN * p9564
    # the prediction on the ground truth's grid: every pixel is some pixel of the half-size map, off by at most the scene's slope
    assert 0 < report["errors"]["l1"] < 0.02 and report["errors"]["ratio_threshold_1.25"] > 0.99


# ------------------------------------------------------------------------------------------------------------ 3. --score-3d
def test_score_3d(clean, native_run, tmp_path):
    zero = ("accuracy", "completeness", "chamfer")
    one = ("precision", "recall", "fscore")
    # native size: the predicted and the ground-truth volume see the same samples
    report, state = _run(clean["dir"], tmp_path / "a", "--fuse", tmp_path / "a.ply", "--score-3d")
    assert state.volume_gt is not None and state.volume_gt.frames == len(TARGETS)
    assert _same_bits(state.volume.volume, state.volume_gt.volume)
    assert np.array_equal(state.volume.volume[1].cpu().numpy(), native_run["W"])
    s = report["recon_3d"]
    assert all(s[k] == 0 for k in zero) and all(s[k] == 1 for k in one) and s["n_pred"] == s["n_gt"] == report["points"] and s["clamped_pred"] == 0
    assert (tmp_path / "a.ply").read_bytes() == native_run["ply"].read_bytes()
    # half size: the scores against the float64 brute force on the two clouds
    report, state = _run(clean["dir"], tmp_path / "b", "--fuse", tmp_path / "b.ply", "--score-3d", size=(320, 240))
    assert not _same_bits(state.volume.volume, state.volume_gt.volume)
    pred = state.volume.extract_points()["xyz"].cpu().numpy()
    gt = state.volume_gt.extract_points()["xyz"].cpu().numpy()
    s = report["recon_3d"]
    assert s["threshold"] == 0.05 and s["max_dist"] == 1.0
    ref = C.metrics64(pred, gt, s["threshold"], s["max_dist"], device=DEV)
    C.check_metrics(s, ref, s["threshold"], "run_stream half size")
    print("RUN-STREAM score-3d half size against native ground truth: accuracy %.6f completeness %.6f m (float64 %.6f %.6f), precision %.4f recall %.4f "
          "fscore %.4f at %.2f m; %d against %d points" % (s["accuracy"], s["completeness"], ref["accuracy"], ref["completeness"], s["precision"], s["recall"],
                                                           s["fscore"], s["threshold"], s["n_pred"], s["n_gt"]))
    assert 0 < s["accuracy"] < S.VOXEL and s["fscore"] > 0.99
    # the cloud of the plain run as GT.ply: the scene against itself
    report, state = _run(clean["dir"], tmp_path / "c", "--fuse", tmp_path / "c.ply", "--score-3d", native_run["ply"])
    s = report["recon_3d"]
    assert state.volume_gt is None and s["ground_truth"] == str(native_run["ply"])
    assert s["accuracy"] == 0 and s["completeness"] == 0 and s["fscore"] == 1 and s["n_pred"] == s["n_gt"] == native_run["report"]["points"]


# ------------------------------------------------------------------------------------------------------------ 4. --render-fused
def test_render_fused(clean, native_ref, native_run, tmp_path):
    from estdepth_amd.metrics import compute_valid_depth_mask
    rb, sc = clean["read"], clean["scene"]
    report, state = _run(clean["dir"], tmp_path, "--fuse", tmp_path / "scene.ply", "--render-fused")
    assert (tmp_path / "scene.ply").read_bytes() == native_run["ply"].read_bytes()
    assert len(state.targets) == len(TARGETS) and not (tmp_path / "fused_rgb").exists()
    K = torch.from_numpy(rb["K"])
    n_gt = n_cov = 0
    renders = {}
    for t in TARGETS:
        maps = state.volume.render(torch.from_numpy(rb["poses"][t]), K, HW, depth_min=S.DEPTH_MIN, depth_max=S.DEPTH_MAX)
        fused = maps["depth"].cpu().numpy()
        renders[t] = fused
        got = np.load(tmp_path / "fused_depth" / (_stem(rb["names"][t]) + ".npy"))
        want = np.float16(fused[None])
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), "frame %d" % t
        gt_ok = compute_valid_depth_mask(rb["depths"][t].astype(np.float64))
        n_gt += int(gt_ok.sum())
        n_cov += int((gt_ok & (fused > 0)).sum())
    assert sorted(os.listdir(tmp_path / "fused_depth")) == sorted(_stem(rb["names"][t]) + ".npy" for t in TARGETS)
    assert report["fused_coverage"] == n_cov / n_gt and report["fused_coverage"] > 0.95
    # the fused depth against the analytic depth, beside the float64 ray caster on the float64 chain's volume.  The reference costs about a
    # second per 20 000 rays on the host: ONE target, every fourth pixel of every fourth row -- the SAME pixels on both sides
    t, step = TARGETS[len(TARGETS) // 2], 4
    M = RC.ray_matrix(rb["poses"][t], rb["K"], native_ref["origin"], S.VOXEL)
    M[:, 0:2] *= np.float32(step)                                                # pixel (u, v) of the sub-grid is pixel (4 u, 4 v) of the image
    n_steps = int(np.ceil((S.DEPTH_MAX - S.DEPTH_MIN) / S.VOXEL)) + 1
    D64, W64 = native_ref["ref"]["D"].astype(np.float32), native_ref["ref"]["Wt"].astype(np.float32)
    ref = RC.raycast(D64, W64, M, HW[0] // step, HW[1] // step, S.DEPTH_MIN, S.VOXEL, n_steps, 1.0)
    analytic, dev = sc["clean"][t][::step, ::step], renders[t][::step, ::step].astype(np.float64)
    err64 = np.abs(ref["depth"] - analytic)[ref["hit"]] / S.VOXEL
    errd = np.abs(dev - analytic)[dev > 0] / S.VOXEL
    whole = np.concatenate([np.abs(renders[k].astype(np.float64) - sc["clean"][k])[renders[k] > 0] for k in TARGETS]) / S.VOXEL
    print("RUN-STREAM render-fused: coverage %.4f; |fused - analytic depth| in voxels on frame %d, every %dth pixel: device median %.4f (%d pixels), "
          "float64 ray caster on the float64 volume median %.4f (%d pixels), device / float64 %.3f (cap %.2f); all covered pixels of all targets: "
          "median %.4f p95 %.4f" % (report["fused_coverage"], t, step, np.median(errd), errd.size, np.median(err64), err64.size,
                                    np.median(errd) / np.median(err64), MARGIN, np.median(whole), np.percentile(whole, 95)))
    assert err64.size > 10000 and errd.size > 10000
    assert np.median(errd) <= MARGIN * np.median(err64)


def test_render_fused_color(clean, native_run, tmp_path):
    from PIL import Image
    rb = clean["read"]
    report, state = _run(clean["dir"], tmp_path, "--fuse", tmp_path / "scene.ply", "--render-fused", "--color")
    assert state.volume.color is not None and report["points"] == native_run["report"]["points"]
    assert _same_bits(state.volume.volume, native_run["state"].volume.volume)    # colour changes no distance and no weight
    assert sorted(os.listdir(tmp_path / "fused_rgb")) == sorted(_stem(rb["names"][t]) + ".png" for t in TARGETS)
    for t in TARGETS:
        with Image.open(tmp_path / "fused_rgb" / (_stem(rb["names"][t]) + ".png")) as im:
            rgb = np.asarray(im.convert("RGB"))
        depth = np.load(tmp_path / "fused_depth" / (_stem(rb["names"][t]) + ".npy"))[0]
        assert rgb.shape == HW + (3,) and depth.shape == HW
        # the scene's frames are nowhere darker than 27 (run_stream_ref.smooth_rgb): a black pixel is a ray without a hit
        assert np.array_equal((rgb == 0).all(-1), depth == 0), "frame %d" % t
        assert (depth > 0).mean() > 0.95


# ------------------------------------------------------------------------------------------------------------ 5. --geo-filter
def test_geo_filter(corrupted, tmp_path):
    from estdepth_amd import consistency
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    from estdepth_amd.metrics import compute_valid_depth_mask
    rb = corrupted["read"]
    report, state = _run(corrupted["dir"], tmp_path / "f", "--fuse", tmp_path / "f.ply", "--geo-filter", 2)
    plain, _ = _run(corrupted["dir"], tmp_path / "u", "--fuse", tmp_path / "u.ply")
    # the same volume from the library, by hand: the window over the 8 targets' maps, then one integrate_filtered per frame, in order
    depths = torch.from_numpy(rb["depths"][TARGETS]).to(DEV)
    poses, K = torch.from_numpy(rb["poses"][TARGETS]), torch.from_numpy(rb["K"])
    out = consistency.filter_window(depths, poses, K, radius=2, min_views=2, px_max=1.0, rel_max=0.01)
    origin = frustum_volume(torch.from_numpy(rb["poses"][0]), K, HW, S.DEPTH_MIN, S.DEPTH_MAX, S.DIMS, S.VOXEL)
    vol = TSDFVolume(S.DIMS, S.VOXEL, origin, device=DEV)
    for k in range(len(TARGETS)):
        vol.integrate_filtered(dict(depth=out["depth"][k], views=out["views"][k], pose=poses[k], K=K, min_views=2))
    torch.cuda.synchronize()
    assert vol.fused_voxels() > 100000 and state.volume.frames == len(TARGETS)    # the clean scene updates 227 000; the filter keeps four pixels in five
    assert _same_bits(state.volume.volume, vol.volume)
    assert [_stem(n) for n, _ in state.fused] == [_stem(rb["names"][t]) for t in TARGETS]
    assert report["consistency"]["frames"] == len(TARGETS) and report["consistency"]["radius"] == 2 and state.geo.returned == len(TARGETS)
    kept = (out["mask"] & (out["depth"] > 0)).cpu().numpy()
    gt_ok = compute_valid_depth_mask(rb["depths"][TARGETS].astype(np.float64))
    assert report["filtered_coverage"] == int((gt_ok & kept).sum()) / int(gt_ok.sum())
    bad_kept = float((kept & corrupted["scene"]["bad"][TARGETS]).sum()) / max(int(corrupted["scene"]["bad"][TARGETS].sum()), 1)
    f, u = S.distance_figures(_cloud(tmp_path / "f.ply")), S.distance_figures(_cloud(tmp_path / "u.ply"))
    print("RUN-STREAM geo-filter: filtered coverage %.4f, corrupted pixels kept %.4f; distance to the analytic surface in voxels: filtered median %.4f "
          "p95 %.4f (%d points), unfiltered median %.4f p95 %.4f (%d points), filtered / unfiltered p95 %.4f"
          % (report["filtered_coverage"], bad_kept, f[0], f[1], report["points"], u[0], u[1], plain["points"], f[1] / u[1]))
    assert 0.5 < report["filtered_coverage"] < 0.96
    assert f[1] < u[1]


# ------------------------------------------------------------------------------------------------------------ 6. --track
def _pose_errors(fused, true):
    return [T.pose_error(pose.numpy(), true[t]) for (_, pose), t in zip(fused, TARGETS)]


@pytest.mark.parametrize("geo", [[], ["--geo-filter", 2]], ids=["plain", "geo-filter"])
def test_track(drifted, geo, tmp_path):
    """drift_from = 4: the poses of frames 4 .. 9 are written about 1 cm and 0.5 degrees off; --track pulls every one of them back, alone
    and on the filtered records of --geo-filter 2"""
    rb, true = drifted["read"], drifted["scene"]["poses"]
    drift_t, drift_a = T.pose_error(T.perturbed(true[4]), true[4])
    written = [T.pose_error(rb["poses"][t], true[t]) for t in TARGETS]
    name = "filtered " if geo else ""
    fig = {}
    for label, flags in (("untracked", geo), ("tracked", geo + ["--track"])):
        report, state = _run(drifted["dir"], tmp_path / label, "--fuse", tmp_path / (label + ".ply"), *flags)
        fig[label] = S.distance_figures(_cloud(tmp_path / (label + ".ply")))
        assert state.volume.frames == len(TARGETS) and [_stem(n) for n, _ in state.fused] == [_stem(rb["names"][t]) for t in TARGETS]
        if label == "untracked":
            assert "tracking" not in report
            for (_, pose), t in zip(state.fused, TARGETS):
                assert np.array_equal(pose.numpy(), rb["poses"][t].astype(np.float64))
            continue
        # one entry per target from the second fused one on: every fused record but the first was refined
        frames = report["tracking"]["frames"]
        assert [_stem(e["frame"]) for e in frames] == [_stem(rb["names"][t]) for t in TARGETS[1:]]
        assert np.array_equal(state.fused[0][1].numpy(), rb["poses"][TARGETS[0]].astype(np.float64))
        after = _pose_errors(state.fused, true)
        for k, t in enumerate(TARGETS):
            e = frames[k - 1] if k else None
            print("RUN-STREAM track (%stracked): frame %d pose error %.2f mm %.3f deg -> %.2f mm %.3f deg%s"
                  % (name, t, 1e3 * written[k][0], np.degrees(written[k][1]), 1e3 * after[k][0], np.degrees(after[k][1]),
                     "" if e is None else "; rmse %.2f -> %.2f mm, correction %.2f mm %.3f deg, matched share %.3f, %s after %d iterations"
                     % (1e3 * e["rmse_before"], 1e3 * e["rmse_after"], 1e3 * e["correction_m"], np.degrees(e["correction_rad"]), e["matched_share"],
                        e["reason"], e["iterations"])))
        for k, t in enumerate(TARGETS):
            if t >= 4:                                                           # a drifted frame: closer to the truth than it was written
                assert after[k][0] < written[k][0] and after[k][1] < written[k][1], "frame %d" % t
                assert frames[k - 1]["rmse_after"] < frames[k - 1]["rmse_before"], "frame %d" % t
            elif k:                                                              # an undrifted frame: corrected by less than the drift
                assert frames[k - 1]["correction_m"] < drift_t and frames[k - 1]["correction_rad"] < drift_a, "frame %d" % t
    print("RUN-STREAM track: distance to the analytic surface in voxels: %stracked median %.4f p95 %.4f, %suntracked median %.4f p95 %.4f, "
          "tracked / untracked %.3f %.3f" % ((name,) + fig["tracked"] + (name,) + fig["untracked"]
                                             + (fig["tracked"][0] / fig["untracked"][0], fig["tracked"][1] / fig["untracked"][1])))
    assert fig["tracked"][0] < fig["untracked"][0] and fig["tracked"][1] < fig["untracked"][1]


# ------------------------------------------------------------------------------------------------------------ 7. the real network
DUMPS = ("init_depth", "refined_depth", "init_prob", "refined_prob")
NET = ["--depth-source", "net", "--synthetic", "7", "--resnet", "18", "--ndepths", "64", "--image-size", "160", "128",
       "--volume-dims", "64", "64", "64", "--voxel-size", "0.08"]


def _dumps(out):
    return {(kind, name): (out / kind / name).read_bytes() for kind in DUMPS for name in sorted(os.listdir(out / kind))}


def test_flags_do_not_leak_into_one_another(tmp_path):
    """the configuration of test_end_to_end_joint_stream through the tool with the network: what a run dumps and the depth errors it
    reports do not depend on the reconstruction flags behind the stream, and the cloud of --fuse not on the read-outs after it"""
    runs = {"plain": [], "fuse": ["--fuse", "PLY"], "all": ["--fuse", "PLY", "--render-fused", "--score-3d", "--geo-filter", "1", "--track", "--color"],
            "fuse + read-outs": ["--fuse", "PLY", "--render-fused", "--score-3d"], "fuse + read-outs again": ["--fuse", "PLY", "--render-fused", "--score-3d"]}
    got, t_start = {}, time.time()
    for label, flags in runs.items():
        if label.startswith("fuse + read-outs") and time.time() - t_start > 20.0:        # the optional runs, only if the time allows
            print("RUN-STREAM net: the fourth run was left out after %.1f s" % (time.time() - t_start))
            continue
        out = tmp_path / label.replace(" ", "_")
        t0 = time.time()
        report, state = TOOL.run(TOOL.parse(NET + ["--out", str(out)] + [str(out / "scene.ply") if f == "PLY" else f for f in flags]))
        torch.cuda.synchronize()
        shutil.rmtree(report["scene"])                                           # the generated scene
        got[label] = dict(report=report, dumps=_dumps(out), ply=(out / "scene.ply").read_bytes() if flags else None)
        print("RUN-STREAM net: run '%s' %.1f s, %d windows" % (label, time.time() - t0, report["windows"]))
    print("RUN-STREAM net: %d runs in %.1f s" % (len(got), time.time() - t_start))
    base = got["plain"]
    assert base["report"]["windows"] == 5 and len(base["dumps"]) == 4 * 5
    d = np.load(tmp_path / "plain" / "refined_depth" / sorted(os.listdir(tmp_path / "plain" / "refined_depth"))[0])
    p = np.load(tmp_path / "plain" / "refined_prob" / sorted(os.listdir(tmp_path / "plain" / "refined_prob"))[0])
    assert d.shape == (1, 128, 160) and p.shape == (128, 160)                    # the layout the ground-truth stand-in reproduces
    for label, g in got.items():
        assert sorted(g["dumps"]) == sorted(base["dumps"]), label
        for key in base["dumps"]:
            assert g["dumps"][key] == base["dumps"][key], (label, key)
        assert g["report"]["errors"] == base["report"]["errors"], label
    everything = got["all"]["report"]
    for key in ("consistency", "errors_filtered", "filtered_coverage", "tracking", "recon_3d", "errors_fused", "fused_coverage", "points"):
        assert key in everything, key
    assert got["fuse"]["report"]["points"] > 0
    if "fuse + read-outs" in got:
        assert got["fuse + read-outs"]["ply"] == got["fuse"]["ply"]
    if "fuse + read-outs again" in got:
        # the same run twice reports the same scores: the two volumes' records reach the comparison in edge order, so a nearest neighbour
        # that has an equally near rival (and with it normal_consistency) does not depend on the order the extraction happened to write them in
        a, b = (dict(got[k]["report"]["recon_3d"], compare_ms=0.0) for k in ("fuse + read-outs", "fuse + read-outs again"))
        print("RUN-STREAM net: recon_3d of two identical runs: normal_consistency %.17g %.17g, accuracy %.17g %.17g"
              % (a["normal_consistency"], b["normal_consistency"], a["accuracy"], b["accuracy"]))
        assert a == b
