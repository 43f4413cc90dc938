"""tools/run_stream.py without a device: its argument checks, the scene writer of tests/run_stream_ref.py against the reader, to_gt_grid
against an exact index formula, the windowing of the --depth-source gt stand-in, and the feasibility of what tests/test_gpu_run_stream.py
asks of the device -- the analytic scene lies inside the tool's volume, the float64 chain's ambiguous share is below tsdf_ref.AMB_CAP, the
float64 chain's own cloud sits on the analytic surface, and the two orderings the GPU suite relies on (filtered closer than unfiltered on
the corrupted scene, tracked closer than untracked on the drifted one) hold by a factor of at least 2 in the numpy-fp32 evaluations of the
references.

Figures (this file prints them, pytest -s): see the docstring of tests/run_stream_ref.py for the scene's; the orderings: filtered /
unfiltered at 640 x 480 with corrupt = 0.05: p95 distance to the analytic surface 0.174 against 4.66 voxels (x 26.8); tracked / untracked at
320 x 240 with drift_from = 4: median 0.034 against 0.150 voxel (x 4.4), p95 0.181 against 0.433 (x 2.4), every drifted frame's pose error
9.85 mm / 0.50 degrees before and at most 1.5 mm / 0.05 degrees after."""
import numpy as np
import pytest
import torch

import run_stream_ref as S
import track_ref as T
import tsdf_ref as R

TOOL = S.load_tool()
HW = (S.IMAGE_SIZE[1], S.IMAGE_SIZE[0])
ORDER_FACTOR = 2.0           # "with room": each ordering of the GPU suite holds by this factor in the fp32 stand-ins


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_clean")
    return dict(written=S.write_scene(d, S.N_FRAMES, seed=5), read=S.read_back(d), dir=d)


# ------------------------------------------------------------------------------------------------------------ the tool's own logic
@pytest.mark.parametrize("flags", [["--render-fused"], ["--color"], ["--score-3d"], ["--track"], ["--score-3d", "gt.ply"]])
def test_parse_rejects_flags_that_need_fuse(flags, capsys):
    with pytest.raises(SystemExit):
        TOOL.parse(["--synthetic", "8", "--out", "o"] + flags)
    capsys.readouterr()
    args = TOOL.parse(["--synthetic", "8", "--out", "o", "--fuse", "s.ply"] + flags)
    assert args.fuse == "s.ply" and args.depth_source == "net"


def test_parse_needs_a_scene_and_knows_the_depth_sources(capsys):
    with pytest.raises(SystemExit):
        TOOL.parse(["--out", "o"])
    with pytest.raises(SystemExit):
        TOOL.parse(["--synthetic", "8", "--out", "o", "--depth-source", "oracle"])
    capsys.readouterr()
    assert TOOL.parse(["--scene-dir", "d", "--out", "o", "--depth-source", "gt"]).depth_source == "gt"
    assert callable(TOOL.run) and callable(TOOL.main)


@pytest.mark.parametrize("src,dst", [((240, 320), (480, 640)), ((480, 640), (240, 320)), ((480, 640), (480, 640)), ((7, 9), (480, 640)),
                                     ((480, 640), (100, 133)), ((3, 5), (1, 1)), ((1, 1), (4, 6))])
def test_to_gt_grid_against_the_index_formula(src, dst):
    """up-sampling, down-sampling, the identity and ratios that are no integers: every output pixel is the input pixel that holds its
    centre, by an exact integer formula"""
    a = np.random.RandomState(src[0] + dst[1]).uniform(size=src)
    ys, xs = S.nearest_index64(dst[0], src[0]), S.nearest_index64(dst[1], src[1])
    got = TOOL.to_gt_grid(a, dst)
    assert got.shape == dst and np.array_equal(got, a[ys][:, xs])
    assert np.array_equal(TOOL.nearest_index(dst[0], src[0]), ys) and np.array_equal(TOOL.nearest_index(dst[1], src[1]), xs)
    if src == dst:
        assert np.array_equal(got, a)


@pytest.mark.parametrize("lwindow", [3, 5])
def test_ground_truth_stream_windowing(lwindow):
    """None until lwindow frames are in, then one target per push: frame lwindow // 2 of the window, on the image grid"""
    h, w, n = 12, 16, lwindow + 4
    stream = TOOL.GroundTruthStream(lwindow=lwindow, image_hw=(6, 8))
    img, seen = torch.zeros(1, 3, 6, 8), []
    for i in range(n):
        dmap = torch.full((1, 1, h, w), float(i + 1))
        dmap[0, 0, :, w // 2:] = 0.0                                             # an invalid half
        dmap[0, 0, 0, 0] = 100.0 + i
        res = stream.push(img, torch.eye(4)[None], torch.eye(3)[None], dmap, dmap > 0)
        if i < lwindow - 1:
            assert res is None
            continue
        outputs = res[0]
        assert sorted(outputs, key=str) == sorted([("depth", 0, 0), ("depth", 0, 2), ("fused_prob", 0), ("init_prob", 0)], key=str)
        for v in outputs.values():
            assert tuple(v.shape) == (1, 1, 6, 8) and v.dtype == torch.float32
        d = outputs[("depth", 0, 0)][0, 0]
        target = i - (lwindow - 1) + lwindow // 2
        seen.append(target)
        assert float(d[3, 1]) == target + 1.0
        expect = torch.full((h, w), target + 1.0)
        expect[:, w // 2:] = 0.0
        expect[0, 0] = 100.0 + target
        assert torch.equal(d, expect[torch.from_numpy(S.nearest_index64(6, h))][:, torch.from_numpy(S.nearest_index64(8, w))])
        assert torch.equal(outputs[("depth", 0, 2)], outputs[("depth", 0, 0)])
        for k in (("fused_prob", 0), ("init_prob", 0)):
            assert torch.equal(outputs[k], (outputs[("depth", 0, 0)] > 0).float())
        assert 0 < int((d > 0).sum()) < d.numel()
    assert seen == S.targets_of(n, lwindow) and stream.windows == len(seen)
    # the identity at the native size
    stream = TOOL.GroundTruthStream(lwindow=3, image_hw=(h, w))
    maps = [torch.rand(1, 1, h, w) + 0.5 for _ in range(3)]
    for m in maps:
        res = stream.push(torch.zeros(1, 3, h, w), torch.eye(4)[None], torch.eye(3)[None], m, m > 0)
    assert torch.equal(res[0][("depth", 0, 0)], maps[1])
    with pytest.raises(RuntimeError):
        TOOL.GroundTruthStream(lwindow=2)


# ------------------------------------------------------------------------------------------------------------ the scene
def test_write_scene_then_read_back(clean):
    sc, rb = clean["written"], clean["read"]
    assert rb["depths"].shape == (S.N_FRAMES,) + HW and rb["depths"].dtype == np.float32
    K = S.reader_intrinsics()
    analytic = np.stack([T.scene_maps(P, K, *HW)[0] for P in T.scene_poses(S.N_FRAMES, seed=S.POSE_SEED)])
    assert np.array_equal(analytic, sc["clean"])
    err = np.abs(rb["depths"].astype(np.float64) - analytic)
    # millimetre storage: half a millimetre, and the fp32 rounding of the metres the reader hands over
    assert err.max() <= 0.5e-3 + 2.0 ** -24 * analytic.max()
    print("RUN-STREAM scene: depths %.3f .. %.3f m, holes %d, storage error %.4f mm" % (analytic.min(), analytic.max(), int((analytic <= 0).sum()), 1e3 * err.max()))
    assert analytic.min() > 1.45 and analytic.max() < 2.97 and (rb["depths"] > 0).all()
    assert rb["poses"].dtype == np.float32 and np.array_equal(rb["poses"], sc["written"].astype(np.float32))
    assert np.array_equal(sc["written"], sc["poses"])
    assert np.array_equal(rb["K"], S.reader_intrinsics().astype(np.float32)) and rb["imgs"].shape == (S.N_FRAMES, 3) + HW
    assert np.array_equal(S.read_back(clean["dir"], (320, 240))["K"], S.reader_intrinsics((320, 240)).astype(np.float32))


def test_write_scene_corrupt_and_drift(tmp_path):
    sc = S.write_scene(tmp_path / "c", 3, corrupt=0.05, seed=5)
    rb = S.read_back(tmp_path / "c")
    share = sc["bad"].mean(axis=(1, 2))
    assert (np.abs(share - 0.05) < 0.005).all()
    assert np.abs(rb["depths"].astype(np.float64) - sc["depths"]).max() <= 0.5e-3 + 2.0 ** -24 * sc["depths"].max()
    assert np.array_equal(sc["depths"][~sc["bad"]], sc["clean"][~sc["bad"]])
    lo, hi = sc["clean"].min(), sc["clean"].max()
    assert (sc["depths"][sc["bad"]] >= lo).all() and (sc["depths"][sc["bad"]] <= hi).all() and np.abs(sc["depths"] - sc["clean"])[sc["bad"]].mean() > 0.2
    again = S.write_scene(tmp_path / "c2", 3, corrupt=0.05, seed=5)
    assert np.array_equal(again["depths"], sc["depths"])
    sd = S.write_scene(tmp_path / "d", 4, drift_from=2, seed=5)
    rd = S.read_back(tmp_path / "d")
    assert np.array_equal(sd["poses"], T.scene_poses(4, seed=S.POSE_SEED))
    for i in range(4):
        want = T.perturbed(sd["poses"][i]) if i >= 2 else sd["poses"][i]
        assert np.array_equal(rd["poses"][i], want.astype(np.float32))
    t, a = T.pose_error(rd["poses"][3], sd["poses"][3])
    assert 0.009 < t < 0.011 and 0.008 < a < 0.010


def test_the_scene_is_feasible(clean):
    """what the GPU suite takes for granted, on the values the tool is fed"""
    rb = clean["read"]
    origin = S.volume_origin(rb["poses"][0], rb["K"], HW)
    lo = np.asarray(origin) + S.TRUNC
    hi = np.asarray(origin) + S.VOXEL * np.asarray(S.DIMS[::-1], np.float64) - S.TRUNC
    for i in range(S.N_FRAMES):
        p = S.backproject(rb["depths"][i], rb["poses"][i], rb["K"])
        assert p.shape[0] == HW[0] * HW[1] and (p >= lo).all() and (p <= hi).all(), "frame %d leaves the volume" % i
    tg = S.targets_of(S.N_FRAMES)
    assert tg == list(range(1, S.N_FRAMES - 1))
    # the library's host matrices against tsdf_ref's own float64 formula: a few ulps of their rows' magnitudes
    mats = S.matrices(rb["poses"][tg], rb["K"], origin)
    mats64 = R.tsdf_matrices64(rb["poses"][tg], rb["K"], origin, S.VOXEL)
    assert (np.abs(mats.astype(np.float64) - mats64) <= 4 * 2.0 ** -24 * np.abs(mats64).max(axis=2, keepdims=True)).all()
    ref, pts = S.fuse64(rb["depths"][tg], rb["poses"][tg], rb["K"], origin)
    n_upd, n_amb = int(ref["updated"].sum()), int(ref["amb"].sum())
    med, p95 = S.distance_figures(pts["xyz"])
    print("RUN-STREAM feasibility: origin %s; updated %d ambiguous %d (%.4f, cap %.2f); %d points, distance to the analytic surface median %.4f "
          "p95 %.4f voxel" % (origin, n_upd, n_amb, n_amb / n_upd, R.AMB_CAP, len(pts["edge"]), med, p95))
    assert n_upd > 200000 and n_amb <= R.AMB_CAP * n_upd
    assert len(pts["edge"]) > 9000
    assert med < 0.05 and p95 < 0.5


# ------------------------------------------------------------------------------------------------------------ the orderings, in fp32
def test_filtered_is_closer_than_unfiltered(tmp_path):
    """corrupt = 0.05, --geo-filter 2: the fp32 stand-ins of the filter and the fusion at the native size"""
    S.write_scene(tmp_path, S.N_FRAMES, corrupt=0.05, seed=5)
    rb = S.read_back(tmp_path)
    tg = S.targets_of(S.N_FRAMES)
    origin = S.volume_origin(rb["poses"][0], rb["K"], HW)
    depths, poses = rb["depths"][tg], rb["poses"][tg]
    kept = S.filter_standin(depths, poses, rb["K"], radius=2, min_views=2, dtype=np.float32)
    fig = {}
    for name, maps in (("unfiltered", depths), ("filtered", kept)):
        _, pts = S.fuse64(maps, poses, rb["K"], origin, dtype=np.float32)
        fig[name] = S.distance_figures(pts["xyz"])
    print("RUN-STREAM ordering (fp32 stand-in): p95 distance filtered %.4f unfiltered %.4f voxel (x %.1f); kept share %.3f"
          % (fig["filtered"][1], fig["unfiltered"][1], fig["unfiltered"][1] / fig["filtered"][1], float((kept > 0).mean())))
    assert ORDER_FACTOR * fig["filtered"][1] <= fig["unfiltered"][1]


def test_tracked_is_closer_than_untracked(tmp_path):
    """drift_from = 4, --track: the fp32 stand-ins of the ray caster, the alignment and the fusion, at half size (the tool's chain under
    --image-size 320 240) to keep the ray caster's reference quick"""
    sc = S.write_scene(tmp_path, S.N_FRAMES, drift_from=4, seed=5)
    hw, size = (240, 320), (320, 240)
    rb = S.read_back(tmp_path, size)
    tg = S.targets_of(S.N_FRAMES)
    origin = S.volume_origin(rb["poses"][0], rb["K"], hw)
    depths, poses, true = S.resample(rb["depths"][tg], hw), rb["poses"][tg], sc["poses"][tg]
    fig = {}
    for name, track in (("tracked", True), ("untracked", False)):
        used, pts = S.track_standin(depths, poses, rb["K"], origin, track=track, dtype=np.float32)
        fig[name] = S.distance_figures(pts["xyz"])
        if track:
            for k, t in enumerate(tg):
                before, after = T.pose_error(poses[k], true[k]), T.pose_error(used[k], true[k])
                print("RUN-STREAM ordering (fp32 stand-in): frame %d pose error %.2f mm %.3f deg -> %.2f mm %.3f deg"
                      % (t, 1e3 * before[0], np.degrees(before[1]), 1e3 * after[0], np.degrees(after[1])))
                if t >= 4:
                    assert ORDER_FACTOR * after[0] <= before[0] and ORDER_FACTOR * after[1] <= before[1]
                else:                                                            # an undrifted frame: corrected by less than the drift
                    assert after[0] < T.pose_error(T.perturbed(true[k]), true[k])[0] / ORDER_FACTOR
    print("RUN-STREAM ordering (fp32 stand-in): tracked median %.4f p95 %.4f, untracked median %.4f p95 %.4f voxel (x %.1f, x %.1f)"
          % (fig["tracked"] + fig["untracked"] + (fig["untracked"][0] / fig["tracked"][0], fig["untracked"][1] / fig["tracked"][1])))
    assert ORDER_FACTOR * fig["tracked"][0] <= fig["untracked"][0] and ORDER_FACTOR * fig["tracked"][1] <= fig["untracked"][1]
