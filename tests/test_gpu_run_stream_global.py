"""tools/run_stream.py --score-3d GT.ply --score-sample DENSITY --score-align plane --score-align-global end to end on the device -- with
the ground truth MOVED by global_reg_ref's 175-degree motion, as a scan in an unrelated frame of reference would be.

The scene is the room of tests/global_reg_ref.py (a floor, two walls, three boxes, a sphere) set before the cameras of
tests/run_stream_ref.py, tilted by 35 degrees so that floor, walls and the sides of the boxes show (``room_before_the_cameras``), and
rendered from its mesh at 160 x 120 with the reader's own intrinsics.  The ground-truth file is, as in
tests/test_gpu_run_stream_sample.py, the OBSERVED part of that surface as a scan describes it: the mesh cut into triangles of some
0.2 m, those whose centroid a camera saw (7.0 of 13.9 m2).  Both are conditions on the inputs, like the 98 mm / 5 degrees of
tests/test_global_reg_ref_cpu.py, and were measured once: the suite's other streaming scene, a plane and two spheres, where nearly
every point's neighbourhood looks like its neighbour's, gives 12 to 59 mutual matches at voxels of 3 to 15 cm and no hypothesis with
more than 15 inliers; against the WHOLE room, unseen walls and far sides included, the best hypothesis at the default voxel has 11
inliers of 155 pairs; in both cases the winner is refused for its inliers (``min_count`` 20), as it must be.  Against the observed part:
29 inliers of 131 pairs, 34.5 mm / 2.1 degrees.  ICP alone cannot bridge 175 degrees; with the global start
  * recon_3d's alignment block gains ``global`` (fitness, count, pairs, hypothesis, T_global) and nothing else changes shape;
  * T is the known transform within the margin tests/test_gpu_run_stream_align.py measures for its own case, measured the same way: 2 x
    the error of the float64 reference registration (rigid_align_ref.refine from the SAME device samples to the same mesh, started at
    the reported T_global, with the tool's default stages) plus the stopping step;
  * the accuracy is below the accuracy of the same command without the two flags, and is printed beside the figure of the unmoved file;
  * --score-align-global without --score-align is refused at parse time."""
import json
import sys

import numpy as np
import pytest
import torch

from estdepth_amd.registration import register_global  # noqa: F401 -- the feature under test: without it this module does not import

import global_reg_ref as GR
import rigid_align_ref as R
import run_stream_ref as S

pytestmark = pytest.mark.gpu
TOOL = S.load_tool()
DENSITY = 1.0 / S.VOXEL ** 2
SIZE = (160, 120)                            # (W, H) of the stored frames: a pixel is 1.8 cm wide on the floor, the voxel 3 cm
G = GR.motion("skew175")


def _argv(scene_dir, out, *flags):
    return ["--scene-dir", str(scene_dir), "--frame-interval", "1", "--out", str(out), "--depth-source", "gt",
            "--image-size", str(SIZE[0]), str(SIZE[1])] + S.VOLUME_ARGS + [str(f) for f in flags]


@pytest.fixture(scope="module")
def moved_gt(tmp_path_factory):
    return build_scene(tmp_path_factory.mktemp("scene_room"))


def build_scene(d):
    """-> (the scene's directory, the ground-truth mesh file, the moved one, the moved mesh)"""
    from estdepth_amd.eval_io import write_synthetic_scene
    from estdepth_amd.fusion3d import write_ply
    w, h = SIZE
    K = S.reader_intrinsics(SIZE)
    poses = S.T.scene_poses(S.N_FRAMES, seed=S.POSE_SEED)
    depths = [GR.render_depth(*GR.room_before_the_cameras(cut=False), P, K, h, w) for P in poses]
    assert min(float((m > 0).mean()) for m in depths) > 0.7 and min(float(m[m > 0].min()) for m in depths) > S.DEPTH_MIN and max(float(m.max()) for m in depths) < S.DEPTH_MAX
    write_synthetic_scene(str(d), list(S.smooth_rgb(S.N_FRAMES, h, w)), depths, list(poses))
    # the ground truth as a scan describes it (tests/test_gpu_run_stream_sample.py): the observed part -- the same surface cut into
    # triangles of some 0.2 m, those whose centroid a camera saw
    xyz, faces = GR.room_before_the_cameras()
    faces = faces[GR.faces_seen(xyz, faces, depths, poses, K, tol=0.05)]
    assert 6.0 < R.face_normals(xyz, faces)[1].sum() < 9.0
    gt = d / "gt_mesh.ply"
    write_ply(str(gt), np.concatenate([xyz, np.zeros_like(xyz)], 1), faces=faces)
    far = (xyz.astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
    path = d / "gt_mesh_moved_far.ply"
    write_ply(str(path), np.concatenate([far, np.zeros_like(far)], 1), faces=faces)
    return d, gt, path, dict(xyz=far, faces=faces)


def test_score_align_global_end_to_end(moved_gt, tmp_path, monkeypatch):
    from estdepth_amd.fusion3d import sample_mesh
    d, gt0, gt, mesh = moved_gt
    al, plain, home = tmp_path / "aligned", tmp_path / "plain", tmp_path / "home"
    flags = ("--score-3d", gt, "--score-sample", DENSITY)
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(d, al, "--fuse", al / "scene.ply", *flags, "--score-align", "plane", "--score-align-global"))
    TOOL.main()
    torch.cuda.synchronize()
    got = json.load(open(al / "metrics.json"))["recon_3d"]
    report, state = TOOL.run(TOOL.parse(_argv(d, plain, "--fuse", plain / "scene.ply", *flags)))
    base = report["recon_3d"]
    unmoved = TOOL.run(TOOL.parse(_argv(d, home, "--fuse", home / "scene.ply", "--score-3d", gt0, "--score-sample", DENSITY)))[0]["recon_3d"]
    torch.cuda.synchronize()
    assert "alignment" not in base and sorted(set(got) - set(base)) == ["alignment"]
    blk = got["alignment"]
    assert sorted(blk) == ["T", "converged", "correction", "global", "iterations", "overlap", "reason", "rmse"] and len(blk["T"]) == 16
    assert sorted(blk["global"]) == ["T_global", "count", "fitness", "hypothesis", "pairs"] and len(blk["global"]["T_global"]) == 16
    samples = sample_mesh(state.volume.extract_mesh(), density=DENSITY, seed=0)["xyz"].cpu().numpy()
    assert samples.shape[0] == got["n_pred"]
    Tg = np.asarray(blk["global"]["T_global"]).reshape(4, 4)
    ref = R.refine(samples, mesh, init=Tg, metric="plane", dist_max=tuple(k * got["threshold"] for k in (8.0, 4.0, 2.0)), pivot=R.target_pivot(mesh))
    T = np.asarray(blk["T"]).reshape(4, 4)
    centre = samples.astype(np.float64).mean(0)
    tg, ag = R.transform_error(Tg, G, centre)
    tr, ar = R.transform_error(ref["T"], G, centre)
    td, ad = R.transform_error(T, G, centre)
    print("RUN-STREAM align global: global stage %.1f mm %.2f deg off the known transform (%s); refined %.3g mm %.3g deg (float64 reference %.3g mm "
          "%.3g deg, %s after %d iterations); %s; accuracy %.6f aligned, %.6f without the flags, %.6f against the unmoved file"
          % (1e3 * tg, np.degrees(ag), {k: v for k, v in blk["global"].items() if k != "T_global"}, 1e3 * td, np.degrees(ad), 1e3 * tr, np.degrees(ar),
             ref["reason"], ref["iterations"], {k: v for k, v in blk.items() if k not in ("T", "global")}, got["accuracy"], base["accuracy"],
             unmoved["accuracy"]))
    assert blk["converged"] is True and blk["reason"] == "converged"
    assert td <= 2 * tr + R.STEP_T and ad <= 2 * ar + R.STEP_R
    assert got["accuracy"] < base["accuracy"]
    # the accuracy RETURNS to the unmoved figure, within a margin that is measured as tests/test_gpu_register_global.py measures it: the
    # sampled score's own repeatability, the largest change of the unmoved figure over three other sampling seeds (the tool's is 0)
    from estdepth_amd.cloud_metrics import compare_meshes
    from estdepth_amd.fusion3d import read_ply
    home_mesh = read_ply(str(gt0), faces=True)
    score = lambda s: compare_meshes(state.volume.extract_mesh(), dict(xyz=home_mesh["xyz"], faces=home_mesh["faces"]), DENSITY,      # noqa: E731
                                     threshold=got["threshold"], max_dist=got["max_dist"], seed=s)["accuracy"]
    assert score(0) == unmoved["accuracy"]
    repeat = max(abs(score(s) - unmoved["accuracy"]) for s in (1, 2, 3))
    print("RUN-STREAM align global: accuracy %.6f against the unmoved figure %.6f: off by %.3g where the figure's repeatability over three other "
          "seeds is %.3g" % (got["accuracy"], unmoved["accuracy"], abs(got["accuracy"] - unmoved["accuracy"]), repeat))
    assert abs(got["accuracy"] - unmoved["accuracy"]) <= repeat


def test_the_parse_time_refusals(moved_gt, tmp_path, capsys):
    d, _, gt, _ = moved_gt
    fuse = ("--fuse", tmp_path / "scene.ply")
    for bad in ((*fuse, "--score-3d", gt, "--score-align-global"), (*fuse, "--score-3d", gt, "--score-align-global", "0.1"),
                (*fuse, "--score-3d", gt, "--score-align", "plane", "--score-align-global", "0"),
                (*fuse, "--score-3d", gt, "--score-align", "plane", "--score-align-global", "-2")):
        with pytest.raises(SystemExit):
            TOOL.parse(_argv(d, tmp_path, *bad))
        assert "--score-align-global" in capsys.readouterr().err, bad
    args = TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-align", "plane", "--score-align-global", "0.08"))
    assert args.score_align_global == 0.08
    assert TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-align", "--score-align-global")).score_align_global == -1.0
    assert TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-align")).score_align_global is None
