"""tools/run_stream.py --score-3d GT.ply --score-sample DENSITY --score-align plane end to end on the device, on the scene and the
170-triangle ground-truth mesh of tests/test_gpu_run_stream_sample.py (its helpers are imported, not edited) -- with the ground truth
MOVED by a known small rigid transform, as a scan in another frame of reference would be: G = Exp(track_ref.TWIST), about 1 cm and 0.5
degrees.  The fused surface then has to be moved by G to lie on the file's surface:
  * with --score-align plane recon_3d gains the ``alignment`` block and nothing else changes shape; its T is G within the margin of
    tests/test_gpu_registration.py -- 2 x the float64 reference registration's own error (rigid_align_ref.refine from the SAME device
    samples to the same mesh) plus the stopping step --, converged is true, and the accuracy is below the accuracy of the same command
    without the flag;
  * without the flag metrics.json's recon_3d and the dumps are what a second run of the same command gives, byte for byte, and no
    ``alignment`` key appears;
  * the flag without --score-3d, or with --score-3d but no file, is refused at parse time."""
import json
import sys

import numpy as np
import pytest
import torch

from estdepth_amd import registration  # noqa: F401 -- the feature under test: without it this module does not import

import rigid_align_ref as R
from test_gpu_run_stream_mesh import _argv, _dumps
from test_gpu_run_stream_sample import DENSITY, TOOL, scene  # noqa: F401 -- the scene fixture

pytestmark = pytest.mark.gpu
G = R.exp_se3(R.TWIST)


@pytest.fixture(scope="module")
def moved_gt(scene):  # noqa: F811
    from estdepth_amd.fusion3d import read_ply, write_ply
    d, gt, _ = scene
    mesh = read_ply(gt, faces=True)
    xyz = (mesh["xyz"].astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
    path = d / "gt_mesh_moved.ply"
    write_ply(str(path), np.concatenate([xyz, np.zeros_like(xyz)], 1), faces=mesh["faces"])
    return d, path, dict(xyz=xyz, faces=mesh["faces"])


def test_score_align_end_to_end(moved_gt, tmp_path, monkeypatch):
    from estdepth_amd.fusion3d import sample_mesh
    d, gt, mesh = moved_gt
    al, plain, again = tmp_path / "aligned", tmp_path / "plain", tmp_path / "again"
    flags = ("--score-3d", gt, "--score-sample", DENSITY)
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(d, al, "--fuse", al / "scene.ply", *flags, "--score-align", "plane"))
    TOOL.main()
    torch.cuda.synchronize()
    got = json.load(open(al / "metrics.json"))["recon_3d"]
    report, state = TOOL.run(TOOL.parse(_argv(d, plain, "--fuse", plain / "scene.ply", *flags)))
    torch.cuda.synchronize()
    base = report["recon_3d"]
    second, _ = TOOL.run(TOOL.parse(_argv(d, again, "--fuse", again / "scene.ply", *flags)))
    # without the flag: today's keys, and the same figures and dumps as a second run of the same command
    assert "alignment" not in base and sorted(set(got) - set(base)) == ["alignment"]
    drop = lambda r: {k: v for k, v in r.items() if k != "compare_ms"}                                        # noqa: E731
    assert json.dumps(drop(base), sort_keys=True) == json.dumps(drop(second["recon_3d"]), sort_keys=True)
    assert (plain / "scene.ply").read_bytes() == (al / "scene.ply").read_bytes() == (again / "scene.ply").read_bytes()
    a, b, c = _dumps(al), _dumps(plain), _dumps(again)
    assert a and sorted(a) == sorted(b) == sorted(c) and all(a[k] == b[k] == c[k] for k in a)
    blk = got["alignment"]
    assert sorted(blk) == ["T", "converged", "correction", "iterations", "overlap", "reason", "rmse"] and len(blk["T"]) == 16
    assert got["sampled"] == base["sampled"] and got["n_pred"] == base["n_pred"] and got["n_gt"] == base["n_gt"]
    # the float64 reference registration from the same device samples, with the tool's default stages (8, 4, 2 thresholds)
    samples = sample_mesh(state.volume.extract_mesh(), density=DENSITY, seed=0)["xyz"].cpu().numpy()
    assert samples.shape[0] == got["n_pred"]
    ref = R.refine(samples, mesh, metric="plane", dist_max=tuple(k * got["threshold"] for k in (8.0, 4.0, 2.0)), pivot=R.target_pivot(mesh))
    T = np.asarray(blk["T"]).reshape(4, 4)
    tr, ar = R.pose_error(ref["T"], G)
    td, ad = R.pose_error(T, G)
    print("RUN-STREAM align: T off the known transform by %.3g mm %.3g deg (float64 reference %.3g mm %.3g deg, %s after %d iterations); %s; "
          "accuracy %.6f aligned, %.6f without the flag; completeness %.6f / %.6f"
          % (1e3 * td, np.degrees(ad), 1e3 * tr, np.degrees(ar), ref["reason"], ref["iterations"], {k: v for k, v in blk.items() if k != "T"},
             got["accuracy"], base["accuracy"], got["completeness"], base["completeness"]))
    assert blk["converged"] is True and blk["reason"] == "converged"
    assert td <= 2 * tr + R.STEP_T and ad <= 2 * ar + R.STEP_R
    assert got["accuracy"] < base["accuracy"]


def test_the_parse_time_refusals(moved_gt, tmp_path, capsys):
    d, gt, _ = moved_gt
    fuse = ("--fuse", tmp_path / "scene.ply")
    for bad in ((*fuse, "--score-align", "plane"), (*fuse, "--score-3d", "--score-align", "plane"), (*fuse, "--score-3d", "--score-align"),
                (*fuse, "--score-3d", gt, "--score-align-dist", "0.2"), (*fuse, "--score-3d", gt, "--score-align", "--score-align-dist", "0.1", "0.2"),
                (*fuse, "--score-3d", gt, "--score-align", "--score-align-iters", "-1")):
        with pytest.raises(SystemExit):
            TOOL.parse(_argv(d, tmp_path, *bad))
        assert "--score-align" in capsys.readouterr().err, bad
    args = TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-sample", DENSITY, "--score-align", "--score-align-dist", "0.4", "0.2"))
    assert args.score_align == "plane" and args.score_align_dist == [0.4, 0.2] and args.score_align_iters == 30
    assert TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-align", "point")).score_align == "point"
