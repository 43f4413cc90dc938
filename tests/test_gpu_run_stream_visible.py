"""tools/run_stream.py --score-3d GT.ply --score-sample DENSITY --score-visible, and --render-gt-mesh, end to end on the device, on the
scene, the 170-triangle ground-truth mesh and the set-up of tests/test_gpu_run_stream_sample.py (its helpers are imported, not edited).

That file's docstring says of the sampled scores: "the unobserved corners of the rectangle and the spheres' shadows on the plane show
(recall 0.75)" -- for a reconstruction a few millimetres off.  With --score-visible the ground-truth mesh is rendered at the pose,
intrinsics and size of each of the eight fused targets (csrc/mesh/mesh_raster.hip) and its samples no target saw are dropped.

The float64 chain on the CPU -- the chain of CHAIN64 there, then the reference rasteriser of tests/mesh_raster_ref.py at the eight target
poses (640 x 480, z_near 1e-3) and its float64 visibility test (tol = the threshold 0.05 m, depth_max 3.1 m, min_views 1) -- keeps 7976 of
the 10186 ground-truth samples (share 0.7830) and gives

                        accuracy  completeness  precision  recall    fscore
    sampled, visible    0.018226  0.018849      0.967534   0.945336  0.956306
    sampled (CHAIN64)   0.018226  0.067967      0.967534   0.746220  0.842587

(computed once with these modules and recorded here: CHAIN64_VISIBLE).  Recall rises from 0.746 to 0.945 and completeness falls from 68 mm
to 19 mm; accuracy and precision do not move, the predicted side is untouched.  The device must meet the restricted figures within
run_stream_ref.MARGIN, its recall with the flag must stand to its recall without as the chain's do (1.2668, less the margin), and its
accuracy and precision must not move beyond the margin.

--render-gt-mesh: under --depth-source gt the predictions ARE the scene's depth maps, so their errors against those maps vanish and
cannot serve as the yardstick; the yardstick is the chain's own figure instead -- the scene's depth maps scored against the reference
rasteriser's renders of the same mesh with the tool's error suite (CHAIN64_MESH_ERRORS: l1 33.7 mm, abs_relative 0.0134, rmse 0.162 m,
coverage 0.999996; the coarse icospheres' silhouettes are what differs), which the device must meet within the margin both ways."""
import json
import sys

import numpy as np
import pytest
import torch

import run_stream_ref as S
from test_gpu_run_stream_mesh import _argv, _dumps
from test_gpu_run_stream_sample import CHAIN64, DENSITY, TOOL, scene  # noqa: F401 -- the scene fixture and the unrestricted chain

pytestmark = pytest.mark.gpu
CHAIN64_VISIBLE = dict(accuracy=0.018226, completeness=0.018849, precision=0.967534, recall=0.945336, fscore=0.956306)
CHAIN64_N_VISIBLE, CHAIN64_N_GT = 7976, 10186
CHAIN64_MESH_ERRORS = dict(l1=0.033746, abs_relative=0.013379, rmse=0.161989, coverage=0.999996)


def test_the_chain_says_the_restriction_matters():
    """if the chain's restricted recall did not come out clearly above the unrestricted one, the visibility test would be wrong"""
    assert CHAIN64_VISIBLE["recall"] > CHAIN64["sampled"]["recall"] + 0.15
    assert abs(CHAIN64_VISIBLE["accuracy"] - CHAIN64["sampled"]["accuracy"]) < 1e-6 and CHAIN64_VISIBLE["precision"] == CHAIN64["sampled"]["precision"]


def test_score_visible_end_to_end(scene, tmp_path, monkeypatch):
    d, gt, _ = scene
    vis, plain = tmp_path / "visible", tmp_path / "plain"
    flags = ("--fuse", "scene.ply", "--score-3d", gt, "--score-sample", DENSITY)
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(d, vis, "--fuse", vis / "scene.ply", *flags[2:], "--score-visible"))
    TOOL.main()
    torch.cuda.synchronize()
    got = json.load(open(vis / "metrics.json"))["recon_3d"]
    report, _ = TOOL.run(TOOL.parse(_argv(d, plain, "--fuse", plain / "scene.ply", *flags[2:])))
    torch.cuda.synchronize()
    base = report["recon_3d"]
    # without the flag: today's keys and the same cloud and dumps, byte for byte
    assert sorted(base["sampled"]) == ["area_gt", "area_pred", "density", "invalid_gt", "invalid_pred", "n_gt", "n_pred"]
    assert sorted(set(got["sampled"]) - set(base["sampled"])) == ["n_gt_visible", "visible_share"] and sorted(got) == sorted(base)
    assert "errors_vs_gt_mesh" not in report and not (plain / "gt_mesh_depth").exists() and not (vis / "gt_mesh_depth").exists()
    assert (plain / "scene.ply").read_bytes() == (vis / "scene.ply").read_bytes()
    a, b = _dumps(vis), _dumps(plain)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    blk = got["sampled"]
    ref, unrestricted = CHAIN64_VISIBLE, CHAIN64["sampled"]
    print("RUN-STREAM visible: %d of %d ground-truth samples seen (share %.4f; chain %d of %d); restricted %s; unrestricted %s; chain %s"
          % (blk["n_gt_visible"], blk["n_gt"], blk["visible_share"], CHAIN64_N_VISIBLE, CHAIN64_N_GT, {k: round(got[k], 6) for k in ref},
             {k: round(base[k], 6) for k in ref}, ref))
    assert blk["n_gt"] == base["sampled"]["n_gt"] == CHAIN64_N_GT and got["n_gt"] == blk["n_gt_visible"]
    assert blk["visible_share"] == blk["n_gt_visible"] / blk["n_gt"] and blk["n_pred"] == base["sampled"]["n_pred"]
    # the same float32 samples and the float64 test: the count may differ by the samples within a rounding of a pixel border or of tol
    assert abs(blk["n_gt_visible"] - CHAIN64_N_VISIBLE) <= 0.001 * CHAIN64_N_GT
    assert got["accuracy"] <= S.MARGIN * ref["accuracy"] and got["completeness"] <= S.MARGIN * ref["completeness"]
    assert got["fscore"] >= ref["fscore"] / S.MARGIN and got["recall"] >= ref["recall"] / S.MARGIN
    # the point of the change: recall with the flag stands to recall without as the chain's do
    assert got["recall"] >= base["recall"] * (ref["recall"] / unrestricted["recall"]) / S.MARGIN
    assert got["recall"] > base["recall"] + 0.1
    # the predicted side is untouched
    assert base["accuracy"] / S.MARGIN <= got["accuracy"] <= base["accuracy"] * S.MARGIN
    assert base["precision"] / S.MARGIN <= got["precision"] <= base["precision"] * S.MARGIN


def test_min_views_restricts_further(scene, tmp_path):
    d, gt, _ = scene
    report, _ = TOOL.run(TOOL.parse(_argv(d, tmp_path, "--fuse", tmp_path / "scene.ply", "--score-3d", gt, "--score-sample", DENSITY, "--score-visible", 8)))
    torch.cuda.synchronize()
    blk = report["recon_3d"]["sampled"]
    assert 0 < blk["n_gt_visible"] < CHAIN64_N_VISIBLE            # seen by all eight targets: fewer than seen by one


def test_render_gt_mesh(scene, tmp_path):
    d, gt, _ = scene
    report, state = TOOL.run(TOOL.parse(_argv(d, tmp_path, "--fuse", tmp_path / "scene.ply", "--score-3d", gt, "--render-gt-mesh")))
    torch.cuda.synchronize()
    names = sorted(p.name for p in (tmp_path / "gt_mesh_depth").iterdir())
    assert len(names) == len(state.fused) == len(S.targets_of(S.N_FRAMES)) and all(n.endswith(".npy") for n in names)
    one = np.load(tmp_path / "gt_mesh_depth" / names[0])
    assert one.shape == (1, S.IMAGE_SIZE[1], S.IMAGE_SIZE[0]) and one.dtype == np.float32 and 1.0 < one.max() < 3.0
    got, ref = report["errors_vs_gt_mesh"], CHAIN64_MESH_ERRORS
    print("RUN-STREAM gt mesh: errors_vs_gt_mesh %s coverage %.6f; chain %s; errors_on_gt_mesh_covered %s"
          % ({k: round(got[k], 6) for k in ("l1", "abs_relative", "rmse")}, report["gt_mesh_coverage"], ref,
             {k: round(report["errors_on_gt_mesh_covered"][k], 6) for k in ("l1", "abs_relative", "rmse")}))
    for k in ("l1", "abs_relative", "rmse"):
        assert ref[k] / S.MARGIN <= got[k] <= ref[k] * S.MARGIN, k
    assert abs(report["gt_mesh_coverage"] - ref["coverage"]) < 1e-4
    assert report["errors_on_gt_mesh_covered"]["l1"] < 1e-6            # --depth-source gt: the predictions are the scene's own depth maps
    assert "sampled" not in report["recon_3d"]
    json.dumps(report)


def test_the_parse_time_refusals(scene, tmp_path, capsys):
    d, gt, cloud = scene
    fuse = ("--fuse", tmp_path / "scene.ply")
    for bad, word in (((*fuse, "--score-visible"), "--score-visible"), ((*fuse, "--score-3d", "--score-visible"), "--score-visible"),
                      ((*fuse, "--score-3d", gt, "--score-visible"), "--score-sample"),
                      ((*fuse, "--score-3d", gt, "--score-sample", DENSITY, "--score-visible", "0"), "at least 1"),
                      ((*fuse, "--score-3d", cloud, "--score-sample", DENSITY, "--score-visible"), "with faces"),
                      ((*fuse, "--render-gt-mesh"), "--render-gt-mesh"), ((*fuse, "--score-3d", "--render-gt-mesh"), "--render-gt-mesh"),
                      ((*fuse, "--score-3d", cloud, "--render-gt-mesh"), "with faces"), (("--score-3d", gt, "--render-gt-mesh"), "--fuse")):
        with pytest.raises(SystemExit):
            TOOL.parse(_argv(d, tmp_path, *bad))
        assert word in capsys.readouterr().err, bad
    TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-sample", DENSITY, "--score-visible", "2", "--render-gt-mesh"))
