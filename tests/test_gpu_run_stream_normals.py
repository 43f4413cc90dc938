"""tools/run_stream.py --score-3d GT.ply --score-align plane --score-normals end to end on the device, on the analytic scene of
tests/test_gpu_run_stream.py (the helpers of the tool's suites are imported, not edited), with a ground truth that arrives as a PLAIN
CLOUD: samples of the scene's surface written as x y z only -- no nx ny nz, no faces -- as a laser scan would be:
  * with --score-normals recon_3d gains the ``normals`` block (estimated == ["gt"]), the registration converges and normal_consistency
    is there;
  * the same command without --score-normals fails as it does today: the plane metric has no normals to work with;
  * the flag without --score-3d GT.ply is refused at parse time."""
import json
import sys

import numpy as np
import pytest
import torch

from estdepth_amd.cloud_metrics import estimate_normals  # noqa: F401 -- the feature under test: without it this module does not import

from test_gpu_run_stream_mesh import _argv
from test_gpu_run_stream_sample import DENSITY, TOOL, scene  # noqa: F401 -- the scene fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bare_gt(scene):  # noqa: F811
    """the ground-truth surface sampled at four points per voxel face, written with x y z only"""
    from estdepth_amd.fusion3d import read_ply, sample_mesh
    d, gt, _ = scene
    xyz = sample_mesh(read_ply(str(gt), faces=True), density=4 * DENSITY, seed=3)["xyz"].cpu().numpy().astype("<f4")
    path = d / "gt_scan.ply"
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                 % xyz.shape[0]).encode("ascii"))
        f.write(xyz.tobytes())
    back = read_ply(str(path))
    assert back["normal"] is None and np.array_equal(back["xyz"], xyz)
    return d, path, xyz.shape[0]


def test_score_normals_end_to_end(bare_gt, tmp_path, monkeypatch):
    d, gt, n = bare_gt
    out = tmp_path / "normals"
    flags = ("--fuse", out / "scene.ply", "--score-3d", gt, "--score-align", "plane")
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(d, out, *flags, "--score-normals"))
    TOOL.main()
    torch.cuda.synchronize()
    got = json.load(open(out / "metrics.json"))["recon_3d"]
    blk = got["normals"]
    assert sorted(blk) == ["estimated", "invalid_gt", "invalid_pred", "k", "radius"]
    assert blk["estimated"] == ["gt"] and blk["k"] == 16 and blk["radius"] == got["threshold"] and 0 <= blk["invalid_gt"] < 0.05 * n
    assert got["alignment"]["converged"] is True and got["n_gt"] == n
    assert 0.8 < got["normal_consistency"] <= 1.0
    print("RUN-STREAM normals: %d ground-truth points, %d invalid; alignment %s; normal_consistency %.6f, accuracy %.6f, completeness %.6f"
          % (n, blk["invalid_gt"], {k: v for k, v in got["alignment"].items() if k != "T"}, got["normal_consistency"], got["accuracy"], got["completeness"]))
    # the same command without the flag: refused, as before
    with pytest.raises(RuntimeError, match="normals"):
        TOOL.run(TOOL.parse(_argv(d, tmp_path / "plain", *("--fuse", tmp_path / "plain.ply", "--score-3d", gt, "--score-align", "plane"))))
    # without alignment and without the flag: no normal score, no block
    report, _ = TOOL.run(TOOL.parse(_argv(d, tmp_path / "bare", "--fuse", tmp_path / "bare.ply", "--score-3d", gt)))
    assert "normals" not in report["recon_3d"] and "normal_consistency" not in report["recon_3d"]


def test_the_parse_time_refusals(bare_gt, tmp_path, capsys):
    d, gt, _ = bare_gt
    fuse = ("--fuse", tmp_path / "scene.ply")
    for bad in ((*fuse, "--score-normals"), (*fuse, "--score-3d", "--score-normals"), (*fuse, "--score-3d", gt, "--score-normals-radius", "0.1"),
                (*fuse, "--score-3d", gt, "--score-normals", "2"), (*fuse, "--score-3d", gt, "--score-normals", "33"),
                (*fuse, "--score-3d", gt, "--score-normals", "--score-normals-radius", "0")):
        with pytest.raises(SystemExit):
            TOOL.parse(_argv(d, tmp_path, *bad))
        assert "--score-normals" in capsys.readouterr().err, bad
    args = TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-normals"))
    assert args.score_normals == 16 and args.score_normals_radius is None
    args = TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-normals", "24", "--score-normals-radius", "0.08"))
    assert args.score_normals == 24 and args.score_normals_radius == 0.08
