"""tools/run_stream.py --score-3d GT.ply --score-sample DENSITY --score-exact end to end on the device, on the scene, the 170-triangle
ground-truth mesh and the set-up of tests/test_gpu_run_stream_sample.py (its helpers are imported, not edited).

That file's chain gives the sampled accuracy of the fused ten-frame scene as 18.2 mm -- for a surface a tenth of a millimetre off the
scene: the figure is the floor of the nearest-SAMPLE distance, about 1 / (2 sqrt(DENSITY)) = 15 mm at DENSITY = 1111 per square metre.
With --score-exact the distances go to the ground-truth mesh itself (csrc/mesh/mesh_distance.hip):
  * recon_3d gains the ``exact`` block and nothing else changes shape; without the flag metrics.json's recon_3d and the dumps are what
    a second run of the same command gives, byte for byte, and no ``exact`` key appears;
  * the exact accuracy is below the sampled one, and agrees with the float64 chain's figure -- the brute-force distance of
    tests/mesh_distance_ref.py from the SAME device samples to the same mesh, clamped and averaged -- within the summed bound
    (2 x the mean e_dist of the winners)."""
import json
import sys

import numpy as np
import pytest
import torch

import mesh_distance_ref as R
from test_gpu_run_stream_mesh import _argv, _dumps
from test_gpu_run_stream_sample import CHAIN64, DENSITY, TOOL, scene  # noqa: F401 -- the scene fixture and the sampled chain

pytestmark = pytest.mark.gpu


def test_score_exact_end_to_end(scene, tmp_path, monkeypatch):
    from estdepth_amd.fusion3d import read_ply, sample_mesh
    d, gt, _ = scene
    ex, plain, again = tmp_path / "exact", tmp_path / "plain", tmp_path / "again"
    flags = ("--score-3d", gt, "--score-sample", DENSITY)
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(d, ex, "--fuse", ex / "scene.ply", *flags, "--score-exact"))
    TOOL.main()
    torch.cuda.synchronize()
    got = json.load(open(ex / "metrics.json"))["recon_3d"]
    report, state = TOOL.run(TOOL.parse(_argv(d, plain, "--fuse", plain / "scene.ply", *flags)))
    torch.cuda.synchronize()
    base = report["recon_3d"]
    second, _ = TOOL.run(TOOL.parse(_argv(d, again, "--fuse", again / "scene.ply", *flags)))
    # without the flag: today's keys, and the same figures and dumps as a second run of the same command
    assert "exact" not in base and sorted(set(got) - set(base)) == ["exact"]
    drop = lambda r: {k: v for k, v in r.items() if k != "compare_ms"}
    assert json.dumps(drop(base), sort_keys=True) == json.dumps(drop(second["recon_3d"]), sort_keys=True)
    assert (plain / "scene.ply").read_bytes() == (ex / "scene.ply").read_bytes() == (again / "scene.ply").read_bytes()
    a, b, c = _dumps(ex), _dumps(plain), _dumps(again)
    assert a and sorted(a) == sorted(b) == sorted(c) and all(a[k] == b[k] == c[k] for k in a)
    mesh = read_ply(gt, faces=True)
    assert got["exact"]["faces_gt"] == mesh["faces"].shape[0] - got["exact"]["invalid_gt"] and got["exact"]["invalid_gt"] == 0
    assert got["exact"]["faces_pred"] > 1000 and got["exact"]["invalid_pred"] >= 0
    assert got["sampled"] == base["sampled"] and got["n_pred"] == base["n_pred"] and got["n_gt"] == base["n_gt"]
    # the float64 chain from the same device samples
    pred = state.volume.extract_mesh()
    samples = sample_mesh(pred, density=DENSITY, seed=0)["xyz"].cpu().numpy()
    assert samples.shape[0] == got["n_pred"]
    dmin, _, bf = R.nearest64(samples, mesh["xyz"], mesh["faces"])
    bound = R.C * float(np.take_along_axis(bf["e_dist"], np.argmin(bf["dist"], 1)[:, None], 1).mean())
    chain = float(np.minimum(dmin, got["max_dist"]).mean())
    print("RUN-STREAM exact: accuracy %.6f (float64 chain %.6f, bound %.3g) completeness %.6f precision %.4f recall %.4f; sampled accuracy %.6f "
          "completeness %.6f (chain %.6f); exact block %s"
          % (got["accuracy"], chain, bound, got["completeness"], got["precision"], got["recall"], base["accuracy"], base["completeness"],
             CHAIN64["sampled"]["accuracy"], got["exact"]))
    assert got["accuracy"] < base["accuracy"]
    assert abs(got["accuracy"] - chain) <= bound
    assert got["completeness"] <= base["completeness"] and got["precision"] >= base["precision"] and got["recall"] >= base["recall"]


def test_the_parse_time_refusals(scene, tmp_path, capsys):
    d, gt, cloud = scene
    fuse = ("--fuse", tmp_path / "scene.ply")
    for bad, word in (((*fuse, "--score-exact"), "--score-exact"), ((*fuse, "--score-3d", "--score-sample", DENSITY, "--score-exact"), "--score-exact"),
                      ((*fuse, "--score-3d", gt, "--score-exact"), "--score-sample"),
                      ((*fuse, "--score-3d", cloud, "--score-sample", DENSITY, "--score-exact"), "with faces")):
        with pytest.raises(SystemExit):
            TOOL.parse(_argv(d, tmp_path, *bad))
        assert word in capsys.readouterr().err, bad
    TOOL.parse(_argv(d, tmp_path, *fuse, "--score-3d", gt, "--score-sample", DENSITY, "--score-exact", "--score-visible"))
