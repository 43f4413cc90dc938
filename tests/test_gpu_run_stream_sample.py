"""tools/run_stream.py --fuse P.ply --score-3d GT.ply --score-sample DENSITY end to end on the device, with the set-up of
tests/test_gpu_run_stream_mesh.py (--depth-source gt on the analytic three-body scene of tests/run_stream_ref.py, write_scene(seed=5)).

The ground truth is a COARSE MESH of the scene's observed part, as a decimated scan describes it (mesh_sample_ref.scene_mesh): the plane
as two triangles over the rectangle the eight targets see, the two spheres as the camera-facing triangles of level-2 icospheres -- 111
vertices, 170 triangles, 9.167 m2.  The fused volume is scored against it twice: with --score-sample 1 / voxel^2 (1111.1 points per m2:
both surfaces sampled by area) and without (today's path: the fused cloud against the file's 111 vertices).

The float64 chain on the CPU -- run_stream_ref.fuse64, tsdf_mesh_ref.mesh, the reference sampler of tests/mesh_sample_ref.py (seed 0 on
both sides, 7300 and 10186 points) and a brute-force nearest neighbour, threshold 0.05 m, distances clamped at 1 m -- gives

                 accuracy  completeness  precision  recall   fscore
    sampled      0.018226  0.067967      0.967534   0.746220 0.842587
    vertex only  0.520383  0.018518      0.127424   0.936937 0.224338

(computed once with these modules and recorded here: CHAIN64).  Scored by its vertices the mesh is close to useless -- half a metre of
"accuracy" for a reconstruction a few millimetres off, one point in eight "precise" -- and its recall, 0.94, counts 111 vertices where the
surface has 9 m2: sampled, the unobserved corners of the rectangle and the spheres' shadows on the plane show (recall 0.75).  The device
must reproduce the sampled figures within the project's semantic margin run_stream_ref.MARGIN (1.25 x), its sampled recall must stand
to its vertex-only recall as the chain's do (0.7964, less the margin), and so must accuracy and precision."""
import json
import sys

import numpy as np
import pytest
import torch

import mesh_sample_ref as MS
import run_stream_ref as S
from test_gpu_run_stream_mesh import _argv, _dumps

pytestmark = pytest.mark.gpu
TOOL = S.load_tool()
DENSITY = 1.0 / S.VOXEL ** 2
CHAIN64 = dict(sampled=dict(accuracy=0.018226, completeness=0.067967, precision=0.967534, recall=0.746220, fscore=0.842587),
               vertex=dict(accuracy=0.520383, completeness=0.018518, precision=0.127424, recall=0.936937, fscore=0.224338))


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from estdepth_amd.fusion3d import write_ply
    d = tmp_path_factory.mktemp("scene_sample")
    S.write_scene(d, S.N_FRAMES, seed=5)
    rb = S.read_back(d)
    tg = S.targets_of(S.N_FRAMES)
    xyz, faces = MS.scene_mesh(rb["depths"][tg], rb["poses"][tg], rb["K"])
    assert xyz.shape == (111, 3) and faces.shape == (170, 3) and abs(MS.face_area(xyz, faces)["area"].sum() - 9.166997) < 1e-5
    gt = d / "gt_mesh.ply"
    write_ply(str(gt), np.concatenate([xyz, np.zeros_like(xyz)], 1), faces=faces)
    cloud = d / "gt_cloud.ply"
    write_ply(str(cloud), np.concatenate([xyz, np.zeros_like(xyz)], 1))
    return d, gt, cloud


def test_score_sample_end_to_end(scene, tmp_path, monkeypatch):
    d, gt, cloud = scene
    sampled, plain = tmp_path / "sampled", tmp_path / "plain"
    # the command as a user gives it: main() = parse + run + metrics.json
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(d, sampled, "--fuse", sampled / "scene.ply", "--score-3d", gt, "--score-sample", DENSITY))
    TOOL.main()
    torch.cuda.synchronize()
    got = json.load(open(sampled / "metrics.json"))["recon_3d"]
    report, _ = TOOL.run(TOOL.parse(_argv(d, plain, "--fuse", plain / "scene.ply", "--score-3d", gt)))
    torch.cuda.synchronize()
    vert = report["recon_3d"]
    # without the flag: today's keys, today's path (the file's vertices), and the same cloud and dumps
    assert "sampled" not in vert and vert["n_gt"] == 111 and sorted(set(got) - set(vert)) == ["sampled"]
    assert (plain / "scene.ply").read_bytes() == (sampled / "scene.ply").read_bytes()
    a, b = _dumps(sampled), _dumps(plain)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    blk = got["sampled"]
    assert sorted(blk) == ["area_gt", "area_pred", "density", "invalid_gt", "invalid_pred", "n_gt", "n_pred"]
    assert blk["density"] == DENSITY and blk["invalid_gt"] == 0 == blk["invalid_pred"] and abs(blk["area_gt"] - 9.166997) < 1e-4
    assert blk["n_gt"] == got["n_gt"] == MS.n_for_density(DENSITY, blk["area_gt"]) == 10186
    assert blk["n_pred"] == got["n_pred"] == MS.n_for_density(DENSITY, blk["area_pred"]) and abs(blk["n_pred"] - 7300) <= 0.01 * 7300
    ref, rv = CHAIN64["sampled"], CHAIN64["vertex"]
    print("RUN-STREAM sample: sampled %s; vertex only %s; float64 chain %s" % (
        {k: round(got[k], 6) for k in ref}, {k: round(vert[k], 6) for k in ref}, CHAIN64))
    assert got["accuracy"] <= S.MARGIN * ref["accuracy"] and got["completeness"] <= S.MARGIN * ref["completeness"]
    assert got["fscore"] >= ref["fscore"] / S.MARGIN
    assert got["recall"] >= vert["recall"] * (ref["recall"] / rv["recall"]) / S.MARGIN
    # what sampling is for: the distance to a surface, not to its nearest corner
    assert got["accuracy"] <= vert["accuracy"] * (ref["accuracy"] / rv["accuracy"]) * S.MARGIN
    assert got["precision"] >= vert["precision"] * (ref["precision"] / rv["precision"]) / S.MARGIN
    assert vert["accuracy"] > 0.3 and vert["precision"] < 0.2


def test_a_ground_truth_without_faces_is_scored_as_a_cloud(scene, tmp_path):
    d, _, cloud = scene
    report, _ = TOOL.run(TOOL.parse(_argv(d, tmp_path, "--fuse", tmp_path / "scene.ply", "--score-3d", cloud, "--score-sample", DENSITY)))
    torch.cuda.synchronize()
    got = report["recon_3d"]
    assert got["sampled"]["area_gt"] is None and got["sampled"]["n_gt"] == 111 == got["n_gt"] and got["sampled"]["area_pred"] > 5.0
    json.dumps(report["recon_3d"])


def test_the_flag_follows_mesh_min_component_and_needs_score_3d(scene, tmp_path, capsys):
    d, gt, _ = scene
    report, state = TOOL.run(TOOL.parse(_argv(d, tmp_path, "--fuse", tmp_path / "scene.ply", "--mesh", tmp_path / "mesh.ply", "--mesh-min-component", 100,
                                              "--score-3d", gt, "--score-sample", DENSITY)))
    torch.cuda.synchronize()
    from estdepth_amd.fusion3d import mesh_area
    kept = mesh_area(state.volume.extract_mesh(min_component=100))["total"]
    assert report["recon_3d"]["sampled"]["area_pred"] == kept < mesh_area(state.volume.extract_mesh())["total"]
    for bad in (("--score-sample", "100"), ("--score-3d", gt, "--score-sample", "0"), ("--score-3d", gt, "--score-sample", "nan")):
        with pytest.raises(SystemExit):
            TOOL.parse(_argv(d, tmp_path, "--fuse", tmp_path / "scene.ply", *bad))
    assert "--score-sample" in capsys.readouterr().err
