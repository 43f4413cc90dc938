"""tools/run_stream.py --fuse P.ply --cloud-min-cluster N end to end on the device, with the set-up of
tests/test_gpu_run_stream_components.py (--depth-source gt on the analytic three-body scene of tests/run_stream_ref.py,
write_scene(seed=5)): the point cloud that is written is the unfiltered run's cloud without the rows ``cloud_metrics.filter_clusters``
drops (the same bytes, row for row), the ``cloud_clusters`` block of metrics.json agrees with the file's point count and with the
clustering of the unfiltered cloud, the 3D scores are those of the filtered cloud, and the same command without the flag writes no
such block and the bytes it wrote before."""
import json
import sys

import numpy as np
import pytest
import torch

import run_stream_ref as S
from test_gpu_run_stream_mesh import _argv

pytestmark = pytest.mark.gpu
TOOL = S.load_tool()
N = 50
EPS, K = 2.0 * S.VOXEL, 6                          # the tool's defaults: two voxel edges, 6 neighbours


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_cloud_clusters")
    S.write_scene(d, S.N_FRAMES, seed=5)
    return d


def test_cloud_min_cluster_flag_end_to_end(scene, tmp_path, monkeypatch):
    from estdepth_amd import cloud_metrics
    from estdepth_amd.fusion3d import read_ply
    filtered, plain = tmp_path / "filtered", tmp_path / "plain"
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(scene, filtered, "--fuse", filtered / "scene.ply", "--cloud-min-cluster", N, "--score-3d"))
    TOOL.main()
    torch.cuda.synchronize()
    metrics = json.load(open(filtered / "metrics.json"))
    block = metrics["cloud_clusters"]
    assert sorted(block) == ["clusters_kept", "dropped", "eps", "kept", "min_points", "min_size", "n_clusters", "noise"]
    assert (block["eps"], block["min_points"], block["min_size"]) == (EPS, K, N)
    # the same command without the flag: no block, and the cloud of the volume as save_ply writes it
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(scene, plain, "--fuse", plain / "scene.ply", "--score-3d"))
    TOOL.main()
    torch.cuda.synchronize()
    written = json.load(open(plain / "metrics.json"))
    assert "cloud_clusters" not in written and "clusters" not in written["recon_3d"]
    report, state = TOOL.run(TOOL.parse(_argv(scene, tmp_path / "again", "--fuse", tmp_path / "again" / "scene.ply", "--score-3d")))
    torch.cuda.synchronize()
    assert "cloud_clusters" not in report and "clusters" not in report["recon_3d"] and report["points"] == written["points"]
    assert (plain / "scene.ply").read_bytes() == (tmp_path / "again" / "scene.ply").read_bytes()
    state.volume.save_ply(str(tmp_path / "direct.ply"))
    assert (plain / "scene.ply").read_bytes() == (tmp_path / "direct.ply").read_bytes()
    whole, back = read_ply(str(plain / "scene.ply")), read_ply(str(filtered / "scene.ply"))
    assert report["points"] == whole["xyz"].shape[0] and metrics["points"] == back["xyz"].shape[0] == block["kept"]
    assert block["kept"] + block["dropped"] == whole["xyz"].shape[0] and block["noise"] <= block["dropped"]
    # the file is the unfiltered file without the rows the clustering drops
    f = cloud_metrics.filter_clusters(torch.from_numpy(whole["xyz"]).cuda(), EPS, K, min_size=N)
    keep = f["keep"].cpu().numpy()
    assert np.array_equal(back["xyz"].view(np.int32), whole["xyz"][keep].view(np.int32))
    assert np.array_equal(back["normal"].view(np.int32), whole["normal"][keep].view(np.int32))
    assert {k: block[k] for k in ("n_clusters", "clusters_kept", "kept", "dropped", "noise")} == {k: f[k] for k in ("n_clusters", "clusters_kept", "kept", "dropped", "noise")}
    sizes = f["sizes"].cpu().numpy()
    assert block["clusters_kept"] == int((sizes >= N).sum()) and block["kept"] == int(sizes[sizes >= N].sum())
    assert block["noise"] == int((f["cluster"] < 0).sum().item()) and block["dropped"] == block["noise"] + int(sizes[sizes < N].sum())
    # the scores are the filtered cloud's
    scored = metrics["recon_3d"]
    assert scored["n_pred"] == block["kept"] and report["recon_3d"]["n_pred"] == whole["xyz"].shape[0]
    assert scored["clusters"]["pred"] == {k: block[k] for k in ("n_clusters", "kept", "dropped", "noise")} and list(scored["clusters"]) == ["pred"]
    assert scored["n_gt"] == report["recon_3d"]["n_gt"]
    print("RUN-STREAM cloud clusters: %d clusters (sizes %s), %d kept; %d of %d points written, %d dropped (%d noise); precision %.6f -> %.6f, accuracy %.6g -> %.6g"
          % (block["n_clusters"], sorted(sizes.tolist(), reverse=True)[:8], block["clusters_kept"], block["kept"], whole["xyz"].shape[0], block["dropped"],
             block["noise"], report["recon_3d"]["precision"], scored["precision"], report["recon_3d"]["accuracy"], scored["accuracy"]))
    # not vacuous: the surface is there, and it is most of the cloud
    assert block["clusters_kept"] >= 1 and block["kept"] > 0.9 * whole["xyz"].shape[0]


def test_the_flags_are_checked(scene, tmp_path):
    for flags in (("--cloud-min-cluster", 5), ("--fuse", tmp_path / "a.ply", "--cloud-min-cluster", 0), ("--fuse", tmp_path / "a.ply", "--cloud-cluster-eps", 0.1),
                  ("--fuse", tmp_path / "a.ply", "--cloud-cluster-min-points", 4), ("--fuse", tmp_path / "a.ply", "--cloud-min-cluster", 5, "--cloud-cluster-eps", 0.0),
                  ("--fuse", tmp_path / "a.ply", "--cloud-min-cluster", 5, "--cloud-cluster-min-points", 0)):
        with pytest.raises(SystemExit):
            TOOL.parse(_argv(scene, tmp_path / "out", *flags))
    args = TOOL.parse(_argv(scene, tmp_path / "out", "--fuse", tmp_path / "a.ply", "--cloud-min-cluster", 5, "--cloud-cluster-eps", 0.1, "--cloud-cluster-min-points", 4))
    assert (args.cloud_min_cluster, args.cloud_cluster_eps, args.cloud_cluster_min_points) == (5, 0.1, 4)
