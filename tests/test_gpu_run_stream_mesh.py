"""tools/run_stream.py --fuse P.ply --mesh M.ply end to end on the device, with --depth-source gt on the analytic three-body scene of
tests/run_stream_ref.py (the set-up of tests/test_gpu_run_stream.py): the mesh file reads back and is the surface-net mesh of the volume
the run fused (tests/tsdf_mesh_ref.py: topology exact, attributes within the bounds), metrics.json carries the ``mesh`` block, --color
reaches the vertices, and the flag changes nothing else: the cloud and the dumps of the same command without it are the same bytes."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import run_stream_ref as S
import tsdf_mesh_ref as M

pytestmark = pytest.mark.gpu
TOOL = S.load_tool()
DUMPS = ("init_depth", "refined_depth", "init_prob", "refined_prob")


def _argv(scene_dir, out, *flags):
    return ["--scene-dir", str(scene_dir), "--frame-interval", "1", "--out", str(out), "--depth-source", "gt",
            "--image-size", str(S.IMAGE_SIZE[0]), str(S.IMAGE_SIZE[1])] + S.VOLUME_ARGS + [str(f) for f in flags]


def _dumps(out):
    return {(kind, name): (out / kind / name).read_bytes() for kind in DUMPS if (out / kind).is_dir() for name in sorted(os.listdir(out / kind))}


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_mesh")
    S.write_scene(d, S.N_FRAMES, seed=5)
    return d


def test_mesh_flag_end_to_end(scene, tmp_path, monkeypatch):
    from estdepth_amd.fusion3d import mesh_edge_stats, read_ply
    with_mesh, without = tmp_path / "with", tmp_path / "without"
    # the command as a user gives it: main() = parse + run + metrics.json
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(scene, with_mesh, "--fuse", with_mesh / "scene.ply", "--mesh", with_mesh / "mesh.ply"))
    TOOL.main()
    torch.cuda.synchronize()
    block = json.load(open(with_mesh / "metrics.json"))["mesh"]
    assert sorted(block) == ["boundary_edges", "faces", "manifold_edges", "non_manifold_edges", "path", "vertices"]
    back = read_ply(str(with_mesh / "mesh.ply"), faces=True)
    assert back["xyz"].shape == (block["vertices"], 3) and back["normal"].shape == (block["vertices"], 3) and back["rgb"] is None
    assert back["faces"].shape == (block["faces"], 3) and block["vertices"] > 1000 and block["faces"] > 1000
    # the same command without the flag, in-process for its volume: the same cloud, the same dumps, no block
    report, state = TOOL.run(TOOL.parse(_argv(scene, without, "--fuse", without / "scene.ply")))
    torch.cuda.synchronize()
    assert "mesh" not in report and not (without / "mesh.ply").exists()
    assert (without / "scene.ply").read_bytes() == (with_mesh / "scene.ply").read_bytes()
    a, b = _dumps(with_mesh), _dumps(without)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    # the file is the mesh of the fused volume
    m = state.volume.extract_mesh()
    assert np.array_equal(back["xyz"].view(np.int32), m["xyz"].cpu().numpy().view(np.int32))
    assert np.array_equal(back["normal"].view(np.int32), m["normal"].cpu().numpy().view(np.int32))
    assert np.array_equal(back["faces"], m["faces"].cpu().numpy())
    stats = mesh_edge_stats(m["faces"])
    assert (block["boundary_edges"], block["manifold_edges"], block["non_manifold_edges"]) == (stats["boundary"], stats["manifold"], stats["non_manifold"])
    host = state.volume.volume.cpu().numpy()
    ref = M.mesh(host[0], host[1], 1.0, state.volume.voxel_size, state.volume.origin.tolist())
    fig = M.compare({k: v.cpu().numpy() for k, v in m.items() if isinstance(v, torch.Tensor)}, ref, "run_stream --mesh")
    assert (stats["boundary"], stats["manifold"], stats["non_manifold"]) == M.edge_stats(ref["faces"])[:3]
    print("RUN-STREAM mesh: %d vertices %d triangles, edges %d / %d / %d; xyz %.3f normal %.3f of the bound"
          % (block["vertices"], block["faces"], stats["boundary"], stats["manifold"], stats["non_manifold"], fig["xyz_ratio"], fig["normal_ratio"]))


def test_mesh_flag_with_colour(scene, tmp_path):
    from estdepth_amd.fusion3d import read_ply
    report, state = TOOL.run(TOOL.parse(_argv(scene, tmp_path, "--fuse", tmp_path / "scene.ply", "--mesh", tmp_path / "mesh.ply", "--color")))
    torch.cuda.synchronize()
    back = read_ply(str(tmp_path / "mesh.ply"), faces=True)
    m = state.volume.extract_mesh()
    assert report["mesh"]["vertices"] == back["xyz"].shape[0] == m["count"] and back["faces"].shape[0] == report["mesh"]["faces"]
    want = np.clip(np.rint(m["color"].cpu().numpy().astype(np.float64)), 0, 255).astype(np.uint8)
    assert back["rgb"] is not None and np.array_equal(back["rgb"], want) and back["rgb"].std() > 0
    host = state.volume.volume.cpu().numpy()
    ref = M.mesh(host[0], host[1], 1.0, state.volume.voxel_size, state.volume.origin.tolist(), state.volume.color.cpu().numpy())
    fig = M.compare({k: v.cpu().numpy() for k, v in m.items() if isinstance(v, torch.Tensor)}, ref, "run_stream --mesh --color")
    print("RUN-STREAM mesh colour: %d vertices, colour %.3f of the bound" % (m["count"], fig["color_ratio"]))
