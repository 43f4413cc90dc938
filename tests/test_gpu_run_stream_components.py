"""tools/run_stream.py --fuse P.ply --mesh M.ply --mesh-min-component 100 end to end on the device, with the set-up of
tests/test_gpu_run_stream_mesh.py (--depth-source gt on the analytic three-body scene of tests/run_stream_ref.py, write_scene(seed=5)):
the mesh file is ``filter_mesh`` of the float64 reference mesh of the volume the run fused (tests/tsdf_mesh_ref.py and the numpy twin of
tests/mesh_components_ref.py: topology exact, attributes within the bounds), the ``mesh`` block's new keys agree with it, and the same
command without the new flag writes the bytes and the six-key block it wrote before.

The float64 chain on the CPU (integrate_targets, tsdf_mesh_ref.mesh) gives 8 components of 11228 / 3870 / 1260 / 10 / 4 / 2 / 2 / 2
triangles and 274 vertices no face uses: N = 100 keeps the plane and the two spheres and has a wide margin on both sides.  So that the
test cannot pass on an empty filter it demands at least 2 components kept, 1 dropped and 1 vertex dropped."""
import json
import sys

import numpy as np
import pytest
import torch

import mesh_components_ref as C
import run_stream_ref as S
import tsdf_mesh_ref as M
from test_gpu_run_stream_mesh import _argv

pytestmark = pytest.mark.gpu
TOOL = S.load_tool()
N = 100


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_components")
    S.write_scene(d, S.N_FRAMES, seed=5)
    return d


def test_min_component_flag_end_to_end(scene, tmp_path, monkeypatch):
    from estdepth_amd.fusion3d import mesh_edge_stats, read_ply
    filtered, plain = tmp_path / "filtered", tmp_path / "plain"
    monkeypatch.setattr(sys, "argv", ["run_stream.py"] + _argv(scene, filtered, "--fuse", filtered / "scene.ply", "--mesh", filtered / "mesh.ply",
                                                               "--mesh-min-component", N))
    TOOL.main()
    torch.cuda.synchronize()
    block = json.load(open(filtered / "metrics.json"))["mesh"]
    assert sorted(block) == ["boundary_edges", "components", "components_kept", "faces", "faces_dropped", "manifold_edges", "non_manifold_edges",
                             "path", "vertices", "vertices_dropped"]
    # the same command without the new flag: today's six keys, and (below) today's bytes = the unfiltered mesh of the same volume
    report, state = TOOL.run(TOOL.parse(_argv(scene, plain, "--fuse", plain / "scene.ply", "--mesh", plain / "mesh.ply")))
    torch.cuda.synchronize()
    assert sorted(report["mesh"]) == ["boundary_edges", "faces", "manifold_edges", "non_manifold_edges", "path", "vertices"]
    assert (plain / "scene.ply").read_bytes() == (filtered / "scene.ply").read_bytes()
    whole = state.volume.extract_mesh()
    state.volume.save_mesh(str(tmp_path / "direct.ply"))
    assert (plain / "mesh.ply").read_bytes() == (tmp_path / "direct.ply").read_bytes()
    assert report["mesh"]["vertices"] == whole["count"] and report["mesh"]["faces"] == whole["faces"].shape[0]
    # the filtered file is filter_mesh of the reference mesh of the fused volume
    host = state.volume.volume.cpu().numpy()
    ref = M.mesh(host[0], host[1], 1.0, state.volume.voxel_size, state.volume.origin.tolist())
    want = C.filter_mesh(ref, min_triangles=N)
    kept = np.isin(ref["cell"], want["cell"])
    for k in ("E_xyz", "E_normal", "E_weight", "normal_ok"):
        want[k] = ref[k][kept]
    back = read_ply(str(filtered / "mesh.ply"), faces=True)
    m = state.volume.extract_mesh(min_component=N)
    assert np.array_equal(back["xyz"].view(np.int32), m["xyz"].cpu().numpy().view(np.int32))
    assert np.array_equal(back["normal"].view(np.int32), m["normal"].cpu().numpy().view(np.int32))
    assert np.array_equal(back["faces"], m["faces"].cpu().numpy()) and np.array_equal(back["faces"], want["faces"])
    fig = M.compare({k: v.cpu().numpy() for k, v in m.items() if isinstance(v, torch.Tensor)}, want, "run_stream --mesh-min-component")
    # the block agrees
    roots, tri, _ = C.summary(C.components(ref["faces"], ref["count"]))
    with_faces = int((tri > 0).sum())
    assert block["vertices"] == want["count"] == back["xyz"].shape[0] and block["faces"] == want["faces"].shape[0]
    assert block["components"] == with_faces and block["components_kept"] == want["components"] == int((tri >= N).sum())
    assert block["vertices_dropped"] == want["dropped"]["vertices"] == ref["count"] - want["count"]
    assert block["faces_dropped"] == want["dropped"]["faces"] == ref["faces"].shape[0] - want["faces"].shape[0]
    stats = mesh_edge_stats(m["faces"])
    assert (block["boundary_edges"], block["manifold_edges"], block["non_manifold_edges"]) == (stats["boundary"], stats["manifold"], stats["non_manifold"])
    assert (stats["boundary"], stats["manifold"], stats["non_manifold"]) == M.edge_stats(want["faces"])[:3]
    print("RUN-STREAM components: %d of %d components kept (triangles %s), %d vertices and %d faces dropped, %d vertices %d triangles written; "
          "xyz %.3f normal %.3f of the bound" % (block["components_kept"], block["components"], sorted(tri[tri > 0].tolist(), reverse=True),
                                                 block["vertices_dropped"], block["faces_dropped"], block["vertices"], block["faces"],
                                                 fig["xyz_ratio"], fig["normal_ratio"]))
    # not vacuous
    assert block["components_kept"] >= 2 and block["components"] - block["components_kept"] >= 1 and block["vertices_dropped"] >= 1
