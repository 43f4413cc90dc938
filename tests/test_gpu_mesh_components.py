"""The mesh components as a feature (fusion3d.mesh_components / filter_mesh, TSDFVolume.extract_mesh(min_component=), save_mesh): repeated
calls and shuffled face orders give the same integers, the host layer's filter equals its numpy twin (tests/mesh_components_ref.py), the
two-sphere volume loses its small sphere and keeps a closed surface on the large one, and the default extract_mesh() is what it was --
no new kernel, the same bits.  The kernels themselves are covered case by case in tests/test_gpu_mesh_components_routes.py."""
import numpy as np
import pytest
import torch

from estdepth_amd.fusion3d import filter_mesh, mesh_components

import mesh_components_ref as C
import tsdf_mesh_ref as M
from test_gpu_mesh_components_routes import profiled
from test_gpu_recon3d_routes import _dev, _same, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MARGIN = 1.25                # the project's margin of a semantic bar over the float64 reference's own figure (tests/test_gpu_tsdf_mesh.py)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _np(d):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def _equal_to_twin(got, want, what):
    """a filter_mesh result against the numpy twin's: the same keys, arrays equal bit for bit, counts equal"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert isinstance(g, torch.Tensor) and g.is_cuda, "%s: %s is not a device tensor" % (what, k)
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differs from the twin" % (what, k)
        else:
            assert g == w, "%s: %s = %r, the twin has %r" % (what, k, g, w)


def test_repeated_calls_and_bindings_are_bit_identical():
    from estdepth_amd import ops
    faces_np, V = C.build_case("grid-320")
    faces = _dev(faces_np)
    first = ops.mesh_components(faces, V)
    for binding in ("torch", "ctypes", "torch", "ctypes"):
        again = under(binding, lambda: ops.mesh_components(faces, V))
        assert all(_same(a, b) for a, b in zip(first, again)), binding
    C.compare(dict(label=first[0].cpu().numpy(), triangles=first[1].cpu().numpy(), invalid=int(first[2].item())), C.reference("grid-320"), "grid-320")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_face_order_changes_nothing(seed):
    faces_np, V = C.build_case("grid-320")
    ref = C.reference("grid-320")
    order = np.random.default_rng(seed).permutation(faces_np.shape[0])
    turned = np.roll(faces_np[order], seed % 3, axis=1)                     # and another vertex of every triangle comes first
    out = mesh_components(np.ascontiguousarray(turned), V)
    assert np.array_equal(out["label"].cpu().numpy(), ref["label"])
    roots, tri, verts = C.summary(ref)
    assert out["count"] == 5 and out["roots"].dtype == torch.int64 and np.array_equal(out["roots"].cpu().numpy(), roots)
    assert np.array_equal(out["triangles"].cpu().numpy(), tri) and np.array_equal(out["vertices"].cpu().numpy(), verts)


def test_n_vertices_defaults_to_the_largest_index_plus_one():
    faces_np, V = C.build_case("one-v7")
    out = mesh_components(_dev(faces_np))
    assert out["label"].shape == (7,) and out["count"] == 5 and out["roots"].tolist() == [0, 1, 2, 3, 4]
    assert out["triangles"].tolist() == [0, 0, 1, 0, 0] and out["vertices"].tolist() == [1, 1, 3, 1, 1]
    out = mesh_components(np.zeros((0, 3), np.int32))
    assert out["count"] == 0 and out["label"].shape == (0,) and out["roots"].shape == (0,)


@pytest.mark.parametrize("name", ["9x17x66", "colour", "holes"])
def test_filter_mesh_equals_its_twin(name):
    """fragments, loose vertices, ties between components of one size: every way of choosing, against the numpy twin"""
    ref = M.reference(M.build_case(name))
    mesh = {k: ref[k] for k in ("xyz", "normal", "weight", "cell", "faces", "edge", "count")}
    mesh["xyz"], mesh["normal"], mesh["weight"] = (mesh[k].astype(np.float32) for k in ("xyz", "normal", "weight"))
    mesh["note"] = "kept as it is"
    for kw in (dict(), dict(min_triangles=0), dict(min_triangles=4), dict(min_triangles=50), dict(keep_largest=1), dict(keep_largest=3),
               dict(min_triangles=4, keep_largest=1000), dict(min_triangles=10 ** 6), dict(min_triangles=0, keep_largest=0)):
        _equal_to_twin(filter_mesh(mesh, **kw), C.filter_mesh(mesh, **kw), "%s %s" % (name, kw))
    on_device = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in mesh.items()}
    _equal_to_twin(filter_mesh(on_device, min_triangles=4), C.filter_mesh(mesh, min_triangles=4), "%s on the device" % name)


@pytest.fixture(scope="module")
def two_spheres():
    from estdepth_amd.fusion3d import TSDFVolume
    D, W, origin, centre = C.two_sphere_volume()
    vol = TSDFVolume(D.shape, M.VOXEL, origin, device=DEV)
    vol.volume.copy_(_dev(np.stack([D, W])))
    return vol, centre


def test_the_default_extract_mesh_is_what_it_was(two_spheres):
    from estdepth_amd import ops
    from estdepth_amd.fusion3d import sorted_mesh
    vol, _ = two_spheres
    m = profiled(set(), lambda: vol.extract_mesh())                       # no mesh_cc_* kernel
    direct = sorted_mesh(ops.tsdf_mesh_vertices, ops.tsdf_mesh_faces, vol.volume, None, vol.voxel_size, vol.origin, 1.0)
    assert sorted(m) == sorted(direct) == ["cell", "count", "edge", "faces", "normal", "weight", "xyz"]
    assert m["count"] == direct["count"] == 1998 and m["faces"].shape == (3988, 3)
    assert all(_same(m[k], direct[k]) for k in m if k != "count")
    assert _same(profiled(set(), lambda: vol.extract_mesh(min_component=0))["faces"], direct["faces"])


def test_min_component_drops_the_small_sphere(two_spheres):
    """extract_mesh(min_component=229) on the two-sphere volume equals the float64 reference's filtered mesh -- topology to the integer,
    attributes within tsdf_mesh_ref's bounds -- has 3760 triangles, is closed with Euler number 2, and its vertices lie as close to the
    0.30 m sphere as the reference's own: median and 95th percentile of | |p - centre| - 0.30 | within 1.25 x the reference's (the
    statistics and the margin of tests/test_gpu_tsdf_mesh.py)."""
    from estdepth_amd.fusion3d import mesh_edge_stats
    vol, centre = two_spheres
    ref = C.two_sphere_mesh()
    want = C.filter_mesh(ref, min_triangles=229)
    kept = np.isin(ref["cell"], want["cell"])
    for k in ("E_xyz", "E_normal", "E_weight", "normal_ok"):
        want[k] = ref[k][kept]
    m = profiled({"mesh_cc_init_kernel", "mesh_cc_hook_kernel", "mesh_cc_flatten_kernel", "mesh_cc_count_kernel"},
                 lambda: vol.extract_mesh(min_component=229))
    got = _np(m)
    fig = M.compare(got, want, "two spheres, min_component=229")
    assert m["faces"].shape == (3760, 3) and m["faces"].dtype == torch.int32 and m["count"] == 1882 == m["xyz"].shape[0]
    assert m["components"] == 1 and m["dropped"] == dict(vertices=116, faces=228, components=1) == want["dropped"]
    stats = mesh_edge_stats(m["faces"])
    assert (stats["boundary"], stats["non_manifold"], stats["euler"]) == (0, 0, 2) and stats["manifold"] == 3760 * 3 // 2
    d_got = np.abs(np.linalg.norm(got["xyz"].astype(np.float64) - centre, axis=1) - 0.30) / M.VOXEL
    d_ref = np.abs(np.linalg.norm(want["xyz"] - centre, axis=1) - 0.30) / M.VOXEL
    med, p95, med_r, p95_r = np.median(d_got), np.percentile(d_got, 95), np.median(d_ref), np.percentile(d_ref, 95)
    print("MESH-CC two spheres: %d vertices %d triangles kept, dropped %s; xyz %.3f normal %.3f of the bound; distance to the sphere in "
          "voxels, median / p95: device %.5f / %.5f, reference %.5f / %.5f" % (m["count"], m["faces"].shape[0], m["dropped"], fig["xyz_ratio"],
                                                                              fig["normal_ratio"], med, p95, med_r, p95_r))
    assert med <= MARGIN * med_r and p95 <= MARGIN * p95_r
    # 228 keeps both spheres; keep_largest=1 is the same choice as 229
    both = vol.extract_mesh(min_component=228)
    assert both["faces"].shape == (3988, 3) and both["dropped"] == dict(vertices=0, faces=0, components=0)
    assert _same(filter_mesh(vol.extract_mesh(), keep_largest=1)["faces"], m["faces"])


def test_save_mesh_and_a_ply_round_trip(two_spheres, tmp_path):
    from estdepth_amd.fusion3d import read_ply
    vol, _ = two_spheres
    assert vol.save_mesh(str(tmp_path / "all.ply")) == (1998, 3988)
    assert vol.save_mesh(str(tmp_path / "big.ply"), min_component=229) == (1882, 3760)
    back, big = read_ply(str(tmp_path / "all.ply"), faces=True), read_ply(str(tmp_path / "big.ply"), faces=True)
    out = filter_mesh(back, min_triangles=229)                           # numpy arrays in, device tensors out
    _equal_to_twin(out, C.filter_mesh(back, min_triangles=229), "ply round trip")
    assert sorted(out) == sorted(list(back) + ["count", "components", "dropped"]) and out["rgb"] is None
    assert np.array_equal(out["xyz"].cpu().numpy().view(np.int32), big["xyz"].view(np.int32))
    assert np.array_equal(out["normal"].cpu().numpy().view(np.int32), big["normal"].view(np.int32))
    assert np.array_equal(out["faces"].cpu().numpy(), big["faces"])
