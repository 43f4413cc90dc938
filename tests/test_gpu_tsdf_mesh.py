"""GPU: the surface-net mesh of a TSDF volume (csrc/mesh/tsdf_mesh.hip behind ops.tsdf_mesh_vertices / ops.tsdf_mesh_faces and
TSDFVolume.extract_mesh) against the float64 reference of tests/tsdf_mesh_ref.py under its ``compare``: cell ids, edge ids and faces
EXACT, the vertex attributes within the derived first-order bounds.

The synthetic volumes are the smallest at which the kernels can go wrong (tsdf_mesh_ref.CASES): one cell, two cells, an X that is no
multiple of 4, volumes past a 63-cell wave, a 4-row workgroup and the 8-plane march, an all-unobserved and an all-positive volume (both
kernels run and append nothing), holes in the weights, exact zeros on crossing edges, a colour volume.  The semantic test fuses the eight
analytic views of tests/test_gpu_track.py into 96 x 128 x 128 voxels of 3 cm and meshes that.  The measured fractions of the bounds:
profiles/tsdf_mesh_gpu_tests.txt."""
import functools

import numpy as np
import pytest
import torch

import track_ref as T
import tsdf_mesh_ref as M
import tsdf_ref as R
from helpers import _binding

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CLEAR = 1e-3                 # a triangle clearly faces an eye: cosine above this (fp32 vertices move a cosine by ~1e-6)
MARGIN = 1.25                # the project's margin of a semantic bar over the float64 reference's own figure: fp32 evaluation only


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = M.build_case(name)
    return c, M.reference(c)


def _inputs(c):
    vol = _dev(np.stack([c["D"], c["W"]]))
    col = _dev(c["C"]) if c["C"] is not None else None
    return vol, col, torch.tensor(c["origin"], dtype=torch.float32)


def _mesh(c, vol=None, col=None):
    from estdepth_amd import fusion3d, ops
    v, k, org = _inputs(c)
    out = fusion3d.sorted_mesh(ops.tsdf_mesh_vertices, ops.tsdf_mesh_faces, v if vol is None else vol, k if col is None else col, c["voxel"], org, c["w_min"])
    torch.cuda.synchronize()
    return out


def _np(m):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in m.items()}


def _bits_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            x, y = a[k].contiguous(), b[k].contiguous()
            assert x.dtype == y.dtype and x.shape == y.shape, k
            if x.is_floating_point():
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), "%s differs" % k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_against_reference(name, binding, monkeypatch):
    _binding(monkeypatch, binding)
    c, ref = _case(name)
    got = _mesh(c)
    assert got["count"] == ref["count"] and got["cell"].dtype == torch.int64 and got["edge"].dtype == torch.int64 and got["faces"].dtype == torch.int32
    assert ("color" in got) == (c["C"] is not None)
    fig = M.compare(_np(got), ref, "%s %s" % (name, binding))
    print("MESH-RATIO %s %s: %d vertices %d triangles; xyz %.3f weight %.3f normal %.3f%s of the bound; normals left out %.4f"
          % (name, binding, fig["vertices"], fig["faces"], fig["xyz_ratio"], fig["weight_ratio"], fig["normal_ratio"],
             " colour %.3f" % fig["color_ratio"] if "color_ratio" in fig else "", fig["normal_left_out"]))


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_calls_and_bindings_give_identical_bits(name, monkeypatch):
    c, _ = _case(name)
    _binding(monkeypatch, "torch")
    a, b = _mesh(c), _mesh(c)
    _binding(monkeypatch, "ctypes")
    d = _mesh(c)
    _bits_equal(a, b)
    _bits_equal(a, d)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_a_capacity_below_the_count_keeps_that_many_whole_records(name, binding, monkeypatch):
    """a third of the count as capacity (0 where there are fewer than three records: the counting call): the counter ends at the total;
    the kept records are records of the full result, each once"""
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    c, ref = _case(name)
    vol, col, org = _inputs(c)
    full = _mesh(c)
    V, Q = ref["count"], ref["edge"].shape[0]
    cap = V // 3
    count, cell, xyz, normal, weight, rgb = ops.tsdf_mesh_vertices(vol, col, c["voxel"], org, c["w_min"], cap)
    assert int(count.item()) == V and cell.shape == (cap,) and xyz.shape == (cap, 3) and (rgb is None) == (col is None)
    assert torch.unique(cell).shape[0] == cap
    at = torch.searchsorted(full["cell"], cell)
    assert torch.equal(full["cell"][at], cell)
    for got, key in ((xyz, "xyz"), (normal, "normal"), (weight, "weight")) + (((rgb, "color"),) if col is not None else ()):
        assert torch.equal(got.view(torch.int32), full[key][at].contiguous().view(torch.int32)), key
    qcap = Q // 3
    count, edge, quad = ops.tsdf_mesh_faces(vol, c["w_min"], qcap)
    assert int(count.item()) == Q and edge.shape == (qcap,) and quad.shape == (qcap, 4) and quad.dtype == torch.int32
    assert torch.unique(edge).shape[0] == qcap
    at = torch.searchsorted(full["edge"], edge)
    assert torch.equal(full["edge"][at], edge)
    index = torch.searchsorted(full["cell"], quad.to(torch.int64))
    tri = index[:, [0, 1, 2, 0, 2, 3]].to(torch.int32)
    assert torch.equal(tri, full["faces"].reshape(-1, 6)[at])
    # capacity 0 counts only
    assert int(ops.tsdf_mesh_vertices(vol, col, c["voxel"], org, c["w_min"], 0)[0].item()) == V
    assert int(ops.tsdf_mesh_faces(vol, c["w_min"], 0)[0].item()) == Q


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_dimension_of_one_has_no_cells(binding, monkeypatch):
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    org = torch.zeros(3)
    for dims in ((1, 5, 8), (4, 1, 8), (4, 5, 1)):
        D, W = M.wavy(dims, holes=False)
        vol = _dev(np.stack([D, W]))
        out = ops.tsdf_mesh_vertices(vol, None, 0.03, org, 1.0, 4)
        assert int(out[0].item()) == 0 and out[1].shape == (4,)
        assert int(ops.tsdf_mesh_faces(vol, 1.0, 4)[0].item()) == 0


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_arguments_raise_before_launch(binding, monkeypatch):
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    c, _ = _case("colour")
    vol, col, org = _inputs(c)
    bad = [lambda: ops.tsdf_mesh_vertices(vol.cpu(), None, 0.03, org, 1.0, 0),
           lambda: ops.tsdf_mesh_vertices(vol[0], None, 0.03, org, 1.0, 0),
           lambda: ops.tsdf_mesh_vertices(vol, col[:, :-1].contiguous(), 0.03, org, 1.0, 0),
           lambda: ops.tsdf_mesh_vertices(vol, col.double(), 0.03, org, 1.0, 0),
           lambda: ops.tsdf_mesh_vertices(vol, None, 0.0, org, 1.0, 0),
           lambda: ops.tsdf_mesh_vertices(vol, None, float("inf"), org, 1.0, 0),
           lambda: ops.tsdf_mesh_vertices(vol, None, 0.03, org, float("nan"), 0),
           lambda: ops.tsdf_mesh_vertices(vol, None, 0.03, org.to(DEV), 1.0, 0),
           lambda: ops.tsdf_mesh_vertices(vol, None, 0.03, torch.tensor([0.0, float("nan"), 0.0]), 1.0, 0),
           lambda: ops.tsdf_mesh_vertices(vol, None, 0.03, org, 1.0, -1),
           lambda: ops.tsdf_mesh_faces(vol.cpu(), 1.0, 0),
           lambda: ops.tsdf_mesh_faces(vol.double(), 1.0, 0),
           lambda: ops.tsdf_mesh_faces(vol, float("nan"), 0),
           lambda: ops.tsdf_mesh_faces(vol, 1.0, -1)]
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail("malformed call %d was accepted" % i)


# ------------------------------------------------------------------------------------------------------------ the semantic test
DIMS, ORIGIN, HW = (96, 128, 128), (-1.92, -1.92, 0.2), (120, 160)


def _scene_distance(p):
    """unsigned distance of the points p [N,3] (float64) to the analytic scene of track_ref: the plane and the two spheres"""
    d = np.abs(p[:, 2] - T.PLANE_Z)
    for centre, radius in T.SPHERES:
        d = np.minimum(d, np.abs(np.linalg.norm(p - np.asarray(centre), axis=1) - radius))
    return d


def test_the_fused_analytic_scene_as_a_mesh():
    """eight views of the three-body scene fused at 3 cm, as tests/test_gpu_track.py does.  The mesh equals the float64 reference on the
    same volume (topology exact, attributes within the bounds); no mesh edge is shared by more than two triangles; the median and the
    95th percentile of the vertices' distance to the analytic scene stay within 1.25 x the reference's own.

    The camera side.  The cameras saw the free space, D grows towards them, and the vertex normals point that way by construction
    (g sums D1 - D0): every triangle's geometric normal must lie on the side of its three vertex normals.  Measured against the eyes
    themselves -- a positive component towards at least one of the eight -- the float64 reference's own mesh of this scene has 21 of
    16686 triangles that face none (numpy fusion of tsdf_ref.integrate, cosines -0.002 .. -0.16): they stand on the walls that TSDF
    fusion raises along the rays grazing a silhouette, between voxels seen free and voxels behind the body, and such a wall is parallel
    to the rays that made it.  That is a property of the fused volume, not of the mesher, so the bar on the eyes is relative: wherever
    the reference's triangle clearly faces an eye (cosine > CLEAR) the device's must face one; the count of the others is printed."""
    from estdepth_amd.fusion3d import TSDFVolume, mesh_edge_stats
    H, W = HW
    K = R.intrinsics(H, W)
    poses = R.scene_poses(8, seed=2)
    depths = np.stack([T.scene_maps(P, K, H, W)[0] for P in poses]).astype(np.float32)
    vol = TSDFVolume(DIMS, R.VOXEL, ORIGIN, device=DEV)
    vol.integrate(_dev(depths), torch.from_numpy(poses), torch.from_numpy(K))
    m = vol.extract_mesh()
    torch.cuda.synchronize()
    host = vol.volume.cpu().numpy()
    ref = M.mesh(host[0], host[1], 1.0, R.VOXEL, ORIGIN)
    got = _np(m)
    fig = M.compare(got, ref, "fused scene")
    stats = mesh_edge_stats(m["faces"])
    assert (stats["boundary"], stats["manifold"], stats["non_manifold"], stats["euler"]) == M.edge_stats(ref["faces"])
    nrm, cen = M.triangle_normals(got["xyz"], got["faces"])
    eyes = poses[:, :3, 3]

    def facing_cos(normals, centroids):
        to_eye = eyes[None] - centroids[:, None]
        return np.max(np.einsum("fj,fej->fe", normals, to_eye) / (np.linalg.norm(normals, axis=1)[:, None] * np.linalg.norm(to_eye, axis=2)), axis=1)
    facing, facing_ref = facing_cos(nrm, cen), facing_cos(*M.triangle_normals(ref["xyz"], ref["faces"]))
    on_normal_side = np.einsum("ij,ij->i", nrm, got["normal"].astype(np.float64)[got["faces"]].sum(1))
    d_got, d_ref = _scene_distance(got["xyz"].astype(np.float64)) / R.VOXEL, _scene_distance(ref["xyz"]) / R.VOXEL
    med, p95, med_r, p95_r = np.median(d_got), np.percentile(d_got, 95), np.median(d_ref), np.percentile(d_ref, 95)
    print("MESH-SEMANTIC %d vertices %d triangles; edges boundary %d manifold %d non-manifold %d; triangles facing no eye %d (reference %d), against "
          "their vertex normals %d; "
          "xyz %.3f weight %.3f normal %.3f of the bound, normals left out %.4f; vertex distance to the scene in voxels, median / p95: "
          "device %.4f / %.4f, reference %.4f / %.4f" % (m["count"], m["faces"].shape[0], stats["boundary"], stats["manifold"], stats["non_manifold"],
                                                         int((facing <= 0).sum()), int((facing_ref <= 0).sum()), int((on_normal_side <= 0).sum()),
                                                         fig["xyz_ratio"], fig["weight_ratio"], fig["normal_ratio"],
                                                         fig["normal_left_out"], med, p95, med_r, p95_r))
    assert m["count"] > 5000 and m["faces"].shape[0] > 10000
    assert stats["non_manifold"] == 0
    assert np.all(on_normal_side > 0)
    assert np.all(facing[facing_ref > CLEAR] > 0)
    assert med <= MARGIN * med_r and p95 <= MARGIN * p95_r
