"""The host layer of the mesh sampling on the device: ``fusion3d.mesh_area`` / ``sample_mesh``, ``cloud_metrics.compare_meshes`` and
``TSDFVolume.compare(sample=)`` against the reference of tests/mesh_sample_ref.py (the kernels' own cases: tests/test_gpu_mesh_sample_routes.py).
Repeated calls and both bindings give the same bits; the refusals name the operator and the argument; a wall as two triangles scores as
a wall once it is sampled."""
import math

import numpy as np
import pytest
import torch

from estdepth_amd.cloud_metrics import compare_clouds, compare_meshes
from estdepth_amd.fusion3d import mesh_area, sample_mesh

import mesh_sample_ref as S
import tsdf_mesh_ref as M
from test_gpu_mesh_sample_routes import ALL, AREA_ONLY, profiled
from test_gpu_recon3d_routes import _cpu, _dev, _same, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _mesh(name, on_device=False):
    xyz, faces, attrs, n, seed = S.build_case(name)
    mesh = dict(xyz=xyz, faces=faces)
    if on_device:
        mesh = {k: _dev(v) for k, v in mesh.items()}
    return mesh, attrs, n, seed


@pytest.mark.parametrize("name", ["one-257", "f65-n1000-seed", "zero-area", "spheres"])
def test_repeated_calls_and_both_bindings_give_the_same_bits(name):
    mesh, _, n, seed = _mesh(name, on_device=True)
    first = under("torch", lambda: sample_mesh(mesh, n=n, seed=seed))
    for binding in ("torch", "ctypes", "ctypes"):
        again = under(binding, lambda: sample_mesh(mesh, n=n, seed=seed))
        assert sorted(again) == sorted(first) == ["area", "bary", "face", "invalid", "n", "normal", "total", "xyz"]
        for k, v in first.items():
            assert _same(v, again[k]) if isinstance(v, torch.Tensor) else v == again[k], "%s: %s differs (%s)" % (name, k, binding)


@pytest.mark.parametrize("where", ["d64", "d64-rotated", "d512"])
def test_the_kernels_away_from_the_origin(where):
    """the 65-face mesh with three attribute channels built 64 m and 512 m out and in the turned world (tests/placement.py) through the
    unchanged comparison: areas and face normals from edge vectors (the differences of nearby coordinates are exact), positions within
    the bound that follows their magnitude, at most 3 % of the normals left out"""
    import placement as PL
    from estdepth_amd import ops
    from test_gpu_mesh_sample_routes import as_got
    host = S.placed_case(PL.PLACES[where])
    xyz, faces, attrs, n, seed = host
    out = ops.mesh_sample(_dev(xyz), _dev(faces), _dev(attrs), n, seed)
    fa = ops.mesh_face_area(_dev(xyz), _dev(faces))
    fig = S.compare(as_got(out, fa[1]), *host, "%s@%s" % (S.PLACED_CASE, where))
    print("PLACEMENT mesh_sample %s@%s: of the bounds: area %.3f face normal %.3f position %.3f attributes %.3f; %d of %d normals left out"
          % (S.PLACED_CASE, where, fig["area"], fig["face_normal"], fig["xyz"], fig["attrs"], fig["left_out"], fig["faces"]))
    assert fig["samples"] == n and float(np.abs(xyz).min()) > PL.PLACES[where][0] / 4


def test_sample_mesh_of_a_host_mesh_with_normals_and_colour():
    """numpy arrays as read_ply returns them: uint8 rgb becomes float32 color, normals='vertex' interpolates and normalises"""
    xyz, faces, nrm, n, seed = S.build_case("spheres")
    rgb = np.random.default_rng(3).integers(0, 256, (xyz.shape[0], 3)).astype(np.uint8)
    mesh = dict(xyz=xyz, faces=faces, normal=nrm, rgb=rgb)
    out = profiled(ALL, lambda: sample_mesh(mesh, n=n, seed=seed, normals="vertex"))
    assert out["n"] == n and out["invalid"] == 0 and out["xyz"].device.type == "cuda" and out["color"].shape == (n, 3)
    attrs = np.concatenate([nrm, rgb.astype(np.float32)], 1)
    ref = S.sample(xyz, faces, attrs, n, seed, area=_cpu(out["area"]))
    assert np.array_equal(_cpu(out["face"]), ref["face"]) and np.array_equal(_cpu(out["bary"]), ref["bary"])
    assert S._worst(_cpu(out["xyz"]).astype(np.float64) - ref["xyz"], ref["xyz_bound"]) <= S.ROUTE
    assert S._worst(_cpu(out["color"]).astype(np.float64) - ref["attrs"][:, 3:], ref["attrs_bound"][:, 3:]) <= S.ROUTE
    want = ref["attrs"][:, :3] / np.linalg.norm(ref["attrs"][:, :3], axis=1, keepdims=True)
    got = _cpu(out["normal"]).astype(np.float64)
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() < 1e-6 and np.abs(got - want).max() < 1e-6
    assert abs(out["total"] - ref["area"].sum()) <= 1e-12 * out["total"]
    # face normals by default; a point of a sphere's mesh has its triangle's normal within the triangle's angular size of the radial one
    face = sample_mesh(mesh, n=n, seed=seed)
    assert _same(face["xyz"], out["xyz"]) and _same(face["color"], out["color"])
    assert float((face["normal"] * out["normal"]).sum(1).min()) > 0.99


def test_density_gives_the_ceiling_of_density_times_area():
    mesh, _, _, _ = _mesh("f65-n1000")
    area = profiled(AREA_ONLY, lambda: mesh_area(mesh))
    ref = S.face_area(mesh["xyz"], mesh["faces"])
    assert area["invalid"] == 0 and area["area"].dtype == torch.float64 and abs(area["total"] - ref["area"].sum()) <= 1e-12 * area["total"]
    assert S._worst(_cpu(area["area"]) - ref["area"], ref["area_bound"]) <= S.ROUTE
    for density in (0.5, 37.0, 1e3):
        out = sample_mesh(mesh, density=density, seed=5)
        assert out["n"] == S.n_for_density(density, area["total"]) == out["xyz"].shape[0] and out["total"] == area["total"]
        assert _same(out["xyz"], sample_mesh(mesh, n=out["n"], seed=5)["xyz"])
    bad, _, _, _ = _mesh("out-of-range")
    assert mesh_area(bad)["invalid"] == 6 and sample_mesh(bad, n=10)["invalid"] == 6
    empty = sample_mesh(dict(xyz=mesh["xyz"], faces=np.zeros((0, 3), np.int32)), density=10.0)
    assert empty["n"] == 0 and empty["xyz"].shape == (0, 3) and empty["total"] == 0.0


def test_the_refusals_name_the_operator_and_the_argument():
    mesh, _, _, _ = _mesh("f65-n1000")
    flat = dict(xyz=mesh["xyz"] * np.asarray([1, 0, 0], np.float32), faces=mesh["faces"])
    with pytest.raises(RuntimeError, match="mesh_sample: the mesh has no area to put n_samples = 10 samples on"):
        sample_mesh(flat, n=10)
    assert sample_mesh(flat, density=100.0)["n"] == 0                      # no area, no points asked for
    few = dict(xyz=np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (1e-5, 0, 0), (0, 1e-5, 0)], np.float32),
               faces=np.asarray([(0, 1, 2)] + [(3, 4, 5)] * 4095, np.int32))
    with pytest.raises(RuntimeError, match="mesh_sample: n_samples = 2147483647 leaves strata of 26[0-9]{4} units of area, fewer than 1048576"):
        sample_mesh(few, n=2 ** 31 - 1)
    nan = mesh["xyz"].copy()
    nan[7, 1] = np.inf
    for fn in (lambda m: sample_mesh(m, n=10), mesh_area):
        with pytest.raises(RuntimeError, match="(sample_mesh|mesh_area): xyz holds a coordinate that is not finite"):
            fn(dict(xyz=nan, faces=mesh["faces"]))
    with pytest.raises(RuntimeError, match="sample_mesh: exactly one of n and density must be given"):
        sample_mesh(mesh)
    with pytest.raises(RuntimeError, match="sample_mesh: exactly one of n and density must be given"):
        sample_mesh(mesh, n=10, density=2.0)
    with pytest.raises(RuntimeError, match="sample_mesh: normal and color must be \\[72,3\\]"):
        sample_mesh(dict(mesh, color=np.zeros((5, 3), np.float32)), n=10)


def _wall():
    """a 4 m x 3 m wall as two triangles"""
    return dict(xyz=np.asarray([(0, 0, 2.6), (4, 0, 2.6), (4, 3, 2.6), (0, 3, 2.6)], np.float32), faces=np.asarray([(0, 1, 2), (0, 2, 3)], np.int32))


def test_a_wall_of_two_triangles_scores_as_a_wall():
    """a dense cloud lying exactly on the wall: against the wall's four vertices its accuracy is metres and nothing is precise; against
    the wall sampled at the cloud's density it is the spacing of the samples"""
    wall = _wall()
    g = np.stack(np.meshgrid(np.arange(0.01, 4, 0.02), np.arange(0.01, 3, 0.02)), -1).reshape(-1, 2)
    cloud = dict(xyz=np.concatenate([g, np.full((g.shape[0], 1), 2.6)], 1).astype(np.float32))
    by_vertex = compare_clouds(_dev(cloud["xyz"]), _dev(wall["xyz"]), threshold=0.05, max_dist=5.0)
    assert by_vertex["accuracy"] > 1.0 and by_vertex["precision"] < 0.01 and by_vertex["recall"] == 1.0
    s = profiled(ALL, lambda: compare_meshes(cloud, wall, 2500.0, threshold=0.05, max_dist=5.0))
    assert s["sampled"] == dict(density=2500.0, n_pred=g.shape[0], n_gt=30000, area_pred=None, area_gt=12.0, invalid_pred=0, invalid_gt=0)
    assert s["accuracy"] < 0.02 and s["completeness"] < 0.02 and s["precision"] == 1.0 and s["recall"] == 1.0 and s["fscore"] == 1.0
    assert s["n_gt"] == 30000 and s["n_pred"] == g.shape[0]
    # both sides meshes: the same wall shifted by 3 cm along its normal is 3 cm away, and the face normals agree
    shifted = dict(xyz=wall["xyz"] + np.asarray([0, 0, 0.03], np.float32), faces=wall["faces"])
    m = compare_meshes(shifted, wall, 2500.0, seed=3)
    assert m["sampled"]["n_pred"] == m["sampled"]["n_gt"] == 30000 and m["sampled"]["area_pred"] == 12.0
    assert 0.0299 <= m["accuracy"] < 0.0301 and 0.0299 <= m["completeness"] < 0.0301 and m["normal_consistency"] == 1.0
    # the same seed on both sides of an identical mesh: the same points
    same = compare_meshes(wall, wall, 100.0)
    assert same["accuracy"] == 0.0 and same["completeness"] == 0.0


@pytest.fixture(scope="module")
def sphere():
    from estdepth_amd.fusion3d import TSDFVolume
    D, W, origin, centre = M.sphere_volume()
    vol = TSDFVolume(D.shape, M.VOXEL, origin, device=DEV)
    vol.volume.copy_(_dev(np.stack([D, W])))
    return vol, centre, M.mesh(D, W, M.W_MIN, M.VOXEL, origin)


def test_the_area_and_the_samples_of_a_fused_sphere(sphere):
    """extract_mesh of the fully observed 0.37 m sphere: its area is 4 pi r^2 less the deficit the float64 reference mesh itself has
    (a surface-net mesh cuts corners), within 1 % of the sphere; every sample lies between the spheres its triangle's vertices allow:
    for p = sum l_i v_i, |p - c|^2 = sum l_i |v_i - c|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2 >= min |v - c|^2 - L^2 / 3 (L the longest edge)"""
    vol, centre, ref = sphere
    mesh = vol.extract_mesh()
    sphere_area = 4 * math.pi * M.SPHERE_R ** 2
    ref_area = S.face_area(ref["xyz"].astype(np.float32), ref["faces"])["area"].sum()
    area = mesh_area(mesh)
    deficit = 1.0 - ref_area / sphere_area
    print("MESH-SAMPLE sphere: area %.6f m2, reference mesh %.6f, sphere %.6f (deficit %.4f)" % (area["total"], ref_area, sphere_area, deficit))
    assert area["invalid"] == 0 and 0 <= deficit < 0.05 and abs(area["total"] / sphere_area - (1.0 - deficit)) <= 0.01
    s = sample_mesh(mesh, density=1.0 / M.VOXEL ** 2, seed=1)
    assert s["n"] == S.n_for_density(1.0 / M.VOXEL ** 2, area["total"])
    xyz, faces = _cpu(mesh["xyz"]).astype(np.float64), _cpu(mesh["faces"]).astype(np.int64)
    tri = xyz[faces[_cpu(s["face"])]]
    r_v = np.linalg.norm(tri - centre, axis=2)
    edge = np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=2).max(1)
    r = np.linalg.norm(_cpu(s["xyz"]).astype(np.float64) - centre, axis=1)
    assert (r <= r_v.max(1) + 1e-6).all() and (r >= np.sqrt(r_v.min(1) ** 2 - edge ** 2 / 3.0) - 1e-6).all()
    assert np.abs(r - M.SPHERE_R).max() < 0.5 * M.VOXEL


def test_volume_compare_with_sample(sphere):
    """TSDFVolume.compare(sample=): the volume against the reference mesh of the same volume, both sampled, is well within a voxel; the
    default path launches nothing of this"""
    vol, _, ref = sphere
    gt = dict(xyz=ref["xyz"].astype(np.float32), faces=ref["faces"].astype(np.int32))
    plain = profiled(set(), lambda: vol.compare(dict(xyz=gt["xyz"])))
    s = profiled(ALL, lambda: vol.compare(gt, sample=1.0 / M.VOXEL ** 2))
    assert abs(s["n_pred"] - s["n_gt"]) <= 1 and s["n_gt"] > 1000 and s["accuracy"] < 0.1 * M.VOXEL and s["completeness"] < 0.1 * M.VOXEL and s["fscore"] == 1.0
    assert s["normal_consistency"] > 0.999
    assert plain["n_gt"] == gt["xyz"].shape[0] and _same_dict(plain, vol.compare(dict(xyz=gt["xyz"]), sample=None))


def _same_dict(a, b):
    return sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
