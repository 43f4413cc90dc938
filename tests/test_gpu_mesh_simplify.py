"""Mesh simplification as a feature (fusion3d.simplify_mesh, TSDFVolume.extract_mesh(simplify=) / save_mesh(simplify=)): the box and the
noisy sphere of tests/test_mesh_simplify_ref_cpu.py equal the numpy reference bit for bit, host glue included; the mean placement is
voxel_downsample's; numpy and device inputs agree; the error paths raise; the default extract_mesh() is what it was -- no new kernel,
the same bits -- and a simplified surface-net mesh stays within one cell of the unsimplified one.  The kernels themselves are covered
case by case in tests/test_gpu_mesh_simplify_routes.py."""
import numpy as np
import pytest
import torch

from estdepth_amd.fusion3d import simplify_mesh

import mesh_components_ref as C
import mesh_simplify_ref as R
import tsdf_mesh_ref as M
from test_gpu_mesh_simplify_routes import ALL, profiled
from test_gpu_recon3d_routes import _dev, _same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACES_ONLY = {"mesh_cluster_faces_kernel"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _got(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _equals_reference(out, want, what):
    got = _got(out)
    n = R.compare(got, want, what, keys=("faces", "xyz", "normal", "placed", "cluster", "cell_key"))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["count"] == want["stats"]["vertices"] and got["faces"].dtype == np.int32 and got["cluster"].dtype == np.int32
    return n


@pytest.fixture(scope="module")
def box():
    xyz, faces = R.box()
    return xyz, faces, (xyz.min(0).astype(np.float64) - 0.013).astype(np.float32)


def test_the_box_equals_the_reference(box):
    xyz, faces, origin = box
    out = profiled(ALL, lambda: simplify_mesh({"xyz": xyz, "faces": faces}, 0.1, origin=origin))
    want = R.simplify(xyz, faces, 0.1, origin)
    n = _equals_reference(out, want, "box")
    from estdepth_amd.fusion3d import mesh_edge_stats
    e = mesh_edge_stats(out["faces"])
    assert out["stats"]["vertices"] == 288 and out["stats"]["faces"] == 572 and out["stats"]["fallback"] == 0
    assert e == dict(boundary=0, manifold=858, non_manifold=0, euler=2)
    worst = R.box_distance(out["xyz"].cpu().numpy()).max()
    print("MESH-SIMPLIFY box: %d values equal to the reference's bits; %s; at most %.3e m off the box" % (n, out["stats"], worst))
    assert sorted(out) == ["cell_key", "cluster", "count", "faces", "normal", "placed", "stats", "xyz"]


@pytest.mark.parametrize("where", ["d64", "d64-rotated", "d512"])
def test_a_placed_patch_equals_the_reference(where):
    """the 257-face patch built 64 m and 512 m out and in the turned world (tests/placement.py; "offset-1000" of the route suite adds its
    offset to fp32 data), the grid's corner moved with it: the cell keys are relative to that corner and the quadrics are accumulated in
    float64 about the cell centres, so the result is the reference's TO THE BIT, as everywhere in this family"""
    import placement as PL
    place = PL.PLACES[where]
    xyz, faces = R.patch(R.PLACED_FACES, place=place)
    origin = (xyz.min(0).astype(np.float64) - 0.013).astype(np.float32)
    for org, what in ((None, "the box's corner"), (origin, "a corner of the caller's")):
        out = simplify_mesh({"xyz": xyz, "faces": faces}, 0.1, origin=org)
        want = R.simplify(xyz, faces, 0.1, org)
        n = _equals_reference(out, want, "patch-%d@%s, %s" % (R.PLACED_FACES, where, what))
        print("PLACEMENT mesh_simplify patch-%d@%s (%s): %d values equal to the reference's bits; %s" % (R.PLACED_FACES, where, what, n, out["stats"]))
        assert 10 < out["stats"]["vertices"] < xyz.shape[0] and out["stats"]["faces"] > 10 and float(np.abs(xyz).min()) > place[0] / 4


def test_the_noisy_sphere_equals_the_reference():
    xyz, faces = R.noisy_sphere()
    rng = np.random.RandomState(4)
    mesh = {"xyz": _dev(xyz), "faces": _dev(faces), "weight": _dev(rng.uniform(1, 9, xyz.shape[0]).astype(np.float32)),
            "color": _dev(rng.uniform(0, 1, xyz.shape).astype(np.float32)), "cell": torch.arange(xyz.shape[0], device=DEV), "edge": None}
    out = profiled(ALL, lambda: simplify_mesh(mesh, 0.04))
    attrs = np.concatenate([mesh["weight"].cpu().numpy()[:, None], mesh["color"].cpu().numpy()], 1)
    want = R.simplify(xyz, faces, 0.04, attrs=attrs)
    n = _equals_reference(out, want, "noisy sphere")
    assert out["stats"]["duplicates"] > 0 and 0 < out["stats"]["fallback"] < out["count"] / 4
    assert np.array_equal(R.bits(out["weight"].cpu().numpy()), R.bits(want["attrs"][:, 0])) and out["weight"].shape == (out["count"],)
    assert np.array_equal(R.bits(out["color"].cpu().numpy()), R.bits(want["attrs"][:, 1:]))
    assert "cell" not in out and "edge" not in out and "rgb" not in out
    again = simplify_mesh(mesh, 0.04)
    assert all(torch.equal(out[k], again[k]) if out[k].dtype == torch.bool else _same(out[k], again[k]) for k in out if isinstance(out[k], torch.Tensor))
    print("MESH-SIMPLIFY noisy sphere: %d values equal to the reference's bits; %s" % (n, out["stats"]))


def test_mean_placement_is_voxel_downsample(box):
    from estdepth_amd.cloud_metrics import voxel_downsample
    xyz, faces = R.noisy_sphere()
    normal = (xyz - np.asarray([0.41, 0.43, 0.39], np.float32)) / np.float32(0.37)
    rng = np.random.RandomState(6)                                          # seven attribute columns: more than one centroid call takes
    weight, color = rng.uniform(1, 9, xyz.shape[0]).astype(np.float32), rng.uniform(0, 255, xyz.shape).astype(np.float32)
    out = profiled(FACES_ONLY, lambda: simplify_mesh({"xyz": xyz, "faces": faces, "normal": normal.astype(np.float32), "weight": weight, "color": color},
                                                     0.04, placement="mean"))
    attrs = R.simplify(xyz, faces, 0.04, placement="mean", attrs=np.concatenate([weight[:, None], color, normal.astype(np.float32)], 1))["attrs"]
    assert np.array_equal(R.bits(out["weight"].cpu().numpy()), R.bits(attrs[:, 0])) and np.array_equal(R.bits(out["color"].cpu().numpy()), R.bits(attrs[:, 1:4]))
    unit = attrs[:, 4:7].astype(np.float64) / np.linalg.norm(attrs[:, 4:7].astype(np.float64), axis=1, keepdims=True)
    assert np.abs(out["normal"].cpu().numpy() - unit).max() < 1e-6
    pts, _, counts = voxel_downsample(_dev(xyz), 0.04)
    assert _same(out["xyz"], pts) and out["count"] == pts.shape[0]
    assert np.array_equal(np.bincount(out["cluster"].cpu().numpy()), counts.cpu().numpy())
    want = R.simplify(xyz, faces, 0.04, placement="mean")
    _equals_reference({k: v for k, v in out.items() if k != "normal"}, want, "mean placement")
    assert not out["placed"].any() and out["stats"]["placed"] == 0 and out["stats"]["fallback"] == 0
    n = out["normal"].cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    quadric = simplify_mesh({"xyz": xyz, "faces": faces}, 0.04)
    assert _same(quadric["faces"], out["faces"]) and _same(quadric["cluster"], out["cluster"])


def test_numpy_and_device_inputs_agree(box):
    xyz, faces, origin = box
    a = simplify_mesh({"xyz": xyz, "faces": faces.astype(np.int64)}, 0.05, origin=origin.tolist())
    b = simplify_mesh({"xyz": _dev(xyz), "faces": _dev(faces)}, 0.05, origin=torch.from_numpy(origin))
    assert a["stats"] == b["stats"] and a["stats"]["vertices"] == 1260 and a["stats"]["faces"] == 2516
    assert all(torch.equal(a[k], b[k]) if a[k].dtype == torch.bool else _same(a[k], b[k]) for k in a if isinstance(a[k], torch.Tensor))
    assert all(v.is_cuda for v in a.values() if isinstance(v, torch.Tensor))


def test_an_empty_mesh_and_a_mesh_without_faces():
    none = simplify_mesh({"xyz": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.int32)}, 0.1)
    assert none["count"] == 0 and none["xyz"].shape == (0, 3) and none["faces"].shape == (0, 3) and none["stats"]["vertices"] == 0
    xyz = np.asarray([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.5, 0.5, 0.5]], np.float32)
    loose = profiled(set(), lambda: simplify_mesh({"xyz": xyz, "faces": np.zeros((0, 3), np.int32)}, 0.1))
    want = R.simplify(xyz, np.zeros((0, 3), np.int32), 0.1)
    _equals_reference(loose, want, "no faces")
    assert loose["count"] == 2 and not loose["placed"].any() and not loose["normal"].any()


def test_the_error_paths_raise(box):
    xyz, faces, origin = box
    mesh = {"xyz": xyz, "faces": faces}
    bad = faces.copy()
    bad[7, 1] = xyz.shape[0]
    for call, text in ((lambda: simplify_mesh(mesh, 0.0), "cell"), (lambda: simplify_mesh(mesh, float("nan")), "cell"),
                       (lambda: simplify_mesh(mesh, -0.1), "cell"), (lambda: simplify_mesh(mesh, "0.1"), "cell"),
                       (lambda: simplify_mesh(mesh, 1e-7), "1e-07"),                       # too many cells per axis: the message names the cell
                       (lambda: simplify_mesh(mesh, 0.1, placement="median"), "placement"), (lambda: simplify_mesh(mesh, 0.1, reg=-1.0), "reg"),
                       (lambda: simplify_mesh(mesh, 0.1, reg=float("inf")), "reg"), (lambda: simplify_mesh(mesh, 0.1, origin=[0.0, 0.0]), "origin"),
                       (lambda: simplify_mesh(mesh, 0.1, origin=[0.5, 0.0, 0.0]), "origin"),   # above the bounding box's minimum
                       (lambda: simplify_mesh(mesh, 0.1, origin=[float("nan"), 0.0, 0.0]), "origin"),
                       (lambda: simplify_mesh({"xyz": xyz}, 0.1), "faces"), (lambda: simplify_mesh({"xyz": xyz, "faces": bad}, 0.1), "1 of 15732 faces"),
                       (lambda: simplify_mesh({"xyz": xyz, "faces": faces, "weight": np.ones(5, np.float32)}, 0.1), "weight"),
                       (lambda: simplify_mesh({"xyz": np.full((3, 3), np.inf, np.float32), "faces": faces[:1] * 0}, 0.1), "finite")):
        with pytest.raises(RuntimeError) as e:
            profiled(set(), call)
        assert text in str(e.value) and "simplify_mesh" in str(e.value), (text, str(e.value))


@pytest.fixture(scope="module")
def two_spheres():
    from estdepth_amd.fusion3d import TSDFVolume
    D, W, origin, centre = C.two_sphere_volume()
    vol = TSDFVolume(D.shape, M.VOXEL, origin, device=DEV)
    vol.volume.copy_(_dev(np.stack([D, W])))
    return vol


def test_the_default_extract_mesh_is_what_it_was(two_spheres):
    from estdepth_amd import ops
    from estdepth_amd.fusion3d import sorted_mesh
    vol = two_spheres
    m = profiled(set(), lambda: vol.extract_mesh())                         # no mesh_cluster_* kernel
    direct = sorted_mesh(ops.tsdf_mesh_vertices, ops.tsdf_mesh_faces, vol.volume, None, vol.voxel_size, vol.origin, 1.0)
    assert sorted(m) == sorted(direct) == ["cell", "count", "edge", "faces", "normal", "weight", "xyz"]
    assert m["count"] == direct["count"] == 1998 and m["faces"].shape == (3988, 3)
    assert all(_same(m[k], direct[k]) for k in m if k != "count")
    none = profiled(set(), lambda: vol.extract_mesh(simplify=None, min_component=0))
    assert all(_same(m[k], none[k]) for k in m if k != "count")


def test_a_simplified_surface_net_mesh_stays_within_a_cell(two_spheres, tmp_path):
    from estdepth_amd.cloud_metrics import point_mesh_distance
    from estdepth_amd.fusion3d import read_ply
    vol = two_spheres
    cell = 2 * M.VOXEL
    full = vol.extract_mesh()
    out = profiled(ALL, lambda: vol.extract_mesh(simplify=cell))
    want = R.simplify(full["xyz"].cpu().numpy(), full["faces"].cpu().numpy(), cell, np.asarray(vol.origin, np.float32))
    _equals_reference(out, want, "two spheres")
    assert 0 < out["faces"].shape[0] < full["faces"].shape[0] and out["count"] < full["count"]
    assert "cell" not in out and "edge" not in out and out["weight"].shape == (out["count"],)
    dist, _ = point_mesh_distance(out["xyz"], {"xyz": full["xyz"], "faces": full["faces"]}, max_dist=1.0)
    print("MESH-SIMPLIFY two spheres, cell %.3f: %d -> %d vertices, %d -> %d faces (%s); at most %.4f m from the unsimplified mesh"
          % (cell, full["count"], out["count"], full["faces"].shape[0], out["faces"].shape[0], out["stats"], float(dist.max())))
    assert float(dist.max()) <= cell
    kept = vol.extract_mesh(min_component=229, simplify=cell)                # after the filter: the small sphere is gone before anything welds
    assert kept["dropped"]["faces"] == 228 and kept["components"] == 1 and kept["stats"]["faces_in"] == 3760
    n_v, n_f = vol.save_mesh(str(tmp_path / "s.ply"), simplify=cell)
    ply = read_ply(str(tmp_path / "s.ply"), faces=True)
    assert (n_v, n_f) == (out["count"], out["faces"].shape[0]) and np.array_equal(ply["faces"], out["faces"].cpu().numpy())
    assert np.array_equal(ply["xyz"], out["xyz"].cpu().numpy())
