"""CPU: the surface-net reference of tests/tsdf_mesh_ref.py checks itself -- the properties of the mesh it defines on a fully observed
sphere (its own figures, recorded below), what an unobserved block does to it, the numpy-fp32 stand-in under ``compare``, every listed
mistake rejected, and the PLY writer / reader with faces.

The reference's own figures on the sphere (radius 0.37 m, 40^3 voxels of 3 cm, centre a few millimetres off the grid):
    2858 vertices, 5712 triangles, 8568 mesh edges, every one shared by exactly two triangles; Euler number 2; every triangle's geometric
    normal on the side of its vertices' normals; enclosed volume 0.99249 of 4/3 pi r^3; vertices at most 0.0295 voxel off the sphere;
    no normal left out; the fp32 stand-in at 0.40 / 0.13 of the xyz / normal bounds."""
import numpy as np
import pytest

import tsdf_mesh_ref as M


@pytest.fixture(scope="module")
def sphere():
    D, W, origin, centre = M.sphere_volume()
    return D, W, origin, centre, M.mesh(D, W, M.W_MIN, M.VOXEL, origin)


def test_the_sphere_is_closed_oriented_and_close(sphere):
    D, W, origin, centre, r = sphere
    boundary, manifold, non_manifold, euler = M.edge_stats(r["faces"])
    assert r["count"] == 2858 and r["faces"].shape == (5712, 3) and r["edge"].shape == (2856,)
    assert (boundary, manifold, non_manifold, euler) == (0, 8568, 0, 2)
    assert np.unique(r["faces"]).shape[0] == r["count"]
    nrm, cen = M.triangle_normals(r["xyz"], r["faces"])
    assert np.all(np.einsum("ij,ij->i", nrm, r["normal"][r["faces"]].sum(1)) > 0)
    assert np.all(np.einsum("ij,ij->i", nrm, cen - centre) > 0)                     # outwards: the free side
    vol = M.enclosed_volume(r["xyz"], r["faces"]) / (4.0 / 3.0 * np.pi * M.SPHERE_R ** 3)
    off = np.abs(np.linalg.norm(r["xyz"] - centre, axis=1) - M.SPHERE_R).max() / M.VOXEL
    print("MESH-REF sphere: volume %.5f of the analytic one, vertices <= %.4f voxel off the sphere" % (vol, off))
    assert 0.98 < vol < 1.0                     # chords of a convex body lie inside it; 2 % is (voxel / r)^2 = 0.66 % three times over
    assert off <= 0.05                          # the mean of crossings of a surface with curvature 1 / r: (voxel / r) / 2 = 0.04 voxel per edge
    assert np.all(r["normal_ok"])
    assert np.all(np.abs(np.linalg.norm(r["normal"], axis=1) - 1) < 1e-12)
    assert np.array_equal(r["cell"], np.sort(r["cell"])) and np.array_equal(r["edge"], np.sort(r["edge"]))
    assert np.allclose(r["weight"], 3.0)


def test_an_unobserved_block_opens_a_boundary_and_nothing_else(sphere):
    D, W, origin, centre, full = sphere
    D, W, origin, _ = M.sphere_volume(hole=(18, 24, 5, 12, 16, 25))
    r = M.mesh(D, W, M.W_MIN, M.VOXEL, origin)
    boundary, manifold, non_manifold, euler = M.edge_stats(r["faces"])
    print("MESH-REF hole: %d vertices, %d triangles, %d boundary edges" % (r["count"], r["faces"].shape[0], boundary))
    assert 0 < r["count"] < full["count"] and boundary > 0 and non_manifold == 0
    assert euler == 1                           # a sphere with one hole is a disc
    assert set(r["cell"]) < set(full["cell"]) and set(r["edge"]) < set(full["edge"])


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_the_fp32_stand_in_meets_compare(name):
    c = M.build_case(name)
    ref = M.reference(c)
    fig = M.compare(M.reference(c, dtype=np.float32), ref, name)
    print("MESH-REF stand-in %s: %s" % (name, fig))
    assert fig["normal_left_out"] <= M.AMB_CAP
    if name in ("unobserved", "positive"):
        assert fig["vertices"] == 0 and fig["faces"] == 0
    elif name == "2x2x2":
        assert fig["vertices"] == 1 and fig["faces"] == 0
    else:
        assert fig["vertices"] >= 2


def test_the_zero_case_has_exact_zeros_on_crossing_edges():
    c = M.build_case("d1-zero")
    D = c["D"]
    assert np.any((D[:, :, :-1] < 0) & (D[:, :, 1:] == 0)) and np.any((D[:, :, :-1] == 0) & (D[:, :, 1:] < 0))
    assert np.signbit(D[2, 3, 4]) and D[2, 3, 4] == 0


@pytest.mark.parametrize("mistake", M.MISTAKES)
def test_compare_rejects_the_mistake(mistake):
    rejected = []
    for name in sorted(M.CASES):
        c = M.build_case(name)
        try:
            M.compare(M.reference(c, dtype=np.float32, mistake=mistake), M.reference(c), name)
        except AssertionError:
            rejected.append(name)
    print("MESH-REF mistake %s rejected on %s" % (mistake, rejected))
    assert rejected


def test_a_perturbed_attribute_fails_compare():
    c = M.build_case("colour")
    ref = M.reference(c)
    for key, ulps in (("xyz", 64), ("weight", 64), ("normal", 64), ("color", 256)):
        got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in M.reference(c, dtype=np.float32).items()}
        got[key] = got[key] * np.float32(1 + ulps * 2.0 ** -23)
        with pytest.raises(AssertionError):
            M.compare(got, ref, key)


def test_ply_round_trip_with_faces(sphere, tmp_path):
    from estdepth_amd.fusion3d import read_ply, write_ply
    r = sphere[4]
    rec = np.concatenate([r["xyz"], r["normal"]], 1).astype(np.float32)
    rgb = (np.arange(rec.shape[0] * 3) % 251).astype(np.uint8).reshape(-1, 3)
    for colour in (None, rgb):
        path = str(tmp_path / "mesh.ply")
        write_ply(path, rec, colour, faces=r["faces"])
        back = read_ply(path, faces=True)
        assert back["faces"].dtype == np.int32 and np.array_equal(back["faces"], r["faces"])
        assert np.array_equal(back["xyz"], rec[:, :3]) and np.array_equal(back["normal"], rec[:, 3:])
        assert (back["rgb"] is None) if colour is None else np.array_equal(back["rgb"], rgb)
        assert sorted(read_ply(path)) == ["normal", "rgb", "xyz"]                    # the default return value has no faces
    write_ply(path, rec)
    assert read_ply(path, faces=True)["faces"].shape == (0, 3)
    with pytest.raises(RuntimeError):
        write_ply(path, rec, faces=np.array([[0, 1, rec.shape[0]]]))


def test_read_ply_refuses_other_list_lengths(tmp_path):
    from estdepth_amd.fusion3d import read_ply
    head = "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n" \
           "property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n"
    quad, tri = tmp_path / "quad.ply", tmp_path / "tri.ply"
    quad.write_text(head + "4 0 1 2 3\n")
    tri.write_text(head + "3 0 1 2\n")
    assert np.array_equal(read_ply(str(tri), faces=True)["faces"], [[0, 1, 2]])
    assert read_ply(str(quad))["xyz"].shape == (4, 3)
    with pytest.raises(RuntimeError):
        read_ply(str(quad), faces=True)
    binary = tmp_path / "quad_bin.ply"
    binary.write_bytes(head.replace("ascii", "binary_little_endian").split("end_header\n")[0].encode() + b"end_header\n"
                       + np.zeros(12, "<f4").tobytes() + bytes([4]) + np.arange(4, dtype="<i4").tobytes())
    with pytest.raises(RuntimeError):
        read_ply(str(binary), faces=True)


def test_write_ply_without_faces_is_byte_identical(tmp_path):
    """the file of today's write_ply, spelled out: header and body literal"""
    from estdepth_amd.fusion3d import write_ply
    rec = np.array([[0.0, 1.0, -2.0, 0.0, 0.0, 1.0], [0.5, 0.25, 4.0, 1.0, 0.0, 0.0]], np.float32)
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
            b"property float nx\nproperty float ny\nproperty float nz\n")
    body = bytes.fromhex("000000000000803f000000c000000000000000000000803f" "0000003f0000803e00008040" "0000803f0000000000000000")
    path = str(tmp_path / "points.ply")
    write_ply(path, rec)
    assert open(path, "rb").read() == head + b"end_header\n" + body
    write_ply(path, rec, np.array([[1, 2, 3], [254, 0, 9]], np.uint8))
    assert open(path, "rb").read() == (head + b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
                                       + body[:24] + bytes([1, 2, 3]) + body[24:] + bytes([254, 0, 9]))
    write_ply(path, rec, faces=np.array([[0, 1, 1]], np.int32))
    assert open(path, "rb").read() == (head + b"element face 1\nproperty list uchar int vertex_indices\nend_header\n" + body
                                       + bytes([3]) + np.array([0, 1, 1], "<i4").tobytes())
