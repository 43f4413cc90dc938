"""CPU: the reference of the mesh-components contract (tests/mesh_components_ref.py) against answers written by hand and against scipy, the
mistakes its comparison must reject, the two-sphere volume whose numbers the GPU suite builds on, and the argument checks of
``fusion3d.mesh_components`` / ``fusion3d.filter_mesh`` and of the ctypes front end that need no device."""
import numpy as np
import pytest
import torch

import mesh_components_ref as C
import tsdf_mesh_ref as M


def _ref(faces, V):
    r = C.components(np.asarray(faces, np.int64).reshape(-1, 3), V)
    return r["label"].tolist(), r["triangles"].tolist(), r["invalid"]


# ------------------------------------------------------------------------------------------------- the reference, by hand
def test_nothing_at_all():
    assert _ref([], 0) == ([], [], 0)


def test_vertices_without_faces_are_their_own_components():
    assert _ref([], 5) == ([0, 1, 2, 3, 4], [0, 0, 0, 0, 0], 0)


def test_one_triangle():
    assert _ref([[2, 0, 1]], 3) == ([0, 0, 0], [1, 0, 0], 0)
    assert _ref([[5, 2, 6]], 7) == ([0, 1, 2, 3, 4, 2, 2], [0, 0, 1, 0, 0, 0, 0], 0)


def test_degenerate_and_duplicated_triangles_count_like_any_other():
    label, tri, bad = _ref([[1, 1, 4], [6, 6, 6], [0, 2, 3], [0, 2, 3], [3, 2, 0], [7, 8, 7]], 10)
    assert label == [0, 1, 0, 0, 1, 5, 6, 7, 7, 9]
    assert tri == [3, 1, 0, 0, 0, 0, 1, 1, 0, 0] and bad == 0


def test_a_chain_links_through_every_vertex_of_a_triangle():
    """(0, 5, 9) and (9, 3, 4) meet in the LAST vertex of the first one: v0-v1 links alone would not join them"""
    label, tri, _ = _ref([[0, 5, 9], [9, 3, 4], [1, 2, 6]], 10)
    assert label == [0, 1, 1, 0, 0, 0, 1, 7, 8, 0] and tri == [2, 1, 0, 0, 0, 0, 0, 0, 0, 0]


def test_out_of_range_triangles_are_counted_and_link_nothing():
    faces, V = C.build_case("out-of-range")
    label, tri, bad = _ref(faces, V)
    assert bad == 6
    assert label == [0, 0, 0, 0, 0, 5, 5, 5, 8, 9, 9, 9]          # 7 and 8 stay apart: (7, 8, -2^31) is ignored
    assert tri == [2, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0]


def test_the_big_cases_have_the_islands_they_were_built_with():
    for name, islands, triangles in (("grid-48", 9, 2 * 16 * 16), ("grid-320", 5, 2 * 64 * 320)):
        roots, tri, verts = C.summary(C.reference(name))
        assert roots.shape[0] == islands and (tri == triangles).all() and (verts == C.build_case(name)[1] // islands).all()
    assert C.build_case("grid-320")[0].shape[0] == 204800
    for name in ("strip-ascending", "strip-descending", "strip-permuted", "star-hub-last", "star-hub-first"):
        roots, tri, verts = C.summary(C.reference(name))
        assert roots.tolist() == [0] and tri.tolist() == [C.build_case(name)[0].shape[0]] and verts.tolist() == [C.build_case(name)[1]]
    for n in (63, 64, 65, 255, 256, 257):
        roots, tri, verts = C.summary(C.reference("disjoint-%d" % n))
        assert roots.tolist() == list(range(n)) and (tri == 1).all() and (verts == 3).all()


@pytest.mark.parametrize("name", sorted(C.TSDF_EXPECTED))
def test_surface_net_meshes_have_fragments_and_loose_vertices(name):
    _, tri, _ = C.summary(C.reference(name))
    assert (int((tri > 0).sum()), int((tri == 0).sum())) == C.TSDF_EXPECTED[name]


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_reference_against_scipy(name):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    faces, V = C.build_case(name)
    ref = C.reference(name)
    f = faces.astype(np.int64)
    f = f[((f >= 0) & (f < V)).all(1)]
    graph = sparse.coo_matrix((np.ones(2 * f.shape[0]), (np.r_[f[:, 0], f[:, 0]], np.r_[f[:, 1], f[:, 2]])), shape=(V, V))
    n, lab = connected_components(graph, directed=False) if V else (0, np.zeros(0, np.int64))
    smallest = np.full(n, V, np.int64)
    np.minimum.at(smallest, lab, np.arange(V))
    assert np.array_equal(smallest[lab], ref["label"])
    assert np.array_equal(np.bincount(smallest[lab[f[:, 0]]], minlength=V), ref["triangles"])
    assert ref["invalid"] == faces.shape[0] - f.shape[0]


@pytest.mark.parametrize("mistake", C.MISTAKES)
def test_compare_rejects(mistake):
    caught = []
    for name in sorted(C.CASES):
        faces, V = C.build_case(name)
        got = C.components(faces, V, mistake=mistake)
        try:
            C.compare(got, C.reference(name), name)
        except AssertionError:
            caught.append(name)
    assert caught, "no case tells %s from the contract" % mistake
    print(mistake, "rejected on", caught)


def test_compare_rejects_a_wrong_dtype_and_a_wrong_count():
    ref = C.reference("one-v7")
    good = dict(label=ref["label"].copy(), triangles=ref["triangles"].copy(), invalid=0)
    C.compare(good, ref)
    with pytest.raises(AssertionError):
        C.compare(dict(good, label=good["label"].astype(np.int64)), ref)
    with pytest.raises(AssertionError):
        C.compare(dict(good, invalid=1), ref)


# ------------------------------------------------------------------------------------------------- the two-sphere volume
def test_two_sphere_volume():
    m = C.two_sphere_mesh()
    assert m["count"] == 1998 and m["faces"].shape == (3988, 3)
    roots, tri, verts = C.summary(C.components(m["faces"], m["count"]))
    assert sorted(tri.tolist()) == [228, 3760] and int(verts.sum()) == 1998          # two components, no loose vertex
    boundary, manifold, non_manifold, euler = M.edge_stats(m["faces"])
    assert (boundary, non_manifold, euler) == (0, 0, 4) and manifold == 3988 * 3 // 2


def test_two_sphere_volume_filtered():
    m = C.two_sphere_mesh()
    f = C.filter_mesh(m, min_triangles=229)
    assert f["faces"].shape == (3760, 3) and f["faces"].dtype == np.int32 and f["count"] == f["xyz"].shape[0] == 1882
    assert f["components"] == 1 and f["dropped"] == dict(vertices=116, faces=228, components=1)
    assert f["edge"].shape == (1880,) and f["cell"].shape == (1882,) and np.all(np.diff(f["cell"]) > 0) and np.all(np.diff(f["edge"]) > 0)
    boundary, manifold, non_manifold, euler = M.edge_stats(f["faces"])
    assert (boundary, non_manifold, euler) == (0, 0, 2)
    roots, tri, _ = C.summary(C.components(f["faces"], f["count"]))
    assert roots.tolist() == [0] and tri.tolist() == [3760]
    # the kept triangles are the input's, vertex for vertex
    kept = np.nonzero(np.isin(m["cell"], f["cell"]))[0]
    assert np.array_equal(m["xyz"][kept], f["xyz"]) and np.array_equal(kept[f["faces"]], m["faces"][np.isin(m["faces"][:, 0], kept)])
    # 228 keeps both, the default drops nothing here (no loose vertex), keep_largest picks by size, ties by root
    assert C.filter_mesh(m, min_triangles=228)["faces"].shape[0] == 3988
    assert C.filter_mesh(m)["dropped"] == dict(vertices=0, faces=0, components=0)
    assert C.filter_mesh(m, keep_largest=1)["faces"].shape[0] == 3760
    assert C.filter_mesh(m, min_triangles=0, keep_largest=2)["faces"].shape[0] == 3988


def test_filter_twin_on_a_mesh_with_loose_vertices_and_ties():
    faces, V = C.build_case("tsdf-holes")
    mesh = dict(xyz=np.arange(3 * V, dtype=np.float32).reshape(V, 3), faces=faces)
    _, tri, _ = C.summary(C.reference("tsdf-holes"))
    f = C.filter_mesh(mesh)
    assert f["dropped"] == dict(vertices=34, faces=0, components=0) and f["components"] == 13 and f["count"] == V - 34
    assert np.unique(f["faces"]).shape[0] == f["count"]                               # every vertex left is used
    big = int(np.sort(tri)[-2])
    f = C.filter_mesh(mesh, min_triangles=big)
    assert f["components"] == int((tri >= big).sum()) and f["faces"].shape[0] == int(tri[tri >= big].sum())
    roots = C.summary(C.components(faces, V))[0]
    one = C.filter_mesh(dict(xyz=np.zeros((189, 3), np.float32), faces=C.build_case("disjoint-63")[0]), keep_largest=2)
    assert one["faces"].tolist() == [[0, 2, 4], [1, 3, 5]]                            # all tie at one triangle: roots 0 and 1 win
    assert roots.shape[0] == 47


# ------------------------------------------------------------------------------------------------- host checks without a device
def test_host_layer_refuses_before_it_touches_a_device():
    from estdepth_amd import fusion3d
    with pytest.raises(RuntimeError, match="mesh_components.*n_vertices"):
        fusion3d.mesh_components(np.zeros((1, 3), np.int32), n_vertices=-1)
    for bad in (np.zeros((4,), np.int32), np.zeros((2, 4), np.int32), np.zeros((2, 3), np.float32), np.array([[0, 1, 2 ** 31]], np.int64)):
        with pytest.raises(RuntimeError, match="mesh_components.*face"):
            fusion3d.mesh_components(bad)
    for bad in (None, [[0, 1, 2]], "faces"):
        with pytest.raises(RuntimeError, match="mesh_components.*faces must be"):
            fusion3d.mesh_components(bad)
    with pytest.raises(RuntimeError, match=r"mesh_components.*\[F,3\]"):
        fusion3d.mesh_components(torch.zeros(3, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="mesh_components: a faces tensor must live on a ROCm device"):
        fusion3d.mesh_components(torch.zeros(2, 3, dtype=torch.int32))                # a CPU tensor: there is no CPU path


def test_filter_mesh_refuses_before_it_touches_a_device():
    from estdepth_amd import fusion3d
    xyz, faces = np.zeros((4, 3), np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    for bad in (None, {}, dict(xyz=xyz), dict(faces=faces)):
        with pytest.raises(RuntimeError, match="filter_mesh.*'xyz' and 'faces'"):
            fusion3d.filter_mesh(bad)
    for kw in (dict(min_triangles=-1), dict(min_triangles=1.5), dict(keep_largest=-1), dict(keep_largest=0.5)):
        with pytest.raises(RuntimeError, match="filter_mesh.*%s" % list(kw)[0]):
            fusion3d.filter_mesh(dict(xyz=xyz, faces=faces), **kw)
    with pytest.raises(RuntimeError, match="filter_mesh.*edge"):
        fusion3d.filter_mesh(dict(xyz=xyz, faces=faces, edge=np.zeros(2, np.int64)))
    with pytest.raises(RuntimeError, match="filter_mesh.*normal"):
        fusion3d.filter_mesh(dict(xyz=xyz, faces=faces, normal=np.zeros((3, 3), np.float32)))
    with pytest.raises(RuntimeError, match="filter_mesh.*faces must be"):
        fusion3d.filter_mesh(dict(xyz=xyz, faces=faces.astype(np.float32)))


def test_ctypes_front_end_argument_rules(monkeypatch):
    from estdepth_amd import ops
    monkeypatch.setattr(ops, "BINDING", "ctypes")
    good = torch.zeros(4, 3, dtype=torch.int32)
    for bad in (None, good.numpy(), good, good.to(torch.int64), good.reshape(3, 4), good.reshape(-1)):
        with pytest.raises(RuntimeError, match=r"mesh_components: faces must be a contiguous int32 tensor \[F,3\] on a ROCm device"):
            ops.mesh_components(bad, 4)
    assert ops._faces.__doc__ and "estd_mesh_components" in ops.mesh_components.__doc__


def test_the_tool_flag_needs_a_mesh(tmp_path):
    import run_stream_ref as S
    tool = S.load_tool()
    base = ["--synthetic", "8", "--out", str(tmp_path), "--fuse", str(tmp_path / "scene.ply")]
    args = tool.parse(base + ["--mesh", str(tmp_path / "m.ply"), "--mesh-min-component", "100"])
    assert args.mesh_min_component == 100 and tool.parse(base + ["--mesh", str(tmp_path / "m.ply")]).mesh_min_component is None
    for bad in (["--mesh-min-component", "100"], ["--mesh", str(tmp_path / "m.ply"), "--mesh-min-component", "0"]):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)


def test_the_keywords_of_the_volume_methods_exist():
    import inspect
    from estdepth_amd.fusion3d import TSDFVolume
    assert inspect.signature(TSDFVolume.extract_mesh).parameters["min_component"].default == 0
    assert inspect.signature(TSDFVolume.save_mesh).parameters["min_component"].default == 0
