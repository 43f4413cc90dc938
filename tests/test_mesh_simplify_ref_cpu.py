"""The reference of the mesh simplification (tests/mesh_simplify_ref.py) held to closed forms, on the CPU: the box whose faces, edges and
corners the quadric placement has to keep, the noisy sphere on which duplicates and fall-backs occur, the route cases doing what their
names say, and the reference's own pieces (the glue, the solve, the order of the sums) against independent forms."""
import math

import numpy as np
import pytest

import mesh_simplify_ref as R


@pytest.fixture(scope="module")
def box():
    xyz, faces = R.box()
    origin = xyz.min(0).astype(np.float64) - 0.013
    return xyz, faces, R.simplify(xyz, faces, 0.1, origin), R.simplify(xyz, faces, 0.1, origin, placement="mean")


def test_the_box_is_the_issue_s(box):
    xyz, faces, _, _ = box
    assert xyz.shape == (7868, 3) and faces.shape == (15732, 3)
    e = R.edge_stats(faces)
    assert e["boundary"] == 0 and e["non_manifold"] == 0 and e["euler"] == 2
    assert np.abs(R.box_distance(xyz)).max() < 1e-7


def test_box_topology_after_clustering(box):
    _, _, q, m = box
    for out in (q, m):
        e = R.edge_stats(out["faces"])
        assert out["stats"]["vertices"] == 288 and out["stats"]["faces"] == 572
        assert e["edges"] == 858 and e["manifold"] == 858 and e["boundary"] == 0 and e["non_manifold"] == 0 and e["euler"] == 2
        assert out["stats"]["duplicates"] == 0 and out["stats"]["invalid"] == 0
        assert out["stats"]["collapsed"] == 15732 - 572
    assert q["stats"]["fallback"] == 0 and q["stats"]["placed"] == 288 and bool(q["placed"].all())
    assert np.array_equal(q["faces"], m["faces"])


def test_quadric_placement_keeps_the_box_where_the_mean_rounds_it_off(box):
    _, _, q, m = box
    dq, dm = R.box_distance(q["xyz"]).max(), R.box_distance(m["xyz"]).max()
    print("MESH-SIMPLIFY-REF box, cell 0.1: quadric placement at most %.3e m off the box, mean placement %.3e m" % (dq, dm))
    assert dm > 0.02 and dq <= dm / 100.0


def test_box_at_half_the_cell():
    xyz, faces = R.box()
    origin = xyz.min(0).astype(np.float64) - 0.013
    q, m = R.simplify(xyz, faces, 0.05, origin), R.simplify(xyz, faces, 0.05, origin, placement="mean")
    e = R.edge_stats(q["faces"])
    dq, dm = R.box_distance(q["xyz"]).max(), R.box_distance(m["xyz"]).max()
    print("MESH-SIMPLIFY-REF box, cell 0.05: %d vertices %d faces, quadric %.3e m, mean %.3e m" % (q["stats"]["vertices"], q["stats"]["faces"], dq, dm))
    assert e["boundary"] == 0 and e["non_manifold"] == 0 and e["euler"] == 2 and q["stats"]["fallback"] == 0
    assert dq <= dm / 100.0


def test_noisy_sphere_has_duplicates_and_fallbacks():
    xyz, faces = R.noisy_sphere()
    out = R.simplify(xyz, faces, 0.04)
    s, e = out["stats"], R.edge_stats(out["faces"])
    print("MESH-SIMPLIFY-REF noisy sphere, cell 0.04: %s; edges %s" % (s, e))
    assert s["duplicates"] > 0 and 0 < s["fallback"] < s["vertices"] / 4
    assert s["placed"] + s["fallback"] == s["vertices"] and s["faces"] + s["collapsed"] + s["duplicates"] == s["faces_in"]
    r = np.linalg.norm(out["xyz"].astype(np.float64) - np.asarray([0.41, 0.43, 0.39]), axis=1)
    assert np.abs(r - 0.37).max() < 0.02                                      # every vertex stays by the surface, fall-backs included


def test_smooth_sphere_both_placements_agree():
    xyz, faces = R.uv_sphere()
    xyz = xyz.astype(np.float32)
    q, m = R.simplify(xyz, faces, 0.04), R.simplify(xyz, faces, 0.04, placement="mean")
    c = np.asarray([0.41, 0.43, 0.39])
    rq, rm = (np.abs(np.linalg.norm(o["xyz"].astype(np.float64) - c, axis=1) - 0.37).max() for o in (q, m))
    print("MESH-SIMPLIFY-REF smooth sphere: radial error quadric %.3e m, mean %.3e m" % (rq, rm))
    assert rq < 2e-3 and rm < 2e-3


@pytest.mark.parametrize("name", R.CASES)
def test_the_cases_are_consistent(name):
    xyz, faces, cell, origin = R.build_case(name)
    out = R.expected(name)
    s = out["stats"]
    assert s["faces"] + s["collapsed"] + s["duplicates"] + s["invalid"] == faces.shape[0]
    assert out["xyz"].shape == (s["vertices"], 3) and out["xyz"].dtype == np.float32 and out["normal"].dtype == np.float32
    assert np.all(np.diff(out["cell_key"]) > 0) and out["cluster"].max(initial=-1) == s["vertices"] - 1
    assert (out["triple"][:, 0] >= 0).sum() == s["faces"] + s["duplicates"]
    f = out["faces"]
    assert np.all((f[:, 0] < f[:, 1]) & (f[:, 0] < f[:, 2])) and np.unique(f, axis=0).shape[0] == f.shape[0]
    assert np.all(np.diff(out["kept"]) > 0)
    # a placed vertex lies in its cell, any other is its mean
    centre = R.centres(out["cell_key"], out["lo"], out["cell"], out["dims"])
    assert np.all(np.abs(out["xyz"][out["placed"]].astype(np.float64) - centre[out["placed"]]) <= 0.5 * out["cell"] * (1 + 1e-6) + 1e-4 * np.abs(centre[out["placed"]]))
    assert np.array_equal(R.bits(out["xyz"][~out["placed"]]), R.bits(out["mean"][~out["placed"]]))
    n = np.linalg.norm(out["normal"].astype(np.float64), axis=1)
    assert np.all((np.abs(n - 1) < 1e-6) | (n == 0))


def test_the_cases_do_what_their_names_say():
    assert [R.build_case("patch-%d" % n)[1].shape[0] for n in (0, 1, 63, 64, 65, 257)] == [0, 1, 63, 64, 65, 257]
    assert R.expected("patch-0")["stats"]["placed"] == 0 and not R.expected("patch-0")["normal"].any()
    assert R.expected("patch-257")["stats"]["faces"] > 0 and R.expected("patch-257")["stats"]["placed"] > 0
    one = R.expected("one-cluster")["stats"]
    assert one["vertices"] == 1 and one["faces"] == 0 and one["collapsed"] == 8
    k65 = R.expected("clusters-65")["stats"]
    assert k65["vertices"] == 65 and k65["collapsed"] == 0 and k65["faces"] == 96
    for n in (1, 64, 65, 300):
        out = R.expected("fan-%d" % n)
        assert (out["corner"] == out["cluster"][0]).sum() == n and (out["cluster"] == out["cluster"][0]).sum() == 1
    assert R.expected("fan-300")["placed"][R.expected("fan-300")["cluster"][0]]
    bad = R.expected("invalid")
    assert bad["stats"]["invalid"] == 6 and all((bad["triple"][f] == -1).all() for f in (0, 63, 64, 127, 128, 256))
    assert all((bad["corner"][3 * f:3 * f + 3] == bad["stats"]["vertices"]).all() for f in (0, 63, 64, 127, 128, 256))
    odd = R.expected("odd-faces")
    F0 = 65
    # three rotated copies and one plain copy go (and whatever equals a face of the patch itself); the reversed ones stay
    assert odd["stats"]["duplicates"] >= 4
    kept = set(odd["kept"].tolist())
    assert not {F0 + 3, F0 + 4, F0 + 5, F0 + 9} & kept and {F0 + 6, F0 + 7, F0 + 8} <= kept
    assert all((odd["triple"][F0 + j] == odd["triple"][F0 + 3 + j]).all() and sorted(odd["triple"][F0 + j]) == sorted(odd["triple"][F0 + 6 + j])
               and (odd["triple"][F0 + j] != odd["triple"][F0 + 6 + j]).any() for j in range(3))
    assert (odd["triple"][-2:] == -1).all()                                   # a vertex named twice collapses
    zero = R.expected("zero-area")
    k = zero["cluster"][-3:]
    assert len(set(k.tolist())) == 3 and (zero["t"][k] == 0).all() and not zero["placed"][k].any() and not zero["normal"][k].any()
    wedge = R.expected("wedge")
    assert wedge["stats"]["vertices"] == 1 and wedge["t"][0] > 0 and not wedge["placed"][0] and abs(wedge["s"][0, 0]) > 0.05
    assert abs(0.05 + wedge["s"][0, 0] - 0.2) < 0.03                          # the minimiser sits by the crease at x = 0.2
    loose = R.expected("loose-vertex")
    k = loose["cluster"][-1]
    assert (loose["cluster"] == k).sum() == 1 and not (loose["corner"] == k).any() and not loose["placed"][k] and not loose["normal"][k].any()
    far = R.expected("offset-1000")
    assert far["stats"]["faces"] > 0 and far["xyz"].min() > 999 and far["stats"]["placed"] > 0


def test_the_glue_keeps_the_smallest_index_and_both_windings():
    t = np.asarray([[-1, -1, -1], [0, 2, 1], [0, 1, 2], [-1, -1, -1], [0, 1, 2], [0, 2, 1], [3, 5, 4], [0, 1, 2]], np.int32)
    faces, kept = R.unique_faces(t)
    assert kept.tolist() == [1, 2, 6] and faces.tolist() == [[0, 2, 1], [0, 1, 2], [3, 5, 4]]
    corner, triple, invalid, collapsed = R.cluster_faces(np.asarray([[0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 0, 1], [0, 1, 9]], np.int32), 3,
                                                         np.asarray([2, 0, 1], np.int32), 3)
    assert triple.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 1], [-1, -1, -1], [-1, -1, -1]] and (invalid, collapsed) == (1, 1)
    assert corner.tolist() == [2, 0, 1, 0, 1, 2, 1, 0, 2, 2, 2, 0, 3, 3, 3]


def test_the_solve_solves():
    """LDL^T without pivoting against numpy's solver on the box's clusters, in float64: the reference's own error"""
    xyz, faces = R.box()
    out = R.simplify(xyz, faces, 0.1, xyz.min(0).astype(np.float64) - 0.013)
    S, centre = R.quadric_sums(xyz, faces, out["corner"], out["cell_key"], out["lo"], out["cell"], out["dims"])
    worst = 0.0
    for k in range(S.shape[0]):
        a = S[k, :6]
        A = np.asarray([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])
        lam = np.trace(A) * R.REG
        g = out["mean"][k].astype(np.float64) - centre[k]
        want = np.linalg.solve(A + lam * np.eye(3), S[k, 6:9] + lam * g)
        worst = max(worst, np.abs(want - out["s"][k]).max())
    print("MESH-SIMPLIFY-REF the elimination is within %.3e m of numpy.linalg.solve on the box" % worst)
    assert worst < 1e-9                                                        # cond <= 2^12 / reg-bounded: 4096 * 2^-53 * 0.1 m ~ 5e-14, with room


def test_the_order_of_the_sum_is_the_stated_tree():
    xyz, faces, cell, origin = R.build_case("fan-300")
    out = R.expected("fan-300")
    S, centre = R.quadric_sums(xyz, faces, out["corner"], out["cell_key"], out["lo"], out["cell"], out["dims"])
    k = out["cluster"][0]
    rec = [r for r in range(3 * faces.shape[0]) if out["corner"][r] == k]
    assert len(rec) == 300
    chains = [0.0] * R.GROUP
    exact = []
    for i, r in enumerate(rec):
        a, b, c = (xyz[v].astype(np.float64) for v in faces[r // 3])
        e1, e2 = b - a, c - a
        mz = e1[0] * e2[1] - e1[1] * e2[0]
        chains[i % R.GROUP] = chains[i % R.GROUP] + mz
        exact.append(mz)
    tree = ((chains[0] + chains[4]) + (chains[2] + chains[6])) + ((chains[1] + chains[5]) + (chains[3] + chains[7]))
    assert tree == S[k, 11] and abs(tree - math.fsum(exact)) <= 300 * 2.0 ** -52 * math.fsum(abs(v) for v in exact)
