"""The point-to-triangle-mesh distance on the device (csrc/mesh/mesh_distance.hip behind cloud_metrics.TriangleGrid) against the float64
brute force of tests/mesh_distance_ref.py and its derived bound (held to 2 x): both bindings, M in {1, 63, 64, 65, 257} x F in {1, 2, 63,
65, 1000}, queries outside the grid's box, two wall-sized triangles among hundreds of small ones (both phases), the big list only, the
grid only, no queries, invalid faces only; the pinned bits of the all-exact cases (a tie, exactly max_dist, one step beyond); invalid
faces counted and without effect; bit identity across calls, bindings, cell edges, forced routes and a permutation of the faces;
malformed arguments; and what the feature is for: a surface scored against itself is within rounding of 0 with ``exact=True`` where
the sampled distance sits on its floor of about 1 / (2 sqrt(density))."""
import math

import numpy as np
import pytest
import torch

from estdepth_amd.cloud_metrics import TriangleGrid, point_mesh_distance  # noqa: F401 -- the feature under test: without it this module does not import

import mesh_distance_ref as R
from test_gpu_recon3d_routes import _cpu, _dev, under

pytestmark = pytest.mark.gpu
_BF = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def brute(name):
    """the reference's brute force of a case, computed once and shared (leave it unchanged)"""
    if name not in _BF:
        case = R.build_case(name)
        _BF[name] = (case, R.brute_force(case["q"], case["xyz"], case["faces"]))
    return _BF[name]


def run(case, binding="torch", cell=None, big_cells=None):
    """-> (the dict mesh_distance_ref.compare takes, the grid)"""
    def go():
        grid = TriangleGrid(dict(xyz=_dev(case["xyz"]), faces=_dev(case["faces"])), case["max_dist"], cell, big_cells)
        return grid, grid.query(_dev(case["q"]), bary=True, closest=True)
    grid, (dist, face, bary, closest) = under(binding, go)
    return dict(dist=_cpu(dist), face=_cpu(face), bary=_cpu(bary), closest=_cpu(closest), invalid=grid.invalid), grid


def same(a, b, keys=("dist", "face", "bary", "closest")):
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)
    return all(a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])) for k in keys) and a["invalid"] == b["invalid"]


@pytest.mark.parametrize("where", ["d64", "d512"])
def test_against_the_reference_away_from_the_origin(where):
    """the 65-query, 65-face soup built 64 m and 512 m out (tests/placement.py) through the unchanged comparison: its allowance follows the
    magnitudes of the differences the kernel forms, so a kernel that worked in absolute coordinates where it should not would miss it"""
    import placement as PL
    case = R.build_case(R.PLACED_CASE, PL.FAMILY_PLACES[where])
    got, grid = run(case)
    fig = R.compare(got, case, "%s@%s" % (R.PLACED_CASE, where))
    print("PLACEMENT mesh_distance %s@%s: %d queries, %d found; of the allowance: dist %.3f face %.3f" % (R.PLACED_CASE, where, fig["queries"], fig["found"],
                                                                                                     fig["dist"], fig["face"]))
    assert fig["found"] > 30 and grid.faces_valid == 65 and float(np.abs(case["xyz"]).min()) > PL.FAMILY_PLACES[where][0] / 4


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", R.CASES)
def test_against_the_reference(name, binding):
    case, bf = brute(name)
    got, grid = run(case, binding)
    fig = R.compare(got, case, name, bf)
    print("MESH-DISTANCE %s [%s]: %d queries, %d found, %d faces (%d invalid), %d pairs + %d big, cell %.4g dims %s; of the allowance: dist %.3f face %.3f"
          % (name, binding, fig["queries"], fig["found"], case["faces"].shape[0], fig["invalid"], grid.n_pairs, grid.n_big, grid.cell, grid.dims,
             fig["dist"], fig["face"]))
    assert grid.faces_valid == case["faces"].shape[0] - fig["invalid"]


def test_both_phases_run_on_the_walls():
    case, bf = brute("walls")
    got, grid = run(case)
    assert grid.n_big == 2 and grid.n_pairs >= 300
    assert (got["face"] < 2).any() and (got["face"] >= 2).any()          # winners from the big list and from the grid


@pytest.mark.parametrize("route", ["big", "grid"])
@pytest.mark.parametrize("name", ["walls", "icosphere", "rand_m257_f1000", "outside", "invalid_mix"])
def test_the_forced_routes(name, route):
    case, bf = brute(name)
    got, grid = run(case, cell=math.inf if route == "big" else 0.11, big_cells=None if route == "big" else "grid")
    assert (grid.n_pairs == 0 and grid.n_big == grid.faces_valid) if route == "big" else (grid.n_big == 0 and grid.n_pairs >= grid.faces_valid)
    R.compare(got, case, "%s/%s" % (name, route), bf)
    assert same(got, run(case)[0]), "%s: the %s route differs from the default one" % (name, route)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("route", [None, "big", "grid"])
@pytest.mark.parametrize("name", R.EXACT_CASES)
def test_the_exact_cases_give_the_analytic_bits(name, route, binding):
    """one query per region of a right triangle; equidistant from two faces: the smaller index; at exactly max_dist: found; one fp32
    step beyond: max_dist and -1"""
    case, want = R.exact_case(name)
    got, _ = run(case, binding, cell=math.inf if route == "big" else 1.0 if route == "grid" else None, big_cells="grid" if route == "grid" else None)
    R.check_exact(got, want, "%s/%s/%s" % (name, route, binding))
    R.compare(got, case, name)
    if name == "tie":                                   # the same two faces the other way round: still the smaller index
        flipped = dict(case, faces=case["faces"][::-1].copy())
        got, _ = run(flipped, binding, cell=math.inf if route == "big" else None)
        assert got["face"].tolist() == [0, 1] and got["dist"].tolist() == [1.0, 0.5]
    if name == "radius":
        assert got["face"].tolist() == [0, -1, 0] and got["dist"].tolist() == [3.0, 3.0, 3.0] and not got["bary"][1].any() and not got["closest"][1].any()


def test_invalid_faces_are_counted_and_change_nothing_else():
    case, bf = brute("invalid_mix")
    got, grid = run(case)
    assert grid.invalid == 10 and grid.faces_valid == 40
    keep = np.nonzero(bf["valid"])[0]
    clean = dict(case, faces=case["faces"][keep])
    ref, g2 = run(clean)
    assert g2.invalid == 0
    assert same(dict(got, invalid=0), ref, ("dist", "bary", "closest"))
    assert np.array_equal(np.where(ref["face"] >= 0, keep[np.maximum(ref["face"], 0)], -1), got["face"])


@pytest.mark.parametrize("name", ["walls", "icosphere", "rand_m257_f1000"])
def test_bit_identity(name):
    """repeated calls, both bindings, three cell edges, the forced routes and a permutation of the faces"""
    case, bf = brute(name)
    first, grid = run(case)
    for kw in (dict(), dict(binding="ctypes"), dict(cell=0.05), dict(cell=0.3), dict(cell=1.7), dict(cell=math.inf), dict(cell=0.2, big_cells="grid"),
               dict(big_cells=3)):
        assert same(first, run(case, **kw)[0]), "%s: %r changes the result" % (name, kw)
    perm = np.random.default_rng(7).permutation(case["faces"].shape[0])
    got, _ = run(dict(case, faces=case["faces"][perm]))
    assert same(first, got, ("dist",))
    D = bf["dist"]
    unique = (np.sort(D.astype(np.float32), 1)[:, 0] < np.sort(D.astype(np.float32), 1)[:, 1]) if D.shape[1] > 1 else np.ones(D.shape[0], bool)
    tied = first["face"] != np.where(got["face"] >= 0, perm[np.maximum(got["face"], 0)], -1)
    # where the faces differ, the two are equidistant on the device as well: same dist bits above; bary / closest belong to the face
    assert not (tied & unique & (first["face"] >= 0)).any(), "%s: a unique minimum moved with the permutation" % name
    ok = ~tied
    assert same(dict(first, **{k: first[k][ok] for k in ("bary", "closest")}), dict(got, **{k: got[k][ok] for k in ("bary", "closest")}), ("bary", "closest"))
    print("MESH-DISTANCE-IDENTITY %s: %d queries, %d with a tie between faces under the permutation" % (name, D.shape[0], int(tied.sum())))


def test_the_one_shot_form_and_empty_inputs():
    case, _ = brute("rand_m65_f63")
    mesh = dict(xyz=_dev(case["xyz"]), faces=_dev(case["faces"]))
    got, _ = run(case)
    dist, face = point_mesh_distance(_dev(case["q"]), mesh, case["max_dist"])
    assert np.array_equal(_cpu(dist), got["dist"]) and np.array_equal(_cpu(face), got["face"])
    dist, face, bary, closest = TriangleGrid(mesh, 0.5).query(torch.empty((0, 3), device="cuda"), bary=True, closest=True)
    assert dist.shape == (0,) and face.shape == (0,) and bary.shape == (0, 2) and closest.shape == (0, 3)
    none = TriangleGrid(dict(xyz=mesh["xyz"], faces=torch.empty((0, 3), device="cuda", dtype=torch.int32)), 0.5)
    dist, face = none.query(_dev(case["q"]))
    assert none.invalid == 0 and none.faces_valid == 0 and (face == -1).all() and (dist == 0.5).all()


def test_malformed_arguments_raise():
    case, _ = brute("rand_m65_f63")
    xyz, faces, q = _dev(case["xyz"]), _dev(case["faces"]), _dev(case["q"])
    mesh = dict(xyz=xyz, faces=faces)
    for bad in (dict(mesh=dict(xyz=xyz)), dict(mesh=dict(xyz=xyz, faces=faces.to(torch.int64))), dict(mesh=dict(xyz=xyz[:, :2], faces=faces)),
                dict(mesh=dict(xyz=xyz, faces=faces.cpu())), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_dist=1e30),
                dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(big_cells=-1), dict(big_cells="all")):
        kw = dict(mesh=mesh, max_dist=0.5)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            TriangleGrid(**kw)
    grid = TriangleGrid(mesh, 0.5)
    nan = q.clone()
    nan[3, 1] = float("nan")
    for bad in (nan, q.double(), q[:, :2], q.cpu(), q.reshape(-1)):
        with pytest.raises(RuntimeError):
            grid.query(bad)


# ------------------------------------------------------------------------------------------------ what it is for
RHO = 400.0          # tests/test_mesh_distance_ref_cpu.py shows the floor condition for this density with the reference alone


def test_a_surface_scored_against_itself():
    """An icosphere against the same surface with its faces in another order (so that the two sides get different samples) at RHO
    points per square metre.  With exact=True accuracy and completeness are within the derived bound of 0: a sample is off its own
    triangle by the rounding of p = fma(v, c - a, fma(u, b - a, a)), at most 4 u (|a| + |b - a| + |c - a|) per coordinate, and the
    kernel's distance by the reference's e_dist (2 x allowed).  The default path's figures sit on the sampling floor, about
    0.5 / sqrt(RHO): at least ten times larger (in fact four orders of magnitude).  Without the feature this test fails."""
    from estdepth_amd import cloud_metrics, fusion3d
    xyz, faces = R.icosphere(2)
    perm = np.random.default_rng(11).permutation(faces.shape[0])
    pred, gt = dict(xyz=_dev(xyz), faces=_dev(faces[perm])), dict(xyz=_dev(xyz), faces=_dev(faces))
    sampled = cloud_metrics.compare_meshes(pred, gt, RHO, threshold=0.05)
    exact = cloud_metrics.compare_meshes(pred, gt, RHO, threshold=0.05, exact=True)
    assert exact["exact"] == dict(faces_pred=320, faces_gt=320, invalid_pred=0, invalid_gt=0)
    assert exact["sampled"] == sampled["sampled"] and exact["n_pred"] == sampled["n_pred"] and exact["n_gt"] == sampled["n_gt"]
    # the float64 chain from the same device samples
    samples = _cpu(fusion3d.sample_mesh(pred, density=RHO, seed=0)["xyz"])
    assert samples.shape[0] == exact["n_pred"]
    dmin, _, bf = R.nearest64(samples, xyz, faces)
    e_mean = float(np.take_along_axis(bf["e_dist"], np.argmin(bf["dist"], 1)[:, None], 1).mean())
    off = 4.0 * math.sqrt(3.0) * R.U * (1.0 + 2.0 * 0.7)
    print("MESH-DISTANCE-SELF rho %g, %d samples: exact accuracy %.3g completeness %.3g (float64 chain %.3g, bound %.3g + %.3g); sampled accuracy %.5f "
          "completeness %.5f = %.3f / sqrt(rho)" % (RHO, exact["n_pred"], exact["accuracy"], exact["completeness"], dmin.mean(), off, R.C * e_mean,
                                                      sampled["accuracy"], sampled["completeness"], sampled["accuracy"] * math.sqrt(RHO)))
    assert abs(exact["accuracy"] - dmin.mean()) <= R.C * e_mean
    for k in ("accuracy", "completeness"):
        assert 0.0 <= exact[k] <= off + R.C * e_mean, (k, exact[k])
        assert sampled[k] >= 10.0 * exact[k] and sampled[k] >= 0.25 / math.sqrt(RHO), (k, sampled[k], exact[k])
    assert exact["precision"] == 1.0 and exact["recall"] == 1.0 and exact["clamped_pred"] == 0 and exact["clamped_gt"] == 0
    assert exact["normal_consistency"] > 0.999999


def test_exact_false_is_todays_result_and_a_cloud_side_keeps_the_sample_search():
    from estdepth_amd import cloud_metrics
    xyz, faces = R.icosphere(1)
    rgb = np.random.default_rng(2).uniform(0, 1, xyz.shape).astype(np.float32)
    pred = dict(xyz=_dev(xyz * np.float32(1.01)), faces=_dev(faces), color=_dev(rgb))
    gt = dict(xyz=_dev(xyz), faces=_dev(faces), color=_dev(rgb))
    a = cloud_metrics.compare_meshes(pred, gt, 200.0)
    b = cloud_metrics.compare_meshes(pred, gt, 200.0, exact=False)
    assert a == b and "exact" not in a
    e = cloud_metrics.compare_meshes(pred, gt, 200.0, exact=True, downsample=0.05)
    assert e["n_pred"] < a["n_pred"] and 0.005 < e["accuracy"] < 0.0101 and 0.0 <= e["color_l1"] < 0.15 and e["normal_consistency"] > 0.999
    cloud = dict(xyz=gt["xyz"])
    c = cloud_metrics.compare_meshes(pred, cloud, 200.0, exact=True)
    assert c["exact"]["faces_gt"] is None and c["exact"]["faces_pred"] == 80 and c["accuracy"] > 5.0 * e["accuracy"] and c["completeness"] < 0.0101
