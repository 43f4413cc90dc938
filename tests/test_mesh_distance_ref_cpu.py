"""The float64 reference of the point-to-mesh distance (tests/mesh_distance_ref.py) held against what is known in closed form, before
the GPU tests hold the kernels against it: the seven regions of one right triangle with dyadic coordinates (exact), a unit cube, an
icosphere within its faceting bound; the planted mistakes are rejected; and the floor the exact distance removes -- the nearest SAMPLE
of a surface is about 1 / (2 sqrt(density)) away from a point on it -- shown with the sampling reference alone.  Needs no device."""
import numpy as np
import pytest

import mesh_distance_ref as R
import mesh_sample_ref as S


def test_one_query_in_each_of_the_seven_regions_is_exact():
    xyz, faces = R.RIGHT
    for code, name in enumerate(("A", "B", "AB", "C", "AC", "BC", "interior")):
        q, (v, w), p, d2 = R.SEVEN[name]
        r = R.closest64(np.asarray(q, np.float64), *(xyz[j].astype(np.float64) for j in faces[0]))
        assert int(r["region"]) == code, (name, int(r["region"]))
        assert float(r["v"]) == v and float(r["w"]) == w and tuple(r["p"].tolist()) == tuple(float(x) for x in p) and float(r["d2"]) == d2, (name, r)
        assert float(r["e_dist"]) < 64 * R.U * max(1.0, float(r["dist"])), (name, r["e_dist"])


@pytest.mark.parametrize("name", R.EXACT_CASES)
def test_the_exact_cases_pin_their_bits(name):
    case, want = R.exact_case(name)
    got = R.nearest_planted(case["q"], case["xyz"], case["faces"], case["max_dist"])
    R.check_exact(got, want, name)
    R.compare(got, case, name)
    # bary and closest of the reference itself
    for i, f in enumerate(want["face"]):
        if f >= 0:
            r = R.closest64(case["q"][i].astype(np.float64), *(case["xyz"][j].astype(np.float64) for j in case["faces"][f]))
            assert (float(r["v"]), float(r["w"])) == tuple(float(x) for x in want["bary"][i]) and r["p"].tolist() == want["closest"][i].astype(np.float64).tolist()


def test_a_unit_cube_inside_and_outside():
    case = R.build_case("cube")
    q = case["q"].astype(np.float64)
    dmin, face, _ = R.nearest64(case["q"], case["xyz"], case["faces"])
    out = np.linalg.norm(np.maximum(np.maximum(-q, q - 1.0), 0.0), axis=1)
    inside = np.minimum(q, 1.0 - q).min(1)
    want = np.where((q >= 0).all(1) & (q <= 1).all(1), inside, out)
    assert ((q >= 0).all(1) & (q <= 1).all(1)).sum() > 5 and (out > 0).sum() > 50
    assert np.abs(dmin - want).max() < 1e-14 and (face >= 0).all()


def test_an_icosphere_within_its_faceting_bound():
    """the mesh lies in the shell r_in <= |x| <= r (vertices on the sphere, r_in the nearest face plane), and a ray from the centre meets
    it: | d - | |q| - r | | <= r - r_in for every query outside the shell"""
    xyz, faces = R.icosphere(2, 1.0)
    tri = xyz[faces].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = np.abs((n / np.linalg.norm(n, axis=1, keepdims=True) * tri[:, 0]).sum(1)).min()
    r = np.linalg.norm(xyz.astype(np.float64), axis=1).max()
    sag = r - r_in
    assert 0 < sag < 0.03
    rng = np.random.default_rng(3)
    d = rng.normal(size=(300, 3))
    radius = np.where(np.arange(300) % 2 == 0, rng.uniform(0.05, r_in - 1e-3, 300), rng.uniform(r + 1e-3, 3.0, 300))
    q = (d / np.linalg.norm(d, axis=1, keepdims=True) * radius[:, None]).astype(np.float32)
    dmin, _, _ = R.nearest64(q, xyz, faces)
    assert np.abs(dmin - np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - r)).max() <= sag + 1e-6


def test_validity_is_the_headers():
    case = R.build_case("invalid_mix")
    valid = R.valid_faces(case["xyz"], case["faces"])
    assert valid[:20].all() and not valid[20:30].any() and valid[30:].all()
    only = R.build_case("invalid_only")
    assert not R.valid_faces(only["xyz"], only["faces"]).any()
    got = R.nearest_planted(only["q"], only["xyz"], only["faces"], only["max_dist"])
    assert (got["face"] == -1).all() and got["invalid"] == 4
    R.compare(got, only, "invalid_only")


@pytest.mark.parametrize("name", ["rand_m65_f63", "walls", "icosphere", "invalid_mix", "outside", "m0"])
def test_the_reference_passes_its_own_comparison(name):
    case = R.build_case(name)
    fig = R.compare(R.nearest_planted(case["q"], case["xyz"], case["faces"], case["max_dist"]), case, name)
    assert fig["dist"] <= 1.0 and fig["face"] <= 1.0
    if name not in ("m0",):
        assert 0 < fig["found"] <= fig["queries"]


def test_planted_mistakes_are_rejected():
    assert set(R.MISTAKES) == {"swapped_edge_region", "strict_radius", "largest_index_on_ties"}
    # the quotient of the wrong edge: caught by the bound on a random case and by the pinned bits
    case = R.build_case("rand_m257_f65")
    with pytest.raises(AssertionError):
        R.compare(R.nearest_planted(case["q"], case["xyz"], case["faces"], case["max_dist"], "swapped_edge_region"), case)
    seven, want = R.exact_case("seven")
    with pytest.raises(AssertionError):
        R.check_exact(R.nearest_planted(seven["q"], seven["xyz"], seven["faces"], seven["max_dist"], "swapped_edge_region"), want)
    # < in place of <= at max_dist, the largest index on a tie: exact arithmetic cannot tell, the pinned cases do
    for mistake, name in (("strict_radius", "radius"), ("largest_index_on_ties", "tie")):
        case, want = R.exact_case(name)
        R.check_exact(R.nearest_planted(case["q"], case["xyz"], case["faces"], case["max_dist"]), want, name)
        with pytest.raises(AssertionError):
            R.check_exact(R.nearest_planted(case["q"], case["xyz"], case["faces"], case["max_dist"], mistake), want, name)
    # a result that is off by more than the allowance, a face that is not the nearest, a wrong invalid count
    case = R.build_case("rand_m65_f63")
    good = R.nearest_planted(case["q"], case["xyz"], case["faces"], case["max_dist"])
    i = int(np.nonzero(good["face"] >= 0)[0][0])
    for k, v in (("dist", good["dist"][i] * np.float32(1 + 1e-4)), ("face", (good["face"][i] + 1) % 63)):
        bad = {kk: np.array(vv, copy=True) if isinstance(vv, np.ndarray) else vv for kk, vv in good.items()}
        bad[k][i] = v
        with pytest.raises(AssertionError):
            R.compare(bad, case)
    with pytest.raises(AssertionError):
        R.compare(dict(good, invalid=1), case)


RHO = 400.0


def test_the_floor_of_the_sampled_distance():
    """A 2 x 2 square sampled at RHO points per square metre (tests/mesh_sample_ref.py), queries on the square: the distance to the
    SURFACE is within its bound of 0, the distance to the nearest SAMPLE averages at least 0.25 / sqrt(RHO) -- Poisson samples would
    give 0.5 / sqrt(RHO), stratified ones are of the same order.  The GPU test of compare_meshes relies on this condition for the
    density it uses."""
    xyz, faces = R.square(2.0)
    n = S.n_for_density(RHO, 4.0)
    samples = S.sample(xyz, faces, None, n, 0)["xyz"]
    rng = np.random.default_rng(5)
    q = np.concatenate([rng.uniform(0.1, 1.9, (400, 2)), np.zeros((400, 1))], 1).astype(np.float32)
    dmin, _, bf = R.nearest64(q, xyz, faces)
    bound = R.C * bf["e_dist"].max()
    assert dmin.max() <= bound and bound < 1e-5
    floor = S.nearest_brute(q, samples).mean()
    print("MESH-DISTANCE-FLOOR rho %g: exact max %.3g (bound %.3g), nearest sample mean %.5f = %.3f / sqrt(rho)" % (RHO, dmin.max(), bound, floor, floor * RHO ** 0.5))
    assert floor >= 0.25 / RHO ** 0.5
    assert floor >= 1000.0 * max(bound, dmin.max())
