"""CPU: the reference of the k-nearest-neighbour search and the PCA normals (tests/cloud_knn_ref.py) against itself, before the GPU
suite (tests/test_gpu_cloud_knn_routes.py) holds the kernels to it: column 0 of ``knn32`` is ``cloud_metrics_ref.nearest32``, ``knn32``
agrees with the float64 brute force wherever float64 order is unambiguous, every plausible mistake the reference can be told to make is
caught by the suite's own comparison on some case, no row of a named case needs the excuse of the validity threshold, exact planes give
+-z, and the outlier rule drops what was planted."""
import numpy as np
import pytest

import cloud_knn_ref as R
import cloud_metrics_ref as CM

ALL = list(R.CASES) + list(R.PLACED)


def standin(case, index, count, mistake=None):
    """what a correct device gives for the lists ``index`` / ``count``, from the float64 reference (``mistake``: with that mistake)"""
    inr = R.rows_in_range(index, count, case["target"].shape[0])
    cov = R.cov64(case["target"], index, count, mistake=mistake)
    ref = R.normals64(cov, np.clip(count, 0, index.shape[1]), inr)
    n = np.where(ref["valid"][:, None], ref["n"], 0.0).astype(np.float32)
    n, _ = R.oriented(n, case["query"], case["toward"])
    return dict(normal=n, eig=np.where(inr[:, None], ref["lam"], 0.0).astype(np.float32), valid=ref["valid"].astype(np.uint8),
                invalid=int((~ref["valid"]).sum()), cov=cov), ref


@pytest.mark.parametrize("name", ALL)
def test_column_zero_is_the_nearest_neighbour(name):
    c, (dist, index, count) = R.expected(name)
    d1, i1 = CM.nearest32(c["query"], c["target"], c["max_dist"])
    assert (index[:, 0] == i1).all() and (dist[:, 0].view(np.uint32) == d1.view(np.uint32)).all(), name
    assert ((count > 0) == (i1 >= 0)).all()


@pytest.mark.parametrize("name", ALL)
def test_the_reference_meets_its_own_comparison(name):
    c, want = R.expected(name)
    fig = R.compare_knn(want, want, c, name)
    got, _ = standin(c, want[1], want[2])
    fig.update(R.compare_normals(got, c, want[1], want[2], name))
    print("CLOUD-KNN-REF %s: %s" % (name, fig))


@pytest.mark.parametrize("name", [n for n in ALL if n != "257x4096_k16"])
def test_fp32_and_float64_agree_where_the_order_is_clear(name):
    c, want = R.expected(name)
    n = R.compare_knn64(want, c, name)
    assert n > 0 or name in ("outside",) or int(want[2].sum()) == 0 or name in R.DEGENERATE or name in ("lattice_ties", "radius_edge"), (name, n)


def test_fma32_rounds_once():
    """against exact rational arithmetic on values that sit on the double-rounding trap and on random ones"""
    from fractions import Fraction
    rng = np.random.RandomState(3)
    a = np.concatenate([rng.uniform(-2, 2, 400), [1.0 + 2.0 ** -12, 3.0, 1e-3]]).astype(np.float32)
    c = np.concatenate([rng.uniform(0, 4, 400), [2.0 ** -25 + 2.0 ** -60, 2.0 ** -30, 1.0]]).astype(np.float32)
    got = R.fma32(a, c)
    for x, y, g in zip(a.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(x) + Fraction(y)
        lo, hi = np.nextafter(np.float32(g), np.float32(-np.inf)), np.nextafter(np.float32(g), np.float32(np.inf))
        assert abs(Fraction(g) - exact) <= abs(Fraction(float(lo)) - exact) and abs(Fraction(g) - exact) <= abs(Fraction(float(hi)) - exact), (x, y, g)


MISTAKE_CASES = {"kth_tie_largest_index": ("lattice_ties", "duplicates"), "ring_stops_on_best": ("sparse",), "strict_radius": ("radius_edge",),
                 "cov_uncentred_fp32": tuple(R.PLACED), "list_order_by_index": ("64x65_k7", "noisy_plane")}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_mistake_is_caught(mistake):
    assert set(MISTAKE_CASES) == set(R.MISTAKES)
    caught = []
    for name in MISTAKE_CASES[mistake]:
        c, want = R.expected(name)
        try:
            if mistake == "cov_uncentred_fp32":
                got, _ = standin(c, want[1], want[2], mistake=mistake)
                assert (got.pop("cov") != R.cov64(c["target"], want[1], want[2])).any()
                R.compare_normals(got, c, want[1], want[2], name)      # without the bit comparison: the eigenvalue bound alone must object
            else:
                cell = c["cell"] if c["cell"] is not None else 0.05
                R.compare_knn(R.knn32(c["query"], c["target"], c["k"], c["max_dist"], mistake=mistake, cell=cell), want, c, name)
        except AssertionError:
            caught.append(name)
    assert caught == list(MISTAKE_CASES[mistake]), (mistake, caught)


@pytest.mark.parametrize("name", ALL)
def test_no_row_needs_the_excuse(name):
    c, want = R.expected(name)
    _, ref = standin(c, want[1], want[2])
    ex = R.excused(ref, want[2], R.rows_in_range(want[1], want[2], c["target"].shape[0]))
    if name in R.DEGENERATE:
        assert not ref["valid"].any() and (ref["lam"][:, :2] == 0).all(), name       # exact zeros, far from the threshold
    else:
        assert not ex.any(), "%s: %d rows within the threshold's excuse, smallest gap ratio %.3g" % (name, int(ex.sum()), float(ref["ratio"].min()))


def test_exact_planes_give_z():
    rng = np.random.RandomState(11)
    plane = np.stack([rng.uniform(0, 1, 400), rng.uniform(0, 1, 400), np.full(400, 0.25)], 1).astype(np.float32)
    lattice = R.build_case("lattice_ties")["target"]
    for pts, k, md in ((plane, 12, 0.3), (lattice, 6, 0.25)):
        c = dict(target=pts, query=pts, k=k, max_dist=md, toward=None)
        dist, index, count = R.knn32(pts, pts, k, md)
        got, ref = standin(c, index, count)
        assert ref["valid"].all()
        assert (np.abs(got["normal"][:, 2]) >= 1.0 - 2.0 ** -23).all() and (np.abs(got["normal"][:, :2]) <= 2.0 ** -23).all()
        assert (got["normal"][:, 2] > 0).all()                   # no viewpoint: the largest component is positive
        assert (got["eig"][:, 0] <= 2.0 ** -40 * got["eig"][:, 2]).all()


def test_the_lattice_tie_is_decided_by_the_index():
    c, (dist, index, count) = R.expected("lattice_ties")
    r = 8 * 17 + 8                                               # an interior point: itself, four at one spacing, one of four diagonals
    assert count[r] == 6 and index[r, 0] == r
    assert sorted(index[r, 1:5].tolist()) == [r - 17, r - 1, r + 1, r + 17] and index[r, 1:5].tolist() == sorted(index[r, 1:5].tolist())
    assert index[r, 5] == r - 18 and dist[r, 5] == np.float32(np.sqrt(np.float32(2.0 ** -7)))


def test_outlier_rule_drops_the_planted_points():
    pts, planted = R.planted_surface()
    dist, index, count = R.knn32(pts, pts, 16, 0.15)
    keep, mean, mu, sigma = R.remove_outliers64(dist, index, 0.15)
    assert not keep[planted].any()
    assert keep[~planted].mean() > 0.9
    assert (mean[planted] > mu + 2.0 * sigma).all() and (mean[planted] == float(np.float32(0.15))).any()      # some have nothing but themselves in reach
    keep_r, _, _, _ = R.remove_outliers64(dist, index, 0.15, std_ratio=1e9, min_neighbours=8)
    assert not keep_r[planted].any() and keep_r[~planted].mean() > 0.9
