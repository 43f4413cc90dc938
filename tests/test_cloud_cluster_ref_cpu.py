"""CPU: the reference of the density-based clustering (tests/cloud_cluster_ref.py) against itself, before the GPU suite
(tests/test_gpu_cloud_cluster_routes.py) holds the kernels to it by equality: ``dbscan32`` agrees with the float64 brute force wherever
no distance lies within the fp32 error of eps, its counts are the rows of ``cloud_knn_ref.knn32`` inside the radius wherever fewer than
32 are, every plausible mistake the reference can be told to make is caught by equality on a named case, the partition does not depend
on the order of the rows, and the closed forms of the constructed cases hold."""
import numpy as np
import pytest

import cloud_cluster_ref as R
import cloud_knn_ref as KR

ALL = list(R.CASES) + list(R.PLACED)
SMALL = [n for n in ALL if n != "clusters_4096"]


@pytest.mark.parametrize("name", ALL)
def test_the_reference_is_consistent(name):
    c, w = R.expected(name)
    n = c["points"].shape[0]
    fig = R.compare(w, w, name)
    assert int(w["size"].sum()) + w["noise"] == n and int(w["sizes"].sum()) == int(w["size"].sum())
    core, label = w["core"], w["label"]
    assert (label[core] >= 0).all() and (label[label >= 0] <= np.arange(n)[label >= 0])[core[label >= 0]].all()
    assert (w["core"][w["roots"]]).all() and (label[w["roots"]] == w["roots"]).all()              # a label is a core point that labels itself
    assert (w["count"] >= 1).all()                                                                  # a point is its own neighbour
    print("CLOUD-CLUSTER-REF %s: %s" % (name, fig))


DYADIC = ("chain", "radius_edge", "duplicates", "bridge_tie", "bridge_near_larger")      # every d2 is exact in fp32 and in float64 alike


@pytest.mark.parametrize("name", SMALL)
def test_fp32_and_float64_agree_where_the_radius_is_clear(name):
    c, w = R.expected(name)
    count, label, clear_radius, clear_border = R.dbscan64(c["points"], c["eps"], c["min_points"])
    assert clear_radius or name in DYADIC, "%s: a distance within the fp32 error of eps: the comparison would be vacuous" % name
    assert (count == w["count"]).all(), name
    assert clear_border, "%s: two border keys within the fp32 error of each other" % name
    assert (label == w["label"]).all(), name


@pytest.mark.parametrize("name", SMALL)
def test_the_counts_are_the_knn_rows_inside_the_radius(name):
    c, w = R.expected(name)
    _, index, found = KR.knn32(c["points"], c["points"], KR.K_MAX, c["eps"])
    few = found < KR.K_MAX
    assert few.any() or name == "duplicates"
    assert (w["count"][few] == found[few]).all(), name
    assert (w["count"][~few] >= KR.K_MAX).all(), name
    assert (index[:, 0] >= 0).all()                                                                 # the point itself, at distance 0


MISTAKE_CASES = {"strict_radius": ("radius_edge",), "count_without_self": ("surface_65", "duplicates"),
                 "border_links_clusters": ("bridge_tie", "bridge_near_larger"), "border_smallest_label": ("bridge_near_larger",),
                 "border_tie_largest_index": ("bridge_tie",), "label_largest_index": ("chain", "bridge_tie"), "ring_early": ("sparse", "surface_64")}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_mistake_is_caught(mistake):
    assert set(MISTAKE_CASES) == set(R.MISTAKES)
    caught = []
    for name in MISTAKE_CASES[mistake]:
        c, want = R.expected(name)
        try:
            R.compare(R.dbscan32(c["points"], c["eps"], c["min_points"], mistake=mistake, cell=c["cell"] if c["cell"] is not None else c["eps"]), want, name)
        except AssertionError:
            caught.append(name)
    assert caught == list(MISTAKE_CASES[mistake]), (mistake, caught)


def test_the_counting_mistakes_are_caught_for_foreign_queries():
    c, want = R.count_case(257, 256)
    assert (R.count_within32(c["query"], c["target"], c["max_dist"]) == want).all() and want.max() > 1 and want.min() == 0
    assert (R.count_within32(c["query"], c["target"], c["max_dist"], mistake="ring_early", cell=0.07) != want).any()
    for t, q in R.COUNT_CASES:
        c, want = R.count_case(t, q)
        assert want.shape == (q,) and want.dtype == np.int32 and (t > 0 or not want.any())
        if t > 1 and q > 1:
            assert want[0] >= 2                                                                     # the first query sits on a duplicated target


@pytest.mark.parametrize("name", SMALL)
def test_the_partition_moves_with_the_rows(name):
    c, w = R.expected(name)
    n = c["points"].shape[0]
    for perm in (np.arange(n)[::-1], np.random.RandomState(n).permutation(n)):
        other = R.dbscan32(c["points"][perm], c["eps"], c["min_points"])
        assert (other["count"] == w["count"][perm]).all() and (other["core"] == w["core"][perm]).all(), name
        tie = name == "bridge_tie"                    # the one case where the index decides which cluster a point joins
        assert R.same_partition(w["label"], other["label"], perm) or tie, name
        assert other["n_clusters"] == w["n_clusters"] and other["noise"] == w["noise"], name
        assert sorted(other["sizes"].tolist()) == sorted(w["sizes"].tolist()), name


def test_the_constructed_cases_have_their_closed_forms():
    c, w = R.expected("chain")
    x = c["points"][:, 0]
    assert w["n_clusters"] == 1 and w["noise"] == 0 and w["sizes"].tolist() == [2049]
    assert sorted(np.nonzero(~w["core"])[0].tolist()) == sorted([int(np.argmin(x)), int(np.argmax(x))])      # both ends are borders
    assert (w["label"] == np.nonzero(w["core"])[0].min()).all()
    c, w = R.expected("radius_edge")
    inner = (np.abs(c["points"][:, :2] - 4 * R.S) < 3.5 * R.S).all(1)
    assert (w["core"] == inner).all() and (w["count"][inner] == 5).all() and w["noise"] == 4 and w["sizes"].tolist() == [77]
    c, w = R.expected("bridge_tie")
    assert w["count"][0] == 3 and not w["core"][0] and w["core"][1:].all() and w["roots"].tolist() == [1, 28]
    assert w["label"][0] == 1 and w["sizes"].tolist() == [28, 27]                                   # the exact tie goes to the smaller core index
    c, w = R.expected("bridge_near_larger")
    assert w["count"][0] == 3 and w["label"][0] == 28 and w["sizes"].tolist() == [27, 28]           # the nearer core wins, not the smaller label
    c, w = R.expected("duplicates")
    assert w["n_clusters"] == 1 and w["sizes"].tolist() == [70] and w["noise"] == 3 and set(w["count"].tolist()) == {70, 3}
    c, w = R.expected("all_core")
    assert w["core"].all() and w["noise"] == 0 and (w["sizes"] == 1).any() and w["n_clusters"] > 1
    c, w = R.expected("all_noise")
    assert not w["core"].any() and w["noise"] == 65 and w["n_clusters"] == 0 and (w["label"] == -1).all() and not w["size"].any()
    c, w = R.expected("clusters_4096")
    assert w["n_clusters"] >= 6 and w["noise"] > 0 and ((w["label"] >= 0) & ~w["core"]).sum() > 0
    first = np.array([int(np.argmax(w["cluster"] == j)) // 256 for j in range(w["n_clusters"])])
    assert len(set(first.tolist())) > 1 and all(len(set((np.nonzero(w["cluster"] == j)[0] // 256).tolist())) > 1 for j in range(6))      # spread over workgroups


def test_the_filter_rule():
    c, w = R.expected("clusters_4096")
    sizes = w["sizes"]
    keep = R.filter32(w, min_size=100)
    assert int(keep.sum()) == int(sizes[sizes >= 100].sum()) and not keep[w["label"] < 0].any()
    big = R.filter32(w, keep_largest=2)
    top = np.sort(sizes)[::-1][:2]
    assert int(big.sum()) == int(top.sum())
    assert not R.filter32(w, keep_largest=0).any() and (R.filter32(w) == (w["label"] >= 0)).all()
    # equal sizes: the smaller label first
    c, w = R.expected("bridge_near_larger")
    w = dict(w, sizes=np.array([27, 27], np.int32))
    assert (R.filter32(w, keep_largest=1) == (w["cluster"] == 0)).all()
