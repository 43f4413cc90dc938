"""The host layer of the density-based clustering (estdepth_amd/cloud_metrics.py: filter_clusters, compare_clouds(clusters=...)) on the
device, on a scene whose answer is known by construction: a lattice-sampled wall, three planted blobs of forty points well off it and a
dozen isolated points, the rows shuffled.  ``filter_clusters(min_size=...)`` keeps exactly the wall's rows -- the numpy reference of
tests/cloud_cluster_ref.py confirms the mask on the CPU --, ``compare_clouds(clusters=...)`` gives the float64 chain's scores of the
FILTERED cloud within cloud_metrics_ref.check_metrics, and with ``clusters=None`` nothing new runs and every result is the same bits."""
import numpy as np
import pytest
import torch

import cloud_cluster_ref as R
import cloud_metrics_ref as CM
from test_gpu_cloud_cluster_routes import BORDER, COUNT, FLATTEN, HOOK, profiled
from test_gpu_recon3d_routes import _cpu, _dev

pytestmark = pytest.mark.gpu
SPACING, EPS, MIN_POINTS, MIN_SIZE = 0.02, 0.03, 6, 200          # eps reaches the 8 lattice neighbours (0.0283), not the next (0.04)
THRESHOLD = 0.05
ALL4 = {COUNT, HOOK, FLATTEN, BORDER}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def scene():
    """-> (points float32 [N,3] shuffled, wall bool [N], the ground truth: the wall sampled on the lattice shifted by half a spacing, 4 mm off)"""
    rng = np.random.RandomState(20)
    g = np.arange(48, dtype=np.float64) * SPACING
    x, y = np.meshgrid(g, g, indexing="ij")
    wall = np.stack([x.ravel(), y.ravel(), np.full(48 * 48, 1.0)], 1)
    blobs = [np.array(c) + 0.008 * rng.standard_normal((40, 3)) for c in ((0.2, 0.3, 0.7), (0.7, 0.6, 1.35), (0.5, 0.1, 0.6))]
    lone = np.stack([np.arange(12) * 0.08, np.full(12, -0.2), 1.0 + 0.1 * np.arange(12)], 1)       # 0.128 apart, 0.2 from the wall
    pts = np.concatenate([wall] + blobs + [lone])
    is_wall = np.arange(pts.shape[0]) < wall.shape[0]
    perm = rng.permutation(pts.shape[0])
    gt = wall + np.array([0.5 * SPACING, 0.5 * SPACING, 0.004])
    return pts[perm].astype(np.float32), is_wall[perm], gt.astype(np.float32)


@pytest.fixture(scope="module")
def planted():
    pts, is_wall, gt = scene()
    ref = R.dbscan32(pts, EPS, MIN_POINTS)
    return pts, is_wall, gt, ref


def test_the_reference_confirms_the_construction(planted):
    pts, is_wall, gt, ref = planted
    assert (R.filter32(ref, min_size=MIN_SIZE) == is_wall).all() and (R.filter32(ref, keep_largest=1) == is_wall).all()
    assert ref["n_clusters"] == 4 and sorted(ref["sizes"].tolist()) == [40, 40, 40, 48 * 48] and ref["noise"] == 12
    assert (ref["label"][is_wall] == ref["label"][is_wall][0]).all() and ((ref["label"] >= 0) & ~ref["core"]).sum() > 0      # the wall's rim: border points


def test_filter_clusters_keeps_exactly_the_wall(planted):
    from estdepth_amd import cloud_metrics as M
    pts, is_wall, gt, ref = planted
    dev = _dev(pts)
    for binding in ("torch", "ctypes"):
        f = profiled(ALL4, lambda: M.filter_clusters(dev, EPS, MIN_POINTS, min_size=MIN_SIZE), binding)
        assert f["keep"].dtype == torch.bool and (_cpu(f["keep"]) == is_wall).all()
        assert (_cpu(f["cluster"]) == ref["cluster"]).all() and (_cpu(f["sizes"]) == ref["sizes"]).all()
        assert (f["n_clusters"], f["clusters_kept"], f["kept"], f["dropped"], f["noise"]) == (4, 1, 48 * 48, 132, 12)
    assert (_cpu(M.filter_clusters(dev, EPS, MIN_POINTS, keep_largest=1)["keep"]) == is_wall).all()
    assert (_cpu(M.filter_clusters(dev, EPS, MIN_POINTS, keep_largest=3)["keep"]) == R.filter32(ref, keep_largest=3)).all()
    assert (_cpu(M.filter_clusters(dev, EPS, MIN_POINTS, min_size=40, keep_largest=2)["keep"]) == R.filter32(ref, min_size=40, keep_largest=2)).all()
    assert (_cpu(M.filter_clusters(dev, EPS, MIN_POINTS)["keep"]) == (ref["label"] >= 0)).all()                  # noise is always dropped
    assert not bool(M.filter_clusters(dev, EPS, MIN_POINTS, min_size=48 * 48 + 1)["keep"].any())
    c = M.cluster_dbscan(dev, EPS, MIN_POINTS)
    R.compare(dict({k: (_cpu(v) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}, size=ref["size"]), ref, "planted")


def test_compare_clouds_scores_the_filtered_cloud(planted):
    from estdepth_amd import cloud_metrics as M
    pts, is_wall, gt, ref = planted
    pred, truth = _dev(pts), _dev(gt)
    max_dist = 20.0 * THRESHOLD
    arg = dict(eps=EPS, min_points=MIN_POINTS, min_size=MIN_SIZE)
    got = profiled(ALL4, lambda: M.compare_clouds(pred, truth, THRESHOLD, clusters=arg))
    CM.check_metrics(got, CM.metrics64(pts[is_wall], gt, THRESHOLD, max_dist), THRESHOLD, "clusters")
    assert got["clusters"] == dict(pred=dict(n_clusters=4, kept=48 * 48, dropped=132, noise=12))
    # ... and it is the call on the cloud filtered by hand, bit for bit; the floaters did move the unfiltered scores
    by_hand = M.compare_clouds(_dev(pts[is_wall]), truth, THRESHOLD)
    assert {k: v for k, v in got.items() if k != "clusters"} == by_hand
    whole = M.compare_clouds(pred, truth, THRESHOLD)
    assert whole["accuracy"] > 1.5 * got["accuracy"] and whole["precision"] < got["precision"] == 1.0 and whole["n_pred"] == pts.shape[0]
    # normals and colours travel with the rows; both sides can be named
    up = np.tile(np.float32([0.0, 0.0, 1.0]), (pts.shape[0], 1))
    up[~is_wall] = np.float32([1.0, 0.0, 0.0])
    colour = np.where(is_wall[:, None], np.float32(100.0), np.float32(250.0)).repeat(3, 1).astype(np.float32)
    both = M.compare_clouds(pred, truth, THRESHOLD, pred_normal=_dev(up), gt_normal=_dev(np.tile(np.float32([0.0, 0.0, 1.0]), (gt.shape[0], 1))),
                            pred_color=_dev(colour), gt_color=_dev(np.full(gt.shape, 100.0, np.float32)), clusters=dict(arg, sides=("pred", "gt")))
    assert both["normal_consistency"] == 1.0 and both["color_l1"] == 0.0
    assert both["clusters"]["gt"] == dict(n_clusters=1, kept=gt.shape[0], dropped=0, noise=0) and both["clusters"]["pred"] == got["clusters"]["pred"]
    assert both["accuracy"] == got["accuracy"] and both["completeness"] == got["completeness"]
    for bad in (dict(min_points=3), dict(eps=EPS, sides=("mesh",)), dict(eps=EPS, radius=1.0), dict(eps=0.0), dict(eps=EPS, min_size=-1), [EPS]):
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: M.compare_clouds(pred, truth, THRESHOLD, clusters=bad))


def test_without_clusters_nothing_new_runs(planted):
    from estdepth_amd import cloud_metrics as M
    pts, is_wall, gt, ref = planted
    pred, truth = _dev(pts), _dev(gt)
    normal = _dev(np.tile(np.float32([0.0, 0.0, 1.0]), (pts.shape[0], 1)))
    for kw in (dict(), dict(downsample=0.03), dict(pred_normal=normal, normals=dict(k=8))):
        for binding in ("torch", "ctypes"):
            plain = profiled(set(), lambda: M.compare_clouds(pred, truth, THRESHOLD, **kw), binding)
            none = profiled(set(), lambda: M.compare_clouds(pred, truth, THRESHOLD, clusters=None, **kw), binding)
            assert plain == none and "clusters" not in plain
    mesh = dict(xyz=pred)
    assert profiled(set(), lambda: M.compare_meshes(mesh, dict(xyz=truth), 1000.0, THRESHOLD)) == M.compare_meshes(mesh, dict(xyz=truth), 1000.0, THRESHOLD, clusters=None)
    through = profiled(ALL4, lambda: M.compare_meshes(mesh, dict(xyz=truth), 1000.0, THRESHOLD, clusters=dict(eps=EPS, min_points=MIN_POINTS, min_size=MIN_SIZE)))
    assert through["clusters"]["pred"]["kept"] == 48 * 48 and through["n_pred"] == 48 * 48 and through["sampled"]["n_pred"] == 48 * 48
    with pytest.raises(RuntimeError):
        M.compare_meshes(mesh, dict(xyz=truth), 1000.0, THRESHOLD, exact=True, clusters=dict(eps=EPS))
