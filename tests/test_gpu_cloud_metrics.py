"""csrc/cloud_nn.hip and estdepth_amd/cloud_metrics.py on the device against the float64 reference of tests/cloud_metrics_ref.py, under both
bindings: every case of cloud_metrics_ref.CASES and a 200 000 x 200 000 surface case under the comparison rule of the reference (BOUND = 7 u
relative to the distance, no leave-out share); independence of the search grid (three cell edges, two bindings, two calls: identical bits);
empty clouds; malformed arguments; voxel_downsample against a float64 group-by; compare_clouds against the reference's numbers; and the
semantic test on the fixtures of tsdf_ref.py: a fused volume scored against points of the analytic surface, clean and with every depth scaled
by 1.02 -- all bars from the float64 reference on the same clouds.

Figures of the device run (this file prints them, pytest -s): profiles/cloud_metrics_gpu_tests.txt."""
import numpy as np
import pytest
import torch

import cloud_metrics_ref as C
import tsdf_ref as R
from helpers import _binding

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BINDINGS = ["torch", "ctypes"]
_REFS = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(name):
    """the case and its float64 minimum distances, once"""
    if name not in _REFS:
        c = C.build_case(name)
        _REFS[name] = (c, C.nearest64(c["query"], c["target"])[0])
    return _REFS[name]


def _nearest(c, cell):
    from estdepth_amd import cloud_metrics as M
    dist, index = M.nearest(_dev(c["query"]), _dev(c["target"]), c["max_dist"], cell=cell)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), index.cpu().numpy()


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("where", ["d64", "d64-rotated", "d512"])
def test_nearest_away_from_the_origin(where):
    """64 targets and 65 queries built 64 m and 512 m out and in the turned world (tests/placement.py; the case "translated" adds its 100 m
    to fp32 data): the bound stays relative to the DISTANCE, because the difference of two nearby fp32 coordinates is exact wherever they
    lie; the grid's corner is the target's own minimum and moves with it"""
    import placement as PL
    c = C.build_case(C.PLACED_CASE, PL.PLACES[where])
    dmin = C.nearest64(c["query"], c["target"])[0]
    dist, index = _nearest(c, None)
    fig = C.compare(dist, index, c["query"], c["target"], c["max_dist"], dmin, c["name"])
    print("PLACEMENT cloud_nearest %s: %d of %d found; of the bound: dist %.3f index %.3f" % (c["name"], fig["found"], fig["n"], fig["e_dist"], fig["e_index"]))
    assert fig["found"] >= 1 and float(np.abs(c["target"]).min()) > PL.PLACES[where][0] / 4


@pytest.mark.parametrize("binding", BINDINGS)
@pytest.mark.parametrize("name", C.CASES)
def test_nearest_against_reference(name, binding, monkeypatch):
    _binding(monkeypatch, binding)
    c, dmin = _case(name)
    dist, index = _nearest(c, c["cell"])
    fig = C.compare(dist, index, c["query"], c["target"], c["max_dist"], dmin, "%s %s" % (name, binding))
    if name == "one_cell":                      # exact duplicates: queries 0..31 ARE targets 31..0 and 63..32 -- the smallest index wins
        assert np.array_equal(index[:32], np.arange(31, -1, -1)) and (dist[:32] == 0).all()
    if name == "sparse":
        assert 0 < fig["found"] < 0.1 * fig["n"]
    if name in ("outside", "clusters"):
        assert 0 < fig["found"] < fig["n"]
    thr = 0.37 * c["max_dist"]
    lo, hi = C.count_bracket(dmin, thr)
    assert lo <= int((dist < np.float32(thr)).sum()) <= hi


def test_surface_200k():
    """200 000 points of the analytic plane + sphere from one camera against 200 000 from another; the reference runs chunked on the device"""
    from estdepth_amd import cloud_metrics as M
    poses, K = R.scene_poses(2, seed=5), R.intrinsics(400, 500)
    target, query = C.surface_points(poses[0], K, 400, 500), C.surface_points(poses[1], K, 400, 500)
    assert target.shape == (200000, 3) and query.shape == (200000, 3)
    dmin, _ = C.nearest64(query, target, device=DEV)
    dist, index, examined = M.PointGrid(_dev(target), 0.15).query(_dev(query), stats=True)
    torch.cuda.synchronize()
    fig = C.compare(dist.cpu().numpy(), index.cpu().numpy(), query, target, 0.15, dmin, "surface 200k")
    print("cloud_nearest surface 200k: %.1f candidates examined per query (max %d)" % (examined.double().mean().item(), examined.max().item()))
    assert fig["found"] > 150000
    plain = M.PointGrid(_dev(target), 0.15).query(_dev(query))
    assert torch.equal(plain[0].view(torch.int32), dist.view(torch.int32)) and torch.equal(plain[1], index)     # the STATS instance: same bits


# ------------------------------------------------------------------------------------------------ independence of the structure
@pytest.mark.parametrize("name", ["rand_4096x4096", "rand_1x63", "outside", "one_cell", "cell_faces", "translated", "clusters"])
def test_cell_edge_never_changes_a_bit(name, monkeypatch):
    from estdepth_amd import cloud_metrics as M
    c, _ = _case(name)
    t = c["target"].astype(np.float64)
    default = M.grid_plan(t.min(0), t.max(0), t.shape[0], c["max_dist"])[0]
    results = []
    for binding in BINDINGS:
        _binding(monkeypatch, binding)
        for cell in (None, 4 * default, 1e7, None):             # the default, 4 x the default, one cell for everything, the default again
            if cell == 1e7:
                assert M.grid_plan(t.min(0), t.max(0), t.shape[0], c["max_dist"], cell)[1] == (1, 1, 1)
            results.append(_nearest(c, cell))
    for dist, index in results[1:]:
        assert np.array_equal(dist.view(np.uint32), results[0][0].view(np.uint32)) and np.array_equal(index, results[0][1])


# ------------------------------------------------------------------------------------------------ everything else
@pytest.mark.parametrize("binding", BINDINGS)
def test_empty_target_and_empty_query(binding, monkeypatch):
    from estdepth_amd import cloud_metrics as M
    _binding(monkeypatch, binding)
    pts = _dev(C.build_case("rand_64x65")["query"])
    none = torch.empty((0, 3), device=DEV)
    dist, index = M.nearest(pts, none, 0.15)
    assert dist.shape == (65,) and bool((dist == np.float32(0.15)).all()) and bool((index == -1).all()) and index.dtype == torch.int64
    dist, index = M.nearest(none, pts, 0.15)
    assert dist.shape == (0,) and index.shape == (0,) and dist.dtype == torch.float32 and index.dtype == torch.int64
    dist, index = M.nearest(none, none, 0.15)
    assert dist.shape == (0,) and index.shape == (0,)
    m = M.compare_clouds(pts, none)
    assert m["precision"] == 0 and m["recall"] == 0 and m["fscore"] == 0 and m["clamped_pred"] == 65 and m["accuracy"] == pytest.approx(1.0, abs=1e-7)
    out, att, counts = M.voxel_downsample(none, 0.02)
    assert out.shape == (0, 3) and att is None and counts.shape == (0,)


@pytest.mark.parametrize("binding", BINDINGS)
def test_malformed_arguments_raise(binding, monkeypatch):
    from estdepth_amd import cloud_metrics as M
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    c = C.build_case("rand_64x65")
    q, t = _dev(c["query"]), _dev(c["target"])
    grid = M.PointGrid(t, 0.15)
    order = torch.arange(65, device=DEV)
    good = dict(query=q, order=order, records=grid.records, cell_start=grid.cell_start, lo=grid.lo, cell=grid.cell, dims=grid.dims, max_dist=0.15)

    def run(**kw):
        a = dict(good, **kw)
        return ops.cloud_nearest(a["query"], a["order"], a["records"], a["cell_start"], a["lo"], a["cell"], a["dims"], a["max_dist"])
    nan_lo = grid.lo.clone()
    nan_lo[1] = float("nan")
    for bad in (dict(query=q.double()), dict(query=q.cpu()), dict(query=q[:, :2]), dict(query=torch.zeros(65, 6, device=DEV)[:, ::2]), dict(query=q.reshape(-1)),
                dict(order=order[:64]), dict(order=order.int()), dict(order=order.cpu()), dict(records=grid.records[:, :3].contiguous()),
                dict(records=grid.records.cpu()), dict(records=grid.records.double()), dict(cell_start=grid.cell_start[:-1].contiguous()),
                dict(cell_start=grid.cell_start.long()), dict(cell_start=grid.cell_start.cpu()), dict(lo=grid.lo.to(DEV)), dict(lo=grid.lo[:2]),
                dict(lo=grid.lo.double()), dict(lo=nan_lo), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=1e-42),
                dict(dims=(1, 1)), dict(dims=(0, 1, 1)), dict(dims=(2000, 1, 1)), dict(dims=(512, 512, 512)), dict(dims=(grid.dims[0] + 1,) + grid.dims[1:]),
                dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(max_dist=1e30)):
        with pytest.raises(RuntimeError):
            run(**bad)
    for bad in (dict(points=q.double()), dict(points=q.cpu()), dict(points=q[:, :2]), dict(lo=grid.lo.to(DEV)), dict(cell=0.0), dict(dims=(0, 1, 1)),
                dict(dims=((1 << 20) + 1, 1, 1))):
        a = dict(dict(points=q, lo=grid.lo, cell=grid.cell, dims=grid.dims), **bad)
        with pytest.raises(RuntimeError):
            ops.cloud_cell_keys(a["points"], a["lo"], a["cell"], a["dims"])
    seg = torch.tensor([0, 30, 65], device=DEV)
    for bad in (dict(points=q.cpu()), dict(attrs=torch.zeros(65, 7, device=DEV)), dict(attrs=torch.zeros(64, 3, device=DEV)), dict(order=order[:10]),
                dict(order=order.int()), dict(segments=seg.int()), dict(segments=seg.cpu()), dict(segments=torch.zeros(67, dtype=torch.int64, device=DEV)),
                dict(segments=torch.zeros(0, dtype=torch.int64, device=DEV))):
        a = dict(dict(points=q, attrs=None, order=order, segments=seg), **bad)
        with pytest.raises(RuntimeError):
            ops.cloud_cell_centroids(a["points"], a["attrs"], a["order"], a["segments"])
    # the host layer: non-finite rows, shapes, dtypes, CPU tensors
    inf_q = q.clone()
    inf_q[7, 2] = float("inf")
    nan_t = t.clone()
    nan_t[0, 0] = float("nan")
    for a, b in ((inf_q, t), (q, nan_t), (q.double(), t), (q, t.half()), (q[:, :2], t), (q, t.reshape(-1)), (q.cpu(), t), (q, t.cpu()), (q.cpu(), t.cpu())):
        with pytest.raises(RuntimeError):
            M.nearest(a, b, 0.15)
        with pytest.raises(RuntimeError):
            M.compare_clouds(a, b)
    for kw in (dict(pred_normal=t, gt_normal=t), dict(pred_color=q.double(), gt_color=t), dict(pred_normal=q.cpu(), gt_normal=t), dict(threshold=0.2, max_dist=0.1)):
        with pytest.raises(RuntimeError):
            M.compare_clouds(q, t, **kw)
    with pytest.raises(RuntimeError):
        M.voxel_downsample(inf_q, 0.02)
    with pytest.raises(RuntimeError):
        M.voxel_downsample(q, 0.02, attrs=torch.zeros(65, 7, device=DEV))
    with pytest.raises(RuntimeError):
        M.voxel_downsample(q, 1e-9)                                  # more than 2^20 cells per axis
    dist, index = run()                                               # a well-formed call still works
    torch.cuda.synchronize()
    assert dist.shape == (65,) and index.shape == (65,)


def _keys32(points, cell):
    """the cell keys of estd_cloud_cell_keys in numpy fp32 (a subtraction, a multiplication, a floor: nothing to fuse) -> (keys, dims)"""
    lo, hi = points.min(0), points.max(0)
    dims = [int(np.floor((float(hi[j]) - float(lo[j])) / float(np.float32(cell)))) + 1 for j in range(3)]
    inv = np.float32(1.0) / np.float32(cell)
    c = [np.clip(np.floor(((points[:, j] - lo[j]).astype(np.float32) * inv).astype(np.float32)), 0, dims[j] - 1).astype(np.int64) for j in range(3)]
    return (c[2] * dims[1] + c[1]) * dims[0] + c[0], dims


@pytest.mark.parametrize("binding", BINDINGS)
def test_voxel_downsample(binding, monkeypatch):
    from estdepth_amd import cloud_metrics as M
    from estdepth_amd import ops
    _binding(monkeypatch, binding)
    rng = np.random.RandomState(11)
    pts = rng.uniform(0.5, 2.5, size=(5000, 3)).astype(np.float32)
    pts[4000:] = pts[:1000]                                           # exact duplicates share a cell
    attrs = rng.uniform(0.25, 1.0, size=(5000, 6)).astype(np.float32)
    cell = 0.13
    keys, dims = _keys32(pts, cell)
    got_keys = ops.cloud_cell_keys(_dev(pts), torch.from_numpy(pts.min(0)), float(np.float32(cell)), dims)
    assert np.array_equal(got_keys.cpu().numpy(), keys)
    ref_pts, ref_att, ref_counts = C.downsample64(pts, keys, attrs)
    out, att, counts = M.voxel_downsample(_dev(pts), cell, _dev(attrs))
    torch.cuda.synchronize()
    assert out.shape == ref_pts.shape and att.shape == ref_att.shape and 1000 < out.shape[0] < 4000
    assert np.array_equal(counts.cpu().numpy(), ref_counts) and int(counts.sum().item()) == 5000 and counts.dtype == torch.int64
    e_pts = np.abs(out.cpu().numpy().astype(np.float64) - ref_pts) / np.abs(ref_pts)
    e_att = np.abs(att.cpu().numpy().astype(np.float64) - ref_att) / np.abs(ref_att)
    print("voxel_downsample %s: %d cells of %d points, means within %.3f u (points) and %.3f u (attributes) of float64" % (binding, out.shape[0], 5000, e_pts.max() / C.U, e_att.max() / C.U))
    assert e_pts.max() <= C.U and e_att.max() <= C.U                   # one rounding of the float64 mean
    out_keys, _ = _keys32(np.concatenate([pts.min(0)[None], out.cpu().numpy(), pts.max(0)[None]]), cell)
    assert (np.diff(out_keys[1:-1]) > 0).all() and np.array_equal(out_keys[1:-1], np.unique(keys))     # one point per cell, ascending key
    again = M.voxel_downsample(_dev(pts), cell, _dev(attrs))
    assert torch.equal(again[0].view(torch.int32), out.view(torch.int32)) and torch.equal(again[1].view(torch.int32), att.view(torch.int32))
    only, none, counts2 = M.voxel_downsample(_dev(pts), cell)
    assert none is None and torch.equal(only.view(torch.int32), out.view(torch.int32)) and torch.equal(counts2, counts)


@pytest.mark.parametrize("binding", BINDINGS)
def test_compare_clouds_against_reference(binding, monkeypatch):
    from estdepth_amd import cloud_metrics as M
    _binding(monkeypatch, binding)
    a, b = C.lattice_pair()
    for thr, share in ((C.DELTA * 0.99, 0.0), (C.DELTA * 1.01, 1.0)):       # precision flips from 0 to 1 across threshold = delta
        got = M.compare_clouds(_dev(a), _dev(b), threshold=thr, max_dist=1.0)
        C.check_metrics(got, C.metrics64(a, b, thr, 1.0), thr, "lattice %s" % binding)
        assert got["precision"] == share and got["recall"] == share and got["fscore"] == share and got["clamped_pred"] == 0 and got["clamped_gt"] == 0
        assert got["accuracy"] == pytest.approx(C.DELTA, rel=1e-14) and got["completeness"] == pytest.approx(C.DELTA, rel=1e-14)
        assert got["accuracy_median"] == C.DELTA                      # the z differences are exact and sqrt(fl(x^2)) = x
    got = M.compare_clouds(_dev(a), _dev(a), threshold=0.01)
    assert got["accuracy"] == 0 and got["chamfer"] == 0 and got["fscore"] == 1
    half = a[::2]
    got = M.compare_clouds(_dev(half), _dev(a), threshold=0.01)
    assert got["precision"] == 1 and got["recall"] == half.shape[0] / a.shape[0] and got["accuracy"] == 0
    c = C.build_case("rand_4096x257")
    ref = C.metrics64(c["query"], c["target"], 0.083, 0.15)
    got = M.compare_clouds(_dev(c["query"]), _dev(c["target"]), threshold=0.083, max_dist=0.15)
    C.check_metrics(got, ref, 0.083, "random %s" % binding)
    assert got["clamped_pred"] == int((ref["d_pred"] > np.float32(0.15)).sum()) and got["clamped_gt"] == int((ref["d_gt"] > np.float32(0.15)).sum()) > 0
    assert got["accuracy_median"] == pytest.approx(np.sort(np.minimum(ref["d_pred"], np.float32(0.15)))[(ref["n_pred"] - 1) // 2], rel=C.BOUND)
    # normals and colours: the nearest neighbour's attribute is the one compared
    n_t = np.tile(np.float32([[0, 0, 1]]), (c["target"].shape[0], 1))
    n_q = np.tile(np.float32([[0, 0.6, -0.8]]), (c["query"].shape[0], 1))
    got = M.compare_clouds(_dev(c["query"]), _dev(c["target"]), threshold=0.083, max_dist=0.15, pred_normal=_dev(n_q), gt_normal=_dev(n_t),
                           pred_color=_dev(n_q), gt_color=_dev(n_t))
    assert got["normal_consistency"] == pytest.approx(0.8, abs=1e-6) and got["color_l1"] == pytest.approx((0 + 0.6 + 1.8) / 3, abs=1e-6)
    ds = M.compare_clouds(_dev(c["query"]), _dev(c["target"]), threshold=0.083, max_dist=0.15, downsample=0.2, pred_normal=_dev(n_q), gt_normal=_dev(n_t))
    assert ds["n_pred"] <= 257 and ds["n_gt"] < 1500 and ds["normal_consistency"] == pytest.approx(0.8, abs=1e-6)      # at most 11^3 cells of 0.2 m


def _fused_cloud(c, scale):
    from estdepth_amd.fusion3d import TSDFVolume
    vol = TSDFVolume(c["dims"], c["voxel"], c["origin"], device=DEV)
    vol.integrate(_dev(c["depths"] * np.float32(scale)), torch.from_numpy(c["poses"]), torch.from_numpy(c["K"]))
    return vol, vol.extract_points()["xyz"].contiguous()


def test_semantic_scaled_depth_scores_worse():
    """the t3 fixture of tsdf_ref.py fused clean and with every depth scaled by 1.02, each scored against points of the analytic surface
    (the cameras' own views at twice the resolution); every bar comes from the float64 reference on the same two clouds"""
    from estdepth_amd import cloud_metrics as M
    c = R.build_case("t3")
    H, W = c["depths"].shape[1:]
    K2 = R.intrinsics(2 * H, 2 * W)
    gt = np.concatenate([C.surface_points(P, K2, 2 * H, 2 * W) for P in c["poses"]])
    thr, md = c["voxel"], 1.0
    got, ref = {}, {}
    for name, scale in (("clean", 1.0), ("scaled", 1.02)):
        _, pred = _fused_cloud(c, scale)
        got[name] = M.compare_clouds(pred, _dev(gt), threshold=thr, max_dist=md)
        ref[name] = C.metrics64(pred.cpu().numpy(), gt, thr, md, device=DEV)
        C.check_metrics(got[name], ref[name], thr, "semantic %s" % name)          # accuracy equals the reference's within the bound
        print("cloud_metrics semantic %s: %d fused points against %d analytic points; float64 reference accuracy %.6f completeness %.6f "
              "precision %.4f recall %.4f fscore %.4f (threshold %.3f); device accuracy %.6f fscore %.4f"
              % (name, ref[name]["n_pred"], ref[name]["n_gt"], ref[name]["accuracy"], ref[name]["completeness"], ref[name]["precision"],
                 ref[name]["recall"], ref[name]["fscore"], thr, got[name]["accuracy"], got[name]["fscore"]))
    ratio_ref = ref["scaled"]["accuracy"] / ref["clean"]["accuracy"]
    ratio = got["scaled"]["accuracy"] / got["clean"]["accuracy"]
    print("cloud_metrics semantic: accuracy ratio scaled / clean %.4f (float64 reference %.4f); fscore %.4f -> %.4f"
          % (ratio, ratio_ref, got["clean"]["fscore"], got["scaled"]["fscore"]))
    assert ref["clean"]["n_pred"] > 5000 and ratio_ref > 1
    assert got["scaled"]["accuracy"] > got["clean"]["accuracy"] and abs(ratio - ratio_ref) <= 0.01 * ratio_ref
    assert got["scaled"]["fscore"] < got["clean"]["fscore"]


def test_volume_compare_with_itself_and_colour():
    from estdepth_amd.fusion3d import TSDFVolume
    c = R.build_case("t1")
    vol, pred = _fused_cloud(c, 1.0)
    m = vol.compare(vol)
    assert m["accuracy"] == 0 and m["completeness"] == 0 and m["fscore"] == 1 and m["n_pred"] == m["n_gt"] == pred.shape[0] > 1000
    assert 0.99 < m["normal_consistency"] <= 1.0 + 1e-6 and "color_l1" not in m              # unit normals (zero vectors where the gradient vanishes)
    cloud = {k: v.cpu().numpy() for k, v in vol.extract_points().items() if k in ("xyz", "normal")}
    m = vol.compare(cloud, threshold=0.03)                             # a dict of numpy arrays, as read_ply returns
    assert m["accuracy"] == 0 and m["fscore"] == 1
    with pytest.raises(RuntimeError):
        vol.compare({"normal": cloud["normal"]})
    col = TSDFVolume(c["dims"], c["voxel"], c["origin"], device=DEV, color=True)
    H, W = c["depths"].shape[1:]
    img = torch.rand((1, 3, H, W), device=DEV)
    col.integrate(_dev(c["depths"]), torch.from_numpy(c["poses"]), torch.from_numpy(c["K"]), images=img)
    m = col.compare(col)
    assert m["color_l1"] == 0 and m["accuracy"] == 0 and m["fscore"] == 1
    assert "color_l1" not in col.compare(vol)
