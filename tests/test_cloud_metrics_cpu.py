"""CPU side of the point-cloud scores (estdepth_amd/cloud_metrics.py, csrc/cloud_nn.hip): the closed forms of the float64 reference of
tests/cloud_metrics_ref.py, the fp32 stand-in of the contract within the bound on every case of the suite, the grid rule, read_ply, argument
errors that need no device, the ABI and the compiler's resource account of the kernels."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import cloud_metrics_ref as C
from helpers import check_desc_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference's closed forms
def test_lattice_pair_closed_form():
    a, b = C.lattice_pair()
    for q, t in ((a, b), (b, a)):
        dmin, arg = C.nearest64(q, t)
        assert (dmin == C.DELTA).all() and np.array_equal(arg, np.arange(q.shape[0]))
    lo, hi = C.metrics64(a, b, C.DELTA * 0.99, 1.0), C.metrics64(a, b, C.DELTA * 1.01, 1.0)
    assert lo["accuracy"] == C.DELTA and lo["completeness"] == C.DELTA and lo["chamfer"] == C.DELTA
    assert lo["precision"] == 0.0 and lo["recall"] == 0.0 and lo["fscore"] == 0.0
    assert hi["precision"] == 1.0 and hi["recall"] == 1.0 and hi["fscore"] == 1.0
    assert lo["precision_counts"] == (0, 0) and hi["precision_counts"] == (a.shape[0], a.shape[0])


def test_cloud_against_itself_and_half_of_itself():
    pts = C.build_case("rand_257x4096")["query"]
    dmin, arg = C.nearest64(pts, pts)
    assert (dmin == 0).all() and np.array_equal(arg, np.arange(pts.shape[0]))
    d32, i32 = C.nearest32(pts, pts, 0.15)
    assert (d32 == 0).all() and np.array_equal(i32, np.arange(pts.shape[0]))
    half = pts[::2]
    m = C.metrics64(half, pts, 1e-4, 0.15)                         # pred = every second point, gt = all of them
    assert m["accuracy"] == 0.0 and m["precision"] == 1.0
    assert m["recall_counts"] == (half.shape[0], half.shape[0]) and m["recall"] == half.shape[0] / pts.shape[0]
    assert m["fscore"] == pytest.approx(2 * m["recall"] / (1 + m["recall"]), abs=1e-15)
    assert m["completeness"] > 0


def test_empty_target_reference():
    q = C.build_case("rand_1x63")["query"]
    dmin, arg = C.nearest64(q, np.zeros((0, 3), np.float32))
    d32, i32 = C.nearest32(q, np.zeros((0, 3), np.float32), 0.15)
    assert np.isinf(dmin).all() and (arg == -1).all() and (i32 == -1).all() and (d32 == np.float32(0.15)).all()
    C.compare(d32, i32, q, np.zeros((0, 3), np.float32), 0.15, dmin, "empty")


@pytest.mark.parametrize("name", C.CASES)
def test_standin_within_bound(name):
    c = C.build_case(name)
    dmin, _ = C.nearest64(c["query"], c["target"])
    dist, index = C.nearest32(c["query"], c["target"], c["max_dist"])
    fig = C.compare(dist, index, c["query"], c["target"], c["max_dist"], dmin, name)
    if name == "one_cell":                                         # queries 0..31 are targets 31..0, each duplicated 32 places later
        assert np.array_equal(index[:32], np.arange(31, -1, -1)) and (dist[:32] == 0).all()
    if name == "sparse":
        assert fig["found"] < 0.1 * fig["n"]
    if name == "outside":
        assert 0 < fig["found"] < fig["n"]
    thr = 0.37 * c["max_dist"]
    lo, hi = C.count_bracket(dmin, thr)
    assert lo <= int((dist < np.float32(thr)).sum()) <= hi


def test_compare_rejects_wrong_results():
    c = C.build_case("rand_64x65")
    dmin, _ = C.nearest64(c["query"], c["target"])
    dist, index = C.nearest32(c["query"], c["target"], 1.0)
    C.compare(dist, index, c["query"], c["target"], 1.0, dmin)
    with pytest.raises(AssertionError):
        C.compare(dist * np.float32(1 + 2e-6), index, c["query"], c["target"], 1.0, dmin)
    with pytest.raises(AssertionError):
        C.compare(dist, (index + 1) % 64, c["query"], c["target"], 1.0, dmin)
    with pytest.raises(AssertionError):
        C.compare(np.full_like(dist, 1.0), np.full_like(index, -1), c["query"], c["target"], 1.0, dmin)


# ------------------------------------------------------------------------------------------------ grid_plan
@pytest.mark.parametrize("n_query", C.ROUTE_SIZES)
@pytest.mark.parametrize("n_target", C.ROUTE_SIZES)
def test_route_cases_standin_within_bound(n_target, n_query):
    """the clouds of tests/test_gpu_recon3d_routes.py: the fp32 stand-in passes the comparison and the tie rule the device is held to"""
    c = C.route_case(n_target, n_query)
    dist, index = C.nearest32(c["query"], c["target"], c["max_dist"])
    C.compare(dist, index, c["query"], c["target"], c["max_dist"], C.nearest64(c["query"], c["target"])[0], "route %d x %d" % (n_target, n_query))
    assert C.check_ties(index, c["target"]) == (1 if n_target > 1 and n_query > 1 else 0)
    if n_target > 1 and n_query > 1:
        assert index[0] == 0 and dist[0] == 0


@pytest.mark.parametrize("mistake", C.MISTAKES)
def test_checks_reject_each_plausible_search_mistake(mistake):
    """each plausible mistake of the search, evaluated by the fp32 stand-in, fails a check the GPU suites apply: the tie rule on exact
    duplicates, the closed form of the lattice pair at max_dist = the distance itself, the comparison on a target three cells away"""
    if mistake == "largest_index_on_ties":
        c = C.build_case("one_cell")
        dist, index = C.nearest32(c["query"], c["target"], c["max_dist"])
        assert C.check_ties(index, c["target"]) == 32
        dist, index = C.nearest32(c["query"], c["target"], c["max_dist"], mistake=mistake)
        C.compare(dist, index, c["query"], c["target"], c["max_dist"], C.nearest64(c["query"], c["target"])[0])     # the bound alone passes it
        with pytest.raises(AssertionError):
            C.check_ties(index, c["target"])
    elif mistake == "strict_radius":
        a, b = C.lattice_pair()
        C.check_lattice(*C.nearest32(a, b, C.DELTA))
        dist, index = C.nearest32(a, b, C.DELTA, mistake=mistake)
        assert (dist == np.float32(C.DELTA)).all()                  # "not found" reports max_dist too, and the bound accepts either side
        C.compare(dist, index, a, b, C.DELTA, C.nearest64(a, b)[0])
        with pytest.raises(AssertionError):
            C.check_lattice(dist, index)
    else:
        a, b = C.lattice_pair(delta=0.11)
        b[:, 2] = -b[:, 2]                                          # queries 2.2 cells below the targets' plane: three rings away
        dmin = C.nearest64(b, a)[0]
        C.compare(*C.nearest32(b, a, 0.15), b, a, 0.15, dmin)
        dist, index = C.nearest32(b, a, 0.15, mistake=mistake, cell=0.05)
        with pytest.raises(AssertionError):
            C.compare(dist, index, b, a, 0.15, dmin)


def test_grid_plan_default_rule():
    from estdepth_amd import cloud_metrics as M
    cell, dims = M.grid_plan([0, 0, 0], [2, 2, 2], 4096, 0.15)
    assert cell == float(np.float32(np.sqrt(2.0 * 4.0 / 4096))) and dims == (46, 46, 46)
    cell, dims = M.grid_plan([0, 0, 0], [4, 2, 0.5], 100, 3.2)       # a sparse cloud: sqrt(2 * 8 / 100) = 0.4 > max_dist / 32
    assert cell == float(np.float32(0.4)) and dims == (10, 5, 2)          # fl32(0.4) > 0.4: 4 / cell = 9.9999998
    cell, dims = M.grid_plan([0, 0, 0], [2, 2, 2], 10 ** 6, 1.0)     # a dense one: the floor max_dist / 32
    assert cell == 1.0 / 32 and dims == (65, 65, 65)
    cell, dims = M.grid_plan([-1, 5, 2], [1, 5.5, 3], 50, 0.15, cell=0.25)       # a given cell is kept
    assert cell == 0.25 and dims == (9, 3, 5)
    assert M.grid_plan([0, 0, 0], [2, 2, 2], 4096, 0.15, cell=2.0 - 1e-3)[1] == (2, 2, 2)
    assert M.grid_plan([0, 0, 0], [2, 2, 2], 4096, 0.15, cell=2.0)[1] == (2, 2, 2)     # floor(ext / cell) + 1: the far face has a cell of its own


def test_grid_plan_cap_enlarges_the_cell():
    from estdepth_amd import cloud_metrics as M
    cell, dims = M.grid_plan([0, 0, 0], [1000, 1, 1], 257, 0.05, cell=0.01)
    assert cell > 0.01 and max(dims) <= M.MAX_DIM and dims[0] > M.MAX_DIM / 1.2
    cell, dims = M.grid_plan([0, 0, 0], [4, 4, 4], 10 ** 6, 0.1, cell=0.005)    # 801^3 cells
    assert dims[0] * dims[1] * dims[2] <= M.MAX_CELLS < (int(4 / (cell / 1.125)) + 1) ** 3 and dims[0] == dims[1] == dims[2]
    cell, dims = M.grid_plan([0, 0, 0], [4, 4, 4], 10 ** 8, 0.05)                # the default rule runs into the cap as well
    assert dims[0] * dims[1] * dims[2] <= M.MAX_CELLS and cell > 0.05 / 32
    cell, dims = M.grid_plan([-1e30, 0, 0], [1e30, 1, 1], 10, 1.0)
    assert max(dims) <= M.MAX_DIM and np.isfinite(cell)


def test_grid_plan_degenerate_boxes_and_errors():
    from estdepth_amd import cloud_metrics as M
    assert M.grid_plan([1, 2, 3], [1, 2, 3], 1, 0.15) == (float(np.float32(0.15 / 32)), (1, 1, 1))      # a single point
    cell, dims = M.grid_plan([0, 0, 5], [2, 2, 5], 1000, 0.15)                                         # a flat box
    assert dims[2] == 1 and dims[0] == dims[1] > 1
    cell, dims = M.grid_plan([0, 7, 5], [2, 7, 5], 1000, 0.15)                                         # a line: no area, the floor
    assert cell == float(np.float32(0.15 / 32)) and dims == (int(2 / cell) + 1, 1, 1)
    for bad in (dict(lo=[0, 0], hi=[1, 1]), dict(lo=[0, 0, 0], hi=[1, 1, float("nan")]), dict(lo=[2, 0, 0], hi=[1, 1, 1]), dict(n=0),
                dict(max_dist=0.0), dict(max_dist=float("inf")), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=1e-60)):
        a = dict(dict(lo=[0, 0, 0], hi=[1, 1, 1], n=10, max_dist=0.1, cell=None), **bad)
        with pytest.raises(RuntimeError):
            M.grid_plan(a["lo"], a["hi"], a["n"], a["max_dist"], a["cell"])


def test_cells_clamp_like_the_kernel():
    """the host's dims = floor(ext / cell) + 1 hold every target without the clamp: the fp32 cell coordinate of the box maximum is below dims"""
    from estdepth_amd import cloud_metrics as M
    rng = np.random.RandomState(3)
    for _ in range(200):
        lo = rng.uniform(-100, 100, 3).astype(np.float32)
        hi = (lo + rng.uniform(0, 50, 3).astype(np.float32)).astype(np.float32)
        cell, dims = M.grid_plan(lo, hi, int(rng.randint(1, 10 ** 6)), float(rng.uniform(0.01, 2.0)))
        t = np.floor(((hi - lo).astype(np.float32) * (np.float32(1.0) / np.float32(cell))).astype(np.float32))
        assert (t <= np.array(dims)).all() and max(dims) <= M.MAX_DIM           # t == dims only through rounding; the kernel clamps it to dims - 1


# ------------------------------------------------------------------------------------------------ read_ply
def test_read_ply_round_trip(tmp_path):
    from estdepth_amd import fusion3d
    rng = np.random.RandomState(0)
    rec = rng.randn(37, 6).astype(np.float32)
    rgb = rng.randint(0, 256, size=(37, 3)).astype(np.uint8)
    fusion3d.write_ply(str(tmp_path / "a.ply"), rec, rgb)
    got = fusion3d.read_ply(str(tmp_path / "a.ply"))
    assert np.array_equal(got["xyz"], rec[:, :3]) and np.array_equal(got["normal"], rec[:, 3:]) and np.array_equal(got["rgb"], rgb)
    assert got["xyz"].dtype == np.float32 and got["rgb"].dtype == np.uint8 and got["xyz"].flags["C_CONTIGUOUS"]
    fusion3d.write_ply(str(tmp_path / "b.ply"), rec)
    got = fusion3d.read_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(got["xyz"], rec[:, :3]) and np.array_equal(got["normal"], rec[:, 3:]) and got["rgb"] is None
    fusion3d.write_ply(str(tmp_path / "e.ply"), rec[:0])
    got = fusion3d.read_ply(str(tmp_path / "e.ply"))
    assert got["xyz"].shape == (0, 3) and got["normal"].shape == (0, 3)


def test_read_ply_ascii_and_skipped_properties(tmp_path):
    from estdepth_amd import fusion3d
    p = tmp_path / "c.ply"
    p.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 2\nproperty float x\nproperty double quality\nproperty float y\n"
                 "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\n"
                 "property list uchar int vertex_indices\nend_header\n1 9.5 2 3 10 20 30\n4 9.5 5 -6.25 40 50 60\n3 0 1 0\n")
    got = fusion3d.read_ply(str(p))
    assert np.array_equal(got["xyz"], np.float32([[1, 2, 3], [4, 5, -6.25]])) and got["normal"] is None
    assert np.array_equal(got["rgb"], np.uint8([[10, 20, 30], [40, 50, 60]]))
    # binary: an extra short and an extra double between the coordinates, faces behind the vertices
    dt = np.dtype([("x", "<f4"), ("flag", "<i2"), ("y", "<f4"), ("z", "<f4"), ("t", "<f8"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")])
    rec = np.zeros(3, dtype=dt)
    for k in ("x", "y", "z", "nx", "ny", "nz", "t"):
        rec[k] = np.random.RandomState(len(k)).randn(3)
    rec["flag"] = [1, -2, 3]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty short flag\nproperty float y\nproperty float z\n"
            "property double t\nproperty float nx\nproperty float ny\nproperty float nz\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
    q = tmp_path / "d.ply"
    q.write_bytes(head.encode() + rec.tobytes() + bytes([3]) + np.int32([0, 1, 2]).tobytes())
    got = fusion3d.read_ply(str(q))
    assert np.array_equal(got["xyz"], np.stack([rec["x"], rec["y"], rec["z"]], 1)) and np.array_equal(got["normal"], np.stack([rec["nx"], rec["ny"], rec["nz"]], 1))
    assert got["rgb"] is None


def test_read_ply_rejects(tmp_path):
    from estdepth_amd import fusion3d
    body = np.zeros(6, dtype="<f4").tobytes()
    xyz = "property float x\nproperty float y\nproperty float z\n"
    files = {
        "big": b"ply\nformat binary_big_endian 1.0\nelement vertex 2\n" + xyz.encode() + b"end_header\n" + body,
        "magic": b"plx\nformat binary_little_endian 1.0\nelement vertex 2\n" + xyz.encode() + b"end_header\n" + body,
        "noend": b"ply\nformat binary_little_endian 1.0\nelement vertex 2\n" + xyz.encode() + body,
        "short": b"ply\nformat binary_little_endian 1.0\nelement vertex 3\n" + xyz.encode() + b"end_header\n" + body,
        "noz": b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nend_header\n" + body,
        "double": b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty double x\nproperty double y\nproperty double z\nend_header\n" + body * 2,
        "novertex": b"ply\nformat binary_little_endian 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n",
        "type": b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty quad x\nend_header\n" + body,
        "ascii_short": b"ply\nformat ascii 1.0\nelement vertex 2\n" + xyz.encode() + b"end_header\n1 2 3\n",
        "ascii_text": b"ply\nformat ascii 1.0\nelement vertex 2\n" + xyz.encode() + b"end_header\n1 2 3\n4 five 6\n",
        "ascii_cols": b"ply\nformat ascii 1.0\nelement vertex 2\n" + xyz.encode() + b"end_header\n1 2 3 4\n4 5 6 7\n",
        "noformat": b"ply\nelement vertex 2\n" + xyz.encode() + b"end_header\n" + body,
    }
    for name, data in files.items():
        p = tmp_path / (name + ".ply")
        p.write_bytes(data)
        with pytest.raises(RuntimeError, match="read_ply"):
            fusion3d.read_ply(str(p))


# ------------------------------------------------------------------------------------------------ argument errors without a device
def test_argument_errors_need_no_device():
    from estdepth_amd import cloud_metrics as M
    a, b = torch.zeros(5, 3), torch.ones(7, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.compare_clouds(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.nearest(a, b, 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.PointGrid(a, 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.voxel_downsample(a, 0.02)
    for kw in (dict(threshold=0.0), dict(threshold=float("nan")), dict(threshold=0.05, max_dist=0.01), dict(max_dist=0.0), dict(max_dist=float("inf")),
               dict(max_dist=1e30), dict(downsample=0.0), dict(downsample=-0.02)):
        with pytest.raises(RuntimeError, match="compare_clouds"):
            M.compare_clouds(a, b, **kw)
    with pytest.raises(RuntimeError):
        M.compare_clouds(a.numpy(), b)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, None, "1"):
        with pytest.raises(RuntimeError, match="max_dist"):
            M.nearest(a, b, bad)
    with pytest.raises(RuntimeError, match="cell"):
        M.PointGrid(a, 0.1, cell=0.0)
    with pytest.raises(RuntimeError, match="cell"):
        M.voxel_downsample(a, 0.0)


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from estdepth_amd import _native, build
    build.build()
    return _native.lib()


def test_entry_points_validate_before_launch(lib):
    from estdepth_amd import _native
    assert lib.estd_cloud_nearest(None, None) == -1
    d = _native.CloudNearestDesc()
    assert lib.estd_cloud_nearest(ctypes.byref(d), None) == -1               # max_dist = 0
    d.max_dist = 0.1
    assert lib.estd_cloud_nearest(ctypes.byref(d), None) == 0                # M = 0: nothing to do, no launch
    d.M = 4
    assert lib.estd_cloud_nearest(ctypes.byref(d), None) == -1               # null query / outputs
    d.M, d.N = 0, 4
    assert lib.estd_cloud_nearest(ctypes.byref(d), None) == -1               # targets without records or a grid
    d.M, d.N = -1, 0
    assert lib.estd_cloud_nearest(ctypes.byref(d), None) == -1
    d.M, d.max_dist = 0, 1e30
    assert lib.estd_cloud_nearest(ctypes.byref(d), None) == -1               # max_dist^2 leaves fp32
    lo, dims = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int * 3)(1, 1, 1)
    assert lib.estd_cloud_cell_keys(None, 0, lo, 0.1, dims, None, None) == 0
    assert lib.estd_cloud_cell_keys(None, 5, lo, 0.1, dims, None, None) == -1
    assert lib.estd_cloud_cell_keys(None, 0, lo, 0.0, dims, None, None) == -1
    assert lib.estd_cloud_cell_keys(None, 0, None, 0.1, dims, None, None) == -1
    assert lib.estd_cloud_cell_keys(None, 0, lo, 0.1, (ctypes.c_int * 3)(1, 0, 1), None, None) == -1
    assert lib.estd_cloud_cell_keys(None, 0, lo, 0.1, (ctypes.c_int * 3)(1, (1 << 20) + 1, 1), None, None) == -1
    assert lib.estd_cloud_cell_centroids(None, None, 0, 0, None, None, 0, None, None, None) == 0
    assert lib.estd_cloud_cell_centroids(None, None, 0, 5, None, None, 2, None, None, None) == -1
    assert lib.estd_cloud_cell_centroids(None, None, 7, 5, None, None, 0, None, None, None) == -1
    assert lib.estd_cloud_cell_centroids(None, None, 0, 1, None, None, 2, None, None, None) == -1


def test_cloud_nearest_desc_struct_layout(lib, tmp_path):
    """sizeof/offsetof of estd_cloud_nearest_desc as the C compiler sees it == the ctypes mirror"""
    from estdepth_amd import _native, ops
    limits = check_desc_layout(tmp_path, "estd_cloud_nearest_desc", _native.CloudNearestDesc,
                               macros=["ESTD_CLOUD_KEY_MAX_DIM", "ESTD_CLOUD_MAX_DIM", "ESTD_CLOUD_MAX_CELLS", "ESTD_CLOUD_MAX_ATTRS"])
    assert limits == [ops.CLOUD_KEY_MAX_DIM, ops.CLOUD_MAX_DIM, ops.CLOUD_MAX_CELLS, ops.CLOUD_MAX_ATTRS]


def test_cloud_kernels_use_no_scratch_and_spill_nothing():
    """every cloud_* kernel instance of csrc/cloud_nn.hip: scratch 0, no VGPR / SGPR spill in the compiler's resource account"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is not installed")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rec, _ = kr.resource_usage(os.path.join(kr.CSRC, "cloud_nn.hip"), isa=False)
    names = kr.demangle(list(rec))
    inst = {names.get(k, k): v for k, v in rec.items() if "cloud_" in names.get(k, k)}
    assert len(inst) >= 4, sorted(names.values())                            # keys, nearest with and without STATS, centroids
    for name, d in inst.items():
        print(name, d)
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d, (name, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (name, d)
