"""The kernels of the density-based clustering (csrc/cloud/cloud_cluster.hip) under the route protocol of
tests/test_gpu_cloud_knn_routes.py, against the numpy reference of tests/cloud_cluster_ref.py: EQUALITY of label, count, size, noise,
cluster and sizes -- every output is an integer, there is no tolerance.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel the source emits (tests/test_cloud_cluster_resources_cpu.py compiles the file and asserts
that the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

Each case of cloud_cluster_ref.CASES (and the placed ones) runs the clustering, asserts WHICH kernels ran (torch.profiler's demangled
names; none for an empty cloud), runs it under both bindings and twice: the same bits, the same bits with two other cell edges, and the
reversed cloud equals the reference of the reversed cloud.  Two cases go through the C ABI (ctypes) with every input and output carved
out of buffers filled with a sentinel: the same bits again and every band intact.  The count for queries that are not the targets is
held to the reference at every pair of cloud_metrics_ref.ROUTE_SIZES."""
import ctypes
import re

import numpy as np
import pytest
import torch

from estdepth_amd.ops import cloud_count_within, cloud_dbscan  # noqa: F401 -- the feature under test: without it this module does not import

import cloud_cluster_ref as R
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

COUNT, HOOK, FLATTEN, BORDER = "dbscan_count_kernel", "dbscan_hook_kernel", "dbscan_flatten_kernel", "dbscan_border_kernel"
INSTANCES = {
    # route: the kernels that reach it
    "cloud_count_within": [COUNT],
    "cloud_dbscan": [HOOK, FLATTEN, BORDER],          # ... after COUNT
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(dbscan_\w+_kernel)(<[^>()]*>)?")
ALL = {k for ks in INSTANCES.values() for k in ks}
_RAN = set()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def profiled(want, fn, binding="torch"):
    """run fn() under ``binding`` and the profiler; the suite's kernels that ran must be exactly ``want`` (a set; empty: no launch)"""
    with _Switches(None, binding):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            out = fn()
            torch.cuda.synchronize()
    ran = {m.group(1) + (m.group(2) or "") for e in prof.key_averages() for m in [KERNEL_RE.search(e.key)] if m}
    assert ran == set(want), "ran %s, expected %s" % (sorted(ran), sorted(want))
    _RAN.update(ran)
    return out


TENSORS = ("label", "cluster", "count", "core", "roots", "sizes")


def cluster(points, c, cell="case"):
    from estdepth_amd import cloud_metrics as M
    return M.cluster_dbscan(points, c["eps"], c["min_points"], cell=c["cell"] if cell == "case" else cell)


def same(a, b):
    """two results of cluster_dbscan, bit for bit"""
    return all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in TENSORS) and a["n_clusters"] == b["n_clusters"] and a["noise"] == b["noise"]


def as_numpy(out, size=None):
    """cluster_dbscan's dict as cloud_cluster_ref.compare takes it (``size``: the kernel's per-index array, where the case has it)"""
    got = {k: (_cpu(v) if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    n = got["label"].shape[0]
    if size is None:                                  # from what the host layer returns: sizes at the roots, 0 elsewhere
        size = np.zeros(n, np.int32)
        size[got["roots"]] = got["sizes"]
    got["size"] = size
    return got


@pytest.mark.parametrize("name", list(R.CASES) + list(R.PLACED))
def test_dbscan_route(name):
    c, want = R.expected(name)
    pts = _dev(c["points"])
    ran = {COUNT, HOOK, FLATTEN, BORDER}
    first = profiled(ran, lambda: cluster(pts, c))
    for binding in ("torch", "ctypes"):
        for again in range(2):
            assert same(first, profiled(ran, lambda: cluster(pts, c), binding)), "%s: the bits differ under %s, call %d" % (name, binding, again)
    fig = R.compare(as_numpy(first), want, name)
    assert first["roots"].dtype == torch.int64 and (_cpu(first["roots"]) == want["roots"]).all() and (_cpu(first["core"]) == want["core"]).all(), name
    # the grid is a tuning parameter: two other cell edges
    for cell in (0.37 * c["eps"], 1e7):
        assert same(first, profiled(ran, lambda: cluster(pts, c, cell))), "%s: the cell edge %g changes a bit" % (name, cell)
    # the order of the rows: the reversed cloud gives the reference's result for the reversed cloud
    rev = c["points"][::-1].copy()
    R.compare(as_numpy(under("torch", lambda: cluster(_dev(rev), c))), R.dbscan32(rev, c["eps"], c["min_points"]), name + " reversed")
    print("CLOUD-CLUSTER-ROUTE %s: eps %g, min_points %d: %s" % (name, c["eps"], c["min_points"], fig))


def test_nothing_runs_for_an_empty_cloud():
    from estdepth_amd import cloud_metrics as M
    none, some = torch.empty((0, 3), device=DEV), _dev(R.build_case("surface_65")["points"])
    for binding in ("torch", "ctypes"):
        out = profiled(set(), lambda: M.cluster_dbscan(none, 0.1, 3), binding)
        assert out["n_clusters"] == 0 and out["noise"] == 0 and all(out[k].shape == (0,) for k in TENSORS)
        f = profiled(set(), lambda: M.filter_clusters(none, 0.1, 3, min_size=2), binding)
        assert f["keep"].shape == (0,) and f["kept"] == 0 and f["dropped"] == 0
        assert profiled(set(), lambda: M.PointGrid(some, 0.1).count_within(none), binding).shape == (0,)
        # no targets: the count runs and finds nothing
        count = profiled({COUNT}, lambda: M.PointGrid(none, 0.1).count_within(some), binding)
        assert count.dtype == torch.int32 and count.shape == (some.shape[0],) and not bool(count.any())


@pytest.mark.parametrize("sizes", R.COUNT_CASES, ids=lambda s: "%dx%d" % s)
def test_count_within_route(sizes):
    from estdepth_amd import cloud_metrics as M
    c, want = R.count_case(*sizes)
    t, q = _dev(c["target"]), _dev(c["query"])
    ran = {COUNT} if sizes[1] else set()
    grid = under("torch", lambda: M.PointGrid(t, c["max_dist"]))
    first = profiled(ran, lambda: grid.count_within(q))
    assert first.dtype == torch.int32 and (_cpu(first) == want).all(), "%dx%d: %d counts differ" % (sizes + (int((_cpu(first) != want).sum()),))
    for binding in ("torch", "ctypes"):
        for again in range(2):
            assert torch.equal(first, profiled(ran, lambda: grid.count_within(q), binding))
    for cell in (0.37 * c["max_dist"], 1e7):
        other = under("torch", lambda: M.PointGrid(t, c["max_dist"], cell))
        assert torch.equal(first, profiled(ran, lambda: other.count_within(q))), "the cell edge %g changes a count" % cell
    # a smaller radius on the same grid, and the queries reversed
    half = 0.5 * c["max_dist"]
    assert (_cpu(under("torch", lambda: grid.count_within(q, half))) == R.count_within32(c["query"], c["target"], half)).all()
    assert torch.equal(first, torch.flip(under("torch", lambda: grid.count_within(torch.flip(q, [0]).contiguous())), [0]))
    with pytest.raises(RuntimeError):
        grid.count_within(q, 2.0 * c["max_dist"])


def test_the_self_count_is_the_clustering_count():
    from estdepth_amd import cloud_metrics as M
    c, want = R.expected("surface_257")
    pts = _dev(c["points"])
    count = profiled({COUNT}, lambda: M.PointGrid(pts, c["eps"]).count_within(pts))
    assert (_cpu(count) == want["count"]).all()


def raw(name):
    """estd_cloud_dbscan on guarded buffers -> (case, grid, guards)"""
    from estdepth_amd import _native, cloud_metrics as M
    c, _ = R.expected(name)
    pts = _dev(c["points"])
    n = pts.shape[0]
    grid = under("torch", lambda: M.PointGrid(pts, c["eps"], c["eps"] if c["cell"] is None else c["cell"]))
    g = dict(records=Guard(grid.records.shape, fill=grid.records), cell_start=Guard(grid.cell_start.shape, torch.int32, fill=grid.cell_start),
             count=Guard((n,), torch.int32), parent=Guard((n,), torch.int32), label=Guard((n,), torch.int32), size=Guard((n,), torch.int32),
             noise=Guard((1,), torch.int32))
    d = _native.CloudDbscanDesc()
    d.N, d.min_points = n, c["min_points"]
    d.records, d.cell_start = g["records"].t.data_ptr(), g["cell_start"].t.data_ptr()
    d.count, d.parent, d.label, d.size, d.noise = (g[k].t.data_ptr() for k in ("count", "parent", "label", "size", "noise"))
    d.cell, d.eps = grid.cell, c["eps"]
    for j in range(3):
        d.lo[j], d.dims[j] = float(grid.lo[j]), grid.dims[j]
    assert _lib().estd_cloud_dbscan(ctypes.byref(d), _stream()) == 0
    torch.cuda.synchronize()
    return c, grid, g


@pytest.mark.parametrize("name", ["surface_257", "clusters_4096"])
def test_the_c_abi_on_guarded_buffers(name):
    from estdepth_amd import ops
    c, grid, g = raw(name)
    _intact(name, **g)
    assert torch.equal(g["records"].t, grid.records) and torch.equal(g["cell_start"].t, grid.cell_start), "%s: an input was written" % name
    want = R.expected(name)[1]
    for k in ("label", "count", "size"):
        assert (_cpu(g[k].t) == want[k]).all(), (name, k)
    assert int(g["noise"].t.item()) == want["noise"]
    op = under("ctypes", lambda: ops.cloud_dbscan(grid.records, grid.cell_start, grid.lo, grid.cell, grid.dims, c["eps"], c["min_points"]))
    assert all(_same(a, g[k].t) for a, k in zip(op, ("label", "count", "size", "noise"))), "%s: the C ABI differs from the operator" % name
    parent = _cpu(g["parent"].t)
    assert ((parent >= 0) & (parent <= np.arange(parent.shape[0]))).all()       # the forest's invariant: itself or a smaller index


def test_the_count_c_abi_on_guarded_buffers_and_a_malformed_order():
    from estdepth_amd import _native, cloud_metrics as M, ops
    c, want = R.count_case(257, 257)
    t, q = _dev(c["target"]), _dev(c["query"])
    M_ = q.shape[0]
    grid = under("torch", lambda: M.PointGrid(t, c["max_dist"]))
    order = torch.sort(under("torch", lambda: ops.cloud_cell_keys(q, grid.lo, grid.cell, grid.dims)), stable=True)[1]
    for malformed in (False, True):
        o = order.clone()
        if malformed:
            o[0], o[1], o[-1] = -1, M_, 2 ** 62
        g = dict(query=Guard(q.shape, fill=q), order=Guard((M_,), torch.int64, fill=o), records=Guard(grid.records.shape, fill=grid.records),
                 cell_start=Guard(grid.cell_start.shape, torch.int32, fill=grid.cell_start), count=Guard((M_,), torch.int32))
        d = _native.CloudCountWithinDesc()
        d.M, d.N = M_, t.shape[0]
        d.query, d.order, d.records, d.cell_start, d.count = (g[k].t.data_ptr() for k in ("query", "order", "records", "cell_start", "count"))
        d.cell, d.radius = grid.cell, c["max_dist"]
        for j in range(3):
            d.lo[j], d.dims[j] = float(grid.lo[j]), grid.dims[j]
        assert _lib().estd_cloud_count_within(ctypes.byref(d), _stream()) == 0
        torch.cuda.synchronize()
        _intact("count_within", **g)
        got = _cpu(g["count"].t)
        rows = np.ones(M_, bool)
        if malformed:
            rows[_cpu(order[[0, 1, -1]])] = False                              # the three queries nobody was sent to keep the sentinel
        assert (got[rows] == want[rows]).all() and (malformed or rows.all())


def _bad_calls():
    from estdepth_amd import cloud_metrics as M, ops
    c, _ = R.expected("surface_65")
    pts = _dev(c["points"])
    grid = under("torch", lambda: M.PointGrid(pts, c["eps"]))
    order = torch.arange(pts.shape[0], device=DEV)
    s = dict(records=grid.records, cell_start=grid.cell_start, lo=grid.lo, cell=grid.cell, dims=list(grid.dims), eps=c["eps"], min_points=c["min_points"])
    nan_lo = grid.lo.clone()
    nan_lo[1] = float("nan")
    grid_bad = [dict(records=grid.records[:, :3].contiguous()), dict(records=grid.records.double()), dict(records=grid.records.cpu()),
                dict(cell_start=grid.cell_start[:-1].contiguous()), dict(cell_start=grid.cell_start.long()), dict(lo=nan_lo), dict(lo=grid.lo.to(DEV)),
                dict(cell=0.0), dict(cell=float("nan")), dict(cell=1e-39), dict(dims=[1, 1]), dict(dims=[0, 1, 1]), dict(dims=[1, 1, 1025])]
    bad_s = grid_bad + [dict(eps=0.0), dict(eps=float("nan")), dict(eps=1e20), dict(min_points=0), dict(min_points=-1), dict(min_points=2 ** 31)]
    w = dict(query=pts, order=order, records=grid.records, cell_start=grid.cell_start, lo=grid.lo, cell=grid.cell, dims=list(grid.dims), radius=c["eps"])
    bad_w = grid_bad + [dict(radius=0.0), dict(radius=float("nan")), dict(radius=1e20), dict(query=pts.double()), dict(query=pts.cpu()),
                        dict(order=order[:-1].contiguous()), dict(order=order.int())]
    return s, bad_s, w, bad_w


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    s, bad_s, w, bad_w = _bad_calls()
    for bad in bad_s:
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.cloud_dbscan(**dict(s, **bad)), binding)
    for bad in bad_w:
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.cloud_count_within(**dict(w, **bad)), binding)


def test_the_messages_are_the_same_under_both_bindings():
    from estdepth_amd import ops
    s, _, w, _ = _bad_calls()
    for op, base, kw in ((ops.cloud_dbscan, s, dict(eps=1e20)), (ops.cloud_dbscan, s, dict(min_points=0)), (ops.cloud_dbscan, s, dict(min_points=2 ** 31)),
                         (ops.cloud_dbscan, s, dict(cell=float("nan"))), (ops.cloud_count_within, w, dict(radius=1e20)),
                         (ops.cloud_count_within, w, dict(cell=float("nan")))):
        texts = []
        for binding in ("torch", "ctypes"):
            with pytest.raises(RuntimeError) as e:
                under(binding, lambda: op(**dict(base, **kw)))
            texts.append(str(e.value).split("\n")[0])
        assert texts[0] == texts[1] and texts[0].startswith(op.__name__ + ": "), texts


def test_the_host_layer_refuses_what_it_documents():
    from estdepth_amd import cloud_metrics as M
    pts = _dev(R.build_case("surface_65")["points"])
    for kw in (dict(eps=0.0), dict(eps=float("inf")), dict(min_points=0), dict(min_points=2.5), dict(min_points=True), dict(cell=0.0)):
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: M.cluster_dbscan(pts, **dict(dict(eps=0.1, min_points=3), **kw)))
    for kw in (dict(min_size=-1), dict(keep_largest=-1), dict(keep_largest=1.5)):
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: M.filter_clusters(pts, 0.1, 3, **kw))
    with pytest.raises(RuntimeError):
        M.cluster_dbscan(pts.cpu(), 0.1, 3)


def test_every_claimed_instance_ran():
    """the kernels the profiler saw under this suite's cases (one more call here, should this test run alone) are exactly the claimed ones"""
    c, _ = R.expected("surface_65")
    profiled({COUNT, HOOK, FLATTEN, BORDER}, lambda: cluster(_dev(c["points"]), c))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
