"""The kernels of the k-nearest-neighbour search and the PCA normals (csrc/cloud/cloud_knn.hip) under the route protocol of
tests/test_gpu_mesh_simplify_routes.py, against the numpy reference of tests/cloud_knn_ref.py: EQUALITY TO THE BIT of dist, index, count
and the covariance sums; the eigenvalues, the residual of the normal and its angle to numpy.linalg.eigh's within the bounds derived there.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel the source emits (tests/test_cloud_knn_resources_cpu.py compiles the file and asserts
that the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

Each case of cloud_knn_ref.CASES (and the placed ones) runs the search and the normals over its lists, asserts WHICH kernels ran
(torch.profiler's demangled names; none for empty inputs), runs everything under both bindings and twice: bit-identical, the same bits
with two explicit cell edges and with the query order reversed.  Two cases go through the C ABI (ctypes) with every input and output
carved out of buffers filled with a sentinel: the same bits again and every band intact -- for estd_cloud_normals with an index array
that names -1, N, 2^31 - 1 and -2^31 at the first row, the last and either side of two wave boundaries."""
import ctypes
import re

import numpy as np
import pytest
import torch

from estdepth_amd.ops import cloud_knn, cloud_normals  # noqa: F401 -- the feature under test: without it this module does not import

import cloud_knn_ref as R
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import SENT32, Guard, _cpu, _dev, _intact, _lib, _p, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernels that reach it
    "cloud_knn": ["knn_search_kernel<false>", "knn_search_kernel<true>"],
    "cloud_normals": ["knn_normals_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(knn_\w+_kernel)(<[^>()]*>)?")
ALL = {k for ks in INSTANCES.values() for k in ks}
SEARCH, SEARCH_STATS, NORMALS = "knn_search_kernel<false>", "knn_search_kernel<true>", "knn_normals_kernel"
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


def _grid(target, max_dist, cell):
    from estdepth_amd import cloud_metrics as M
    return M.PointGrid(target, max_dist, cell)


def search_and_fit(grid, q, k, toward, stats=False):
    """the two operators as cloud_metrics chains them -> (dist, index, count, normal, eig, valid, invalid, cov[, stats])"""
    from estdepth_amd import ops
    out = grid.knn(q, k, stats=stats)
    fit = ops.cloud_normals(grid.target, q, out[1], out[2], toward, cov=True)
    return tuple(out[:3]) + tuple(fit) + tuple(out[3:])


def same(a, b):
    """tuples of tensors, bit for bit (the one-byte ``valid`` is compared as it is)"""
    return len(a) == len(b) and all(torch.equal(x, y) if x.element_size() == 1 else _same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(R.CASES) + list(R.PLACED))
def test_knn_route(name):
    c, want = R.expected(name)
    t, q, k = _dev(c["target"]), _dev(c["query"]), c["k"]
    toward = None if c["toward"] is None else _dev(np.asarray(c["toward"], np.float32))
    grid = under("torch", lambda: _grid(t, c["max_dist"], c["cell"]))
    ran = {SEARCH, NORMALS}
    first = profiled(ran, lambda: search_and_fit(grid, q, k, toward))
    for binding in ("torch", "ctypes"):
        for again in range(2):
            assert same(first, profiled(ran, lambda: search_and_fit(grid, q, k, toward), binding)), "%s: the bits differ under %s, call %d" % (name, binding, again)
    # the grid is a tuning parameter: two explicit cell edges, and the STATS instance
    for cell in (0.37 * c["max_dist"], 1e7):
        other = under("torch", lambda: _grid(t, c["max_dist"], cell))
        assert same(first[:3], profiled({SEARCH}, lambda: other.knn(q, k))), "%s: the cell edge %g changes a bit" % (name, cell)
    st = profiled({SEARCH_STATS}, lambda: grid.knn(q, k, stats=True))
    assert same(first[:3], st[:3]) and st[3].dtype == torch.int32 and int(st[3].min()) >= 0, name
    # the order the queries are taken in: reversed, the rows come back reversed
    rev = torch.flip(q, [0]).contiguous()
    back = [torch.flip(x, [0]) for x in under("torch", lambda: grid.knn(rev, k))]
    assert same(first[:3], back), "%s: the query order changes a bit" % name
    got = tuple(_cpu(x) for x in first[:3])
    fig = R.compare_knn(got, want, c, name)
    if name != "257x4096_k16":
        R.compare_knn64(got, c, name)
    d1, i1 = under("torch", lambda: grid.query(q))
    assert _same(first[0][:, 0].contiguous(), d1) and torch.equal(first[1][:, 0].long(), i1), "%s: column 0 is not cloud_nearest's result" % name
    fit = dict(normal=_cpu(first[3]), eig=_cpu(first[4]), valid=_cpu(first[5]), invalid=int(first[6].item()), cov=_cpu(first[7]))
    fig.update(R.compare_normals(fit, c, got[1], got[2], name))
    if name in R.DEGENERATE:
        assert fig["valid"] == 0 and (fit["eig"][:, :2] == 0).all(), name
    print("CLOUD-KNN-ROUTE %s: %d x %d at k = %d: %s; %.1f candidates per query" % (name, c["target"].shape[0], c["query"].shape[0], k, fig, float(st[3].double().mean())))


def test_nothing_runs_for_empty_inputs():
    from estdepth_amd import ops
    t, none = _dev(R.build_case("5x3_k8")["target"]), torch.empty((0, 3), device=DEV)
    for binding in ("torch", "ctypes"):
        dist, index, count = profiled(set(), lambda: _grid(t, 1.0, None).knn(none, 4), binding)
        assert dist.shape == (0, 4) and index.shape == (0, 4) and count.shape == (0,)
        fit = profiled(set(), lambda: ops.cloud_normals(t, none, index, count, None, cov=True), binding)
        assert fit[0].shape == (0, 3) and fit[2].shape == (0,) and int(fit[3].item()) == 0 and fit[4].shape == (0, 6)
        # no targets: the search runs and finds nothing
        dist, index, count = profiled({SEARCH}, lambda: _grid(none, 1.0, None).knn(t, 3), binding)
        assert bool((index == -1).all()) and bool((count == 0).all()) and bool((dist == 1.0).all())
        fit = profiled({NORMALS}, lambda: ops.cloud_normals(none, t, index, count, None), binding)
        assert int(fit[3].item()) == t.shape[0] and not bool(fit[2].any()) and bool((fit[0] == 0).all())


BAD_INDEX = (-1, None, 2 ** 31 - 1, -2 ** 31)       # None: N itself


def raw(name, poison):
    """both entry points on guarded buffers -> (the operators' tuple, guards, the index array the normals saw)"""
    from estdepth_amd import _native
    c, _ = R.expected(name)
    t, q, k = _dev(c["target"]), _dev(c["query"]), c["k"]
    N_, M_ = t.shape[0], q.shape[0]
    grid = under("torch", lambda: _grid(t, c["max_dist"], c["cell"]))
    from estdepth_amd import ops
    order = torch.sort(under("torch", lambda: ops.cloud_cell_keys(q, grid.lo, grid.cell, grid.dims)), stable=True)[1]
    g = dict(query=Guard(q.shape, fill=q), order=Guard((M_,), torch.int64, fill=order), records=Guard(grid.records.shape, fill=grid.records),
             cell_start=Guard(grid.cell_start.shape, torch.int32, fill=grid.cell_start), dist=Guard((M_, k)), index=Guard((M_, k), torch.int32),
             count=Guard((M_,), torch.int32), points=Guard(t.shape, fill=t), normal=Guard((M_, 3)), eig=Guard((M_, 3)),
             valid=Guard(((M_ + 3) // 4 * 4,), torch.uint8), invalid=Guard((1,), torch.int64), cov=Guard((M_, 6), torch.float64))
    d = _native.CloudKnnDesc()
    d.M, d.N, d.k = M_, N_, k
    d.query, d.order, d.records, d.cell_start = (g[x].t.data_ptr() for x in ("query", "order", "records", "cell_start"))
    d.dist, d.index, d.count, d.stats = g["dist"].t.data_ptr(), g["index"].t.data_ptr(), g["count"].t.data_ptr(), None
    d.cell, d.max_dist = grid.cell, c["max_dist"]
    for j in range(3):
        d.lo[j], d.dims[j] = float(grid.lo[j]), grid.dims[j]
    assert _lib().estd_cloud_knn(ctypes.byref(d), _stream()) == 0
    torch.cuda.synchronize()
    found = tuple(x.clone() for x in (g["dist"].t, g["index"].t, g["count"].t))
    rows = []
    if poison:                                       # the first row, the last, either side of two wave boundaries
        rows = list(dict.fromkeys(r for r in (0, 63, 64, 127, 128, M_ - 1) if r < M_))
        for j, r in enumerate(rows):
            bad = BAD_INDEX[j % 4]
            g["index"].t[r, 0] = N_ if bad is None else bad
            g["count"].t[r] = max(int(g["count"].t[r]), 1)
    seen = (g["index"].t.clone(), g["count"].t.clone())
    toward = None if c["toward"] is None else _dev(np.asarray(c["toward"], np.float32))
    st = _lib().estd_cloud_normals(_p(g["points"].t), N_, _p(g["query"].t), M_, _p(g["index"].t), _p(g["count"].t), k, _p(toward),
                                   int(toward is not None and toward.dim() == 2), _p(g["normal"].t), _p(g["eig"].t), _p(g["valid"].t), _p(g["invalid"].t),
                                   _p(g["cov"].t), _stream())
    torch.cuda.synchronize()
    assert st == 0
    pad = g["valid"].t.shape[0]
    assert torch.equal(g["valid"].t[M_:], torch.full((pad,), SENT32, dtype=torch.int32, device=DEV).view(torch.uint8)[M_:pad]), "written behind valid[M - 1]"
    fit =(g["normal"].t, g["eig"].t, g["valid"].t[:M_], g["invalid"].t, g["cov"].t)
    return c, grid, (q, k, toward), found, seen, fit, g, rows


@pytest.mark.parametrize("name", ["sphere", "257x4096_k16"])
def test_the_c_abi_on_guarded_buffers(name):
    from estdepth_amd import ops
    c, grid, (q, k, toward), found, seen, fit, g, rows = raw(name, poison=True)
    _intact(name, **g)
    assert torch.equal(g["query"].t, q) and torch.equal(g["points"].t, grid.target) and torch.equal(g["records"].t, grid.records), "%s: an input was written" % name
    assert torch.equal(g["index"].t, seen[0]) and torch.equal(g["count"].t, seen[1]), "%s: the lists were written by the normals" % name
    assert same(found, under("ctypes", lambda: grid.knn(q, k))), "%s: the C ABI differs from the operator" % name
    assert same(fit, under("ctypes", lambda: ops.cloud_normals(grid.target, q, seen[0], seen[1], toward, cov=True))), "%s: the C ABI differs" % name
    R.compare_knn(tuple(_cpu(x) for x in found), R.expected(name)[1], c, name)
    valid, normal, eig, cov = _cpu(fit[2]), _cpu(fit[0]), _cpu(fit[1]), _cpu(fit[4])
    assert len(rows) >= 5
    for r in rows:                                   # nothing addressed: the row is invalid, counted, and zero
        assert valid[r] == 0 and (normal[r] == 0).all() and (eig[r] == 0).all() and (cov[r] == 0).all(), (name, r)
    assert int(fit[3].item()) == int((valid == 0).sum()) >= len(rows)
    got = dict(normal=normal, eig=eig, valid=valid, invalid=int(fit[3].item()), cov=cov)
    R.compare_normals(got, c, _cpu(seen[0]), _cpu(seen[1]), name)


def test_a_malformed_order_writes_nothing_out_of_bounds():
    from estdepth_amd import _native
    c, _ = R.expected("64x65_k7")
    t, q, k = _dev(c["target"]), _dev(c["query"]), c["k"]
    M_ = q.shape[0]
    grid = under("torch", lambda: _grid(t, c["max_dist"], None))
    order = torch.arange(M_, device=DEV)
    order[0], order[1], order[-1] = -1, M_, 2 ** 62
    gd, gi, gc = Guard((M_, k)), Guard((M_, k), torch.int32), Guard((M_,), torch.int32)
    d = _native.CloudKnnDesc()
    d.M, d.N, d.k = M_, t.shape[0], k
    d.query, d.order, d.records, d.cell_start = q.data_ptr(), order.data_ptr(), grid.records.data_ptr(), grid.cell_start.data_ptr()
    d.dist, d.index, d.count, d.stats = gd.t.data_ptr(), gi.t.data_ptr(), gc.t.data_ptr(), None
    d.cell, d.max_dist = grid.cell, c["max_dist"]
    for j in range(3):
        d.lo[j], d.dims[j] = float(grid.lo[j]), grid.dims[j]
    assert _lib().estd_cloud_knn(ctypes.byref(d), _stream()) == 0
    torch.cuda.synchronize()
    _intact("malformed order", dist=gd, index=gi, count=gc)
    full = under("torch", lambda: grid.knn(q, k))
    assert _same(gd.t[2:-1].contiguous(), full[0][2:-1].contiguous()) and _same(gc.t[2:-1].contiguous(), full[2][2:-1].contiguous())


def _bad_calls(c):
    from estdepth_amd import ops
    t, q = _dev(c["target"]), _dev(c["query"])
    grid = under("torch", lambda: _grid(t, c["max_dist"], None))
    order = torch.sort(under("torch", lambda: ops.cloud_cell_keys(q, grid.lo, grid.cell, grid.dims)), stable=True)[1]
    s = dict(query=q, order=order, records=grid.records, cell_start=grid.cell_start, lo=grid.lo, cell=grid.cell, dims=list(grid.dims),
             max_dist=c["max_dist"], k=c["k"])
    nan_lo = grid.lo.clone()
    nan_lo[1] = float("nan")
    bad_s = [dict(k=0), dict(k=33), dict(k=-1), dict(query=q.double()), dict(query=q.cpu()), dict(order=order[:-1].contiguous()), dict(order=order.int()),
             dict(records=grid.records[:, :3].contiguous()), dict(cell_start=grid.cell_start[:-1].contiguous()), dict(cell_start=grid.cell_start.long()),
             dict(lo=nan_lo), dict(lo=grid.lo.to(DEV)), dict(cell=0.0), dict(cell=float("nan")), dict(cell=1e-39), dict(dims=[1, 1]), dict(dims=[0, 1, 1]),
             dict(dims=[1, 1, 1025]), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_dist=1e20)]
    dist, index, count = under("torch", lambda: ops.cloud_knn(**s))
    n = dict(points=t, query=q, index=index, count=count, toward=None)
    bad_n = [dict(points=t.double()), dict(points=t.cpu()), dict(query=q[:-1].contiguous()), dict(index=index.long()), dict(index=index[:-1].contiguous()),
             dict(index=index.t().contiguous().t()), dict(index=torch.zeros((q.shape[0], 33), dtype=torch.int32, device=DEV)), dict(count=count.long()),
             dict(count=count[:-1].contiguous()), dict(toward=torch.zeros(4, device=DEV)), dict(toward=torch.zeros(3)), dict(toward=torch.zeros(3, device=DEV).double())]
    return s, bad_s, n, bad_n


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    s, bad_s, n, bad_n = _bad_calls(R.expected("65x64_k7")[0])
    for bad in bad_s:
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.cloud_knn(**dict(s, **bad)), binding)
    for bad in bad_n:
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.cloud_normals(**dict(n, **bad)), binding)


def test_the_messages_are_the_same_under_both_bindings():
    from estdepth_amd import ops
    s, _, n, _ = _bad_calls(R.expected("65x64_k7")[0])
    for op, base, kw in ((ops.cloud_knn, s, dict(k=0)), (ops.cloud_knn, s, dict(k=33)), (ops.cloud_knn, s, dict(cell=float("nan"))),
                         (ops.cloud_knn, s, dict(max_dist=1e20)), (ops.cloud_normals, n, dict(index=n["index"].long())),
                         (ops.cloud_normals, n, dict(toward=torch.zeros(4, device=DEV)))):
        texts = []
        for binding in ("torch", "ctypes"):
            with pytest.raises(RuntimeError) as e:
                under(binding, lambda: op(**dict(base, **kw)))
            texts.append(str(e.value).split("\n")[0])
        assert texts[0] == texts[1] and texts[0].startswith(op.__name__ + ": "), texts


def test_every_claimed_instance_ran():
    """the kernels the profiler saw under this suite's cases (one more call here, should this test run alone) are exactly the claimed ones"""
    c, _ = R.expected("5x3_k8")
    grid = under("torch", lambda: _grid(_dev(c["target"]), c["max_dist"], None))
    profiled({SEARCH, NORMALS}, lambda: search_and_fit(grid, _dev(c["query"]), c["k"], None))
    profiled({SEARCH_STATS}, lambda: grid.knn(_dev(c["query"]), c["k"], stats=True))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
