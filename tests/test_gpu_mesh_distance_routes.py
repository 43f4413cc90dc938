"""The kernels of the point-to-mesh distance (csrc/mesh/mesh_distance.hip) under the route protocol of tests/test_gpu_mesh_sample_routes.py.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel the source emits (tests/test_mesh_distance_resources_cpu.py compiles the file and asserts
that the emitted set equals the claimed one, with no scratch and nothing spilled), and every entry has a case here that
  * asserts WHICH kernels ran (torch.profiler's demangled names);
  * runs the operator under both bindings and through the C ABI (ctypes) with every input and output carved out of buffers filled with a
    NaN sentinel: the three results are bit-identical and every band is intact -- for a mesh whose faces name vertices at -1, V,
    2^31 - 1 and -2^31 and vertices that are not finite.
The host layer's routes (cloud_metrics.TriangleGrid) are asserted the same way: invalid faces only -> the binning kernel alone, no
queries -> no search, the big list only -> no fill."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from estdepth_amd.cloud_metrics import TriangleGrid  # noqa: F401 -- the feature under test: without it this module does not import

import mesh_distance_ref as R
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _p, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernels that reach it
    "mesh_tri_bins": ["mesh_tri_bins_kernel"],
    "mesh_tri_fill": ["mesh_tri_fill_kernel"],
    "mesh_nearest": ["mesh_nearest_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(mesh_tri_bins_kernel|mesh_tri_fill_kernel|mesh_nearest_kernel)(<[^>()]*>)?")
ALL = {k for ks in INSTANCES.values() for k in ks}
BINS, FILL, NEAREST = ({k} for k in ("mesh_tri_bins_kernel", "mesh_tri_fill_kernel", "mesh_nearest_kernel"))
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


@pytest.fixture(scope="module")
def setup():
    """the mesh with every kind of invalid face, on the device, and the structure the host layer builds for it"""
    case = R.build_case("invalid_mix")
    xyz, faces, q = _dev(case["xyz"]), _dev(case["faces"]), _dev(case["q"])
    grid = TriangleGrid(dict(xyz=xyz, faces=faces), case["max_dist"], cell=0.11, big_cells=4)
    assert grid.n_big > 0 and grid.n_pairs > 0 and grid.invalid == 10
    return dict(case=case, xyz=xyz, faces=faces, q=q, grid=grid, big=4)


def _grid_args(grid):
    return (ctypes.c_float * 3)(*grid.lo.tolist()), grid.cell, (ctypes.c_int * 3)(*grid.dims)


def test_bins_route(setup):
    from estdepth_amd import ops
    s, grid = setup, setup["grid"]
    V, F = s["xyz"].shape[0], s["faces"].shape[0]
    call = lambda: ops.mesh_tri_bins(s["xyz"], s["faces"], grid.lo, grid.cell, grid.dims, s["big"])
    rt, rc = profiled(BINS, call), profiled(BINS, call, "ctypes")
    g = dict(xyz=Guard((V, 3), fill=s["xyz"]), faces=Guard((F, 3), torch.int32, fill=s["faces"]), count=Guard((F,), torch.int32),
             flag=Guard((F,), torch.int32), invalid=Guard((1,), torch.int64))
    lo3, cell, dims3 = _grid_args(grid)
    st = _lib().estd_mesh_tri_bins(_p(g["xyz"].t), V, _p(g["faces"].t), F, lo3, cell, dims3, s["big"], _p(g["count"].t), _p(g["flag"].t),
                                   _p(g["invalid"].t), _stream())
    torch.cuda.synchronize()
    assert st == 0
    _intact("bins", **g)
    for k, a, b, c in zip(("count", "flag", "invalid"), rt, rc, (g["count"].t, g["flag"].t, g["invalid"].t)):
        assert _same(a, b) and _same(a, c), "bins: %s differs between the torch binding, the ctypes binding and the C ABI" % k
    flag, count = _cpu(rt[1]), _cpu(rt[0])
    valid = R.valid_faces(s["case"]["xyz"], s["case"]["faces"])
    assert np.array_equal(flag > 0, valid) and int(rt[2].item()) == int((~valid).sum())
    assert ((flag == 1) == (count > 0)).all() and (count <= s["big"]).all() and (flag == 2).sum() == grid.n_big and count.sum() == grid.n_pairs


def test_fill_route(setup):
    from estdepth_amd import ops
    s, grid = setup, setup["grid"]
    V, F = s["xyz"].shape[0], s["faces"].shape[0]
    count = ops.mesh_tri_bins(s["xyz"], s["faces"], grid.lo, grid.cell, grid.dims, s["big"])[0]
    offset = (torch.cumsum(count.long(), 0) - count).contiguous()
    P = grid.n_pairs
    call = lambda: ops.mesh_tri_fill(s["xyz"], s["faces"], grid.lo, grid.cell, grid.dims, s["big"], offset, P)
    rt, rc = profiled(FILL, call), profiled(FILL, call, "ctypes")
    g = dict(xyz=Guard((V, 3), fill=s["xyz"]), faces=Guard((F, 3), torch.int32, fill=s["faces"]), offset=Guard((F,), torch.int64, fill=offset),
             keys=Guard((P,), torch.int64), pair_face=Guard((P,), torch.int32))
    lo3, cell, dims3 = _grid_args(grid)
    st = _lib().estd_mesh_tri_fill(_p(g["xyz"].t), V, _p(g["faces"].t), F, lo3, cell, dims3, s["big"], _p(g["offset"].t), P, _p(g["keys"].t),
                                   _p(g["pair_face"].t), _stream())
    torch.cuda.synchronize()
    assert st == 0
    _intact("fill", **g)
    for k, a, b, c in zip(("keys", "pair_face"), rt, rc, (g["keys"].t, g["pair_face"].t)):
        assert _same(a, b) and _same(a, c), "fill: %s differs between the torch binding, the ctypes binding and the C ABI" % k
    keys, pf = _cpu(rt[0]), _cpu(rt[1])
    cells = grid.dims[0] * grid.dims[1] * grid.dims[2]
    assert (keys >= 0).all() and (keys < cells).all() and np.array_equal(pf, np.repeat(np.arange(F), _cpu(count)))
    # offsets that point outside the pair arrays: nothing is written out of bounds, the status is fine
    g2 = dict(keys=Guard((P,), torch.int64), pair_face=Guard((P,), torch.int32))
    wild = Guard((F,), torch.int64, fill=offset + P - 3)
    st = _lib().estd_mesh_tri_fill(_p(s["xyz"]), V, _p(s["faces"]), F, lo3, cell, dims3, s["big"], _p(wild.t), P, _p(g2["keys"].t), _p(g2["pair_face"].t),
                                   _stream())
    torch.cuda.synchronize()
    assert st == 0
    _intact("fill with foreign offsets", **g2)


def test_nearest_route(setup):
    from estdepth_amd import ops
    s, grid = setup, setup["grid"]
    q, M = s["q"], s["q"].shape[0]
    order = torch.sort(ops.cloud_cell_keys(q, grid.lo, grid.cell, grid.dims), stable=True)[1]
    call = lambda: ops.mesh_nearest(q, order, grid.big_records, grid.records, grid.cell_start, grid.lo, grid.cell, grid.dims, grid.max_dist, True, True)
    rt, rc = profiled(NEAREST, call), profiled(NEAREST, call, "ctypes")
    from estdepth_amd import _native
    B, P = grid.big_records.shape[0], grid.records.shape[0]
    g = dict(q=Guard((M, 3), fill=q), order=Guard((M,), torch.int64, fill=order), big=Guard((B, 12), fill=grid.big_records),
             records=Guard((P, 12), fill=grid.records), cell_start=Guard(tuple(grid.cell_start.shape), torch.int32, fill=grid.cell_start),
             dist=Guard((M,)), face=Guard((M,), torch.int32), bary=Guard((M, 2)), closest=Guard((M, 3)))
    d = _native.MeshNearestDesc()
    d.M, d.B, d.P = M, B, P
    d.query, d.order, d.big_records, d.records, d.cell_start = (g[k].t.data_ptr() for k in ("q", "order", "big", "records", "cell_start"))
    d.dist, d.face, d.bary, d.closest = (g[k].t.data_ptr() for k in ("dist", "face", "bary", "closest"))
    d.cell, d.max_dist = grid.cell, grid.max_dist
    d.lo[:], d.dims[:] = grid.lo.tolist(), grid.dims
    st = _lib().estd_mesh_nearest(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    assert st == 0
    _intact("nearest", **g)
    for k, a, b, c in zip(("dist", "face", "bary", "closest"), rt, rc, (g["dist"].t, g["face"].t, g["bary"].t, g["closest"].t)):
        assert _same(a, b) and _same(a, c), "nearest: %s differs between the torch binding, the ctypes binding and the C ABI" % k
    got = dict(dist=_cpu(rt[0]), face=_cpu(rt[1]), bary=_cpu(rt[2]), closest=_cpu(rt[3]), invalid=grid.invalid)
    fig = R.compare(got, s["case"], "nearest route")
    assert fig["found"] > 0
    # without the optional outputs: the same dist and face, and a permutation with entries outside 0..M-1 writes nothing out of bounds
    plain = under("torch", lambda: ops.mesh_nearest(q, order, grid.big_records, grid.records, grid.cell_start, grid.lo, grid.cell, grid.dims, grid.max_dist))
    assert plain[2] is None and plain[3] is None and _same(plain[0], rt[0]) and _same(plain[1], rt[1])
    bad = order.clone()
    bad[::7] = M + 5
    bad[3] = -1
    g3 = dict(dist=Guard((M,)), face=Guard((M,), torch.int32))
    d.order, d.dist, d.face, d.bary, d.closest = bad.data_ptr(), g3["dist"].t.data_ptr(), g3["face"].t.data_ptr(), None, None
    assert _lib().estd_mesh_nearest(ctypes.byref(d), _stream()) == 0
    torch.cuda.synchronize()
    _intact("nearest with a malformed order", **g3)


def test_the_host_layers_routes():
    on = lambda name: (lambda c: (dict(xyz=_dev(c["xyz"]), faces=_dev(c["faces"])), _dev(c["q"]), c["max_dist"]))(R.build_case(name))
    for binding in ("torch", "ctypes"):
        mesh, q, md = on("invalid_only")
        grid = profiled(BINS, lambda: TriangleGrid(mesh, md), binding)
        dist, face = profiled(set(), lambda: grid.query(q), binding)
        assert grid.invalid == 4 and (face == -1).all() and (dist == md).all()
        mesh, q, md = on("m0")
        grid = profiled(BINS | FILL, lambda: TriangleGrid(mesh, md), binding)
        assert profiled(set(), lambda: grid.query(q), binding)[0].shape == (0,)
        mesh, q, md = on("walls")
        grid = profiled(BINS, lambda: TriangleGrid(mesh, md, cell=math.inf), binding)
        profiled(NEAREST, lambda: grid.query(q), binding)
        grid = profiled(BINS | FILL, lambda: TriangleGrid(mesh, md), binding)
        profiled(NEAREST, lambda: grid.query(q), binding)
        no_faces = dict(xyz=mesh["xyz"], faces=torch.empty((0, 3), device=DEV, dtype=torch.int32))
        profiled(set(), lambda: TriangleGrid(no_faces, md).query(q), binding)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(setup, binding):
    from estdepth_amd import ops
    s, grid = setup, setup["grid"]
    xyz, faces, q = s["xyz"], s["faces"], s["q"]
    M = q.shape[0]
    order = torch.arange(M, device=DEV)
    offset = torch.zeros(faces.shape[0], device=DEV, dtype=torch.int64)
    ok = dict(xyz=xyz, faces=faces, lo=grid.lo, cell=grid.cell, dims=grid.dims, big=4)
    for bad in (dict(faces=faces.to(torch.int64)), dict(faces=faces.cpu()), dict(xyz=xyz.double()), dict(xyz=xyz[:, :2].contiguous()), dict(xyz=xyz.cpu()),
                dict(lo=grid.lo.double()), dict(lo=torch.tensor([0.0, float("nan"), 0.0])), dict(cell=0.0), dict(cell=float("inf")), dict(dims=(0, 1, 1)),
                dict(dims=(1025, 1, 1)), dict(dims=(512, 512, 512)), dict(big=-1)):
        kw = dict(ok, **bad)
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_tri_bins(kw["xyz"], kw["faces"], kw["lo"], kw["cell"], kw["dims"], kw["big"]), binding)
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_tri_fill(kw["xyz"], kw["faces"], kw["lo"], kw["cell"], kw["dims"], kw["big"], offset, 10), binding)
    for bad in (dict(offset=offset[:-1]), dict(offset=offset.to(torch.int32)), dict(n=-1), dict(n=(1 << 23) + 1)):
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_tri_fill(xyz, faces, grid.lo, grid.cell, grid.dims, 4, bad.get("offset", offset), bad.get("n", 10)), binding)
    ok = dict(q=q, order=order, big=grid.big_records, rec=grid.records, cs=grid.cell_start, lo=grid.lo, cell=grid.cell, dims=grid.dims, md=0.5)
    for bad in (dict(q=q.double()), dict(q=q.cpu()), dict(q=q[:, :2].contiguous()), dict(order=order[:-1]), dict(order=order.to(torch.int32)),
                dict(big=grid.big_records[:, :11].contiguous()), dict(rec=grid.records.view(torch.int32)), dict(rec=grid.records.cpu()),
                dict(cs=grid.cell_start[:-1]), dict(cs=grid.cell_start.long()), dict(md=0.0), dict(md=float("nan")), dict(md=1e30), dict(cell=-1.0),
                dict(dims=(1, 1))):
        kw = dict(ok, **bad)
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_nearest(kw["q"], kw["order"], kw["big"], kw["rec"], kw["cs"], kw["lo"], kw["cell"], kw["dims"], kw["md"]), binding)


def test_every_claimed_instance_ran():
    """the kernels the profiler saw under this suite's cases (one more case here, should this test run alone) are exactly the claimed ones"""
    c = R.build_case("walls")
    profiled(ALL, lambda: TriangleGrid(dict(xyz=_dev(c["xyz"]), faces=_dev(c["faces"])), c["max_dist"]).query(_dev(c["q"])))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
