"""The kernel instances of the surface-net mesh (csrc/mesh/tsdf_mesh.hip) under the route protocol of tests/test_gpu_recon3d_routes.py,
against the float64 reference of tests/tsdf_mesh_ref.py and its comparison.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel instance the source emits (tests/test_tsdf_mesh_resources_cpu.py compiles the file and
asserts that the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

A route is one kernel instance.  Each case
  * asserts WHICH instances ran (torch.profiler's demangled names, template arguments included): the plain or the colour cell kernel and
    the face kernel, nothing else -- under the counting call (capacity 0) and under the filling call alike;
  * runs the operators under both bindings and once more through the C ABI (ctypes) with every device input and output -- the volume and
    colour planes, the two counters, the cell ids, xyz, normals, weights, colours, the edge ids and the quads -- carved out of buffers
    filled with a NaN sentinel: the three results are bit-identical after sorting (the record order is the atomic counter's) and every
    band keeps the sentinel;
  * compares with the float64 reference under tsdf_mesh_ref.compare;
  * sits on the edges of the launch shapes (tsdf_mesh_ref.CASES): one cell, X in 2 / 3 / 7 / 66 / 130 round the 63-cell wave, Y round
    the 4-row workgroup, Z round the 8-plane march, volumes that append nothing."""
import ctypes
import re

import numpy as np
import pytest
import torch

from estdepth_amd.fusion3d import sorted_mesh  # noqa: F401 -- the feature under test: without it this module does not import

import tsdf_mesh_ref as M
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _p, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernel instances that reach it (surface_net_cells_kernel<COLOR>)
    "mesh_vertices": ["surface_net_cells_kernel<false>", "surface_net_cells_kernel<true>"],
    "mesh_faces": ["surface_net_faces_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(surface_net_\w+_kernel)(<[^>()]*>)?")
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


def _cells(colour):
    return "surface_net_cells_kernel<%s>" % ("true" if colour else "false")


def _run(vol, col, c, org):
    from estdepth_amd import ops
    return sorted_mesh(ops.tsdf_mesh_vertices, ops.tsdf_mesh_faces, vol, col, c["voxel"], org, c["w_min"])


def _raw(c, vol, col, n_v, n_q, w_min=None, voxel=None):
    """estd_tsdf_mesh_vertices and estd_tsdf_mesh_faces on guarded outputs of exactly n_v / n_q records -> (statuses, guards dict)"""
    Z, Y, X = c["dims"]
    zero = torch.zeros(1, dtype=torch.int64)
    g = dict(n_v=Guard((1,), torch.int64, fill=zero), n_q=Guard((1,), torch.int64, fill=zero), cell=Guard((n_v,), torch.int64), xyz=Guard((n_v, 3)),
             normal=Guard((n_v, 3)), weight=Guard((n_v,)), edge=Guard((n_q,), torch.int64), quad=Guard((n_q, 4), torch.int32))
    if col is not None:
        g["color"] = Guard((n_v, 3))
    org = (ctypes.c_float * 3)(*c["origin"])
    w_min = c["w_min"] if w_min is None else w_min
    wt = ctypes.c_void_p(vol.data_ptr() + 4 * Z * Y * X)
    st_v = _lib().estd_tsdf_mesh_vertices(_p(vol), wt, _p(col), Z, Y, X, float(c["voxel"] if voxel is None else voxel), org, float(w_min), _p(g["n_v"].t),
                                          n_v, _p(g["cell"].t), _p(g["xyz"].t), _p(g["normal"].t), _p(g["weight"].t),
                                          _p(g["color"].t) if col is not None else None, _stream())
    st_q = _lib().estd_tsdf_mesh_faces(_p(vol), wt, Z, Y, X, float(w_min), _p(g["n_q"].t), n_q, _p(g["edge"].t), _p(g["quad"].t), _stream())
    torch.cuda.synchronize()
    return (st_v, st_q), g


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_mesh_route(name):
    c = M.build_case(name)
    ref = M.reference(c)
    colour = c["C"] is not None
    vol, col = _dev(np.stack([c["D"], c["W"]])), _dev(c["C"]) if colour else None
    org = torch.tensor(c["origin"], dtype=torch.float32)
    want = {_cells(colour), "surface_net_faces_kernel"}
    what = "mesh %s" % name
    rt = profiled(want, lambda: _run(vol, col, c, org))
    rc = under("ctypes", lambda: _run(vol, col, c, org))
    gv = Guard(vol.shape, fill=vol)
    gc = Guard(col.shape, fill=col) if colour else None
    n_v, n_q = ref["count"], ref["edge"].shape[0]
    st, g = _raw(c, gv.t, gc.t if colour else None, n_v, n_q)
    assert st == (0, 0)
    _intact(what, volume=gv, **({"colour": gc} if colour else {}), **g)
    assert int(g["n_v"].t.item()) == n_v and int(g["n_q"].t.item()) == n_q
    # the guarded records in the public order
    cell, order = torch.sort(g["cell"].t)
    edge, q_order = torch.sort(g["edge"].t)
    index = torch.searchsorted(cell, g["quad"].t[q_order].to(torch.int64))
    raw = dict(cell=cell, edge=edge, faces=index[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3).to(torch.int32), xyz=g["xyz"].t[order], normal=g["normal"].t[order],
               weight=g["weight"].t[order])
    if colour:
        raw["color"] = g["color"].t[order]
    for k in raw:
        assert _same(rt[k], rc[k]) and _same(rt[k], raw[k]), "%s: %s differs between the three launches" % (what, k)
    fig = M.compare({k: _cpu(v) for k, v in rt.items() if isinstance(v, torch.Tensor)}, ref, what)
    print("MESH-ROUTE %s: %d vertices %d triangles xyz %.3f normal %.3f" % (name, fig["vertices"], fig["faces"], fig["xyz_ratio"], fig["normal_ratio"]))


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("name", ["unobserved", "positive"])
def test_nothing_to_append_still_launches_both(name, binding):
    """a volume without a surface: the kernels run (counting and filling call alike) and leave the counters at zero"""
    from estdepth_amd import ops
    c = M.build_case(name)
    vol, org = _dev(np.stack([c["D"], c["W"]])), torch.tensor(c["origin"], dtype=torch.float32)
    out = profiled({_cells(False)}, lambda: ops.tsdf_mesh_vertices(vol, None, c["voxel"], org, c["w_min"], 8), binding)
    assert int(out[0].item()) == 0
    out = profiled({"surface_net_faces_kernel"}, lambda: ops.tsdf_mesh_faces(vol, c["w_min"], 8), binding)
    assert int(out[0].item()) == 0
    st, g = _raw(c, vol, None, 8, 8)
    assert st == (0, 0) and int(g["n_v"].t.item()) == 0 and int(g["n_q"].t.item()) == 0
    assert all(g[k].untouched() for k in ("cell", "xyz", "normal", "weight", "edge", "quad"))


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    c = M.build_case("3x5x7")
    vol, org = _dev(np.stack([c["D"], c["W"]])), torch.tensor(c["origin"], dtype=torch.float32)
    with pytest.raises(RuntimeError):
        profiled(set(), lambda: ops.tsdf_mesh_vertices(vol, None, 0.0, org, c["w_min"], 8), binding)
    with pytest.raises(RuntimeError):
        profiled(set(), lambda: ops.tsdf_mesh_faces(vol, float("nan"), 8), binding)
    st, g = _raw(c, vol, None, 8, 8, w_min=float("nan"))
    assert st == (-1, -1) and all(x.untouched() for k, x in g.items() if k not in ("n_v", "n_q"))
    assert int(g["n_v"].t.item()) == 0 and int(g["n_q"].t.item()) == 0
    st, g = _raw(c, vol, None, 8, 8, voxel=-1.0)
    assert st[0] == -1 and all(g[k].untouched() for k in ("cell", "xyz", "normal", "weight"))


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_dimension_of_one_launches_nothing(binding):
    from estdepth_amd import ops
    D, W = M.wavy((1, 6, 8), holes=False)
    vol = _dev(np.stack([D, W]))
    out = profiled(set(), lambda: (ops.tsdf_mesh_vertices(vol, None, 0.03, torch.zeros(3), 1.0, 4), ops.tsdf_mesh_faces(vol, 1.0, 4)), binding)
    assert int(out[0][0].item()) == 0 and int(out[1][0].item()) == 0


def test_every_claimed_instance_ran():
    """the instances the profiler saw under this suite's cases (two more cases here, should this test run alone) are exactly the claimed ones"""
    for name in ("3x5x7", "colour"):
        c = M.build_case(name)
        colour = c["C"] is not None
        vol, col = _dev(np.stack([c["D"], c["W"]])), _dev(c["C"]) if colour else None
        profiled({_cells(colour), "surface_net_faces_kernel"}, lambda: _run(vol, col, c, torch.tensor(c["origin"], dtype=torch.float32)))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
