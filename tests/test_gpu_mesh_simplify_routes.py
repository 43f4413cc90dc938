"""The kernels of the mesh simplification (csrc/mesh/mesh_simplify.hip) under the route protocol of tests/test_gpu_mesh_raster_routes.py,
against the numpy reference of tests/mesh_simplify_ref.py: EQUALITY TO THE BIT of the corner records, the triples, the two counts, the
placed flags, the vertices and the normals.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel the source emits (tests/test_mesh_simplify_resources_cpu.py compiles the file and asserts
that the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

Each case of mesh_simplify_ref.CASES takes the clusters and their means from the reference (the ranking is host glue), runs the two
operators with torch's stable sort between them, asserts WHICH kernels ran (torch.profiler's demangled names; none without faces),
runs everything under both bindings and twice: bit-identical, and equal to the reference's bits.  Two cases go through the C ABI
(ctypes) with every input and output carved out of buffers filled with a sentinel: the same bits again and every band intact -- with
faces that name vertices at -1, V, 2^31 - 1 and -2^31 at the first position, the last and either side of two wave boundaries."""
import ctypes
import re

import numpy as np
import pytest
import torch

from estdepth_amd.ops import mesh_cluster_faces, mesh_cluster_quadrics  # noqa: F401 -- the feature under test: without it this module does not import

import mesh_simplify_ref as R
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import SENT32, Guard, _cpu, _dev, _intact, _lib, _p, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernels that reach it
    "mesh_cluster_faces": ["mesh_cluster_faces_kernel"],
    "mesh_cluster_quadrics": ["mesh_cluster_quadric_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(mesh_cluster_faces_kernel|mesh_cluster_quadric_kernel)(<[^>()]*>)?")
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


def on_device(name):
    """the case and the reference's host glue on the device -> dict"""
    xyz, faces, cell, origin = R.build_case(name)
    want = R.expected(name)
    return dict(xyz=_dev(xyz), faces=_dev(faces), cluster=_dev(want["cluster"]), cell_key=_dev(want["cell_key"]), mean=_dev(want["mean"]),
                lo=torch.from_numpy(np.ascontiguousarray(want["lo"])), cell=want["cell"], dims=list(want["dims"]), K=int(want["cell_key"].shape[0]))


def sort_records(corner, K):
    """the glue between the launches: the corner records sorted by cluster (stable) -> (order int64 [3F], segments int64 [K + 1])"""
    rec_cluster, order = torch.sort(corner, stable=True)
    return order.contiguous(), torch.searchsorted(rec_cluster, torch.arange(K + 1, device=corner.device, dtype=torch.int32)).contiguous()


def both(c, reg=R.REG):
    from estdepth_amd import ops
    corner, triple, counts = ops.mesh_cluster_faces(c["faces"], c["cluster"], c["K"])
    order, segments = sort_records(corner, c["K"])
    xyz, normal, placed = ops.mesh_cluster_quadrics(c["xyz"], c["faces"], order, segments, c["cell_key"], c["mean"], c["lo"], c["cell"], c["dims"], reg)
    return corner, triple, counts, xyz, normal, placed


def as_got(out):
    corner, triple, counts, xyz, normal, placed = out
    return dict(corner=_cpu(corner), triple=_cpu(triple), xyz=_cpu(xyz), normal=_cpu(normal), placed=_cpu(placed)), [int(v) for v in counts.tolist()]


def same(a, b):
    return all(torch.equal(x, y) if x.dtype == torch.bool else _same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", R.CASES)
def test_simplify_route(name):
    c = on_device(name)
    want = R.expected(name)
    ran = ALL if c["faces"].shape[0] and c["K"] else set()
    first = profiled(ran, lambda: both(c))
    for binding in ("torch", "ctypes"):
        for again in range(2):
            assert same(first, profiled(ran, lambda: both(c), binding)), "%s: the bits differ under %s, call %d" % (name, binding, again)
    got, counts = as_got(first)
    n = R.compare(got, want, name, keys=("corner", "triple", "xyz", "normal", "placed"))
    assert counts == [want["stats"]["invalid"], want["stats"]["collapsed"]], (name, counts, want["stats"])
    print("MESH-SIMPLIFY-ROUTE %s: %d faces (%d invalid, %d collapsed) on %d clusters, %d placed: %d values equal to the reference's bits"
          % (name, c["faces"].shape[0], counts[0], counts[1], c["K"], int(got["placed"].sum()), n))


def raw(c, reg=R.REG):
    """both entry points on guarded buffers -> (the operators' tuple, guards dict)"""
    V, F, K = c["xyz"].shape[0], c["faces"].shape[0], c["K"]
    pad = (K + 3) // 4 * 4
    g = dict(xyz=Guard((V, 3), fill=c["xyz"]), faces=Guard((F, 3), torch.int32, fill=c["faces"]), cluster=Guard((V,), torch.int32, fill=c["cluster"]),
             corner=Guard((3 * F,), torch.int32), triple=Guard((F, 3), torch.int32), counts=Guard((2,), torch.int64),
             cell_key=Guard((K,), torch.int64, fill=c["cell_key"]), mean=Guard((K, 3), fill=c["mean"]), out=Guard((K, 3)), normal=Guard((K, 3)),
             placed=Guard((pad,), torch.uint8))
    st = _lib().estd_mesh_cluster_faces(_p(g["faces"].t), F, V, _p(g["cluster"].t), K, _p(g["corner"].t), _p(g["triple"].t), _p(g["counts"].t), _stream())
    torch.cuda.synchronize()
    assert st == 0
    order, segments = sort_records(g["corner"].t, K)
    g["order"], g["segments"] = Guard((3 * F,), torch.int64, fill=order), Guard((K + 1,), torch.int64, fill=segments)
    st = _lib().estd_mesh_cluster_quadrics(_p(g["xyz"].t), V, _p(g["faces"].t), F, _p(g["order"].t), _p(g["segments"].t), _p(g["cell_key"].t), K,
                                           _p(g["mean"].t), (ctypes.c_float * 3)(*c["lo"].tolist()), c["cell"], (ctypes.c_int * 3)(*c["dims"]), reg,
                                           _p(g["out"].t), _p(g["normal"].t), _p(g["placed"].t), _stream())
    torch.cuda.synchronize()
    assert st == 0
    tail = g["placed"].t[K:]
    assert torch.equal(tail, torch.full((pad,), SENT32, dtype=torch.int32, device=DEV).view(torch.uint8)[K:pad]), "written behind placed[K - 1]"
    assert bool(((g["placed"].t[:K] == 0) | (g["placed"].t[:K] == 1)).all())
    return (g["corner"].t, g["triple"].t, g["counts"].t, g["out"].t, g["normal"].t, g["placed"].t[:K].to(torch.bool)), g


@pytest.mark.parametrize("name", ["invalid", "fan-300"])
def test_the_c_abi_on_guarded_buffers(name):
    c = on_device(name)
    out, g = raw(c)
    _intact(name, **g)
    for k in ("xyz", "faces", "cluster", "cell_key", "mean"):
        assert torch.equal(g[k].t, c[k]), "%s: the input %s was written" % (name, k)
    assert same(out, under("ctypes", lambda: both(c))), "%s: the C ABI differs from the operator" % name
    got, counts = as_got(out)
    R.compare(got, R.expected(name), name, keys=("corner", "triple", "xyz", "normal", "placed"))
    assert counts == [R.expected(name)["stats"]["invalid"], R.expected(name)["stats"]["collapsed"]]


def test_the_regulariser_is_an_argument():
    """reg = 0 leaves the wedge's crease direction without a pivot; a large reg pulls every vertex to its mean: the reference's bits both times"""
    for name, reg in (("wedge", 0.0), ("patch-257", 0.0), ("patch-257", 4.0)):
        c = on_device(name)
        xyz, faces, cell, origin = R.build_case(name)
        want = R.simplify(xyz, faces, cell, origin, reg=reg)
        got, _ = as_got(profiled(ALL, lambda: both(c, reg)))
        R.compare(got, want, "%s reg %g" % (name, reg), keys=("xyz", "normal", "placed"))


def _bad_calls(c):
    """(operator, keyword changes) pairs each of which must be refused"""
    from estdepth_amd import ops
    corner = ops.mesh_cluster_faces(c["faces"], c["cluster"], c["K"])[0]
    torch.cuda.synchronize()
    order, segments = sort_records(corner, c["K"])
    q = dict(xyz=c["xyz"], faces=c["faces"], order=order, segments=segments, cell_key=c["cell_key"], mean=c["mean"], lo=c["lo"], cell=c["cell"],
             dims=c["dims"], reg=R.REG)
    f = dict(faces=c["faces"], cluster=c["cluster"], n_clusters=c["K"])
    bad_f = [dict(faces=c["faces"].to(torch.int64)), dict(faces=c["faces"].cpu()), dict(faces=c["faces"].t().contiguous().t()),
             dict(cluster=c["cluster"].to(torch.int64)), dict(cluster=c["cluster"].cpu()), dict(n_clusters=-1), dict(n_clusters=0),
             dict(n_clusters=c["cluster"].shape[0] + 1)]
    nan_lo = c["lo"].clone()
    nan_lo[1] = float("nan")
    bad_q = [dict(xyz=c["xyz"].double()), dict(xyz=c["xyz"].cpu()), dict(faces=c["faces"].to(torch.int64)), dict(order=order[:-1].contiguous()),
             dict(order=order.to(torch.int32)), dict(segments=segments.to(torch.int32)), dict(segments=segments.new_zeros(c["xyz"].shape[0] + 2)),
             dict(cell_key=c["cell_key"][:-1].contiguous()), dict(mean=c["mean"][:-1].contiguous()), dict(mean=c["mean"].cpu()), dict(lo=nan_lo),
             dict(lo=c["lo"].double()), dict(lo=c["lo"].to(DEV)), dict(cell=0.0), dict(cell=float("nan")), dict(cell=1e-39), dict(dims=[1, 1]),
             dict(dims=[0, 1, 1]), dict(dims=[1, 1, (1 << 20) + 1]), dict(reg=-1e-9), dict(reg=float("nan")), dict(reg=float("inf"))]
    return f, bad_f, q, bad_q


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    f, bad_f, q, bad_q = _bad_calls(on_device("patch-65"))
    for bad in bad_f:
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_cluster_faces(**dict(f, **bad)), binding)
    for bad in bad_q:
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_cluster_quadrics(**dict(q, **bad)), binding)


def test_the_messages_are_the_same_under_both_bindings():
    from estdepth_amd import ops
    c = on_device("patch-65")
    f, _, q, _ = _bad_calls(c)
    nan_lo = c["lo"].clone()
    nan_lo[0] = float("inf")
    for op, base, kw in ((ops.mesh_cluster_faces, f, dict(faces=c["faces"].to(torch.int64))), (ops.mesh_cluster_faces, f, dict(n_clusters=0)),
                         (ops.mesh_cluster_faces, f, dict(n_clusters=c["cluster"].shape[0] + 1)), (ops.mesh_cluster_quadrics, q, dict(reg=float("nan"))),
                         (ops.mesh_cluster_quadrics, q, dict(cell=float("nan"))), (ops.mesh_cluster_quadrics, q, dict(lo=nan_lo)),
                         (ops.mesh_cluster_quadrics, q, dict(mean=c["mean"][:-1].contiguous())),
                         (ops.mesh_cluster_quadrics, q, dict(segments=q["segments"].new_zeros(c["xyz"].shape[0] + 2)))):
        texts = []
        for binding in ("torch", "ctypes"):
            with pytest.raises(RuntimeError) as e:
                under(binding, lambda: op(**dict(base, **kw)))
            texts.append(str(e.value).split("\n")[0])
        assert texts[0] == texts[1] and texts[0].startswith(op.__name__ + ": "), texts


def test_the_entry_points_refuse_before_a_launch():
    c = on_device("patch-65")
    V, F, K = c["xyz"].shape[0], c["faces"].shape[0], c["K"]
    g = dict(corner=Guard((3 * F,), torch.int32), triple=Guard((F, 3), torch.int32), counts=Guard((2,), torch.int64), out=Guard((K, 3)),
             normal=Guard((K, 3)), placed=Guard((4 * K,), torch.uint8))
    order, segments = torch.arange(3 * F, device=DEV), torch.zeros(K + 1, dtype=torch.int64, device=DEV)
    lo, d3 = (ctypes.c_float * 3)(*c["lo"].tolist()), (ctypes.c_int * 3)(*c["dims"])
    for kw in (dict(F=-1), dict(V=-1), dict(K=-1), dict(K=V + 1), dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1, V=2 ** 31 - 1)):
        st = _lib().estd_mesh_cluster_faces(_p(c["faces"]), kw.get("F", F), kw.get("V", V), _p(c["cluster"]), kw.get("K", K), _p(g["corner"].t),
                                            _p(g["triple"].t), _p(g["counts"].t), _stream())
        torch.cuda.synchronize()
        assert st in (-1, -3) and all(x.untouched() for x in g.values()), (kw, st)
    bad_lo, bad_d = (ctypes.c_float * 3)(0.0, float("nan"), 0.0), (ctypes.c_int * 3)(1, 0, 1)
    for kw in (dict(F=-1), dict(V=-1), dict(K=-1), dict(K=V + 1), dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1, V=2 ** 31 - 1), dict(lo=bad_lo),
               dict(lo=None), dict(d3=bad_d), dict(d3=None), dict(cell=0.0), dict(cell=float("inf")), dict(reg=-1.0), dict(reg=float("nan")),
               dict(reg=float("inf"))):
        st = _lib().estd_mesh_cluster_quadrics(_p(c["xyz"]), kw.get("V", V), _p(c["faces"]), kw.get("F", F), _p(order), _p(segments), _p(c["cell_key"]),
                                               kw.get("K", K), _p(c["mean"]), kw.get("lo", lo), kw.get("cell", c["cell"]), kw.get("d3", d3),
                                               kw.get("reg", R.REG), _p(g["out"].t), _p(g["normal"].t), _p(g["placed"].t), _stream())
        torch.cuda.synchronize()
        assert st in (-1, -3) and all(x.untouched() for x in g.values()), (kw, st)


def test_every_claimed_instance_ran():
    """the kernels the profiler saw under this suite's cases (one more call here, should this test run alone) are exactly the claimed ones"""
    profiled(ALL, lambda: both(on_device("patch-65")))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
