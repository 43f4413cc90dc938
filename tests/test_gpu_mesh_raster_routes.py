"""The kernels of the mesh rasteriser (csrc/mesh/mesh_raster.hip) under the route protocol of tests/test_gpu_mesh_sample_routes.py,
against the float64 reference of tests/mesh_raster_ref.py: EQUALITY TO THE BIT of depth, face, bary, facing and the invalid count.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel the source emits (tests/test_mesh_raster_resources_cpu.py compiles the file and asserts
that the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

Each case of mesh_raster_ref.CASES
  * asserts WHICH kernels ran (torch.profiler's demangled names): the raster kernel and the resolve kernel; the instance with the load
    in front of the atomic with ``preload=True``; the resolve kernel alone without faces;
  * runs the operator under both bindings and with and without the load: bit-identical, and equal to the reference's bits.
One case goes through the C ABI (ctypes) with every input and output carved out of buffers filled with a sentinel: the same bits
again, every band intact -- for the mesh whose faces name vertices at -1, V and 2^31 - 1 too; a launch split over two face ranges
gives the bits of one."""
import ctypes
import re

import numpy as np
import pytest
import torch

from estdepth_amd.ops import mesh_raster  # noqa: F401 -- the feature under test: without it this module does not import

import mesh_raster_ref as R
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _p, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernels that reach it
    "mesh_raster": ["mesh_raster_kernel<0>"],
    "mesh_raster_preload": ["mesh_raster_kernel<1>"],
    "mesh_raster_resolve": ["mesh_resolve_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(mesh_raster_kernel|mesh_resolve_kernel)(<[^>()]*>)?")
ALL = {k for ks in INSTANCES.values() for k in ks}
RESOLVE = {"mesh_resolve_kernel"}
WITH_LOAD, WITHOUT_LOAD = RESOLVE | {"mesh_raster_kernel<1>"}, RESOLVE | {"mesh_raster_kernel<0>"}
NAMES = ("depth", "face", "bary", "facing", "invalid")
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
    xyz, faces, mat, H, W, zn = R.build_case(name)
    return _dev(xyz), _dev(faces), torch.from_numpy(np.ascontiguousarray(mat)), H, W, zn


def as_got(out):
    return dict(depth=_cpu(out[0]), face=_cpu(out[1]), bary=_cpu(out[2]), facing=_cpu(out[3]), invalid=int(out[4].item()))


def raw(xyz, faces, mat, H, W, zn, ranges=None, flags=0):
    """estd_mesh_raster over ``ranges`` [(first, count), ...] into one guarded key buffer, then estd_mesh_raster_resolve on guarded maps
    -> (the operator's tuple with the invalid counts summed, guards dict)"""
    V, F = xyz.shape[0], faces.shape[0]
    m = (ctypes.c_double * 12)(*mat.tolist())
    g = dict(xyz=Guard((V, 3), fill=xyz), faces=Guard((F, 3), torch.int32, fill=faces), keys=Guard((H, W), torch.int64),
             invalid=Guard((1,), torch.int64), depth=Guard((H, W)), face=Guard((H, W), torch.int32), bary=Guard((H, W, 2)),
             facing=Guard((H, W), torch.int32))
    px, pf = (_p(g["xyz"].t) if V else None), (_p(g["faces"].t) if F else None)
    invalid = 0
    for i, (first, count) in enumerate(ranges or [(0, F)]):
        st = _lib().estd_mesh_raster(px, V, pf, F, first, count, m, H, W, zn, flags | (2 if i == 0 else 0), _p(g["keys"].t), _p(g["invalid"].t),
                                     _stream())
        torch.cuda.synchronize()
        assert st == 0
        invalid += int(g["invalid"].t.item())
    st = _lib().estd_mesh_raster_resolve(px, V, pf, F, m, H, W, _p(g["keys"].t), _p(g["depth"].t), _p(g["face"].t), _p(g["bary"].t),
                                         _p(g["facing"].t), _stream())
    torch.cuda.synchronize()
    assert st == 0
    return (g["depth"].t, g["face"].t, g["bary"].t, g["facing"].t, torch.tensor([invalid])), g


@pytest.mark.parametrize("name", R.CASES)
def test_raster_route(name):
    from estdepth_amd import ops
    xyz, faces, mat, H, W, zn = on_device(name)
    none = faces.shape[0] == 0
    rt = profiled(RESOLVE if none else WITHOUT_LOAD, lambda: ops.mesh_raster(xyz, faces, mat, H, W, zn))
    rc = profiled(RESOLVE if none else WITHOUT_LOAD, lambda: ops.mesh_raster(xyz, faces, mat, H, W, zn), "ctypes")
    rn = profiled(RESOLVE if none else WITH_LOAD, lambda: ops.mesh_raster(xyz, faces, mat, H, W, zn, preload=True))
    rm = profiled(RESOLVE if none else WITH_LOAD, lambda: ops.mesh_raster(xyz, faces, mat, H, W, zn, preload=True), "ctypes")
    for other, what in ((rc, "between the bindings"), (rn, "with the load"), (rm, "with the load under ctypes")):
        for k, a, b in zip(NAMES, rt, other):
            assert _same(a, b), "%s: %s differs %s" % (name, k, what)
    fig = R.compare(as_got(rt), R.expected(name), name)
    print("MESH-RASTER-ROUTE %s: %d faces %d invalid, %d x %d: %d pixels covered by %d faces, equal to the reference's bits"
          % (name, faces.shape[0], int(rt[4].item()), W, H, fig["covered"], fig["seen"]))


@pytest.mark.parametrize("name", ["out-of-range", "interpenetrating"])
def test_the_c_abi_on_guarded_buffers(name):
    """every input and output between sentinel bands: the operator's bits again and no band touched, with indices at -1, V and 2^31 - 1
    among the faces"""
    from estdepth_amd import ops
    xyz, faces, mat, H, W, zn = on_device(name)
    out, g = raw(xyz, faces, mat, H, W, zn)
    _intact(name, **g)
    assert torch.equal(g["xyz"].t, xyz) and torch.equal(g["faces"].t, faces), "%s: an input was written" % name
    ref = under("ctypes", lambda: ops.mesh_raster(xyz, faces, mat, H, W, zn))
    for k, a, b in zip(NAMES, out, ref):
        assert _same(a.cpu(), b.cpu()), "%s: %s differs from the operator's" % (name, k)
    R.compare(as_got(out), R.expected(name), name)


@pytest.mark.parametrize("name", ["out-of-range", "stacked-4096", "degenerate"])
def test_a_split_launch_gives_the_same_bits(name):
    """a minimum does not depend on who arrives first: two face ranges, in either order, with either instance"""
    xyz, faces, mat, H, W, zn = on_device(name)
    F = faces.shape[0]
    cut = F // 3
    for ranges, flags in (([(0, cut), (cut, F - cut)], 0), ([(cut, F - cut), (0, cut)], 1), ([(0, 0), (0, F), (F, 0)], 0)):
        out, g = raw(xyz, faces, mat, H, W, zn, ranges, flags)
        _intact("split", **g)
        R.compare(as_got(out), R.expected(name), "%s split %s" % (name, ranges))


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    xyz, faces, mat, H, W, zn = on_device("interpenetrating")
    nan = mat.clone()
    nan[5] = float("nan")
    for bad in (dict(faces=faces.to(torch.int64)), dict(faces=faces.t().contiguous().t()), dict(faces=faces.cpu()), dict(xyz=xyz.double()),
                dict(xyz=xyz[:, :2].contiguous()), dict(xyz=xyz.cpu()), dict(mat=mat.float()), dict(mat=mat[:11].contiguous()),
                dict(mat=mat.to(DEV)), dict(mat=nan), dict(mat=torch.full((12,), float("inf"), dtype=torch.float64)), dict(H=0), dict(W=0),
                dict(H=-3), dict(H=65536, W=65536), dict(zn=-1e-3), dict(zn=float("nan")), dict(zn=float("inf"))):
        kw = dict(xyz=xyz, faces=faces, mat=mat, H=H, W=W, zn=zn)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_raster(kw["xyz"], kw["faces"], kw["mat"], kw["H"], kw["W"], kw["zn"]), binding)


def test_the_entry_points_refuse_before_a_launch():
    xyz, faces, mat, H, W, zn = on_device("interpenetrating")
    V, F = xyz.shape[0], faces.shape[0]
    m = (ctypes.c_double * 12)(*mat.tolist())
    bad_m = (ctypes.c_double * 12)(*([float("nan")] + mat.tolist()[1:]))
    g = dict(keys=Guard((H, W), torch.int64), invalid=Guard((1,), torch.int64), depth=Guard((H, W)), face=Guard((H, W), torch.int32),
             bary=Guard((H, W, 2)), facing=Guard((H, W), torch.int32))
    for kw in (dict(V=-1), dict(F=-1), dict(H=0), dict(W=-1), dict(zn=-1.0), dict(zn=float("nan")), dict(zn=float("inf")), dict(m=bad_m), dict(m=None),
               dict(first=-1), dict(first=F + 1, count=0), dict(count=F + 1), dict(first=1, count=F), dict(count=-1), dict(flags=4),
               dict(V=2 ** 31), dict(F=2 ** 31 // 3 + 1), dict(H=65536, W=65536)):
        st = _lib().estd_mesh_raster(_p(xyz), kw.get("V", V), _p(faces), kw.get("F", F), kw.get("first", 0), kw.get("count", min(F, kw.get("F", F))),
                                     kw.get("m", m), kw.get("H", H), kw.get("W", W), kw.get("zn", zn), kw.get("flags", 2), _p(g["keys"].t),
                                     _p(g["invalid"].t), _stream())
        torch.cuda.synchronize()
        assert st in (-1, -3) and all(x.untouched() for x in g.values()), (kw, st)
        if not {"zn", "first", "count", "flags"} & set(kw):
            st = _lib().estd_mesh_raster_resolve(_p(xyz), kw.get("V", V), _p(faces), kw.get("F", F), kw.get("m", m), kw.get("H", H), kw.get("W", W),
                                                 _p(g["keys"].t), _p(g["depth"].t), _p(g["face"].t), _p(g["bary"].t), _p(g["facing"].t), _stream())
            torch.cuda.synchronize()
            assert st in (-1, -3) and all(x.untouched() for x in g.values()), (kw, st)


def test_the_messages_are_the_same_under_both_bindings():
    from estdepth_amd import ops
    xyz, faces, mat, H, W, zn = on_device("interpenetrating")
    nan = mat.clone()
    nan[0] = float("nan")
    for kw in (dict(faces=faces.to(torch.int64)), dict(mat=mat.float()), dict(mat=nan), dict(H=0), dict(zn=float("nan"))):
        a = dict(xyz=xyz, faces=faces, mat=mat, H=H, W=W, zn=zn)
        a.update(kw)
        texts = []
        for binding in ("torch", "ctypes"):
            with pytest.raises(RuntimeError) as e:
                under(binding, lambda: ops.mesh_raster(a["xyz"], a["faces"], a["mat"], a["H"], a["W"], a["zn"]))
            texts.append(str(e.value).split("\n")[0])
        assert texts[0] == texts[1] and texts[0].startswith("mesh_raster: "), texts


def test_every_claimed_instance_ran():
    """the kernels the profiler saw under this suite's cases (two more calls here, should this test run alone) are exactly the claimed ones"""
    from estdepth_amd import ops
    xyz, faces, mat, H, W, zn = on_device("tri-9x7")
    profiled(WITHOUT_LOAD, lambda: ops.mesh_raster(xyz, faces, mat, H, W, zn))
    profiled(WITH_LOAD, lambda: ops.mesh_raster(xyz, faces, mat, H, W, zn, preload=True))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
