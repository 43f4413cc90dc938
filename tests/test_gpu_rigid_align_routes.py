"""The kernel instances of the rigid registration (csrc/track/rigid_align.hip) under the route protocol of tests/test_gpu_track_routes.py,
against the float64 reference of tests/rigid_align_ref.py and its comparison.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel instance the source emits (tests/test_rigid_align_resources_cpu.py compiles the file and
asserts that the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

A route is one kernel instance.  Each case
  * asserts WHICH instances ran (torch.profiler's demangled names): the apply kernel for ops.rigid_apply, the system kernel and the
    reduction behind it for ops.rigid_system, nothing else;
  * runs the ops under both bindings and once more through the C ABI (ctypes) with every device input and output carved out of buffers
    filled with a NaN sentinel: the three results are bit-identical and every band keeps the sentinel;
  * compares with the float64 reference under rigid_align_ref.compare (ambiguous share <= 0.03 included);
  * sits on the edges of the launch shape: N = 1, 255, 256, 257 (one point short of / exactly / past one 256-point workgroup), 64 * 256 + 1
    (65 workgroups: the reduce loop wraps) and 16 641 (66 workgroups); with and without source normals, both metrics, the target read by
    index and in place, the cosine gate one- and two-sided, an index of -1 and one equal to Nt among valid ones (every case from N = 16
    on)."""
import ctypes
import re

import pytest
import torch

from estdepth_amd import registration  # noqa: F401 -- the feature under test: without it this module does not import

import rigid_align_ref as R
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernel instances that reach it (no template arguments: one instance each)
    "rigid_apply": ["rigid_apply_kernel"],
    "rigid_system": ["rigid_system_kernel"],
    "rigid_reduce": ["rigid_reduce_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(rigid_\w+_kernel)(<[^>()]*>)?")
APPLY = set(INSTANCES["rigid_apply"])
SYSTEM = set(INSTANCES["rigid_system"]) | set(INSTANCES["rigid_reduce"])
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


def _inputs(c):
    """the device tensors of a case: (apply's, system's)"""
    a = dict(src=_dev(c["src"]), src_normal=_dev(c["src_normal"]) if c["src_normal"] is not None else None)
    s = dict(moved=_dev(c["moved"]), moved_normal=_dev(c["moved_normal"]) if c["moved_normal"] is not None else None,
             index=_dev(c["index"]), target=_dev(c["target"]), normal=_dev(c["normal"]))
    return a, s


def _apply(c, a):
    from estdepth_amd import ops
    return ops.rigid_apply(a["src"], a["src_normal"], torch.from_numpy(c["T12"]))


def _system(c, s, dist_max=None):
    from estdepth_amd import ops
    return ops.rigid_system(s["moved"], s["moved_normal"], s["index"], s["target"], s["normal"], c["by_index"], c["metric"],
                            c["dist_max"] if dist_max is None else dist_max, c["cos_min"], c["two_sided"])


def _raw_apply(c, a):
    n = c["N"]
    g = dict(moved=Guard((n, 3)))
    if a["src_normal"] is not None:
        g["moved_normal"] = Guard((n, 3))
    st = _lib().estd_rigid_apply(a["src"].data_ptr(), a["src_normal"].data_ptr() if a["src_normal"] is not None else None, n,
                                 (ctypes.c_float * 12)(*c["T12"].reshape(-1).tolist()), g["moved"].t.data_ptr(),
                                 g["moved_normal"].t.data_ptr() if "moved_normal" in g else None, _stream())
    torch.cuda.synchronize()
    return st, g


def _raw_system(c, s, dist_max=None):
    """estd_rigid_system on guarded outputs -> (status, guards dict)"""
    from estdepth_amd import _native, ops
    n = c["N"]
    n_part = _lib().estd_rigid_system_partials(n) // 8
    g = dict(residual=Guard((n,)), match=Guard((n,), torch.int64), sums=Guard((R.N_SUMS,), torch.float64), partials=Guard((n_part,), torch.float64))
    d = _native.RigidSystemDesc()
    d.N, d.Nt, d.Nn = n, s["target"].shape[0], s["normal"].shape[0]
    d.metric, d.by_index, d.two_sided = ops.RIGID_METRICS[c["metric"]], int(c["by_index"]), int(c["two_sided"])
    d.dist_max = c["dist_max"] if dist_max is None else dist_max
    d.cos_min = float("-inf") if c["cos_min"] is None else c["cos_min"]
    d.moved, d.index, d.target, d.normal = (s[k].data_ptr() for k in ("moved", "index", "target", "normal"))
    d.moved_normal = s["moved_normal"].data_ptr() if s["moved_normal"] is not None else None
    d.residual, d.match, d.sums, d.partials = (g[k].t.data_ptr() for k in ("residual", "match", "sums", "partials"))
    st = _lib().estd_rigid_system(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    return st, g


def _guarded(t):
    return {k: (Guard(v.shape, v.dtype, fill=v) if v is not None else None) for k, v in t.items()}


ROUTE_CASES = sorted(k for k in R.CASES if not k.startswith("cond-")) + ["tie"]


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_rigid_align_route(name):
    c, ref = R.build_case(name), R.reference(name)
    a, s = _inputs(c)
    what = "rigid_align %s" % name
    # the apply kernel
    mt = profiled(APPLY, lambda: _apply(c, a))
    mc = under("ctypes", lambda: _apply(c, a))
    ga = _guarded(a)
    st, g = _raw_apply(c, {k: (v.t if v is not None else None) for k, v in ga.items()})
    assert st == 0
    _intact(what, **{k: v for k, v in ga.items() if v is not None}, **g)
    assert _same(mt[0], mc[0]) and _same(mt[0], g["moved"].t), "%s: moved differs between the three launches" % what
    assert (mt[1] is None) == (c["src_normal"] is None) == (mc[1] is None)
    if mt[1] is not None:
        assert _same(mt[1], mc[1]) and _same(mt[1], g["moved_normal"].t), "%s: moved_normal differs between the three launches" % what
    # the system kernels, on the case's own fp32 moved cloud
    rt = profiled(SYSTEM, lambda: _system(c, s))
    rc = under("ctypes", lambda: _system(c, s))
    gs = _guarded(s)
    st, g = _raw_system(c, {k: (v.t if v is not None else None) for k, v in gs.items()})
    assert st == 0
    _intact(what, **{k: v for k, v in gs.items() if v is not None}, **g)
    for x, y, k in zip(rt, rc, ("residual", "match", "sums")):
        assert _same(x, y) and _same(x, g[k].t), "%s: %s differs between the three launches" % (what, k)
    got = dict(moved=_cpu(mt[0]), moved_normal=_cpu(mt[1]) if mt[1] is not None else None, residual=_cpu(rt[0]), match=_cpu(rt[1]), sums=_cpu(rt[2]))
    fig = R.compare(got, c, ref, what)
    assert fig["matched"] >= 1
    if name == "tie":
        assert got["match"][5] == 5 and fig["matched"] == 6                    # e2 == dist_max^2 passes the gate
    if c["N"] >= 16 and name != "tie":
        assert c["index"][3] == -1 and c["index"][9] == c["target"].shape[0] + (0 if c["by_index"] else 7)
        assert got["match"][3] == -1 and got["match"][9] == -1                  # the index -1 and the index Nt
    print("RIGID-RATIO %s moved %.3f residual %.3f sums %.3f amb %.4f matched %d" % (name, fig["moved_ratio"], fig["residual_ratio"], fig["sum_ratio"],
                                                                                  fig["amb_share"], fig["matched"]))


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_nothing_matches_launches_both_and_sums_to_zero(binding):
    """every partner beyond the gate: both kernels run, every match is -1, every residual 0 and the 29 sums are exactly +0"""
    c = R.build_case("none")
    _, s = _inputs(c)
    res, mt, sums = profiled(SYSTEM, lambda: _system(c, s), binding)
    assert bool((mt == -1).all()) and bool((res.view(torch.int32) == 0).all()) and bool((sums.view(torch.int64) == 0).all())
    R.compare(dict(residual=_cpu(res), match=_cpu(mt), sums=_cpu(sums)), c, R.reference("none"), "rigid_align none %s" % binding)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    c = R.build_case("plane-n257")
    a, s = _inputs(c)
    with pytest.raises(RuntimeError):
        profiled(set(), lambda: _system(c, s, dist_max=0.0), binding)
    bad = torch.from_numpy(c["T12"]).clone()
    bad[1, 2] = float("nan")
    with pytest.raises(RuntimeError):
        profiled(set(), lambda: ops.rigid_apply(a["src"], a["src_normal"], bad), binding)
    st, g = _raw_system(c, s, dist_max=0.0)
    assert st == -1 and all(x.untouched() for x in g.values())
    st, g = _raw_apply(dict(c, T12=bad.numpy()), a)
    assert st == -1 and all(x.untouched() for x in g.values())


def test_no_points_launches_only_the_reduction():
    from estdepth_amd import ops
    c = R.build_case("plane-n257")
    _, s = _inputs(c)
    empty, none = torch.empty((0, 3), device=DEV), torch.empty((0,), device=DEV, dtype=torch.int64)
    moved, mn = profiled(set(), lambda: ops.rigid_apply(empty, None, torch.from_numpy(c["T12"])))
    assert moved.shape == (0, 3) and mn is None
    for binding in ("torch", "ctypes"):
        res, mt, sums = profiled(set(INSTANCES["rigid_reduce"]), lambda: ops.rigid_system(empty, None, none, s["target"], s["normal"]), binding)
        assert res.shape == (0,) and mt.shape == (0,) and bool((sums.view(torch.int64) == 0).all())


def test_every_claimed_instance_ran():
    """the instances the profiler saw under this suite's cases (one more case here, should this test run alone) are exactly the claimed ones"""
    c = R.build_case("plane-n257")
    a, s = _inputs(c)
    profiled(APPLY, lambda: _apply(c, a))
    profiled(SYSTEM, lambda: _system(c, s))
    assert _RAN == APPLY | SYSTEM, (sorted(_RAN), sorted(APPLY | SYSTEM))
