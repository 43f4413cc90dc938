"""The kernel instances of the frame-to-model alignment (csrc/track/frame_align.hip) under the route protocol of
tests/test_gpu_recon3d_routes.py, against the float64 reference of tests/track_ref.py and its comparison.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel instance the source emits (tests/test_track_resources_cpu.py compiles the file and asserts
that the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

A route is one kernel instance.  Each case
  * asserts WHICH instances ran (torch.profiler's demangled names): the alignment kernel and the reduction behind it, nothing else;
  * runs the op under both bindings and once more through the C ABI (ctypes) with every device input and output -- the live depth and
    confidence, the model maps, the residual and match maps, the 29 sums and the partials -- carved out of buffers filled with a NaN
    sentinel: the three results are bit-identical and every band keeps the sentinel;
  * compares with the float64 reference under track_ref.compare (ambiguous share <= 0.03 included);
  * sits on the edges of the launch shape: one pixel, one pixel short of / past / exactly one 16 x 16 workgroup, a map of 6 tiles and one
    of 17 tiles in one row, with and without a confidence map, against model maps of the same and of another size."""
import ctypes
import re

import numpy as np
import pytest
import torch

from estdepth_amd import tracking  # noqa: F401 -- the feature under test: without it this module does not import

import track_ref as T
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernel instances that reach it (no template arguments: one instance each)
    "frame_align": ["frame_align_kernel"],
    "frame_align_reduce": ["frame_align_reduce_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(frame_align\w*_kernel)(<[^>()]*>)?")
BOTH = {k for ks in INSTANCES.values() for k in ks}
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


def _mats(c):
    return torch.from_numpy(np.ascontiguousarray(c["mats"].reshape(3, 12)))


def _raw(c, depth, conf, m_depth, m_normal):
    """estd_frame_align on guarded outputs -> (status, guards dict)"""
    from estdepth_amd import _native
    H, W = depth.shape
    n_part = _lib().estd_frame_align_partials(H, W) // 8
    g = dict(residual=Guard((H, W)), match=Guard((H, W), torch.int32), sums=Guard((T.N_SUMS,), torch.float64),
             partials=Guard((n_part,), torch.float64))
    d = _native.FrameAlignDesc()
    d.H, d.W, d.Hm, d.Wm = H, W, m_depth.shape[0], m_depth.shape[1]
    d.dist_max, d.z_near, d.conf_min = c["dist_max"], c["z_near"], c["conf_min"]
    d.depth, d.conf = depth.data_ptr(), conf.data_ptr() if conf is not None else None
    d.m_depth, d.m_normal = m_depth.data_ptr(), m_normal.data_ptr()
    d.residual, d.match, d.sums, d.partials = (g[k].t.data_ptr() for k in ("residual", "match", "sums", "partials"))
    flat = c["mats"].reshape(-1).tolist()
    for i in range(12):
        d.L[i], d.Fm[i], d.Bm[i] = flat[i], flat[12 + i], flat[24 + i]
    st = _lib().estd_frame_align(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    return st, g


ROUTE_CASES = ["r%dx%d" % hw for hw in T.ROUTE_SIZES] + ["small-model"]


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_frame_align_route(name):
    from estdepth_amd import ops
    c, ref = T.build_case(name), T.reference(name)
    depth, m_depth, m_normal = _dev(c["depth"]), _dev(c["m_depth"]), _dev(c["m_normal"])
    conf = _dev(c["conf"]) if c["conf"] is not None else None
    run = lambda: ops.frame_align(depth, conf, m_depth, m_normal, _mats(c), c["dist_max"], c["z_near"], c["conf_min"])      # noqa: E731
    rt = profiled(BOTH, run)
    rc = under("ctypes", run)
    gi = dict(depth=Guard(depth.shape, fill=depth), m_depth=Guard(m_depth.shape, fill=m_depth), m_normal=Guard(m_normal.shape, fill=m_normal))
    if conf is not None:
        gi["conf"] = Guard(conf.shape, fill=conf)
    st, g = _raw(c, gi["depth"].t, gi["conf"].t if conf is not None else None, gi["m_depth"].t, gi["m_normal"].t)
    what = "frame_align %s" % name
    assert st == 0
    _intact(what, **gi, **g)
    for a, b, k in zip(rt, rc, ("residual", "match", "sums")):
        assert _same(a, b) and _same(a, g[k].t), "%s: %s differs between the three launches" % (what, k)
    fig = T.compare(dict(residual=_cpu(rt[0]), match=_cpu(rt[1]), sums=_cpu(rt[2])), c, ref, what)
    assert fig["matched"] >= 1
    print("TRACK-RATIO %s residual %.3f sums %.3f amb %.4f matched %d" % (name, fig["residual_ratio"], fig["sum_ratio"], fig["amb_share"], fig["matched"]))


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_nothing_matches_launches_both_and_sums_to_zero(binding):
    """a guess that looks away from the model: both kernels run, every match is -1, every residual 0 and the 29 sums are exactly +0"""
    from estdepth_amd import ops
    c = T.build_case("away")
    depth, m_depth, m_normal = _dev(c["depth"]), _dev(c["m_depth"]), _dev(c["m_normal"])
    res, mt, sums = profiled(BOTH, lambda: ops.frame_align(depth, None, m_depth, m_normal, _mats(c), c["dist_max"], c["z_near"], 0.0), binding)
    assert bool((mt == -1).all()) and bool((res.view(torch.int32) == 0).all()) and bool((sums.view(torch.int64) == 0).all())
    T.compare(dict(residual=_cpu(res), match=_cpu(mt), sums=_cpu(sums)), c, T.reference("away"), "frame_align away %s" % binding)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    c = T.build_case("r16x16")
    depth, m_depth, m_normal = _dev(c["depth"]), _dev(c["m_depth"]), _dev(c["m_normal"])
    with pytest.raises(RuntimeError):
        profiled(set(), lambda: ops.frame_align(depth, None, m_depth, m_normal, _mats(c), 0.0, c["z_near"], 0.0), binding)
    st, g = _raw(dict(c, dist_max=0.0), depth, None, m_depth, m_normal)
    assert st == -1 and all(x.untouched() for x in g.values())


def test_every_claimed_instance_ran():
    """the instances the profiler saw under this suite's cases (one more case here, should this test run alone) are exactly the claimed ones"""
    from estdepth_amd import ops
    c = T.build_case("r17x33")
    depth, m_depth, m_normal = _dev(c["depth"]), _dev(c["m_depth"]), _dev(c["m_normal"])
    profiled(BOTH, lambda: ops.frame_align(depth, None, m_depth, m_normal, _mats(c), c["dist_max"], c["z_near"], 0.0))
    assert _RAN == BOTH, (sorted(_RAN), sorted(BOTH))
