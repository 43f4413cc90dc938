"""The kernels of the mesh sampling (csrc/mesh/mesh_sample.hip) under the route protocol of tests/test_gpu_mesh_components_routes.py,
against the float64 / integer reference of tests/mesh_sample_ref.py and its comparison (bounds derived there, held to 2 x).

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel the source emits (tests/test_mesh_sample_resources_cpu.py compiles the file and asserts that
the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

Each case of mesh_sample_ref.CASES
  * asserts WHICH kernels ran (torch.profiler's demangled names): the area kernel and the sample kernel, the area kernel alone with no
    samples asked for, none without faces;
  * runs the operator under both bindings: bit-identical, and within the reference's bounds (areas, face normals, positions and
    attributes; invalid count, triangles and barycentric pairs equal; the triangles chosen from the device's own areas).
One case goes through the C ABI (ctypes) with every input and output carved out of buffers filled with a NaN sentinel: the same bits
again, every band intact -- for the mesh whose faces name vertices at -1, V and 2^31 - 1 too."""
import re

import numpy as np
import pytest
import torch

from estdepth_amd.fusion3d import sample_mesh  # noqa: F401 -- the feature under test: without it this module does not import

import mesh_sample_ref as S
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _p, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernels that reach it
    "mesh_face_area": ["mesh_face_area_kernel"],
    "mesh_sample": ["mesh_sample_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(mesh_face_area_kernel|mesh_sample_kernel)(<[^>()]*>)?")
ALL = {k for ks in INSTANCES.values() for k in ks}
AREA_ONLY = {"mesh_face_area_kernel"}
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
    xyz, faces, attrs, n, seed = S.build_case(name)
    return _dev(xyz), _dev(faces), None if attrs is None else _dev(attrs), n, seed


def as_got(out, face_normal=None):
    """the operator's tuple as mesh_sample_ref.compare takes it"""
    return dict(xyz=_cpu(out[0]), face=_cpu(out[1]), bary=_cpu(out[2]), normal=_cpu(out[3]), attrs=None if out[4] is None else _cpu(out[4]),
                area=_cpu(out[5]), invalid=int(out[6].item()), face_normal=None if face_normal is None else _cpu(face_normal))


def raw(xyz, faces, attrs, n, seed, first=0, count=None, w=None):
    """estd_mesh_face_area, the glue, estd_mesh_sample on guarded buffers -> (the operator's tuple + face_normal, guards dict).
    ``first`` / ``count``: the rows of a split launch; ``w``: a stratum of the caller's"""
    V, F = xyz.shape[0], faces.shape[0]
    C = 0 if attrs is None else attrs.shape[1]
    count = n - first if count is None else count
    g = dict(xyz=Guard((V, 3), fill=xyz), faces=Guard((F, 3), torch.int32, fill=faces), area=Guard((F,), torch.float64),
             face_normal=Guard((F, 3)), invalid=Guard((1,), torch.int64))
    if C:
        g["attrs"] = Guard((V, C), fill=attrs)
    assert _lib().estd_mesh_face_area(_p(g["xyz"].t), V, _p(g["faces"].t), F, _p(g["area"].t), _p(g["face_normal"].t), _p(g["invalid"].t),
                                      _stream()) == 0
    area = g["area"].t
    q = torch.floor(area * 2.0 ** S.scale_exponent(F, float(area.max().item()))).to(torch.int64)
    g["cum"] = Guard((F,), torch.int64, fill=torch.cumsum(q, 0))
    if w is None:
        w = S.stratum(int(g["cum"].t[-1].item()), n)
    g.update(out_xyz=Guard((count, 3)), face=Guard((count,), torch.int32), bary=Guard((count, 2)), normal=Guard((count, 3)))
    if C:
        g["out_attrs"] = Guard((count, C))
    st = _lib().estd_mesh_sample(_p(g["xyz"].t), V, _p(g["faces"].t), F, _p(g["attrs"].t) if C else None, C, _p(g["cum"].t), _p(g["face_normal"].t),
                                 count, first, w, seed & 0xffffffffffffffff, _p(g["out_xyz"].t), _p(g["face"].t), _p(g["bary"].t),
                                 _p(g["normal"].t), _p(g["out_attrs"].t) if C else None, _stream())
    torch.cuda.synchronize()
    assert st == 0
    out = (g["out_xyz"].t, g["face"].t, g["bary"].t, g["normal"].t, g["out_attrs"].t if C else None, area, g["invalid"].t, g["face_normal"].t)
    return out, g


@pytest.mark.parametrize("name", S.CASES)
def test_sample_route(name):
    from estdepth_amd import ops
    xyz, faces, attrs, n, seed = on_device(name)
    host = S.build_case(name)
    want = set() if faces.shape[0] == 0 else (AREA_ONLY if n == 0 else ALL)
    what = "sample %s" % name
    rt = profiled(want, lambda: ops.mesh_sample(xyz, faces, attrs, n, seed))
    rc = profiled(want, lambda: ops.mesh_sample(xyz, faces, attrs, n, seed), "ctypes")
    fa_t = profiled(want & AREA_ONLY, lambda: ops.mesh_face_area(xyz, faces))
    fa_c = profiled(want & AREA_ONLY, lambda: ops.mesh_face_area(xyz, faces), "ctypes")
    for k, a, b in zip(("xyz", "face", "bary", "normal", "attrs", "area", "invalid"), rt, rc):
        assert (a is None and b is None) or _same(a, b), "%s: %s differs between the bindings" % (what, k)
    for k, a, b, c in zip(("area", "face_normal", "invalid"), fa_t, fa_c, (rt[5], None, rt[6])):
        assert _same(a, b) and (c is None or _same(a, c)), "%s: %s of mesh_face_area differs" % (what, k)
    fig = S.compare(as_got(rt, fa_t[1]), *host, what)
    print("MESH-SAMPLE-ROUTE %s: %d faces %d invalid %d samples; of the bounds (2 allowed): area %.3f face_normal %.3f xyz %.3f attrs %.3f; "
          "%d normals left out" % (name, fig["faces"], fig["invalid"], fig["samples"], fig["area"], fig.get("face_normal", 0.0), fig["xyz"],
                                   fig.get("attrs", 0.0), fig["left_out"]))


@pytest.mark.parametrize("name", ["out-of-range", "attrs-6"])
def test_the_c_abi_on_guarded_buffers(name):
    """every input and output between NaN bands: the operator's bits again and no band touched, with indices at -1, V and 2^31 - 1 among the faces"""
    from estdepth_amd import ops
    xyz, faces, attrs, n, seed = on_device(name)
    out, g = raw(xyz, faces, attrs, n, seed)
    _intact(name, **g)
    for k in ("xyz", "faces", "attrs"):
        if k in g:
            assert torch.equal(g[k].t, dict(xyz=xyz, faces=faces, attrs=attrs)[k]), "%s: %s was written" % (name, k)
    ref = under("ctypes", lambda: ops.mesh_sample(xyz, faces, attrs, n, seed))
    for k, a, b in zip(("xyz", "face", "bary", "normal", "attrs", "area", "invalid"), out, ref):
        assert (a is None and b is None) or _same(a, b), "%s: %s differs from the operator's" % (name, k)
    S.compare(as_got(out, out[7]), *S.build_case(name), name)


def test_a_split_launch_gives_the_same_rows():
    """sample i is a function of (seed, i) and the mesh: the launch shape does not enter"""
    xyz, faces, attrs, n, seed = on_device("attrs-3")
    whole, _ = raw(xyz, faces, attrs, n, seed)
    for first, count in ((0, 1), (1, 63), (64, 192), (256, n - 256)):
        part, g = raw(xyz, faces, attrs, n, seed, first, count)
        _intact("split", **g)
        for k, a, b in zip(("xyz", "face", "bary", "normal", "attrs"), part, whole):
            assert _same(a, b[first:first + count]), "%s from sample %d on differs" % (k, first)


def test_a_target_on_a_prefix_sum_takes_the_next_triangle():
    """t_0 = 0 = cum[0] behind a first triangle of no area: the upper bound skips it (mesh_sample_ref.tie_case)"""
    xyz, faces, n, seed, w = S.tie_case()
    out, g = raw(_dev(xyz), _dev(faces), None, n, seed, w=w)
    _intact("tie", **g)
    assert S.h64_int(seed, 0, 0) % w == 0 and int(out[1][0].item()) == 1
    S.compare(as_got(out, out[7]), xyz, faces, None, n, seed, "tie", w=w)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    xyz, faces, attrs, n, seed = on_device("attrs-3")
    V = xyz.shape[0]
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(faces=faces.to(torch.int64)), dict(faces=faces.t().contiguous().t()), dict(faces=faces.cpu()),
                dict(xyz=xyz.double()), dict(xyz=xyz[:, :2].contiguous()), dict(xyz=xyz.cpu()), dict(attrs=attrs[:-1].contiguous()),
                dict(attrs=torch.zeros((V, 7), device=DEV)), dict(attrs=torch.zeros((V, 0), device=DEV)), dict(attrs=attrs.double()),
                dict(attrs=attrs.reshape(-1))):
        kw = dict(xyz=xyz, faces=faces, attrs=attrs, n=n)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_sample(kw["xyz"], kw["faces"], kw["attrs"], kw["n"], seed), binding)
    # the refusals that need the areas come after the area kernel, before the sample kernel
    flat = xyz.clone()
    flat[:, 1:] = 0.0
    with pytest.raises(RuntimeError, match="mesh_sample: the mesh has no area"):
        profiled(AREA_ONLY, lambda: ops.mesh_sample(flat, faces, None, 10, 0), binding)
    # one triangle of 2^49 units and 4095 of 2^-33 of its area: 2^31 - 1 strata would be 2^18 units wide
    few = _dev(np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (1e-5, 0, 0), (0, 1e-5, 0)], np.float32))
    many = _dev(np.asarray([(0, 1, 2)] + [(3, 4, 5)] * 4095, np.int32))
    with pytest.raises(RuntimeError, match="mesh_sample: n_samples = 2147483647 leaves strata of 26[0-9]{4} units of area, fewer than 1048576"):
        profiled(AREA_ONLY, lambda: ops.mesh_sample(few, many, None, 2 ** 31 - 1, 0), binding)
    nan = xyz.clone()
    nan[int(faces[3, 1])] = float("nan")
    with pytest.raises(RuntimeError, match="mesh_sample: xyz holds a coordinate that is not finite"):
        profiled(AREA_ONLY, lambda: ops.mesh_sample(nan, faces, None, 10, 0), binding)


def test_the_entry_points_refuse_before_a_launch():
    xyz, faces, attrs, n, seed = on_device("attrs-3")
    V, F = xyz.shape[0], faces.shape[0]
    g = dict(area=Guard((F,), torch.float64), face_normal=Guard((F, 3)), invalid=Guard((1,), torch.int64))
    for kw in (dict(V=-1), dict(F=-1), dict(V=2 ** 31), dict(F=2 ** 31 // 3 + 1)):
        st = _lib().estd_mesh_face_area(_p(xyz), kw.get("V", V), _p(faces), kw.get("F", F), _p(g["area"].t), _p(g["face_normal"].t),
                                        _p(g["invalid"].t), _stream())
        torch.cuda.synchronize()
        assert st in (-1, -3) and all(x.untouched() for x in g.values()), kw
    assert _lib().estd_mesh_face_area(_p(xyz), V, _p(faces), F, _p(g["area"].t), _p(g["face_normal"].t), None, _stream()) == -1
    out, _ = raw(xyz, faces, None, n, seed)
    cum = torch.cumsum(torch.floor(out[5] * 2.0 ** S.scale_exponent(F, float(out[5].max().item()))).to(torch.int64), 0)
    o = dict(xyz=Guard((n, 3)), face=Guard((n,), torch.int32), bary=Guard((n, 2)), normal=Guard((n, 3)))
    for kw in (dict(n=-1), dict(first=-1), dict(C=-1), dict(C=7), dict(w=0), dict(w=-5), dict(w=2 ** 61), dict(V=0), dict(F=0), dict(first=2 ** 31 - 1),
               dict(n=2 ** 31), dict(C=3)):
        st = _lib().estd_mesh_sample(_p(xyz), kw.get("V", V), _p(faces), kw.get("F", F), None, kw.get("C", 0), _p(cum), _p(out[7]), kw.get("n", n),
                                     kw.get("first", 0), kw.get("w", 1 << 20), 0, _p(o["xyz"].t), _p(o["face"].t), _p(o["bary"].t), _p(o["normal"].t),
                                     None, _stream())
        torch.cuda.synchronize()
        assert st in (-1, -3) and all(x.untouched() for x in o.values()), kw


def test_the_messages_are_the_same_under_both_bindings():
    from estdepth_amd import ops
    xyz, faces, attrs, n, seed = on_device("attrs-3")
    for kw in (dict(n=-1), dict(faces=faces.to(torch.int64)), dict(attrs=attrs[:-1].contiguous()), dict(attrs=torch.zeros((xyz.shape[0], 7), device=DEV))):
        a = dict(xyz=xyz, faces=faces, attrs=attrs, n=n)
        a.update(kw)
        texts = []
        for binding in ("torch", "ctypes"):
            with pytest.raises(RuntimeError) as e:
                under(binding, lambda: ops.mesh_sample(a["xyz"], a["faces"], a["attrs"], a["n"], seed))
            texts.append(str(e.value).split("\n")[0])
        assert texts[0] == texts[1] and texts[0].startswith("mesh_sample: "), texts


def test_every_claimed_instance_ran():
    """the kernels the profiler saw under this suite's cases (one more case here, should this test run alone) are exactly the claimed ones"""
    from estdepth_amd import ops
    xyz, faces, attrs, n, seed = on_device("f65-n64")
    profiled(ALL, lambda: ops.mesh_sample(xyz, faces, attrs, n, seed))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
