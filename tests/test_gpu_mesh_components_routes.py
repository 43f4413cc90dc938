"""The kernels of the mesh components (csrc/mesh/mesh_components.hip) under the route protocol of tests/test_gpu_tsdf_mesh_routes.py,
against the numpy reference of tests/mesh_components_ref.py and its comparison: integer equality, no tolerance.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel the source emits (tests/test_mesh_components_resources_cpu.py compiles the file and asserts
that the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

Each case of mesh_components_ref.CASES
  * asserts WHICH kernels ran (torch.profiler's demangled names): init, hook, flatten and count, or the init kernel alone when there are
    no faces or no vertices -- it defines the outputs then, and nothing else may run;
  * runs the operator under both bindings and once more through the C ABI (ctypes) with the faces, the labels (which are the union-find's
    only scratch), the triangle counts and the invalid counter carved out of buffers filled with a sentinel: the three results are
    bit-identical and every band keeps the sentinel -- also in the case whose faces name vertices at -1, V, 2^30 and 2^31 - 1;
  * equals the reference.
The shapes: nothing at all; vertices without faces; one triangle; degenerate and duplicated triangles; strips of 300 triangles (long
chains) with ascending, descending and permuted ids; stars of 500 triangles round the last and round the first vertex (every hook meets
in one root); disjoint triangles round the 64-lane wave and the 256-lane workgroup (64 distinct roots per wave in the count); permuted
and shuffled quad grids of 18 workgroups and of 800 (all eight XCDs hook into the same five trees at once); surface-net meshes with
fragments and loose vertices."""
import re

import pytest
import torch

from estdepth_amd.fusion3d import mesh_components  # noqa: F401 -- the feature under test: without it this module does not import

import mesh_components_ref as C
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _p, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernels that reach it
    "mesh_components": ["mesh_cc_init_kernel", "mesh_cc_hook_kernel", "mesh_cc_flatten_kernel", "mesh_cc_count_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(mesh_cc_\w+_kernel)(<[^>()]*>)?")
ALL = {k for ks in INSTANCES.values() for k in ks}
INIT_ONLY = {"mesh_cc_init_kernel"}
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


def _raw(faces, V, n_faces=None, n_vertices=None):
    """estd_mesh_components on guarded buffers -> (status, guards dict); the invalid counter starts at the sentinel: the call defines it"""
    F = faces.shape[0]
    g = dict(faces=Guard((F, 3), torch.int32, fill=faces), label=Guard((V,), torch.int32), triangles=Guard((V,), torch.int32),
             invalid=Guard((1,), torch.int64))
    st = _lib().estd_mesh_components(_p(g["faces"].t), F if n_faces is None else n_faces, V if n_vertices is None else n_vertices,
                                     _p(g["label"].t), _p(g["triangles"].t), _p(g["invalid"].t), _stream())
    torch.cuda.synchronize()
    return st, g


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_components_route(name):
    from estdepth_amd import ops
    faces_np, V = C.build_case(name)
    ref = C.reference(name)
    faces = _dev(faces_np)
    want = ALL if V > 0 and faces.shape[0] > 0 else INIT_ONLY
    what = "components %s" % name
    rt = profiled(want, lambda: ops.mesh_components(faces, V))
    rc = profiled(want, lambda: ops.mesh_components(faces, V), "ctypes")
    st, g = _raw(faces, V)
    assert st == 0
    _intact(what, **g)
    assert torch.equal(g["faces"].t, faces), "%s: the faces were written" % what
    raw = (g["label"].t, g["triangles"].t, g["invalid"].t)
    for k, a, b, c in zip(("label", "triangles", "invalid"), rt, rc, raw):
        assert _same(a, b) and _same(a, c), "%s: %s differs between the three launches" % (what, k)
    fig = C.compare(dict(label=_cpu(rt[0]), triangles=_cpu(rt[1]), invalid=int(rt[2].item())), ref, what)
    print("MESH-CC-ROUTE %s: %d faces %d vertices %d components (%d with faces) %d invalid" % (
        name, faces.shape[0], fig["vertices"], fig["components"], fig["with_faces"], fig["invalid"]))


def test_out_of_range_indices_are_reported_and_never_an_address():
    """-1, V, 2^30, -2^31 and 2^31 - 1 among valid triangles: the count comes back, nothing outside the arrays is touched, and the host
    layer names the count"""
    faces_np, V = C.build_case("out-of-range")
    st, g = _raw(_dev(faces_np), V)
    assert st == 0 and int(g["invalid"].t.item()) == 6 == C.reference("out-of-range")["invalid"]
    _intact("out of range", **g)
    with pytest.raises(RuntimeError, match="mesh_components: 6 of 10 faces"):
        mesh_components(faces_np, V)
    # without vertices every face is out of range: the init kernel alone reports them
    from estdepth_amd import ops
    for binding in ("torch", "ctypes"):
        out = profiled(INIT_ONLY, lambda: ops.mesh_components(_dev(faces_np), 0), binding)
        assert out[0].shape == (0,) and out[1].shape == (0,) and int(out[2].item()) == 10
    st, g = _raw(_dev(faces_np), 0)
    assert st == 0 and int(g["invalid"].t.item()) == 10 and g["label"].untouched() and g["triangles"].untouched()


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    from estdepth_amd import ops
    faces = _dev(C.build_case("degenerate")[0])
    for bad, V in ((faces, -1), (faces, 2 ** 31), (faces.to(torch.int64), 10), (faces.t().contiguous().t(), 10), (faces.reshape(-1), 10),
                   (faces.reshape(2, 3, 3), 10), (faces.cpu(), 10)):
        with pytest.raises(RuntimeError):
            profiled(set(), lambda: ops.mesh_components(bad, V), binding)
    for kw in (dict(n_faces=-1), dict(n_vertices=-1), dict(n_vertices=2 ** 31), dict(n_faces=2 ** 31 // 3 + 1)):
        st, g = _raw(faces, 10, **kw)
        assert st in (-1, -3) and all(g[k].untouched() for k in ("label", "triangles", "invalid")), kw


def test_the_messages_are_the_same_under_both_bindings():
    from estdepth_amd import ops
    faces = _dev(C.build_case("degenerate")[0])
    assert not faces.t().contiguous().t().is_contiguous()
    for bad, V in ((faces, -1), (faces.to(torch.int64), 10), (faces.t().contiguous().t(), 10), (faces.reshape(-1), 10)):
        texts = []
        for binding in ("torch", "ctypes"):
            with pytest.raises(RuntimeError) as e:
                under(binding, lambda: ops.mesh_components(bad, V))
            texts.append(str(e.value).split("\n")[0])
        assert texts[0] == texts[1] and texts[0].startswith("mesh_components: "), texts


def test_every_claimed_instance_ran():
    """the kernels the profiler saw under this suite's cases (one more case here, should this test run alone) are exactly the claimed ones"""
    from estdepth_amd import ops
    faces_np, V = C.build_case("grid-48")
    profiled(ALL, lambda: ops.mesh_components(_dev(faces_np), V))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
