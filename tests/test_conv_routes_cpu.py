"""CPU: which route ops.Conv3dPlan.route / ops.Conv2dPlan.route choose, and what ops.CONV3D_ROUTES / ops.CONV2D_ROUTES wire to it.

The route functions are pure, so a plan on the CPU answers them with no library loaded (``_native.has_ab`` is replaced: the plan captures it
at construction).  The cases of the GPU route tests are imported, not copied: the names checked here are the names whose kernels
tests/test_gpu_conv3d_routes.py and tests/test_gpu_conv2d_routes.py assert on the device."""
import pytest
import torch

import test_gpu_conv2d_routes as G2
import test_gpu_conv3d_routes as G3
from estdepth_amd import _native, ops, packing

PLANS3D = ("32>32", "33>32", "33>33", "32>16", "16>16", "16>16h")
DEFAULT2D = dict(CONV2D_ARITH="f32", CONV2D_ALGO="wino2", CONV2D_NT="auto", C2W2_DIL2=True)


@pytest.fixture
def build(monkeypatch):
    """build(ab): the library 'carries the A/B kernels' or not, for the plans constructed afterwards"""
    def set_ab(ab):
        monkeypatch.setattr(_native, "has_ab", lambda: ab)
    return set_ab


@pytest.fixture
def switches(monkeypatch):
    def set_switches(**sw):
        for k, v in {**G3.DEFAULT, "CONV3D_ARITH": "f32", **DEFAULT2D, **sw}.items():
            monkeypatch.setattr(ops, k, v)
    return set_switches


def _plan3d(plan, acts=("relu",)):
    return ops.Conv3dPlan(device="cpu", **G3._plan_args(plan, acts, 1))


def _call(plan, epi=()):
    """the arguments of Conv3dPlan.route for the call tests/test_gpu_conv3d_routes.py::_launch makes of a case"""
    out = plan.head_w is None or "main" in epi
    return dict(out=out, in_extra=plan.has_extra, out_extra=plan.n_tiles == 3, out_head="head" in epi, residual="res" in epi,
                residual2="res2" in epi, stats_partials="stats" in epi, gate="gate" in epi, out_channels=16 * min(plan.n_tiles, 2) if out else None,
                accumulate="acc" in epi, out_scale=0.37 if "scale" in epi else 1.0)


def _forms(plan, route):
    """the weight forms CONV3D_ROUTES names for the route, as far as the plan's shape defines them"""
    return sorted({form for la in ops.CONV3D_ROUTES[route] for form in la.weights.values() if plan._packs.has(form)})


@pytest.mark.parametrize("case", G3.CASES + G3.READBACK)
def test_conv3d_default_build_routes(case, build, switches):
    build(False)
    switches(**{k: v for k, v in case["sw"].items() if k != "BINDING"})
    plan = _plan3d(case["plan"], case["acts"])
    assert plan.route(**_call(plan, case["epi"])) == case["route"]


# (plan, activations, switches, epilogue) -> the route in an ESTD_BUILD_AB=1 build, in the default build (None: RuntimeError, the switch
# needs the A/B kernels); from a run of every switch and argument combination against the dispatch this table replaced
AB_ROUTES = [
    ("32>32", ("relu",), dict(CONV3D_ARITH="bf16x3"), (), "split", None),
    ("33>32", ("tanh",), dict(CONV3D_ARITH="bf16x3"), (), "split", None),
    ("33>33", ("relu",), dict(CONV3D_ARITH="bf16x3"), (), "split", None),
    ("32>32", ("tanh",), dict(CONV3D_ARITH="bf16x3"), (), "wino3", None),          # (no tanh instance of the split kernel)
    ("32>16", ("none",), dict(CONV3D_ARITH="bf16x3"), (), "split", None),
    ("16>16h", ("relu",), dict(CONV3D_ARITH="bf16x3"), ("head",), "wino2_c16", None),    # (no split weights with a 1x1x1 head)
    ("32>32", ("relu",), dict(CONV3D_ALGO="wino"), ("res", "acc"), "wino", None),
    ("33>32", ("relu",), dict(CONV3D_ALGO="wino"), (), "wino", None),
    ("33>33", ("tanh",), dict(CONV3D_ALGO="wino"), (), "wino", None),
    ("32>16", ("relu",), dict(CONV3D_ALGO="wino"), (), "direct", None),
    ("32>32", ("relu",), dict(W2X=True, W3=False), ("stats",), "wino2x", None),
    ("32>32", ("relu",), dict(W2X=True), (), "wino3", None),                       # (the three-axis kernel goes first)
    ("32>32", ("tanh",), dict(W2X=True, W3=False), (), "wino2", None),
    ("32>32", ("relu",), dict(W2X=True, W3=False), ("stats", "res"), "wino2", None),
    ("33>33", ("relu",), dict(W2_XOUT=False), (), "wino", "direct"),               # dres2 under ESTD_W2_XOUT=0
    ("33>33", ("relu",), dict(W2_XOUT=False, W3_XOUT=False), (), "wino", "direct"),
    ("33>33", ("relu",), dict(), ("res",), "wino", "direct"),                      # (no read-back stream in the 33 -> 33 instances)
    ("33>32", ("none",), dict(), ("stats",), "direct", "direct"),
]


@pytest.mark.parametrize("plan,acts,sw,epi,with_ab,default", AB_ROUTES)
def test_conv3d_ab_build_routes(plan, acts, sw, epi, with_ab, default, build, switches):
    switches(**sw)
    for ab, want in ((True, with_ab), (False, default)):
        build(ab)
        p = _plan3d(plan, acts)
        if want is None:
            with pytest.raises(RuntimeError, match="A/B kernels"):
                p.route(**_call(p, epi))
        else:
            assert p.route(**_call(p, epi)) == want, "ab=%s" % ab


def test_conv3d_route_refuses(build, switches):
    build(False)
    switches()
    p = _plan3d("32>32")
    with pytest.raises(RuntimeError, match="mismatch"):
        p.route(in_extra=True)
    with pytest.raises(RuntimeError, match="reset gate"):
        p.route(gate=True)
    q = _plan3d("33>33")
    with pytest.raises(RuntimeError, match="reset gate"):                          # (dres2 in two launches: the same check as every route)
        q.route(in_extra=True, out_extra=True, gate=True)
    assert _plan3d("32>16").route(gate=True, out_channels=16) == "wino2_o16"
    for sw in (dict(CONV3D_ALGO="wino3"), dict(CONV3D_ARITH="bf16")):
        switches(**sw)
        with pytest.raises(RuntimeError, match="must be"):
            p.route()


class _Ops:
    """stand-in for torch.ops.estdepth_hip: records (operator, variant), and holds every launch to the argument rules the operators
    check themselves (csrc/torch_ops.cpp)"""

    def __init__(self):
        self.calls = []

    def conv3d_k3(self, *a):
        assert len(a) == 32
        x_extra, w_main, w_extra, w_alt, variant = a[1], a[2], a[3], a[5], a[27]
        assert (x_extra is None) == (w_extra is None), "scalar input channel and its weights go together, in every launch"
        assert (w_main if variant == 0 else w_alt) is not None
        assert a[28] is None or variant == 3
        assert variant != 6 or a[22] is not None
        self.calls.append(("conv3d_k3", variant))

    def conv2d_k3(self, *a):
        assert len(a) == 12
        assert (a[1] if a[11] == 0 else a[2]) is not None
        self.calls.append(("conv2d_k3", a[11]))
        return "out"


@pytest.fixture
def stub_launch(monkeypatch):
    """packing.* returns placeholders and the torch binding records its calls: Conv3dPlan.run / Conv2dPlan.run on the CPU"""
    for name in dir(packing):
        if name.startswith("pack_"):
            monkeypatch.setattr(packing, name, lambda *a, **k: torch.zeros(2, 1))      # (pack_conv3d's result is indexed)
    rec = _Ops()
    monkeypatch.setattr(ops, "T", lambda: rec)
    monkeypatch.setattr(ops, "BINDING", "torch")
    monkeypatch.setattr(ops, "PROFILE", None)
    return rec


def _run3d(plan, epi):
    c = _call(plan, epi)
    t = torch.zeros(1)
    kw = {k: t for k in ("out", "in_extra", "out_extra", "out_head", "residual", "residual2", "stats_partials") if c[k]}
    if c["gate"]:
        kw["gate"] = (t, t, t, t)
    plan.run(t, (1, 1, 1, 1), out_channels=c["out_channels"], accumulate=c["accumulate"], out_scale=c["out_scale"], **kw)


@pytest.mark.parametrize("plan,sw,epi,route,forms", [
    ("32>32", {}, (), "wino3", ["w_wino3"]),
    ("33>33", {}, (), "wino3+xout", ["w_wino3", "w_wino3_extra", "w_xout_taps"]),
    ("33>33", G3.DIRECT, (), "direct", ["w_extra", "w_main", "w_xout"]),
])
def test_conv3d_packs_the_forms_of_its_route(plan, sw, epi, route, forms, build, switches, stub_launch):
    build(False)
    switches(**sw)
    p = _plan3d(plan)
    assert p.route(**_call(p, epi)) == route and p._packs.packed() == []            # routing packs nothing
    _run3d(p, epi)
    assert p._packs.packed() == forms == _forms(p, route)
    assert stub_launch.calls == [("conv3d_k3", la.variant) for la in ops.CONV3D_ROUTES[route]]


@pytest.mark.parametrize("case", G3.CASES + G3.READBACK)
def test_conv3d_every_case_packs_the_forms_the_table_names(case, build, switches, stub_launch):
    build(False)
    switches(**{k: v for k, v in case["sw"].items() if k != "BINDING"})
    p = _plan3d(case["plan"], case["acts"])
    _run3d(p, case["epi"])
    assert p._packs.packed() == _forms(p, case["route"])
    assert stub_launch.calls == [("conv3d_k3", la.variant) for la in ops.CONV3D_ROUTES[case["route"]]]


def _plan2d(cin, cout, dil):
    conv = torch.nn.Conv2d(cin, cout, 3, padding=dil, dilation=dil, bias=False)
    return ops.Conv2dPlan(conv, torch.nn.BatchNorm2d(cout).eval())


def test_route_tables_name_real_fields_and_forms(build):
    build(True)
    defined = set()
    for plan in PLANS3D:
        defined |= set(_plan3d(plan)._packs._fns)
    for table, desc, defined in ((ops.CONV3D_ROUTES, _native.Conv3dDesc, defined),
                                 (ops.CONV2D_ROUTES, _native.Conv2dDesc, set(_plan2d(32, 64, 1)._packs._fns))):
        fields = {f for f, _ in desc._fields_}
        for route, launches in table.items():
            for la in launches:
                assert la.entry in _native._SIGNATURES, (route, la.entry)
                assert set(la.weights) | set(la.overrides) <= fields, (route, la.entry)
                assert {form.format(nt=nt) for form in la.weights.values() for nt in (2, 4)} <= defined, (route, la.entry)
    assert set(ops.CONV3D_ROUTES) == set(G3.KERNELS) | {"split", "wino", "wino2x"}
    assert set(ops.CONV2D_ROUTES) == {"k3", "k3_split", "wino", "wino2"}


# (the cases marked ab exist in an ESTD_BUILD_AB=1 build only)
@pytest.mark.parametrize("case,ab", [pytest.param(c, ab, id="%s-ab%d" % (c["id"], ab)) for c in G2.PLAN_CASES for ab in (False, True)
                                     if ab or not c.get("ab")])
def test_conv2d_routes(case, ab, build, switches, stub_launch):
    build(ab)
    switches(**(case.get("sw") or {}))
    plan = _plan2d(case["cin"], case["cout"], case["dil"])
    kern = case["kern_ab"] if ab and case.get("kern_ab") else case["kern"]
    want = G2._route(kern)
    for n, h, w in case["shapes"]:
        route, nt = plan.route(n, h, w)
        assert route == want, (n, h, w)
        if kern.startswith(("conv2d_k3_kernel<", "conv2d_wino_kernel<")):           # (the work-item width is their first template argument)
            assert nt == int(kern.split("<")[1].split(",")[0]), (n, h, w)
        assert nt in plan.nts and (nt == 2 or not (plan.dil == 2 and route in ("wino", "wino2")))
    n, h, w = case["shapes"][0]
    assert plan.run(torch.zeros(n, h, w, case["cin"])) == "out"
    la, = ops.CONV2D_ROUTES[want]
    assert plan._packs.packed() == sorted(form.format(nt=nt) for form in la.weights.values())
    assert stub_launch.calls == [("conv2d_k3", la.variant)]


@pytest.mark.parametrize("ab,sw,want", [
    (False, dict(CONV2D_NT="4"), ("wino2", 2)),
    (True, dict(CONV2D_NT="4", CONV2D_ALGO="wino"), ("wino", 2)),
    (True, dict(CONV2D_NT="4", C2W2_DIL2=False), ("wino", 2)),
    (False, dict(CONV2D_NT="4", C2W2_DIL2=False), ("k3", 2)),          # (the fallback of the row-only kernel keeps its width)
    (False, dict(CONV2D_NT="4", CONV2D_ALGO="direct"), ("k3", 4)),
    (True, dict(CONV2D_NT="4", CONV2D_ARITH="bf16x3"), ("k3_split", 4)),
])
def test_conv2d_dilation2_work_item_width(ab, sw, want, build, switches):
    build(ab)
    switches(**sw)
    assert _plan2d(64, 64, 2).route(5, 120, 160) == want
