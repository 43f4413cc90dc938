"""Every instance of the 2D glue kernels (the elementwise / layout / pooling passes around the 2D convolutions of stage A:
csrc/est_fusion.hip bn_act / spp_upsample_cat, csrc/conv2d_taps.hip maxpool / avgpool, csrc/refine2d.hip planes_cat / nhwc_to_planes /
upsample2_cat / normalise) against the fp64 reference of tests/glue2d_ref.py.

A route is one kernel instance.  Each case
  * asserts WHICH instance ran, template argument included (torch.profiler's demangled names): ``<64>`` or ``<32>`` of the two LDS
    transposes is predicted from the channel count as the entry point chooses it (C * 65 * 4 <= 64 KiB);
  * compares every output element (sampled rows above 2^31 bytes) with the reference, |gpu - ref| <= C 2^-24 A + pos, C derived from the
    rounding count of the contract (glue2d_ref's docstring; C = 0: bits);
  * runs the op under both bindings and once more through the C ABI directly, with every input, the residual and the output carved out of
    buffers filled with a NaN sentinel: the three results are bit-identical and every band keeps the sentinel (a read outside an input
    would show as NaN in the output -- except under a ReLU, which is why every ReLU route also runs without it);
  * runs shapes at the edges: one float4, maps that are no multiple of a block, more elements than the capped grids of bn_act
    (256 * 16 blocks) and spp_upsample_cat (256 * 32 blocks) so that their grid-stride loops iterate, the channel counts on both sides of the
    <64> / <32> threshold and at the 496-channel limit, HW around the 64- and 32-pixel tiles, and one bn_act above 2^31 bytes."""
import ctypes
import math
import re

import pytest
import torch

import glue2d_ref as R
from test_gpu_conv2d_routes import KERNEL_RE as CONV_KERNEL_RE
from test_gpu_conv2d_routes import SENT32, _guarded, _Switches, _untouched
from test_gpu_sweep_fusion_routes import _as_tuple, _malformed, _sent, _short

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# The constants are glue2d_ref.C_ROUTE / c_avgpool(k): derived there, not fitted, with the worst ratio measured on an MI355X beside each
# (bn_act 1.925 of 3, spp_upsample_cat 3.570 of 6, avgpool 4.288 of 64 at k = 8; the exact routes are bits).

INSTANCES = {
    # route: the kernel instances that reach it
    "bn_act": ["bn_act_nhwc_kernel"],
    "spp_upsample_cat": ["spp_upsample_cat_kernel"],
    "maxpool": ["maxpool3x3s2_nhwc_kernel"],
    "avgpool": ["avgpool_nhwc_kernel"],
    "planes_cat": ["planes_cat_nhwc_kernel<64>", "planes_cat_nhwc_kernel<32>"],
    "nhwc_to_planes": ["nhwc_to_planes_kernel<64>", "nhwc_to_planes_kernel<32>"],
    "upsample2_cat": ["upsample2_cat_nhwc_kernel"],
    "normalise": ["normalise_nhwc_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(bn_act_nhwc_kernel|spp_upsample_cat_kernel|maxpool3x3s2_nhwc_kernel|avgpool_nhwc_kernel|planes_cat_nhwc_kernel|"
                       r"nhwc_to_planes_kernel|upsample2_cat_nhwc_kernel|normalise_nhwc_kernel)(<[^>()]*>)?")
BN_CAP, SPP_CAP = 256 * 16 * 256, 256 * 32 * 256          # float4 elements one sweep of the capped grids covers


def tile_instance(name, C):
    """the instance estd_planes_cat_nhwc / estd_nhwc_to_planes launch for C channels: 64 pixels per block while [C][65] floats fit 64 KiB"""
    return "%s<%d>" % (name, 64 if C * 65 * 4 <= 64 * 1024 else 32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale + shift


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from estdepth_amd import _native
    return _native.lib()


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_route(what, want, inputs, op, raw, out_shape, inplace=None):
    """the protocol of one launch: ``op(inputs)`` under both bindings (the torch one under the profiler), ``raw(guarded inputs, guarded
    output)`` through the C ABI -> the output (of the torch binding; the other two are bit-identical to it).
    ``inplace``: the name of the input the kernel overwrites -- the op works on a copy, the guarded launch on the guarded copy."""
    with _Switches(None, "torch"):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            out_t = op(inputs)
            torch.cuda.synchronize()
    ran = {m.group(1) + (m.group(2) or "") for e in prof.key_averages() for m in [KERNEL_RE.search(e.key)] if m}
    assert ran == {want}, "%s: ran %s, expected %s" % (what, sorted(ran), want)
    assert tuple(out_t.shape) == tuple(out_shape), (what, tuple(out_t.shape))
    with _Switches(None, "ctypes"):
        out_c = op(inputs)
        torch.cuda.synchronize()
    assert _bits_equal(out_t, out_c), "%s: the bindings differ" % what
    del out_c
    guards = {k: _guarded(tuple(v.shape), v) for k, v in inputs.items() if v is not None}
    g_in = {k: (guards[k][1] if v is not None else None) for k, v in inputs.items()}
    if inplace is None:
        guards["out"] = _guarded(tuple(out_shape))
    og = guards[inplace or "out"][1]
    status = raw(g_in, og)
    torch.cuda.synchronize()
    assert status == 0, "%s: estd status %d" % (what, status)
    for k, (buf, _, (lo, hi)) in guards.items():
        assert _untouched(buf, lo, hi) == 0, "%s: written outside %s" % (what, k)
    for k, v in inputs.items():
        if v is not None and k != inplace:
            assert _bits_equal(guards[k][1], v), "%s: input %s was modified" % (what, k)
    assert _bits_equal(og, out_t), "%s: the guarded launch differs from the op" % what
    return out_t


def _report(route, cid, ratio, kern):
    print("ROUTE-RATIO %s %s %.3f %s" % (route, cid, ratio, kern))


# -------------------------------------------------------------------------------------------------------------------------- bn_act
def _bn_op(relu):
    def op(i):
        from estdepth_amd import ops
        x = i["x"].clone().permute(0, 3, 1, 2)
        r = i["res"].permute(0, 3, 1, 2) if i["res"] is not None else None
        out = ops.bn_act_nhwc_(x, i["scale"], i["shift"], relu, r)
        assert out.data_ptr() == x.data_ptr()
        return out.permute(0, 2, 3, 1)
    return op


def _bn_raw(relu):
    def raw(i, og):
        N, H, W, C = i["x"].shape
        return _lib().estd_bn_act_nhwc(_p(og), _p(i["scale"]), _p(i["shift"]), _p(i["res"]), int(relu), N * H * W, C, _stream())
    return raw


def _bn_inputs(shape, res, seed):
    C = shape[3]
    return dict(x=_rand(shape, seed), scale=_rand((C,), seed + 1, 0.3, 1.0), shift=_rand((C,), seed + 2, 0.3),
                res=_rand(shape, seed + 3) if res else None)


BN_SHAPES = [(1, 1, 1, 4), (1, 3, 5, 8), (2, 7, 9, 36), (1, 16, 16, 64), (1, 130, 129, 256)]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_act_route(shape, res, relu):
    assert (math.prod(shape) // 4 > BN_CAP) == (shape == BN_SHAPES[-1])           # the last shape alone iterates the grid-stride loop
    i = _bn_inputs(shape, res, sum(shape) + 2 * res + relu)
    what = "bn_act %s res=%s relu=%s" % ("x".join(map(str, shape)), res, relu)
    out = run_route(what, "bn_act_nhwc_kernel", i, _bn_op(relu), _bn_raw(relu), shape, inplace="x")
    ref, A = R.bn_act_ref(i["x"], i["scale"], i["shift"], i["res"], relu)
    _report("bn_act", what.replace(" ", "-"), R.compare(out, ref, A, R.C_ROUTE["bn_act"], None, what), "bn_act_nhwc_kernel")


def test_bn_act_above_2_31_bytes():
    """(3, 480, 640, 640): 2.36e9 bytes per tensor, generated on the device; the reference at sampled pixels (the first and last included)"""
    shape = (3, 480, 640, 640)
    assert math.prod(shape) * 4 > 2 ** 31
    i = _bn_inputs(shape, True, 77)
    what = "bn_act %s" % (shape,)
    out = run_route(what, "bn_act_nhwc_kernel", i, _bn_op(True), _bn_raw(True), shape, inplace="x")
    npix = shape[0] * shape[1] * shape[2]
    rows = torch.cat([torch.randint(0, npix, (4000,), generator=torch.Generator().manual_seed(5)), torch.tensor([0, 1, npix - 2, npix - 1]),
                      torch.arange(2 ** 31 // (4 * 640) - 2, 2 ** 31 // (4 * 640) + 3)]).to(DEV)     # ... and the pixels around byte 2^31
    flat = lambda t: t.reshape(npix, shape[3])[rows]                            # noqa: E731
    ref, A = R.bn_act_ref(flat(i["x"]), i["scale"], i["shift"], flat(i["res"]), True)
    _report("bn_act", "big", R.compare(flat(out), ref, A, R.C_ROUTE["bn_act"], None, what), "bn_act_nhwc_kernel")


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_relu_turns_nan_into_zero_where_torch_propagates_it(binding):
    """pinned (include/estd_hip.h states it beside the two contracts): fmaxf(v, 0) in bn_act and v > 0 ? v : 0 in planes_cat give 0 for a
    NaN; without the ReLU the NaN passes through"""
    from estdepth_amd import ops
    x = torch.tensor([math.nan, -1.0, 2.0, math.nan, 1.0, math.nan, -3.0, 0.5], device=DEV).reshape(1, 1, 2, 4)
    one, zero = torch.ones(4, device=DEV), torch.zeros(4, device=DEV)
    with _Switches(None, binding):
        y = ops.bn_act_nhwc_(x.clone().permute(0, 3, 1, 2), one, zero, True).permute(0, 2, 3, 1)
        z = ops.bn_act_nhwc_(x.clone().permute(0, 3, 1, 2), one, zero, False).permute(0, 2, 3, 1)
        a, b = torch.ones(1, 1, 2, 4, device=DEV), x.reshape(1, 1, 2, 4)
        c = ops.planes_cat_nhwc(a, b, True)
        d = ops.planes_cat_nhwc(a, b, False)
    assert y.flatten().tolist() == [0.0, 0.0, 2.0, 0.0, 1.0, 0.0, 0.0, 0.5]
    assert torch.equal(torch.isnan(z), torch.isnan(x)) and bool(torch.isnan(torch.relu(x)).any())
    assert c[..., 1].flatten().tolist() == [0.0, 0.0, 2.0, 0.0, 1.0, 0.0, 0.0, 0.5]
    assert torch.equal(torch.isnan(d[..., 1]).flatten(), torch.isnan(x).flatten())


# --------------------------------------------------------------------------------------------------------------- spp_upsample_cat
def _spp_op(i):
    from estdepth_amd import ops
    return ops.spp_upsample_cat(i["raw"], i["skip"], [i[k] for k in sorted(i) if k.startswith("b")])


def _spp_raw(i, og):
    brs = [i[k] for k in sorted(i) if k.startswith("b")]
    nb = len(brs)
    N, H, W, cr = i["raw"].shape
    arr = (ctypes.c_void_p * nb)(*[b.data_ptr() for b in brs])
    bh, bw = (ctypes.c_int * nb)(*[b.shape[1] for b in brs]), (ctypes.c_int * nb)(*[b.shape[2] for b in brs])
    return _lib().estd_spp_upsample_cat(_p(i["raw"]), cr, _p(i["skip"]), i["skip"].shape[3], arr, bh, bw, nb, brs[0].shape[3], _p(og),
                                        N, H, W, _stream())


def _spp_case(what, N, H, W, cr, cs, cb, maps, seed):
    i = dict(raw=_rand((N, H, W, cr), seed), skip=_rand((N, H, W, cs), seed + 1))
    for k, (bh, bw) in enumerate(maps):
        i["b%d" % k] = _rand((N, bh, bw, cb), seed + 2 + k)
    out = run_route(what, "spp_upsample_cat_kernel", i, _spp_op, _spp_raw, (N, H, W, cr + cs + len(maps) * cb))
    ref, A, pos = R.spp_upsample_cat_ref(i["raw"], i["skip"], [i["b%d" % k] for k in range(len(maps))])
    return R.compare(out, ref, A, R.C_ROUTE["spp_upsample_cat"], pos, what)


@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("HW", [(1, 1), (5, 7), (30, 40)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("nb", [1, 4])
def test_spp_upsample_cat_route(nb, HW, C):
    """N = 2 (the branch batch offset); branch maps 1 x 1, 2 x 3 and the output's own size (exact coordinates: a copy)"""
    kinds = [(1, 1), (2, 3), HW]
    worst = 0.0
    for maps in ([[k] for k in kinds] if nb == 1 else [kinds + [(2, 3)], [HW, (1, 1), (3, 2), HW]]):
        what = "spp %dx%d C%d maps %s" % (HW + (C, maps))
        worst = max(worst, _spp_case(what, 2, HW[0], HW[1], C, C, C, maps, 100 * nb + HW[0] + C))
    _report("spp_upsample_cat", "nb%d-%dx%d-C%d" % ((nb,) + HW + (C,)), worst, "spp_upsample_cat_kernel")


def test_spp_upsample_cat_past_the_block_cap():
    """the PSM tail's own shape at N = 2: 2 * 120 * 160 * 80 float4 > 256 * 32 * 256, the grid-stride loop iterates"""
    N, H, W, cr, cs, cb, maps = 2, 120, 160, 64, 128, 32, [(30, 40), (15, 20), (7, 10), (3, 5)]
    assert N * H * W * (cr + cs + 4 * cb) // 4 > SPP_CAP
    _report("spp_upsample_cat", "past-cap", _spp_case("spp past the cap", N, H, W, cr, cs, cb, maps, 9), "spp_upsample_cat_kernel")


# ------------------------------------------------------------------------------------------------------------------------ pooling
def _pool_raw(fn, *tail):
    def raw(i, og):
        N, H, W, C = i["x"].shape
        return getattr(_lib(), fn)(_p(i["x"]), _p(og), N, H, W, C, *tail, _stream())
    return raw


@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("W", [1, 2, 7, 8])
@pytest.mark.parametrize("H", [1, 2, 7, 8])
def test_maxpool_route(H, W, C):
    """inputs hold a NaN, -inf values and one window that is all -inf; bits"""
    from estdepth_amd import ops
    x = _rand((2, H, W, C), 10 * H + W + C, 1.0, -1.0)
    x[0, :3, :3, 1] = -math.inf                     # every tap of output (0, 0) of channel 1
    x[1, H // 2, W // 2, 2] = math.nan
    x[1, H - 1, W - 1, 3] = -math.inf
    what = "maxpool %dx%dx%d" % (H, W, C)
    out = run_route(what, "maxpool3x3s2_nhwc_kernel", dict(x=x), lambda i: ops.maxpool3x3s2_nhwc(i["x"]), _pool_raw("estd_maxpool3x3s2_nhwc"),
                    (2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C))
    ref, A = R.maxpool3x3s2_ref(x)
    assert float(ref[0, 0, 0, 1]) == -math.inf and bool(torch.isnan(ref[1, H // 4, W // 4, 2]))
    R.compare(out, ref, A, R.C_ROUTE["maxpool"], None, what)


@pytest.mark.parametrize("k,H,W,C", [(1, 3, 5, 4), (2, 2, 2, 4), (2, 7, 9, 12), (5, 5, 13, 4), (5, 12, 16, 12), (8, 8, 8, 4), (8, 30, 41, 12),
                                     (4, 60, 83, 32)])
def test_avgpool_route(k, H, W, C):
    """k = H, H and W no multiples of k (floor output size), more than one block"""
    from estdepth_amd import ops
    x = _rand((2, H, W, C), 100 * k + H + W, 1.0, 0.5)
    what = "avgpool k%d %dx%dx%d" % (k, H, W, C)
    out = run_route(what, "avgpool_nhwc_kernel", dict(x=x), lambda i: ops.avgpool_nhwc(i["x"], k), _pool_raw("estd_avgpool_nhwc", k),
                    (2, H // k, W // k, C))
    ref, A = R.avgpool_ref(x, k)
    _report("avgpool-k%d" % k, what.replace(" ", "-"), R.compare(out, ref, A, R.c_avgpool(k), None, what), "avgpool_nhwc_kernel")


# ------------------------------------------------------------------------------------------------------------------------ layouts
TILE_C = [2, 252, 253, 496]                 # 252: the last <64> channel count, 253: the first <32>, 496: the last supported
TILE_HW = [(1, 1), (7, 9), (8, 8), (5, 13), (60, 81)]            # HW = 1, 63, 64, 65, 4860


@pytest.mark.parametrize("relu_b", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("hw", TILE_HW, ids=lambda s: "hw%d" % (s[0] * s[1]))
@pytest.mark.parametrize("C", TILE_C)
def test_planes_cat_route(C, hw, relu_b):
    from estdepth_amd import ops
    Ca = C // 2 if C > 2 else 1
    a, b = _rand((2, Ca) + hw, C + hw[0]), _rand((2, C - Ca) + hw, C + hw[1] + 1)
    what = "planes_cat C%d+%d %dx%d relu_b=%s" % ((Ca, C - Ca) + hw + (relu_b,))
    want = tile_instance("planes_cat_nhwc_kernel", C)
    assert want.endswith("<64>") == (C <= 252)

    def raw(i, og):
        return _lib().estd_planes_cat_nhwc(_p(i["a"]), Ca, _p(i["b"]), C - Ca, int(relu_b), _p(og), 2, hw[0] * hw[1], _stream())
    out = run_route(what, want, dict(a=a, b=b), lambda i: ops.planes_cat_nhwc(i["a"], i["b"], relu_b), raw, (2,) + hw + (C,))
    ref, A = R.planes_cat_ref(a, b, relu_b)
    R.compare(out, ref, A, R.C_ROUTE["planes_cat"], None, what)


@pytest.mark.parametrize("hw", TILE_HW, ids=lambda s: "hw%d" % (s[0] * s[1]))
@pytest.mark.parametrize("C", TILE_C)
def test_nhwc_to_planes_route(C, hw):
    from estdepth_amd import ops
    x = _rand((2,) + hw + (C,), C + hw[0] * hw[1])
    what = "nhwc_to_planes C%d %dx%d" % ((C,) + hw)

    def raw(i, og):
        return _lib().estd_nhwc_to_planes(_p(i["x"]), C, _p(og), 2, hw[0] * hw[1], _stream())
    out = run_route(what, tile_instance("nhwc_to_planes_kernel", C), dict(x=x), lambda i: ops.nhwc_to_planes(i["x"]), raw, (2, C) + hw)
    ref, A = R.nhwc_to_planes_ref(x)
    R.compare(out, ref, A, R.C_ROUTE["nhwc_to_planes"], None, what)


@pytest.mark.parametrize("N,H,W", [(2, 2, 2), (2, 6, 10), (3, 240, 320)], ids=lambda v: str(v))
@pytest.mark.parametrize("Cx,Cs", [(4, 4), (4, 12), (12, 4), (12, 12)])
def test_upsample2_cat_route(Cx, Cs, N, H, W):
    from estdepth_amd import ops
    x, skip = _rand((N, H // 2, W // 2, Cx), Cx + H), _rand((N, H, W, Cs), Cs + W)
    what = "upsample2_cat %d+%d %dx%dx%d" % (Cx, Cs, N, H, W)

    def raw(i, og):
        return _lib().estd_upsample2_cat_nhwc(_p(i["x"]), Cx, _p(i["skip"]), Cs, _p(og), N, H, W, _stream())
    out = run_route(what, "upsample2_cat_nhwc_kernel", dict(x=x, skip=skip), lambda i: ops.upsample2_cat_nhwc(i["x"], i["skip"]), raw,
                    (N, H, W, Cx + Cs))
    ref, A = R.upsample2_cat_ref(x, skip)
    R.compare(out, ref, A, R.C_ROUTE["upsample2_cat"], None, what)


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (1, 15, 17), (1, 16, 16), (1, 1, 257), (2, 7, 9)], ids=lambda v: str(v))
def test_normalise_route(N, H, W):
    """N * HW = 1, 255, 256, 257 and 2 * 63: bit-identical to the model's three fp32 CPU ops"""
    from estdepth_amd import ops
    g = torch.Generator(device=DEV).manual_seed(H * W)
    imgs = torch.rand(N, 3, H, W, device=DEV, generator=g) * 255.0
    what = "normalise %dx%dx%d" % (N, H, W)

    def raw(i, og):
        return _lib().estd_normalise_nhwc(_p(i["imgs"]), _p(og), N, H * W, _stream())
    out = run_route(what, "normalise_nhwc_kernel", dict(imgs=imgs), lambda i: ops.normalise_nhwc(i["imgs"]), raw, (N, H, W, 3))
    ref, A = R.normalise_ref(imgs)
    R.compare(out, ref, A, R.C_ROUTE["normalise"], None, what)


# ---------------------------------------------------------------------------------------------------------------- refused shapes
def _refused(call, match=None, after=None):
    """the call (or every call of a list, under one trace) raises and launches none of the kernels of the 2D suites; ``after(i, message)``
    looks at the i-th refusal before the next call -> the messages"""
    calls = call if isinstance(call, list) else [call]
    messages = []
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for i, c in enumerate(calls):
            with pytest.raises(RuntimeError, match=match) as e:
                c()
            messages.append(str(e.value))
            if after is not None:
                after(i, messages[-1])
        torch.cuda.synchronize()
    ran = [e.key for e in prof.key_averages() if KERNEL_RE.search(e.key) or CONV_KERNEL_RE.search(e.key)]
    assert not ran, ran
    return messages


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_497_channels_are_unsupported(binding):
    """[497][33] floats do not fit the 64 KiB tile: ESTD_ERR_UNSUPPORTED (-3) from both transposes, nothing launched"""
    from estdepth_amd import ops
    a, b, x = torch.zeros(1, 249, 2, 2, device=DEV), torch.zeros(1, 248, 2, 2, device=DEV), torch.zeros(1, 2, 2, 497, device=DEV)
    with _Switches(None, binding):
        _refused(lambda: ops.planes_cat_nhwc(a, b, False), r"estd_status -3\)|unsupported configuration")
        _refused(lambda: ops.nhwc_to_planes(x), r"estd_status -3\)|unsupported configuration")
    assert _lib().estd_planes_cat_nhwc(_p(a), 249, _p(b), 248, 0, _p(x), 1, 4, _stream()) == -3
    assert _lib().estd_nhwc_to_planes(_p(x), 497, _p(x), 1, 4, _stream()) == -3


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("H,W", [(5, 6), (6, 5)])
def test_upsample2_cat_refuses_an_odd_map(binding, H, W):
    from estdepth_amd import ops
    x, skip = torch.zeros(1, H // 2, W // 2, 4, device=DEV), torch.zeros(1, H, W, 4, device=DEV)
    with _Switches(None, binding):
        _refused(lambda: ops.upsample2_cat_nhwc(x, skip))
    out = torch.zeros(1, H, W, 8, device=DEV)
    assert _lib().estd_upsample2_cat_nhwc(_p(x), 4, _p(skip), 4, _p(out), 1, H, W, _stream()) == -1


# ------------------------------------------------------------------------------------------------------------ malformed arguments
def _arg_table():
    """The 2D operators in the form of test_gpu_sweep_fusion_routes._arg_table: (the operator's name in messages, call(**args), valid() ->
    its arguments by name, the argument it writes or None, [(label, the argument replaced, its malformed value[, the name the message
    gives it])]).  Maps of a few pixels, no two sizes of a tensor equal; weights are random floats of the packed size (the checks and the
    parity of the bindings do not depend on their values)."""
    from estdepth_amd import ops
    r = lambda *s: _rand(s, 11 + sum(s))                                        # noqa: E731
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)              # noqa: E731
    f64 = lambda t: t.double()                                                  # noqa: E731
    x16, x32, img, pool = r(1, 3, 5, 16), r(1, 3, 5, 32), r(1, 5, 7, 3), r(1, 4, 6, 4)
    s16, s32, s64 = r(16), r(32), r(64)
    br = lambda n: [r(1, 1, 2, 4) + k for k in range(n)]                        # noqa: E731
    spp = lambda n: (lambda: dict(raw=pool, skip=r(1, 4, 6, 8), branches=br(n)))  # noqa: E731
    w_taps, w_small, w_to16, w_stem7 = r(9, 32, 16), r(512), r(9 * 256), r(7 * 6 * 4 * 64)
    return [
        ("bn_act_nhwc_", ops.bn_act_nhwc_, lambda: dict(x=cl(r(1, 8, 3, 5)), scale=r(8), shift=r(8), relu=True, residual=cl(r(1, 8, 3, 5) + 1)), "x", [
            ("a 7-float scale", "scale", _short(r(8), 7)), ("a 7-float shift", "shift", _short(r(8), 7)), ("float64 scale", "scale", f64(r(8))), ("x [C,H,W]", "x", _sent(8, 3, 5)), ("x in NCHW memory", "x", _sent(1, 8, 3, 5)),
            ("residual [N,C,W,H]", "residual", cl(r(1, 8, 5, 3))), ("residual in NCHW memory", "residual", r(1, 8, 3, 5)),
            ("float64 residual", "residual", cl(f64(r(1, 8, 3, 5)))), ("a list for scale", "scale", [1.0] * 8)]),
        ("bn_act_nhwc_", ops.bn_act_nhwc_, lambda: dict(x=cl(r(1, 8, 3, 5)), scale=r(8), shift=r(8), relu=False, residual=None), "x", []),
        ("spp_upsample_cat", ops.spp_upsample_cat, spp(2), None, [
            ("no branch", "branches", []), ("five branches", "branches", br(5)), ("skip [N,W,H,C]", "skip", r(1, 6, 4, 8)),
            ("skip of two images", "skip", r(2, 4, 6, 8)), ("skip [H,W,C]", "skip", r(4, 6, 8)), ("raw [H,W,C]", "raw", r(4, 6, 4)),
            ("a branch of two images", "branches", [r(1, 1, 2, 4), r(2, 1, 2, 4)]), ("a branch of 8 channels", "branches", [r(1, 1, 2, 4), r(1, 1, 2, 8)]),
            ("a branch [H,W,C]", "branches", [r(1, 2, 4), r(1, 1, 2, 4)]), ("a float64 branch", "branches", [r(1, 1, 2, 4), f64(r(1, 1, 2, 4))])]),
        ("spp_upsample_cat", ops.spp_upsample_cat, spp(1), None, []),
        ("spp_upsample_cat", ops.spp_upsample_cat, spp(3), None, []),
        ("spp_upsample_cat", ops.spp_upsample_cat, spp(4), None, []),
        ("conv1x1_nhwc", ops.conv1x1_nhwc, lambda: dict(x=x16, w2=r(32, 16), scale=s32, shift=s32 + 1, stride=1, relu=True, residual=r(1, 3, 5, 32)), None, [
            ("w [cin,cout]", "w2", r(16, 32), "w"), ("a 31-float scale", "scale", _short(s32, 31)), ("a 31-float shift", "shift", _short(s32, 31)),
            ("stride 0", "stride", 0), ("stride 3", "stride", 3), ("residual [N,W,H,C]", "residual", r(1, 5, 3, 32)), ("x [H,W,C]", "x", r(3, 5, 16)),
            ("float64 w", "w2", f64(r(32, 16)), "w")]),
        ("conv1x1_nhwc", ops.conv1x1_nhwc, lambda: dict(x=x16, w2=r(32, 16), scale=None, shift=None, stride=2), None, []),
        ("conv2d_taps_nhwc", ops.conv2d_taps_nhwc, lambda: dict(x=x16, w_taps=w_taps, scale=s32, shift=s32 + 1, ksize=3, stride=1, pad=1, relu=True,
                                                              residual=r(1, 3, 5, 32)), None, [
            ("x [H,W,C]", "x", r(3, 5, 16)), ("w of 8 taps", "w_taps", _short(w_taps, 8 * 32 * 16).view(8, 32, 16), "w"),
            ("w [taps,cin,cout]", "w_taps", r(9, 16, 32), "w"), ("a 31-float scale", "scale", _short(s32, 31)),
            ("a 31-float shift", "shift", _short(s32, 31)), ("stride 0", "stride", 0), ("residual [N,W,H,C]", "residual", r(1, 5, 3, 32))]),
        ("conv2d_small_nhwc", ops.conv2d_small_nhwc, lambda: dict(x=x32, w_packed=w_small, scale=s16, shift=s16 + 1, cout=16, ksize=1, stride=1, relu=True),
         None, [
            ("w one float short", "w_packed", _short(w_small, 511)), ("a 15-float scale", "scale", _short(s16, 15)),
            ("a 15-float shift", "shift", _short(s16, 15)), ("x [H,W,C]", "x", r(3, 5, 32)), ("ksize 2", "ksize", 2), ("float64 x", "x", f64(x32))]),
        ("conv2d_k3_to16_nhwc", ops.conv2d_k3_to16_nhwc, lambda: dict(x=x16, w_packed=w_to16, scale=s16, shift=s16 + 1, upsample=False), None, [
            ("w one float short", "w_packed", _short(w_to16, 9 * 256 - 1)), ("a 15-float scale", "scale", _short(s16, 15)),
            ("a 15-float shift", "shift", _short(s16, 15)), ("x of 8 channels", "x", r(1, 3, 5, 8)), ("x [H,W,C]", "x", r(3, 5, 16))]),
        ("conv2d_k3_to16_nhwc", ops.conv2d_k3_to16_nhwc, lambda: dict(x=r(1, 2, 3, 16), w_packed=w_to16, scale=s16, shift=s16 + 1, upsample=True), None, []),
        ("stem7x7s2_nhwc", ops.stem7x7s2_nhwc, lambda: dict(x=img, w_packed=w_stem7, scale=s64, shift=s64 + 1), None, [
            ("x [N,3,H,W]", "x", r(1, 3, 5, 7)), ("x of 4 channels", "x", r(1, 5, 7, 4)), ("w one float short", "w_packed", _short(w_stem7, 10751)),
            ("a 63-float scale", "scale", _short(s64, 63)), ("a 63-float shift", "shift", _short(s64, 63))]),
        ("stem3x3s2_nhwc", ops.stem3x3s2_nhwc, lambda: dict(x=img, weight=r(32, 3, 3, 3), scale=s32, shift=s32 + 1), None, [
            ("x of 4 channels", "x", r(1, 5, 7, 4)), ("weight [3,3,3,32]", "weight", r(3, 3, 3, 32)), ("a 31-float scale", "scale", _short(s32, 31)),
            ("a 31-float shift", "shift", _short(s32, 31))]),
        ("maxpool3x3s2_nhwc", ops.maxpool3x3s2_nhwc, lambda: dict(x=pool), None, [
            ("x [H,W,C]", "x", r(4, 6, 4)), ("float64 x", "x", f64(pool)), ("a list", "x", [[[[1.0] * 4]]])]),
        ("avgpool_nhwc", ops.avgpool_nhwc, lambda: dict(x=pool, k=2), None, [
            ("k = 0", "k", 0), ("k = 5 on a 4 x 6 map", "k", 5), ("x [H,W,C]", "x", r(4, 6, 4))]),
        ("normalise_nhwc", ops.normalise_nhwc, lambda: dict(imgs=r(1, 3, 5, 7)), None, [
            ("imgs [N,H,W,3]", "imgs", img), ("imgs [3,H,W]", "imgs", r(3, 5, 7)), ("float64 imgs", "imgs", f64(r(1, 3, 5, 7)))]),
        ("nhwc_to_planes", ops.nhwc_to_planes, lambda: dict(x=pool), None, [("x [H,W,C]", "x", r(4, 6, 4)), ("float64 x", "x", f64(pool))]),
        ("planes_cat_nhwc", ops.planes_cat_nhwc, lambda: dict(a=r(1, 2, 3, 5), b=r(1, 4, 3, 5), relu_b=True), None, [
            ("b [N,C,W,H]", "b", r(1, 4, 5, 3)), ("b of two stacks", "b", r(2, 4, 3, 5)), ("a [C,H,W]", "a", r(2, 3, 5)),
            ("b [C,H,W]", "b", r(4, 3, 5)), ("float64 b", "b", f64(r(1, 4, 3, 5)))]),
        ("upsample2_cat_nhwc", ops.upsample2_cat_nhwc, lambda: dict(x=r(1, 2, 3, 4), skip=r(1, 4, 6, 8)), None, [
            ("skip [N,W,H,C]", "skip", r(1, 6, 4, 8)), ("skip of two images", "skip", r(2, 4, 6, 8)), ("skip of 5 rows", "skip", r(1, 5, 6, 8)),
            ("x [H,W,C]", "x", r(2, 3, 4)), ("skip [H,W,C]", "skip", r(4, 6, 8))]),
        ("disp_head_nhwc", ops.disp_head_nhwc, lambda: dict(x=x16, weight=r(1, 16, 3, 3), bias=r(1), depth_max=10.0, upscale=1), None, [
            ("weight [C,1,3,3]", "weight", r(16, 1, 3, 3)), ("weight for 32 channels", "weight", r(1, 32, 3, 3)), ("a 2-float bias", "bias", r(2)),
            ("x [H,W,C]", "x", r(3, 5, 16))]),
    ]


def test_the_valid_call_of_every_2d_operator_runs_alike_under_both_bindings():
    """the rule set refuses nothing it should accept: bit-identical outputs"""
    for op, fn, valid, _, _ in _arg_table():
        outs = []
        for binding in ("torch", "ctypes"):
            with _Switches(None, binding):
                outs.append(_as_tuple(fn(**valid())))
        torch.cuda.synchronize()
        assert len(outs[0]) == len(outs[1]) and all(_bits_equal(a, b) for a, b in zip(*outs)), op


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_2d_arguments_raise_before_any_launch(binding):
    """every malformed call of the table is a RuntimeError under both bindings with the operator's and the argument's name in the message,
    launches no kernel of the 2D suites and leaves the tensor bn_act_nhwc_ writes untouched"""
    cases = _malformed(_arg_table(), fill_dest=True)
    assert len(cases) >= 75 and len({c[0] for c in cases}) == len(cases)

    def after(i, message):
        label, op, arg, _, dest = cases[i]
        assert op in message and arg in message, "%s / %s: the message names neither %s nor %s: %s" % (binding, label, op, arg, message)
        if dest is not None and dest.is_cuda:
            assert bool((dest.view(torch.int32) == SENT32).all()), "%s / %s wrote into its destination" % (binding, label)
    with _Switches(None, binding):
        _refused([c[3] for c in cases], after=after)


def test_sentinel_is_a_nan_no_kernel_computes():
    assert math.isnan(torch.tensor([SENT32], dtype=torch.int32).view(torch.float32).item())
