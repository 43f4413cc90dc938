"""Every dispatch route of ops.Conv3dPlan.run (the 3x3x3 convolution) against the fp64 reference of tests/conv3d_ref.py.

One case per (route, plan, activation, epilogue, strides, switches).  Each case
  * asserts WHICH kernels ran (torch.profiler kernel names): a silent fallback to another route is a failure, and the deliberate
    fallback cases assert the route they fall back to;
  * compares every output (out_main, out_extra, out_head, the finalised GroupNorm statistics) element by element with the reference:
    |gpu - ref| <= C_ROUTE[route] * 2^-24 * A (A: the same pipeline on absolute values), next to the max-relative bar 3e-6 max |ref|;
  * carves every output out of a larger buffer filled with a NaN sentinel and requires everything the contract does not write -- channels
    out_channels .. out_stride - 1, the voxels before and after the volume, stats_partials past conv3d_grid(...) * 4 -- to still be the
    sentinel, bit for bit;
  * runs small shapes at the tile edges of the kernels (8 x 16 tiles of the direct / Winograd kernels, 16 x 16 of the channel-32 pass and
    the stereo-head kernel, its 32-plane depth segments, the Winograd depth pairs), a full-size volume per route family and one batch whose
    total size crosses 2^31 bytes (64-bit batch offsets; the reference then at sampled voxels only);
  * runs every small-shape case again where each workgroup of the persistent grid walks a range of several tiles (thin columns, a large batch,
    two grid sizes: test_conv3d_route_over_multi_tile_ranges).
Both bindings launch from one wiring (ops.CONV3D_ROUTES): one small-shape case of every route, and the reset-gate cases, run under both and
must agree bit for bit."""
import re

import numpy as np
import pytest
import torch

import conv3d_ref as R
import tile_ranges_ref as TR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# per-element bound constants, in units of 2^-24 A: the worst ratio measured on an MI355X over every case and output of the route
# (in the comments), times at least 3.  The Winograd routes sit BELOW the direct kernel: their transforms shorten the fp32 sums.
# The many-tile cases added later (test_conv3d_route_over_multi_tile_ranges) are held to the same constants; their sums have the same 27 x cin
# terms, their worst ratios (in brackets, over 2 x 90 k voxels per case instead of a few thousand) are the tail of the same distribution.
C_ROUTE = {
    "direct": 18.0,           # measured 5.79 (33 -> 33, out_main) [6.43: 33 -> 32]
    "wino3": 7.0,             # measured 2.25 (32 -> 32, out_main) [2.29: 33 -> 32]
    "wino2": 8.0,             # measured 2.47 (32 -> 32 + statistics, out_main) [2.55]
    "wino2_xout": 7.0,        # measured 2.16 (out_main; channel 32: 0.70) [3.15; channel 32: 0.91]
    "wino2_o16": 5.0,         # measured 1.63 (with statistics, out_main) [1.83]
    "wino2_c16": 2.0,         # measured 0.63 (head) [0.71]
    "wino3+xout": 7.0,        # measured 2.26 (out_main; channel 32: 0.93) [2.33]
}
KERNELS = {
    "direct": {"conv3d_k3_kernel"},
    "wino3": {"conv3d_wino3_kernel"},
    "wino2": {"conv3d_wino2_kernel"},
    "wino2_xout": {"conv3d_wino2_kernel"},
    "wino2_o16": {"conv3d_wino2_kernel"},
    "wino2_c16": {"conv3d_wino2_c16_kernel"},
    "wino3+xout": {"conv3d_wino3_kernel", "conv3d_xout_kernel"},
}
SWITCHES = ("CONV3D_ALGO", "W3", "W3_EXTRA", "W3_XOUT", "W2_XOUT", "W2X", "BINDING")
DEFAULT = dict(CONV3D_ALGO="wino2", W3=True, W3_EXTRA=True, W3_XOUT=True, W2_XOUT=True, W2X=False)
DIRECT = dict(CONV3D_ALGO="direct")
W2 = dict(W3=False)
W2XOUT = dict(W3_XOUT=False)

# D: 1, 2, 31, 33, 65 (depth pairs of the Winograd kernels, 32-plane segments of the channel-32 pass); H, W just below / at / above 8 and 16
SMALL = [(1, 1, 7, 15), (2, 2, 9, 17), (1, 31, 8, 16), (1, 33, 17, 15), (1, 65, 7, 17), (3, 2, 15, 33)]
FULL = [(1, 64, 120, 160)]                 # a cfg2 volume
BIG = [(14, 64, 120, 160)]                 # 14 x 157 MB of 32-channel records: 2.2 GB per tensor, each volume under the 2^31-byte limit


def C(cid, route, plan, acts=("relu",), epi=(), ins=None, outs=None, sw=None, shapes=SMALL, both=False):
    return pytest.param(dict(route=route, plan=plan, acts=acts, epi=set(epi), ins=ins, outs=outs, sw=dict(DEFAULT, **(sw or {})),
                             shapes=shapes, both=both), id=cid)


CASES = [
    # ---- the direct kernel (ESTD_CONV3D_ALGO=direct): every instance, every epilogue
    C("direct-32-split20-res-res2-scale-acc", "direct", "32>32", ("tanh", "relu", 20), ("res", "res2", "scale", "acc"), 36, 40, DIRECT, both=True),
    C("direct-32-none-stats-res", "direct", "32>32", ("none",), ("stats", "res"), 32, 32, DIRECT),
    C("direct-33to32-split8", "direct", "33>32", ("relu", "tanh", 8), (), 64, 36, DIRECT),
    C("direct-33to33-split33", "direct", "33>33", ("relu", "none", 33), (), 36, 32, DIRECT),
    C("direct-33to33-split32-tanh", "direct", "33>33", ("none", "tanh", 32), (), 32, 40, DIRECT),
    C("direct-32to16-split8-stats", "direct", "32>16", ("none", "tanh", 8), ("stats",), 32, 32, DIRECT),
    C("direct-16to16-relu-res-acc", "direct", "16>16", ("relu",), ("res", "acc", "scale"), 32, 24, DIRECT),
    C("direct-16to16-head-and-main", "direct", "16>16h", ("relu", "none", 8), ("head", "main"), 16, 16, DIRECT),
    # ---- three-axis Winograd (the default 32 -> 32 and 33 -> 32 launches)
    C("wino3-32-relu", "wino3", "32>32", ("relu",), both=True),
    C("wino3-32-tanh-res-res2-scale", "wino3", "32>32", ("tanh",), ("res", "res2", "scale"), 32, 36),
    C("wino3-32-split16-acc-scale", "wino3", "32>32", ("tanh", "relu", 16), ("acc", "scale"), 36, 64),
    C("wino3-32-split8-res", "wino3", "32>32", ("relu", "tanh", 8), ("res",), 64, 32),
    C("wino3-32-split20-acc", "wino3", "32>32", ("tanh", "none", 20), ("acc",), 32, 40),
    C("wino3-32-none-stats", "wino3", "32>32", ("none",), ("stats",), 32, 36),
    C("wino3-33to32-relu", "wino3", "33>32", ("relu",), (), 36, 40),
    C("wino3-33to32-split16", "wino3", "33>32", ("tanh", "relu", 16), ()),
    # ---- two-axis Winograd (ESTD_W3=0)
    C("wino2-32-split20-res-res2-scale-acc", "wino2", "32>32", ("tanh", "relu", 20), ("res", "res2", "scale", "acc"), 64, 36, W2, both=True),
    C("wino2-32-none-stats", "wino2", "32>32", ("none",), ("stats",), 36, 32, W2),
    C("wino2-33to32-tanh", "wino2", "33>32", ("tanh",), (), 36, 40, W2),
    C("wino2-33to32-relu-res-acc", "wino2", "33>32", ("relu",), ("res", "acc"), 32, 32, W2),
    # ---- the two-axis kernel's 33 -> 33 instance (ESTD_W3_XOUT=0)
    C("wino2xout-33-relu", "wino2_xout", "33>33", ("relu",), (), 36, 40, W2XOUT, both=True),
    C("wino2xout-33-split32", "wino2_xout", "33>33", ("tanh", "relu", 32), (), 32, 32, W2XOUT),
    C("wino2xout-33-split33", "wino2_xout", "33>33", ("tanh", "none", 33), (), 64, 32, W2XOUT),
    # ---- dres2 in two launches (the default 33 -> 33 route): 33 -> 32 three-axis + the channel-32 pass
    C("split33-relu", "wino3+xout", "33>33", ("relu",), (), 36, 40, both=True),
    C("split33-split32", "wino3+xout", "33>33", ("none", "relu", 32), (), 32, 32, both=True),
    C("split33-split33", "wino3+xout", "33>33", ("relu", "none", 33), (), 32, 36),
    C("split33-none", "wino3+xout", "33>33", ("none",), (), 64, 32),
    # ---- the 32 -> 16 instance (the ConvGRU output convolution), with and without the folded reset gate
    C("o16-none-stats", "wino2_o16", "32>16", ("none",), ("stats",), 32, 16),
    C("o16-split8-res-res2-scale-acc", "wino2_o16", "32>16", ("relu", "tanh", 8), ("res", "res2", "scale", "acc"), 36, 32),
    C("o16-gate-stats", "wino2_o16", "32>16", ("none",), ("gate", "stats"), 32, 24, both=True),
    C("o16-gate-relu", "wino2_o16", "32>16", ("relu",), ("gate",), 32, 16, both=True),
    # ---- the stereo heads: 16 -> 16 + 1x1x1 head, only the logit volume
    C("c16-relu", "wino2_c16", "16>16h", ("relu",), ("head",), 32, both=True),
    C("c16-split8", "wino2_c16", "16>16h", ("relu", "none", 8), ("head",), 16),
    # ---- deliberate fallbacks under the default switches
    C("fallback-33to33-residual-to-direct", "direct", "33>33", ("relu",), ("res",), 32, 32),
    C("fallback-33to32-stats-to-direct", "direct", "33>32", ("none",), ("stats",), 32, 32),
    C("fallback-tanh-dres2-to-wino2xout", "wino2_xout", "33>33", ("tanh",), (), 36, 32),
    C("fallback-head-tanh-to-direct", "direct", "16>16h", ("tanh",), ("head",), 32),
    # ---- one full-size volume per route family (reference at sampled voxels)
    C("full-direct", "direct", "32>32", ("tanh", "relu", 16), ("res", "acc"), 32, 32, DIRECT, shapes=FULL),
    C("full-wino3", "wino3", "32>32", ("relu",), ("res", "res2", "scale"), 32, 32, shapes=FULL),
    C("full-wino3-33to32", "wino3", "33>32", ("relu",), (), 32, 32, shapes=FULL),
    C("full-wino2", "wino2", "32>32", ("tanh",), ("acc",), 32, 32, W2, shapes=FULL),
    C("full-wino2xout", "wino2_xout", "33>33", ("relu",), (), 32, 32, W2XOUT, shapes=FULL),
    C("full-split33", "wino3+xout", "33>33", ("relu",), (), 32, 32, shapes=FULL),
    C("full-o16-gate", "wino2_o16", "32>16", ("none",), ("gate",), 32, 16, shapes=FULL),
    C("full-c16", "wino2_c16", "16>16h", ("relu",), ("head",), 32, shapes=FULL),
    # ---- batches of more than 2^31 bytes (64-bit batch offsets)
    C("big-batch-wino3", "wino3", "32>32", ("relu",), (), 32, 32, shapes=BIG),
    C("big-batch-split33", "wino3+xout", "33>33", ("relu",), (), 32, 32, shapes=BIG),
]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


SENT32 = 0x7FC0DEAD                    # a quiet-NaN payload no kernel computes
SENT64 = 0x7FF8DEADBEEF0123


def _guarded(n_rec, stride, dtype=torch.float32, fill=None):
    """a view of n_rec records of `stride` elements inside a buffer filled with the sentinel: 4 records before (16-byte alignment kept),
    5 after.  Returns (buffer, view, (lo, hi) element range of the view)."""
    lo, hi = 4 * stride, (4 + n_rec) * stride
    it = torch.int32 if dtype == torch.float32 else torch.int64
    buf = torch.full((hi + 5 * stride,), SENT32 if dtype == torch.float32 else SENT64, dtype=it, device=DEV).view(dtype)
    view = buf[lo:hi]
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return buf, view, (lo, hi)


def _untouched(buf, lo, hi, stride=1, keep_from=None):
    """the elements outside [lo, hi) and channels keep_from.. of the records inside are still the sentinel (count of changed elements)"""
    b = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int64)
    s = SENT32 if buf.dtype == torch.float32 else SENT64
    bad = int((b[:lo] != s).sum()) + int((b[hi:] != s).sum())
    if keep_from is not None and keep_from < stride:
        bad += int((b[lo:hi].view(-1, stride)[:, keep_from:] != s).sum())
    return bad


def _plan_args(plan, acts, seed):
    g = torch.Generator().manual_seed(seed)
    n_in, n_out = {"32>32": (32, 32), "33>32": (33, 32), "33>33": (33, 33), "32>16": (32, 16), "16>16h": (16, 16), "16>16": (16, 16)}[plan]
    w = torch.randn(n_out, n_in, 3, 3, 3, generator=g) / np.sqrt(27.0 * n_in)
    a = dict(weight=w, scale=torch.rand(n_out, generator=g) + 0.5, shift=torch.randn(n_out, generator=g) * 0.3, act_a=acts[0])
    if len(acts) > 1:
        a.update(act_b=acts[1], act_split=acts[2])
    if plan == "33>33":
        a.update(main_idx=list(range(1, 33)), extra_idx=0, out_idx=list(range(33)), n_tiles=3)
    else:
        a.update(main_idx=list(range(32 if n_in >= 32 else 16)), extra_idx=32 if n_in == 33 else None, out_idx=list(range(n_out)),
                 n_tiles=n_out // 16)
    if plan == "16>16h":
        a.update(head_w=torch.randn(16, generator=g) * 0.3, head_b=torch.randn(1, generator=g))
    return a


def _sample_points(dims, g):
    """2000 random voxels + every voxel of the last batch element's W = W-1 face + its eight corners"""
    N, D, H, W = dims
    rnd = torch.stack([torch.randint(0, s, (2000,), generator=g) for s in dims], 1)
    dd, hh = torch.meshgrid(torch.arange(D), torch.arange(H), indexing="ij")
    face = torch.stack([torch.full_like(dd, N - 1), dd, hh, torch.full_like(dd, W - 1)], -1).reshape(-1, 4)
    corners = torch.tensor([[N - 1, d, h, w] for d in (0, D - 1) for h in (0, H - 1) for w in (0, W - 1)])
    return torch.cat([rnd, face, corners])


class _Switches:
    def __init__(self, sw):
        self.sw = sw

    def __enter__(self):
        from estdepth_amd import ops
        self.old = {k: getattr(ops, k) for k in SWITCHES}
        for k, v in self.sw.items():
            setattr(ops, k, v)

    def __exit__(self, *exc):
        from estdepth_amd import ops
        for k, v in self.old.items():
            setattr(ops, k, v)
        return False


def _launch(case, plan, dims, binding, seed):
    """one run of the case: inputs, guarded outputs, the launch under the case's switches and the profiler -> (kernels, results)"""
    from estdepth_amd import ops
    N, D, H, W = dims
    nvox = N * D * H * W
    n_tiles, epi = plan.n_tiles, case["epi"]
    ins = case["ins"] or plan.cin_main
    oc = 16 * min(n_tiles, 2)
    outs = case["outs"] or oc
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)                   # noqa: E731
    x = rnd(N, D, H, W, ins)
    kw = dict(in_stride=ins)
    if plan.has_extra:
        kw["in_extra"] = rnd(N, D, H, W)
    bufs = {}
    if plan.head_w is None or "main" in epi:
        prior = rnd(nvox, outs) if "acc" in epi else None
        if prior is not None:
            prior[:, oc:] = float("nan")
        buf, view, rng = _guarded(nvox, outs, fill=prior)
        if prior is not None:                                                    # (channels past out_channels: the sentinel again)
            buf.view(torch.int32)[rng[0]:rng[1]].view(-1, outs)[:, oc:] = SENT32
        bufs["out"] = (buf, rng, outs, oc)
        kw.update(out=view.view(N, D, H, W, outs), out_stride=outs, out_channels=oc)
    if "res" in epi:
        kw["residual"] = rnd(N, D, H, W, outs)
    if "res2" in epi:
        kw["residual2"] = rnd(N, D, H, W, outs)
    if "scale" in epi:
        kw["out_scale"] = 0.37
    if "acc" in epi:
        kw["accumulate"] = True
    if n_tiles == 3:
        buf, view, rng = _guarded(nvox, 1)
        bufs["extra"] = (buf, rng, 1, 1)
        kw["out_extra"] = view.view(N, D, H, W)
    if "head" in epi:
        buf, view, rng = _guarded(nvox, 1)
        bufs["head"] = (buf, rng, 1, 1)
        kw["out_head"] = view.view(N, D, H, W)
    if "stats" in epi:
        nblk = ops.conv3d_grid(N, D, H, W)
        buf, view, rng = _guarded(nblk * 4, 1, dtype=torch.float64)
        bufs["stats"] = (buf, rng, 1, 1)
        kw["stats_partials"] = view
    if "gate" in epi:
        kw["gate"] = (rnd(N, D, H, W, 32), torch.tensor([0.12, 1.3, 0.0, 0.0], device=DEV), torch.rand(16, device=DEV, generator=g) + 0.5,
                      rnd(16) * 0.2)
    before = kw["out"].clone() if "out" in kw else None
    with _Switches(dict(case["sw"], BINDING=binding)):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            plan.run(x, dims, **kw)
            torch.cuda.synchronize()
    kernels = set()
    for e in prof.key_averages():
        m = re.search(r"(conv3d_\w*?_kernel)", e.key)
        if m:
            kernels.add(m.group(1))
    return kernels, x, kw, before, bufs


def _finalize(bufs, dims):
    from estdepth_amd import ops
    buf, (lo, hi), _, _ = bufs["stats"]
    N, D, H, W = dims
    return ops.groupnorm_finalize(buf[lo:hi], (hi - lo) // 4, 16.0 * N * D * H * W)


def _reference(pa, dims, x, kw, before):
    """the fp64 reference of one launch -> (conv3d_ref's dict, the sampled voxels or None)"""
    points = None
    if dims in FULL or dims in BIG:
        points = _sample_points(dims, torch.Generator().manual_seed(sum(dims)))
    ref_kw = dict(kw)
    if before is not None:
        ref_kw["out"] = before
    return R.conv3d_ref(**pa, x=x, dims=dims, points=points, **ref_kw), points


def _compare(case, pa, dims, x, kw, before, bufs, worst, what):
    _check(case, dims, _reference(pa, dims, x, kw, before), bufs, worst, what)


def _check(case, dims, reference, bufs, worst, what):
    route = case["route"]
    c = C_ROUTE[route]
    N, D, H, W = dims
    ref, points = reference
    at = (lambda t: R._at(t, points)) if points is not None else (lambda t: t)     # noqa: E731
    for key in ("out", "extra", "head"):
        if key not in bufs:
            continue
        buf, (lo, hi), stride, keep = bufs[key]
        assert key in ref, key
        got = buf[lo:hi].view(N, D, H, W, stride) if key == "out" else buf[lo:hi].view(N, D, H, W)
        got, r, a = at(got), ref[key], ref[key + "_A"]
        if key == "out":
            got, r, a = got[..., :keep], r[..., :keep], a[..., :keep]
        worst[key] = max(worst.get(key, 0.0), R.check_bound(got, r, a, c, "%s %s %s" % (what, key, dims)))
        assert _untouched(buf, lo, hi, stride, keep if key == "out" else None) == 0, "%s: %s written outside its region" % (what, key)
    if "stats" in bufs:
        buf, (lo, hi), _, _ = bufs["stats"]
        assert _untouched(buf, lo, hi) == 0, "%s: stats_partials written past conv3d_grid * 4" % what
        groups = 2 if case["plan"] in ("32>32", "33>32") else 1
        got = _finalize(bufs, dims).double().cpu()[: 2 * groups]
        r, a = ref["stats"][: 2 * groups], ref["stats_A"][: 2 * groups]
        ratio = R.bound_ratio(got, r, a)
        assert ratio <= c, "%s: GroupNorm statistics %s vs %s (%.1f x 2^-24 A)" % (what, got.tolist(), r.tolist(), ratio)
        assert float((got - r).abs().max()) < 1e-5 * max(1.0, float(r.abs().max()))
        worst["stats"] = max(worst.get("stats", 0.0), ratio)


@pytest.mark.parametrize("case", CASES)
def test_conv3d_route_against_fp64(case):
    from estdepth_amd import ops
    seed = sum(map(ord, case["route"] + case["plan"]))
    pa = _plan_args(case["plan"], case["acts"], seed)
    plan = ops.Conv3dPlan(device=DEV, **pa)
    worst = {}
    for dims in case["shapes"]:
        got = {}
        for binding in ("torch", "ctypes") if case["both"] else ("torch",):
            kernels, x, kw, before, bufs = _launch(case, plan, dims, binding, seed + sum(dims))
            what = "%s/%s" % (case["route"], binding)
            _compare(case, pa, dims, x, kw, before, bufs, worst, what)          # (first: a wrong result names the output it is wrong in)
            assert kernels == KERNELS[case["route"]], "%s %s: ran %s" % (what, dims, sorted(kernels))
            got[binding] = {k: v[0].clone() for k, v in bufs.items()}
            del x, kw, before, bufs
        if case["both"]:
            for k in got["torch"]:
                assert torch.equal(got["torch"][k].view(torch.int8), got["ctypes"][k].view(torch.int8)), "bindings differ on %s" % k
        del got
        torch.cuda.empty_cache()
    print("ROUTE-RATIO %s %s %s" % (case["route"], case["plan"], " ".join("%s=%.2f" % kv for kv in sorted(worst.items()))))


def _written_blocks(bufs):
    """the 4-double GroupNorm partial blocks a launch wrote completely (the rest keeps the sentinel)"""
    buf, (lo, hi), _, _ = bufs["stats"]
    return int((buf[lo:hi].view(torch.int64).view(-1, 4) != SENT64).all(1).sum())


@pytest.mark.parametrize("case", [p for p in CASES if p.values[0]["shapes"] is SMALL])
def test_conv3d_route_over_multi_tile_ranges(case, request):
    """Every tile-edge case once more on the many-tile shapes of tests/tile_ranges_ref.py (thin columns, a large batch: ranges of 4-12 tiles
    per workgroup with middle tiles, whole columns inside a range, ranges across batch elements and starts on the odd last depth pair),
    under the full grid and under set_reserved_cus(128): every element of every output against one fp64 reference per shape, the same
    bound, sentinel bands and kernel names, and the outputs of the two grids (and of both bindings, where the case runs both) bit-identical.
    The GroupNorm partials are indexed by the canonical 8 x 16 tile (n, d, h-tile, w-tile), not by workgroup: each grid writes exactly
    ops.conv3d_grid(...) blocks -- the direct kernel's tile count, which the model reproduces -- and the same bits."""
    from estdepth_amd import ops
    family = TR.ROUTE_FAMILY[case["route"]]
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    seed = sum(map(ord, case["route"] + case["plan"]))
    pa = _plan_args(case["plan"], case["acts"], seed)
    plan = ops.Conv3dPlan(device=DEV, **pa)
    worst = {}
    prev = ops.get_reserved_cus()
    try:
        for dims in TR.ranges3d(family):
            assert TR.geometry3d("direct", dims)[3] == ops.conv3d_grid(*dims), dims
            counts = [TR.classes3d(family, dims, cus, r) for r in TR.RESERVES]
            assert max(c["len_min"] for c in counts) >= 3 and counts[0]["G"] != counts[1]["G"], (dims, counts)
            reference, x0, got = None, None, {}
            for r in TR.RESERVES:
                assert ops.set_reserved_cus(r) == r
                for binding in ("torch", "ctypes") if case["both"] else ("torch",):
                    kernels, x, kw, before, bufs = _launch(case, plan, dims, binding, seed + sum(dims))
                    if reference is None:
                        reference, x0 = _reference(pa, dims, x, kw, before), x
                    assert torch.equal(x, x0)                                   # (one reference serves every launch of the shape)
                    what = "%s/%s reserve %d" % (case["route"], binding, r)
                    _check(case, dims, reference, bufs, worst, what)
                    assert kernels == KERNELS[case["route"]], "%s %s: ran %s" % (what, dims, sorted(kernels))
                    if "stats" in bufs:
                        assert _written_blocks(bufs) == TR.geometry3d("direct", dims)[3], "%s %s: partial blocks written" % (what, dims)
                    got[r, binding] = {k: v[0].clone() for k, v in bufs.items()}
                    del x, kw, before, bufs
            first = got.pop((TR.RESERVES[0], "torch"))
            for key, other in got.items():
                for k in first:
                    assert torch.equal(first[k].view(torch.int8), other[k].view(torch.int8)), "%s differs on %s (%s)" % (key, k, dims)
            print("TILE-RANGES %s %s %s" % (request.node.callspec.id, dims, " | ".join(
                "G=%d len %d-%d middle=%d whole=%d cross_n=%d" % (c["G"], c["len_min"], c["len_max"], c["middle"], c["whole_inside"], c["cross_n"])
                for c in counts)))
            del got, first, reference, x0
            torch.cuda.empty_cache()
    finally:
        ops.set_reserved_cus(prev)
    print("ROUTE-RATIO %s %s ranges[%s] %s" % (case["route"], case["plan"], request.node.callspec.id,
                                               " ".join("%s=%.2f" % kv for kv in sorted(worst.items()))))
