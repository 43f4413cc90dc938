"""Every dispatch route of ops.Conv3dPlan.run (the 3x3x3 convolution) against the fp64 reference of tests/conv3d_ref.py.

One case per (route, plan, activation, epilogue, strides, switches).  Each case
  * asserts WHICH kernel instances ran (torch.profiler kernel names, template arguments included, against the copy of the launchers'
    instance choice in tests/conv3d_instances.py): a silent fallback to another route or to a sibling instance (a wider read-back kind, a
    lost STATS) is a failure, and the deliberate fallback cases assert the instance they fall back to;
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
  * runs every subset of the read-back streams per kernel family (READBACK: test_conv3d_readback_subsets) and the four-wave form of the
    two-axis kernel in a child process (test_conv3d_wino2_four_wave_form); test_every_claimed_instance_ran closes the module: all 25
    instances of the default library ran.
Both bindings launch from one wiring (ops.CONV3D_ROUTES): one small-shape case of every route, and the reset-gate cases, run under both and
must agree bit for bit."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv3d_ref as R
import tile_ranges_ref as TR
from conv3d_instances import ALL, INSTANCES, KERNELS, SHARED, Refused, instance       # noqa: F401 (INSTANCES: tests/test_kernel_ledger_cpu.py)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# per-element bound constants, in units of 2^-24 A: the worst ratio measured on an MI355X over every case and output of the route
# (in the comments), times at least 3.  The Winograd routes sit BELOW the direct kernel: their transforms shorten the fp32 sums.
# The many-tile cases added later (test_conv3d_route_over_multi_tile_ranges) are held to the same constants; their sums have the same 27 x cin
# terms, their worst ratios (in brackets, over 2 x 90 k voxels per case instead of a few thousand) are the tail of the same distribution.
# So are the read-back subsets (READBACK; second brackets: the worst family x subset) and the four-wave form of the two-axis kernel, whose
# outputs are the eight-wave form's bit for bit; every family x subset is in profiles/conv3d_instances_gpu_tests.txt.
C_ROUTE = {
    "direct": 18.0,           # measured 5.79 (33 -> 33, out_main) [6.43: 33 -> 32] [5.15: 32 -> 32 scale; 33 -> 32 3.91, 16 -> 16 4.54]
    "wino3": 7.0,             # measured 2.25 (32 -> 32, out_main) [2.29: 33 -> 32] [1.55: scale]
    "wino2": 8.0,             # measured 2.47 (32 -> 32 + statistics, out_main) [2.55] [2.19: 32 -> 32 scale; 33 -> 32 1.91; four waves 2.51]
    "wino2_xout": 7.0,        # measured 2.16 (out_main; channel 32: 0.70) [3.15; channel 32: 0.91]
    "wino2_o16": 5.0,         # measured 1.63 (with statistics, out_main) [1.83] [1.28: res + res2]
    "wino2_c16": 2.0,         # measured 0.63 (head) [0.71]
    "wino3+xout": 7.0,        # measured 2.26 (out_main; channel 32: 0.93) [2.33]
}
# INSTANCES (tests/conv3d_instances.py): route -> the template instances it launches, the table tests/test_kernel_ledger_cpu.py holds
# against the emitted kernels; every case asserts the exact set instance(route, plan, epilogue) predicts.  No kernel named conv3d_* of the
# default build is left to another suite:
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(conv3d_\w*?_kernel)(<[^>()]*>)?")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# csrc/conv3d_wino2.hip latches ESTD_WINO2_WAVES at the first call: the form this process runs
WAVES = 4 if os.environ.get("ESTD_WINO2_WAVES", "").strip() == "4" else 8
_RAN = set()                           # every conv3d instance the profiler saw in this process, and in the children it started
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
    C("wino2-32-acc", "wino2", "32>32", ("relu", "tanh", 16), ("acc",), 32, 40, W2),                 # RBK 1
    C("wino2-32-res-scale", "wino2", "32>32", ("relu",), ("res", "scale"), 36, 32, W2),               # RBK 2
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

# ---- every subset of the read-back streams, per kernel family.  An RBK = 3 instance also serves the RBK 1 and 2 calls of the forms that have
# no narrower one (scalar channel, 32 -> 16, four waves), an RBK = 2 instance "scale only" and "residual2 only", and the direct kernel takes
# all of it as run-time flags: a stream that is absent is a NULL pointer / accumulate = 0 INSIDE an instance compiled for it.
# a batch, an odd depth whose last pair is half empty, H and W one past a tile (W one short of two)
RB_SHAPES = [(2, 2, 9, 17), (1, 33, 17, 15)]
RB_SUBSETS = [("res",), ("res2",), ("scale",), ("acc",), ("res", "res2"), ("res", "acc"), ("scale", "acc"), ("res", "res2", "scale", "acc")]
RB_BOTH = ("res2",)                    # under both bindings: the first stream NULL, the second not
RB_FAMILIES = [
    # (id, route, plan, activations, in_stride, out_stride, switches, subsets an existing small-shape case runs already)
    # wino3-32-split8-res, wino3-32-split20-acc, wino3-32-split16-acc-scale
    ("wino3-32", "wino3", "32>32", ("tanh", "relu", 16), 36, 40, None, [("res",), ("acc",), ("scale", "acc")]),
    # wino2-32-acc, wino2-32-split20-res-res2-scale-acc
    ("wino2-32", "wino2", "32>32", ("relu",), 32, 36, W2, [("acc",), ("res", "res2", "scale", "acc")]),
    # wino2-33to32-relu-res-acc
    ("wino2-33to32", "wino2", "33>32", ("tanh",), 36, 32, W2, [("res", "acc")]),
    # o16-split8-res-res2-scale-acc
    ("o16", "wino2_o16", "32>16", ("relu", "tanh", 8), 32, 24, None, [("res", "res2", "scale", "acc")]),
    # direct-32-split20-res-res2-scale-acc
    ("direct-32", "direct", "32>32", ("tanh", "relu", 20), 36, 40, DIRECT, [("res", "res2", "scale", "acc")]),
    ("direct-33to32", "direct", "33>32", ("relu", "tanh", 8), 64, 36, DIRECT, []),
    ("direct-16to16", "direct", "16>16", ("relu",), 32, 24, DIRECT, []),
]
READBACK = [C("%s-%s" % (fid, "-".join(sub)), route, plan, acts, sub, ins, outs, sw, shapes=RB_SHAPES, both=sub == RB_BOTH)
            for fid, route, plan, acts, ins, outs, sw, have in RB_FAMILIES for sub in RB_SUBSETS if sub not in have] + [
    # under the default switches the three-axis kernel's scalar-channel instance has no read-back stream: the two-axis kernel's takes the call
    C("fallback-33to32-residual-to-wino2", "wino2", "33>32", ("relu",), ("res",), 36, 32, shapes=RB_SHAPES),
    # the gated 32 -> 16 instance has none either, and nothing to fall back to: refused by the launcher, before any launch
    C("refused-o16-gate-res", "wino2_o16", "32>16", ("none",), ("gate", "res"), 32, 16, shapes=RB_SHAPES[:1], both=True),
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


def _launch(case, plan, dims, binding, seed, refused=False):
    """one run of the case: inputs, guarded outputs, the launch under the case's switches and the profiler -> (kernel instances, results);
    ``refused``: the call must raise instead"""
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
            if refused:
                with pytest.raises(RuntimeError):
                    plan.run(x, dims, **kw)
            else:
                plan.run(x, dims, **kw)
            torch.cuda.synchronize()
    kernels = {m.group(1) + (m.group(2) or "") for e in prof.key_averages() for m in [KERNEL_RE.search(e.key)] if m}
    _RAN.update(kernels)
    return kernels, x, kw, before, bufs


def _want(case):
    """the instances the case must run in this process (None: the launcher refuses the call)"""
    try:
        return instance(case["route"], case["plan"], case["epi"], WAVES)
    except Refused:
        return None


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


def _against_fp64(case, tag=""):
    """the protocol of the module docstring for one case on its shapes, under one binding or both"""
    from estdepth_amd import ops
    seed = sum(map(ord, case["route"] + case["plan"]))
    pa = _plan_args(case["plan"], case["acts"], seed)
    plan = ops.Conv3dPlan(device=DEV, **pa)
    want = _want(case)
    worst = {}
    for dims in case["shapes"]:
        got = {}
        for binding in ("torch", "ctypes") if case["both"] else ("torch",):
            kernels, x, kw, before, bufs = _launch(case, plan, dims, binding, seed + sum(dims), refused=want is None)
            what = "%s/%s" % (case["route"], binding)
            if want is None:                                                    # refused before any launch: no kernel, every byte the sentinel
                assert not kernels, "%s %s: refused, but ran %s" % (what, dims, sorted(kernels))
                for key, (buf, _, _, _) in bufs.items():
                    assert _untouched(buf, 0, 0) == 0, "%s %s: refused, but %s was written" % (what, dims, key)
                continue
            _compare(case, pa, dims, x, kw, before, bufs, worst, what)          # (first: a wrong result names the output it is wrong in)
            assert kernels == want, "%s %s: ran %s, expected %s" % (what, dims, sorted(kernels), sorted(want))
            got[binding] = {k: v[0].clone() for k, v in bufs.items()}
            del x, kw, before, bufs
        if case["both"] and want is not None:
            for k in got["torch"]:
                assert torch.equal(got["torch"][k].view(torch.int8), got["ctypes"][k].view(torch.int8)), "bindings differ on %s" % k
        del got
        torch.cuda.empty_cache()
    print("ROUTE-RATIO %s %s %s%s" % (case["route"], case["plan"], tag, " ".join("%s=%.2f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("case", CASES)
def test_conv3d_route_against_fp64(case):
    _against_fp64(case)


@pytest.mark.parametrize("case", READBACK)
def test_conv3d_readback_subsets(case, request):
    """Every subset of {residual, residual2, out_scale, accumulate} no small-shape case above runs, per kernel family (READBACK), under the
    protocol of test_conv3d_route_against_fp64: the fp64 reference, the route's bound, the sentinel bands, the exact instance -- which for
    the forms without an instance per read-back kind is the RBK = 3 one with NULL streams.  A call the launcher refuses must raise under
    both bindings with no conv3d kernel in the profile and every output byte still the sentinel."""
    _against_fp64(case, "readback[%s] " % request.node.callspec.id)


def _written_blocks(bufs):
    """the 4-double GroupNorm partial blocks a launch wrote completely (the rest keeps the sentinel)"""
    buf, (lo, hi), _, _ = bufs["stats"]
    return int((buf[lo:hi].view(torch.int64).view(-1, 4) != SENT64).all(1).sum())


@pytest.mark.parametrize("case", [p for p in CASES if p.values[0]["shapes"] is SMALL])
def test_conv3d_route_over_multi_tile_ranges(case, request):
    """Every tile-edge case once more on the many-tile shapes of tests/tile_ranges_ref.py (thin columns, a large batch: ranges of 4-12 tiles
    per workgroup with middle tiles, whole columns inside a range, ranges across batch elements and starts on the odd last depth pair),
    under the full grid and under set_reserved_cus(128): every element of every output against one fp64 reference per shape, the same
    bound, sentinel bands and kernel instances, and the outputs of the two grids (and of both bindings, where the case runs both) bit-identical.
    The GroupNorm partials are indexed by the canonical 8 x 16 tile (n, d, h-tile, w-tile), not by workgroup: each grid writes exactly
    ops.conv3d_grid(...) blocks -- the direct kernel's tile count, which the model reproduces -- and the same bits."""
    from estdepth_amd import ops
    family = TR.ROUTE_FAMILY[case["route"]]
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    seed = sum(map(ord, case["route"] + case["plan"]))
    pa = _plan_args(case["plan"], case["acts"], seed)
    plan = ops.Conv3dPlan(device=DEV, **pa)
    want = _want(case)
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
                    assert kernels == want, "%s %s: ran %s, expected %s" % (what, dims, sorted(kernels), sorted(want))
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


# ------------------------------------------------------------------------------------- the four-wave form (a child process)
def _job(jid, route, plan, acts, epi, ins, outs, sw, shapes, reserves):
    """a case in JSON form for run_job: it crosses into a child process"""
    return dict(id=jid, route=route, plan=plan, acts=list(acts), epi=sorted(epi), ins=ins, outs=outs, sw=sw or {},
                shapes=[list(s) for s in shapes], reserves=list(reserves))


def run_job(job, check=True):
    """One case on every shape of the job under every grid of job["reserves"], in THIS process (whose ESTD_WINO2_WAVES is latched):
    the exact instance per launch, the grids bit-identical and, with ``check``, every output against the fp64 reference with the route's
    bound and the sentinel bands.  -> dict(ran, worst ratios, sums: SHA-256 of every guarded buffer per shape)"""
    from estdepth_amd import ops
    case = dict(route=job["route"], plan=job["plan"], acts=tuple(job["acts"]), epi=set(job["epi"]), ins=job["ins"], outs=job["outs"],
                sw=dict(DEFAULT, **job["sw"]))
    seed = sum(map(ord, case["route"] + case["plan"]))
    pa = _plan_args(case["plan"], case["acts"], seed)
    plan = ops.Conv3dPlan(device=DEV, **pa)
    want = instance(case["route"], case["plan"], case["epi"], WAVES)
    worst, ran, sums = {}, set(), {}
    prev = ops.get_reserved_cus()
    try:
        for dims in map(tuple, job["shapes"]):
            reference, first = None, None
            for r in job["reserves"]:
                assert ops.set_reserved_cus(r) == r
                kernels, x, kw, before, bufs = _launch(case, plan, dims, "torch", seed + sum(dims))
                what = "%s reserve %d" % (job["id"], r)
                if check:
                    if reference is None:
                        reference = _reference(pa, dims, x, kw, before)
                    _check(case, dims, reference, bufs, worst, what)
                assert kernels == want, "%s %s: ran %s, expected %s" % (what, dims, sorted(kernels), sorted(want))
                ran |= kernels
                got = {k: v[0].clone() for k, v in bufs.items()}
                if first is None:
                    first = got
                for k in first:
                    assert torch.equal(first[k].view(torch.int8), got[k].view(torch.int8)), "%s: the grids differ on %s (%s)" % (what, k, dims)
                del x, kw, before, bufs, got
            for k, v in first.items():
                sums["%s %s" % ("x".join(map(str, dims)), k)] = hashlib.sha256(v.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
            del first, reference
            torch.cuda.empty_cache()
    finally:
        ops.set_reserved_cus(prev)
    return dict(ran=sorted(ran), worst=worst, sums=sums)


def _child(env, jobs):
    """run_job of every job in ONE fresh process with ``env`` (the latched switch) -> {job id: run_job's result}; failures are reported
    per job.  The child starts nothing more on the device once a synchronize fails."""
    code = ("import json, sys, traceback\n"
            "sys.path.insert(0, 'tests')\n"
            "import torch\n"
            "import test_gpu_conv3d_routes as T\n"
            "for j in json.loads(sys.argv[1]):\n"
            "    try:\n"
            "        print('CASE ' + json.dumps([j['id'], T.run_job(j)]), flush=True)\n"
            "    except BaseException:\n"
            "        print('FAIL ' + json.dumps([j['id'], traceback.format_exc()[-1500:]]), flush=True)\n"
            "        try:\n"
            "            torch.cuda.synchronize()\n"
            "        except BaseException:\n"
            "            sys.exit(3)\n")
    r = subprocess.run([sys.executable, "-c", code, json.dumps(jobs)], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    if r.returncode < 0 or r.returncode in (3, 134, 139):       # a crashed GPU process: start nothing more on this device
        pytest.exit("child %s ended with status %d:\n%s\n%s" % (env, r.returncode, r.stdout[-3000:], r.stderr[-3000:]), returncode=1)
    got, fails = {}, []
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            jid, res = json.loads(line[5:])
            got[jid] = res
            _RAN.update(res["ran"])
        elif line.startswith("FAIL "):
            fails.append(json.loads(line[5:]))
    assert r.returncode == 0, (env, r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert not fails, "%s: %s" % (env, "\n".join("%s: %s" % tuple(f) for f in fails))
    assert sorted(got) == sorted(j["id"] for j in jobs), (env, sorted(got))
    return got


FOUR_WAVES = dict(ESTD_WINO2_WAVES="4")
# read-back kinds 0, 1, 2, 3 of the plain 32 -> 32 form: the two tile-edge shapes of READBACK and one many-tile shape, both grids
W4_JOBS = [_job("w4-32-" + ("-".join(epi) or "plain"), "wino2", "32>32", acts, epi, ins, outs, W2,
                RB_SHAPES + TR.ranges3d(TR.ROUTE_FAMILY["wino2"])[:1], TR.RESERVES)
           for acts, epi, ins, outs in ((("relu",), (), 32, 32), (("relu", "tanh", 16), ("acc",), 32, 40), (("relu",), ("res", "scale"), 36, 32),
                                        (("tanh", "relu", 20), ("res", "res2", "scale", "acc"), 64, 36))]
# the forms that have no four-wave version: one launch each
W4_JOBS += [_job("w4-33to32", "wino2", "33>32", ("tanh",), (), 36, 40, W2, RB_SHAPES[:1], (0,)),
            _job("w4-o16", "wino2_o16", "32>16", ("none",), (), 32, 16, None, RB_SHAPES[:1], (0,)),
            _job("w4-33to33", "wino2_xout", "33>33", ("relu",), (), 36, 40, W2XOUT, RB_SHAPES[:1], (0,))]
W4_INSTANCES = {"w4-32-plain": "conv3d_wino2_kernel<4, 0, false, false, false, false>",
                "w4-33to32": "conv3d_wino2_kernel<8, 0, true, false, false, false>",
                "w4-o16": "conv3d_wino2_kernel<8, 0, false, true, false, false>",
                "w4-33to33": "conv3d_wino2_kernel<8, 0, true, false, true, false>"}       # every other job: <4, 3, false, ...>


def test_conv3d_wino2_four_wave_form():
    """ESTD_WINO2_WAVES=4 (latched at the first call, hence a fresh child process): one wave per SIMD holds both channel halves,
    conv3d_wino2_kernel<4, 0, ...> and <4, 3, ...>.  The child runs the read-back kinds 0 - 3 of the plain 32 -> 32 form under the whole
    protocol (fp64 reference, C_ROUTE["wino2"], sentinel bands, exact instance, both grids bit-identical), and one launch of each form
    that has no four-wave version, which must still run its <8, ...> instance.

    Both forms form every output with the same operations in the same order.  A wave of the eight-wave form owns the channel half
    nh0 = wave >> 2, a wave of the four-wave form loops over x = 0, 1 in its place; per (product t, half x) the MFMA chain runs
    step -> component pair h -> component e over the same fragments and the same weights (load_w: byte offset x * 2048 against
    nh0 * 2048), the output transforms (fold_sd) and the epilogue (bn_act, residuals, scale, running sum) are written once for both.
    So the parent, which runs the same inputs in the eight-wave form, requires the SAME BITS of every output."""
    if WAVES != 8:
        pytest.fail("run this suite without ESTD_WINO2_WAVES: the parent process is the eight-wave side of the comparison")
    got = _child(FOUR_WAVES, W4_JOBS)
    for job in W4_JOBS:
        res = got[job["id"]]
        want = W4_INSTANCES.get(job["id"], "conv3d_wino2_kernel<4, 3, false, false, false, false>")
        assert res["ran"] == [want], (job["id"], res["ran"])
        print("ROUTE-RATIO %s %s four-wave[%s] %s" % (job["route"], job["plan"], job["id"],
                                                      " ".join("%s=%.2f" % kv for kv in sorted(res["worst"].items()))))
        mine = run_job(job, check=False)                     # the eight-wave form on the same inputs (its own cases hold it to the reference)
        assert mine["ran"] == sorted(instance(job["route"], job["plan"], job["epi"], 8)), (job["id"], mine["ran"])
        diff = sorted(k for k in res["sums"] if res["sums"][k] != mine["sums"].get(k))
        assert sorted(res["sums"]) == sorted(mine["sums"]) and not diff, "%s: four and eight waves differ on %s" % (job["id"], diff)


def _first_case(inst):
    """a case of this module that runs the instance in the eight-wave form"""
    for p in CASES + READBACK:
        case = p.values[0]
        if case["shapes"] is not BIG and case["shapes"] is not FULL and inst in (_want(case) or ()):
            return case
    return None


def test_every_claimed_instance_ran():
    """the instances the profiler saw under this module's cases and in the four-wave child are exactly the claimed ones (should this
    test run alone: one small launch per missing instance, one small child for the four-wave pair)"""
    from estdepth_amd import ops
    if WAVES == 8 and not any(k.startswith("conv3d_wino2_kernel<4,") for k in _RAN):
        _child(FOUR_WAVES, [_job(j["id"], j["route"], j["plan"], j["acts"], j["epi"], j["ins"], j["outs"], j["sw"], RB_SHAPES[:1], (0,))
                            for j in (W4_JOBS[0], W4_JOBS[3])])
    for inst in sorted(ALL - _RAN):
        case = _first_case(inst)
        if case is None:
            continue
        seed = sum(map(ord, case["route"] + case["plan"]))
        plan = ops.Conv3dPlan(device=DEV, **_plan_args(case["plan"], case["acts"], seed))
        kernels = _launch(case, plan, RB_SHAPES[0], "torch", seed)[0]
        assert kernels == _want(case), (inst, sorted(kernels))
    print("CONV3D-INSTANCES %d ran:\n  %s" % (len(_RAN), "\n  ".join(sorted(_RAN))))
    assert _RAN == ALL, "never ran: %s; not claimed: %s" % (sorted(ALL - _RAN), sorted(_RAN - ALL))
