"""Every dispatch route of the 2D convolutions (stage A of a step: the PSM matching features, the ResNet-18/50 semantic trunk, the 2D decoder
and refinement tail) against the fp64 reference of tests/conv2d_ref.py.

A route is one kernel instance, reached through the op or switch that reaches it.  Each case
  * asserts WHICH kernel instance ran, template arguments included (torch.profiler's demangled names): a silent fallback to another
    instance is a failure.  The instance of conv1x1 / taps is predicted by a Python copy of their dispatchers (``c1x1_kernel``,
    ``taps_kernel``), so the forced configurations that fall back (an odd chunk count under a split-K / multi-chunk-stage instance, cout
    not a multiple of 64 under TN = 4) assert the instance they fall back to;
  * compares every output element with the reference: |gpu - ref| <= C_ROUTE[route] * 2^-24 * A (A: the same pipeline on absolute values);
  * runs the op under both bindings and, through the C ABI directly (ctypes), once more with the input, the residual and the output
    carved out of buffers filled with a NaN sentinel: everything outside the output must keep the sentinel bit for bit (a read outside
    the input or the residual would show as NaN in the output).  The three results must be bit-identical;
  * runs shapes at the tile edges (1x1 maps; just below / at / above the 8 x 16 tiles of the 3x3 kernels and the 16-pixel rows of the
    refine / stem kernels; odd maps for stride 2; batches 1-3; 1, 2, 4 and odd counts of 16-channel chunks; cout 320 on the 128-wide
    tiles), the two persistent 3x3 kernels over ranges of several work items per workgroup (many thin images, two grid sizes:
    tests/tile_ranges_ref.py), the full-size layers of each family at the benchmark's 5 x 480 x 640 (reference at sampled pixels) and the 32-bit limits:
    conv1x1 / taps just below 0x7fffff00 bytes over the batch (and at / above it: refused by both bindings), and one batch of more than
    2^31 bytes through each per-image kernel.
ESTD_C1X1_CFG / ESTD_CTAPS_CFG / ESTD_C1X1_LDS are latched at the first call: each forced configuration runs its cases in a child process
of its own, one child at a time; the child prints one line per case (worst ratio, kernel) for the parent to assert."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv2d_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# per-element bound constants, in units of 2^-24 A: at least 3 x the worst ratio measured on an MI355X over every case of the route
# (in the comments).  The many-item cases added later (test_conv2d_plan_over_multi_item_ranges) are held to the same constants; their worst
# ratios, over every pixel of 20 - 192 images, are in brackets.
C_ROUTE = {
    "wino2": 8.0,             # measured 2.50 (full-plan-resnet-layer2) [2.99: plan-wino2-d2-cout192]
    "k3": 17.0,               # measured 5.49 (plan-k3-nt4-d2-res-relu_after) [7.02: plan-k3-nt2-d2-res]
    "wino": 17.0,             # not measured (ESTD_BUILD_AB=1 builds only): the direct kernel's constant
    "k3_split": 17.0,         # not measured (ESTD_BUILD_AB=1 builds only): the direct kernel's constant
    "conv1x1": 19.0,          # measured 6.06 (full-lds0-11: 2048 -> 512 at 15 x 20 on the direct form)
    "conv1x1_lds": 18.0,      # measured 5.77 (full-conv1x1-9: 1024 -> 2048, stride 2)
    "taps": 14.0,             # measured 4.63 (taps-241-4)
    "stem7x7": 13.0,          # measured 4.18 (full-stem7x7)
    "stem3x3": 15.0,          # measured 4.96 (stem3x3-edges)
    "small": 12.0,            # measured 3.93 (small-64-1-1-2)
    "to16": 16.0,             # measured 5.11 (to16-16-True)
    "disp_head": 8.0,         # measured 2.47 (disp-32-x1)
}

# ---------------------------------------------------------------------------------------------------------------- expected instances
C1X1_LDS = {1441: (128, 128, 2, 2, 1, 3), 1442: (128, 128, 2, 2, 2, 3), 1421: (128, 64, 2, 2, 1, 3), 1422: (128, 64, 2, 2, 2, 3),
            1241: (64, 128, 2, 2, 1, 3), 1242: (64, 128, 2, 2, 2, 3), 1221: (64, 64, 2, 2, 1, 4), 1222: (64, 64, 2, 2, 2, 3),
            1224: (64, 64, 2, 2, 4, 3), 1122: (32, 64, 1, 4, 2, 3), 1124: (32, 64, 1, 4, 4, 3)}
DIRECT = {441: (4, 4, 2, 1), 421: (4, 2, 3, 1), 241: (2, 4, 3, 1), 221: (2, 2, 4, 1), 444: (4, 4, 2, 4), 424: (4, 2, 3, 4),
          244: (2, 4, 3, 4), 224: (2, 2, 4, 4), 124: (1, 2, 4, 4), 121: (1, 2, 8, 1)}


def _inst(name, args):
    return "%s<%s>" % (name, ", ".join(str(a).lower() for a in args))


def _direct_cfg(cfg, heuristic, cin, cout):
    if cfg == 0:
        cfg = heuristic()
    if cfg % 10 == 4 and cin % 64:
        cfg -= 3
    if (cfg // 10) % 10 == 4 and cout % 64:
        cfg -= 20
    return cfg if cfg in DIRECT else 121


def c1x1_kernel(cfg_env, lds_env, N, H, W, cin, cout, stride, cus):
    """the instance estd_conv1x1_nhwc (csrc/conv1x1.hip) launches"""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = N * Ho * Wo
    want = cus * 7 // 2
    tiles = lambda tm, tn: ((M + 16 * tm - 1) // (16 * tm)) * (cout // (16 * tn))      # noqa: E731
    sk4 = cin % 64 == 0 and cin >= 256
    cfg = cfg_env
    if cfg == 0 and lds_env and cout % 64 == 0:
        wgs = lambda bm, bn: ((M + bm - 1) // bm) * ((cout + bn - 1) // bn)             # noqa: E731
        c64 = 1222 if cin >= 512 and cin % 32 == 0 else 1221
        if wgs(64, 64) >= cus * 7 // 4:
            cfg = c64
        elif wgs(32, 64) >= cus * 7 // 4 and cin % 64 == 0:
            cfg = 1124
        elif wgs(64, 64) >= cus * 7 // 8:
            cfg = c64
        elif wgs(32, 64) >= cus * 3 // 4 and cin % 64 == 0:
            cfg = 1124
    if cfg >= 1000 and cin % (16 * (cfg % 10)):
        cfg = 0
    if cfg in C1X1_LDS:
        return _inst("conv1x1_lds_kernel", C1X1_LDS[cfg])
    if cfg >= 1000:
        cfg = 0

    def heuristic():
        c64 = cout % 64 == 0
        if c64 and tiles(4, 4) >= want:
            return 441
        if sk4 and cin >= 1024 and c64 and tiles(4, 4) >= want // 4:
            return 444
        if tiles(4, 2) >= want:
            return 421
        if sk4 and c64 and tiles(4, 4) >= want // 4:
            return 444
        if sk4 and c64 and tiles(2, 4) >= want // 4:
            return 244
        if tiles(2, 2) >= want:
            return 221
        if sk4 and tiles(2, 2) >= want // 4:
            return 224
        return 121
    return _inst("conv1x1_nhwc_kernel", DIRECT[_direct_cfg(cfg, heuristic, cin, cout)])


def taps_kernel(cfg_env, N, H, W, cin, cout, k, stride, pad, cus):
    """the instance estd_conv2d_taps_nhwc (csrc/conv2d_taps.hip) launches"""
    Ho, Wo = R.out_size(H, W, k, stride, pad)
    M = N * Ho * Wo
    want = cus * 7 // 2
    tiles = lambda tm, tn: ((M + 16 * tm - 1) // (16 * tm)) * (cout // (16 * tn))      # noqa: E731
    sk4 = cin % 64 == 0 and k * k * cin >= 256
    c64 = cout % 64 == 0

    def heuristic():
        if c64 and tiles(4, 4) >= want:
            return 441
        if tiles(4, 2) >= want:
            return 421
        if sk4 and c64 and tiles(4, 4) >= want // 4:
            return 444
        if tiles(2, 2) >= want:
            return 221
        if sk4 and c64 and tiles(2, 4) >= want // 4:
            return 244
        if sk4 and tiles(2, 2) >= want // 4:
            return 224
        return 124 if sk4 else 121
    return _inst("conv2d_taps_kernel", DIRECT[_direct_cfg(cfg_env, heuristic, cin, cout)])


def small_rows(N, Ho, Wo, cout, ntw):
    """rows of 16 pixels per wave of conv2d_small_kernel (estd_conv2d_small_nhwc)"""
    rows, segs, groups = 8, (Wo + 15) // 16, cout // (16 * ntw)
    while rows > 1 and N * ((Ho + rows - 1) // rows) * segs * groups < 8192:
        rows >>= 1
    return rows


# ---------------------------------------------------------------------------------------------------------------------------- cases
PLAN_EDGE = [(1, 1, 1), (2, 7, 15), (1, 8, 16), (3, 9, 17), (1, 17, 33)]
MAP_EDGE = [(1, 1, 1), (2, 7, 15), (1, 8, 16), (3, 9, 17), (1, 15, 33)]
WINO2 = dict(CONV2D_ALGO="wino2", CONV2D_NT="auto", C2W2_DIL2=True)
DIRECT2, DIRECT4 = dict(CONV2D_ALGO="direct", CONV2D_NT="2"), dict(CONV2D_ALGO="direct", CONV2D_NT="4")


# Many work items on few pixels (tests/tile_ranges_ref.py): ``many`` images of 9 x 17 (2 x 2 tiles, three of them ragged; 3 x 2 of the
# 64-channel items of conv2d_wino2) give every workgroup of the reserve-128 grid a range of three or four items, of which the kernel prefetches
# the next one while it works: another tile of the image, the next image, the next output-channel group.  ``many`` is the smallest batch that
# does it for the case's cout (tile_ranges_ref.batch2d; tests/test_tile_ranges_cpu.py).
MANY_HW = (9, 17)


def K(cid, fam, route, shapes, **kw):
    return dict(id=cid, fam=fam, route=route, shapes=[list(s) for s in shapes], **kw)


PLAN_CASES = [
    # Conv2dPlan: every instance of the two NHWC 3x3 kernels (ops.CONV2D_ALGO / CONV2D_NT / C2W2_DIL2), every epilogue
    K("plan-wino2-d1-relu_before", "plan", "wino2", PLAN_EDGE, many=129, cin=32, cout=64, dil=1, rb=True, kern="conv2d_wino2_kernel<1>"),
    K("plan-wino2-d1-res-relu_after", "plan", "wino2", PLAN_EDGE, many=192, cin=96, cout=32, dil=1, res=True, ra=True, kern="conv2d_wino2_kernel<1>"),
    K("plan-wino2-d1-res", "plan", "wino2", PLAN_EDGE, many=26, cin=64, cout=320, dil=1, res=True, kern="conv2d_wino2_kernel<1>"),
    K("plan-wino2-d2-relu_before", "plan", "wino2", PLAN_EDGE, many=192, cin=32, cout=32, dil=2, rb=True, kern="conv2d_wino2_kernel<2>"),
    K("plan-wino2-d2-res-relu_after", "plan", "wino2", PLAN_EDGE, many=129, cin=64, cout=64, dil=2, res=True, ra=True, kern="conv2d_wino2_kernel<2>"),
    K("plan-k3-nt2-d1-relu_before", "plan", "k3", PLAN_EDGE, many=96, cin=32, cout=64, dil=1, rb=True, sw=DIRECT2, kern="conv2d_k3_kernel<2, 1>"),
    K("plan-k3-nt4-d1-res-relu_after", "plan", "k3", PLAN_EDGE, many=96, cin=96, cout=128, dil=1, res=True, ra=True, sw=DIRECT4,
      kern="conv2d_k3_kernel<4, 1>"),
    K("plan-k3-nt2-d2-res", "plan", "k3", PLAN_EDGE, many=96, cin=64, cout=64, dil=2, res=True, sw=dict(WINO2, C2W2_DIL2=False),
      kern="conv2d_k3_kernel<2, 2>", kern_ab="conv2d_wino_kernel<2, 2>"),
    K("plan-k3-nt4-d2-res-relu_after", "plan", "k3", PLAN_EDGE, many=39, cin=32, cout=320, dil=2, res=True, ra=True, sw=DIRECT4,
      kern="conv2d_k3_kernel<4, 2>"),
    K("plan-k3-nt2-d1-cout320", "plan", "k3", PLAN_EDGE, many=20, cin=32, cout=320, dil=1, ra=True, sw=DIRECT2, kern="conv2d_k3_kernel<2, 1>"),
    # the ESTD_BUILD_AB=1 kernels (skipped in the default build; no many-item shape)
    K("plan-wino-ab", "plan", "wino", PLAN_EDGE, cin=32, cout=64, dil=1, res=True, ra=True, sw=dict(CONV2D_ALGO="wino", CONV2D_NT="4"),
      kern="conv2d_wino_kernel<4, 1>", ab=True),
    K("plan-k3-split-ab", "plan", "k3_split", PLAN_EDGE, cin=32, cout=64, dil=1, res=True, sw=dict(CONV2D_ARITH="bf16x3"),
      kern="conv2d_k3_split_kernel<1, true>", ab=True),
    # full size (5 x 480 x 640 images): the ResNet-50 3x3 convolutions of layer1..4, the dilated PSM layer
    K("full-plan-resnet-layer1", "plan", "wino2", [(5, 120, 160)], cin=64, cout=64, dil=1, ra=True, kern="conv2d_wino2_kernel<1>"),
    K("full-plan-resnet-layer2", "plan", "wino2", [(5, 60, 80)], cin=128, cout=128, dil=1, ra=True, kern="conv2d_wino2_kernel<1>"),
    K("full-plan-resnet-layer3", "plan", "wino2", [(5, 30, 40)], cin=256, cout=256, dil=1, ra=True, kern="conv2d_wino2_kernel<1>"),
    K("full-plan-resnet-layer4", "plan", "wino2", [(5, 15, 20)], cin=512, cout=512, dil=1, ra=True, kern="conv2d_wino2_kernel<1>"),
    K("full-plan-psm-dil2-res", "plan", "wino2", [(5, 120, 160)], cin=128, cout=128, dil=2, res=True, kern="conv2d_wino2_kernel<2>"),
    K("full-plan-k3-psm-32", "plan", "k3", [(5, 120, 160)], cin=32, cout=32, dil=1, res=True, sw=DIRECT2, kern="conv2d_k3_kernel<2, 1>"),
    # per-image descriptors: one batch of more than 2^31 bytes per tensor
    K("big-plan-wino2", "plan", "wino2", [(56, 480, 640)], cin=32, cout=32, dil=1, res=True, ra=True, kern="conv2d_wino2_kernel<1>"),
    K("big-plan-k3", "plan", "k3", [(56, 480, 640)], cin=32, cout=32, dil=1, rb=True, sw=DIRECT2, kern="conv2d_k3_kernel<2, 1>"),
]

# only on the many-item shape: a cout of three groups for the instances whose cases above have one or two (the boundary between TWO groups is
# always a boundary between two ranges as well: the grid is even)
RANGE_CASES = [
    K("plan-wino2-d1-cout96", "plan", "wino2", [], many=64, cin=32, cout=96, dil=1, res=True, ra=True, kern="conv2d_wino2_kernel<1>"),
    K("plan-wino2-d2-cout96", "plan", "wino2", [], many=64, cin=64, cout=96, dil=2, rb=True, kern="conv2d_wino2_kernel<2>"),
    K("plan-wino2-d2-cout192", "plan", "wino2", [], many=43, cin=32, cout=192, dil=2, res=True, kern="conv2d_wino2_kernel<2>"),
    K("plan-k3-nt4-d1-cout192", "plan", "k3", [], many=64, cin=32, cout=192, dil=1, res=True, sw=DIRECT4, kern="conv2d_k3_kernel<4, 1>"),
    K("plan-k3-nt2-d2-cout96", "plan", "k3", [], many=64, cin=32, cout=96, dil=2, ra=True, sw=DIRECT2, kern="conv2d_k3_kernel<2, 2>"),
]

# (N, H, W, cin, cout, stride, relu, residual, affine): tile edges of both 1x1 forms -- 1x1 maps, ragged pixel tiles, odd maps at stride 2,
# 3 / 6 / 12 chunks (odd counts and odd per-wave shares under SK = 4 and U = 2 | 4), cout 32 and 320 (partly empty channel tiles)
C1X1_EDGE = [(1, 1, 1, 64, 64, 1, True, True, "bn"), (2, 7, 15, 48, 96, 2, True, True, "bn"), (3, 9, 17, 128, 320, 1, True, True, "bn"),
             (1, 8, 16, 96, 64, 1, False, False, "none"), (2, 5, 33, 192, 128, 2, False, True, "bias"), (1, 3, 5, 256, 64, 1, True, False, "bn"),
             (3, 17, 31, 64, 32, 1, True, True, "bn")]
# the full-size 1x1 convolutions: ResNet-50 layer1..4 at 5 x 480 x 640 (conv1, conv3 + shortcut, downsample) and the PSM channel mix
C1X1_FULL = [(5, 120, 160, 64, 64, 1, True, False, "bn"), (5, 120, 160, 64, 256, 1, True, True, "bn"), (5, 120, 160, 256, 64, 1, True, False, "bn"),
             (5, 120, 160, 256, 512, 2, False, False, "bn"), (5, 60, 80, 512, 128, 1, True, False, "bn"), (5, 60, 80, 128, 512, 1, True, True, "bn"),
             (5, 60, 80, 512, 1024, 2, False, False, "bn"), (5, 30, 40, 1024, 256, 1, True, False, "bn"), (5, 30, 40, 256, 1024, 1, True, True, "bn"),
             (5, 30, 40, 1024, 2048, 2, False, False, "bn"), (5, 15, 20, 2048, 512, 1, True, False, "bn"), (5, 15, 20, 512, 2048, 1, True, True, "bn"),
             (5, 120, 160, 32, 32, 1, False, False, "bias"), (5, 120, 160, 32, 32, 1, False, False, "none")]
# (N, H, W, cin, cout, k, stride, pad, relu, residual, affine): k 1 / 3 / 5 x stride 1 / 2 x pad 0 / k // 2 at the tile edges
TAPS_EDGE = [(1, 7, 9, 64, 64, 3, 1, 1, True, True, "bn"), (2, 11, 13, 64, 128, 3, 2, 1, True, False, "bn"),
             (1, 9, 11, 48, 96, 5, 2, 2, True, True, "bn"), (2, 8, 16, 128, 64, 5, 1, 0, False, False, "none"),
             (3, 9, 17, 64, 320, 1, 1, 0, False, True, "bn"), (1, 6, 10, 192, 64, 1, 2, 0, True, False, "bias"),
             (1, 1, 1, 32, 32, 3, 1, 1, True, False, "bn"), (2, 5, 7, 64, 32, 5, 1, 2, False, True, "bn"),
             (1, 10, 12, 256, 64, 3, 2, 0, True, False, "bn")]
# the full-size taps layers: ResNet-50 stride-2 3x3 of layer2..4, ResNet-18 layer2[0].conv1, the decoder's first 3x3 on the 1/32 map (K 18432)
TAPS_FULL = [(5, 120, 160, 128, 128, 3, 2, 1, True, False, "bn"), (5, 60, 80, 256, 256, 3, 2, 1, True, False, "bn"),
             (5, 30, 40, 512, 512, 3, 2, 1, True, False, "bn"), (5, 120, 160, 64, 128, 3, 2, 1, True, False, "bn"),
             (5, 15, 20, 2048, 256, 3, 1, 1, True, False, "bn")]
# 32-bit limits over the whole batch (64 -> 64): one pixel (1x1) / one image row (taps) short of 0x7fffff00 bytes, and at / above it
C1X1_BELOW, C1X1_AT = (3, 1366, 2047, 64, 64, 1, True, True, "bn"), (1, 47, 178481, 64, 64, 1, True, False, "bn")
TAPS_BELOW, TAPS_ABOVE = (4, 44619, 47, 64, 64, 3, 1, 1, True, False, "bn"), (4, 44621, 47, 64, 64, 3, 1, 1, True, False, "bn")

C1X1_CFGS = sorted(C1X1_LDS) + sorted(DIRECT)
TAPS_CFGS = sorted(DIRECT)


def _c1(cid, shapes, **kw):
    return [K("%s-%d" % (cid, i), "c1x1", None, [s[:5]], stride=s[5], relu=s[6], res=s[7], affine=s[8], **kw) for i, s in enumerate(shapes)]


def _tp(cid, shapes, **kw):
    return [K("%s-%d" % (cid, i), "taps", "taps", [s[:5]], k=s[5], stride=s[6], pad=s[7], relu=s[8], res=s[9], affine=s[10], **kw)
            for i, s in enumerate(shapes)]


IMG_EDGE = [(1, 1, 1), (2, 7, 15), (1, 16, 31), (3, 17, 33), (1, 31, 32)]   # stride 2: 1, 4 x 8, 8 x 16, 9 x 17, 16 x 16 outputs
OTHER_CASES = (
    _c1("full-conv1x1", C1X1_FULL) + _tp("full-taps", TAPS_FULL) + [
        K("stem7x7-edges", "stem7", "stem7x7", IMG_EDGE, kern="stem7x7s2_nhwc_kernel"),
        K("full-stem7x7", "stem7", "stem7x7", [(5, 480, 640)], kern="stem7x7s2_nhwc_kernel"),
        K("big-stem7x7", "stem7", "stem7x7", [(110, 480, 640)], kern="stem7x7s2_nhwc_kernel"),
        K("stem3x3-edges", "stem3", "stem3x3", IMG_EDGE, kern="stem3x3s2_nhwc_kernel"),
        K("full-stem3x3", "stem3", "stem3x3", [(5, 480, 640)], kern="stem3x3s2_nhwc_kernel"),
        # conv2d_small: (CIN, KS, STRIDE, NTW); NTW 1 where cout % 32 != 0 or cin > 64; rows 8 on the large maps, fewer on the small ones
        K("small-32-3-2-2", "small", "small", MAP_EDGE + [(5, 240, 320)], cin=32, cout=32, k=3, stride=2, kern="conv2d_small_kernel<32, 3, 2, 2>"),
        K("small-32-3-2-1", "small", "small", MAP_EDGE + [(5, 480, 640)], cin=32, cout=48, k=3, stride=2, kern="conv2d_small_kernel<32, 3, 2, 1>"),
        K("small-32-1-2-2", "small", "small", MAP_EDGE + [(5, 480, 640)], cin=32, cout=64, k=1, stride=2, kern="conv2d_small_kernel<32, 1, 2, 2>"),
        K("small-32-1-2-1", "small", "small", MAP_EDGE, cin=32, cout=16, k=1, stride=2, kern="conv2d_small_kernel<32, 1, 2, 1>"),
        K("small-32-1-1-2", "small", "small", MAP_EDGE + [(5, 240, 320)], cin=32, cout=128, k=1, stride=1, kern="conv2d_small_kernel<32, 1, 1, 2>"),
        K("small-32-1-1-1", "small", "small", MAP_EDGE, cin=32, cout=16, k=1, stride=1, relu=False, kern="conv2d_small_kernel<32, 1, 1, 1>"),
        K("small-64-1-1-2", "small", "small", MAP_EDGE + [(5, 240, 320)], cin=64, cout=128, k=1, stride=1, kern="conv2d_small_kernel<64, 1, 1, 2>"),
        K("small-64-1-1-1", "small", "small", MAP_EDGE, cin=64, cout=48, k=1, stride=1, kern="conv2d_small_kernel<64, 1, 1, 1>"),
        K("small-128-1-1-1", "small", "small", MAP_EDGE + [(5, 120, 160)], cin=128, cout=32, k=1, stride=1, relu=False,
          kern="conv2d_small_kernel<128, 1, 1, 1>"),
    ] + [K("to16-%d-%s" % (c, up), "to16", "to16", MAP_EDGE + [(5, 120, 160)], cin=c, up=up, kern="conv2d_k3_to16_kernel<%d, %s>" % (c, str(up).lower()))
         for c in (16, 32) for up in (False, True)] + [
        K("big-to16-32-up", "to16", "to16", [(110, 240, 320)], cin=32, up=True, kern="conv2d_k3_to16_kernel<32, true>"),
    ] + [K("disp-%d-x%d" % (c, up), "disp", "disp_head", MAP_EDGE + [(5, 240, 320)], cin=c, up=up, kern="disp_head_nhwc_kernel<%d>" % c)
         for c in (16, 32) for up in (1, 2)] + [
        # 32-bit limits of the whole-batch descriptors
        K("limit-conv1x1-below", "c1x1", "conv1x1", [C1X1_BELOW[:5]], stride=1, relu=True, res=True, affine="bn"),
        K("limit-taps-below", "taps", "taps", [TAPS_BELOW[:5]], k=3, stride=1, pad=1, relu=True, res=False, affine="bn"),
    ])
BIG_IDS = ("big-", "limit-")


# ---------------------------------------------------------------------------------------------------------------------- the families
def _bn(n, g):
    bn = torch.nn.BatchNorm2d(n).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(n, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(n, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(n, generator=g) + 0.5)
    return bn


def _affine(kind, cout, g):
    if kind == "bn":
        from estdepth_amd import packing
        return packing.fold_bn_fp32(_bn(cout, g), list(range(cout)))
    if kind == "bias":
        return None, torch.randn(cout, generator=g) * 0.3
    return None, None


def _dev(t):
    return t.to(DEV) if t is not None else None


def _rand_dev(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g)


def _make(case, shape, seed):
    """-> dict(x, res (or None), out_shape, args for the op / raw call / reference)"""
    from estdepth_amd import ops, packing
    g = torch.Generator().manual_seed(seed)
    fam = case["fam"]
    N, H, W = shape[:3]
    m = dict()
    if fam == "plan":
        cin, cout, dil = case["cin"], case["cout"], case["dil"]
        conv = torch.nn.Conv2d(cin, cout, 3, padding=dil, dilation=dil, bias=False)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9.0 * cin))
        bn = _bn(cout, g)
        m["plan"] = ops.Conv2dPlan(conv.to(DEV), bn.to(DEV), relu_before=case.get("rb", False), relu_after=case.get("ra", False))
        sc, sh = packing.fold_bn_fp32(bn, list(range(cout)))
        m.update(w=conv.weight.detach().cpu(), sc=sc, sh=sh, x_shape=(N, H, W, cin), out_shape=(N, H, W, cout))
        m["ref_kw"] = dict(pad=dil, dilation=dil, relu_before=case.get("rb", False), relu_after=case.get("ra", False))
    elif fam in ("c1x1", "taps"):
        cin, cout = shape[3], shape[4]
        k = 1 if fam == "c1x1" else case["k"]
        pad = 0 if fam == "c1x1" else case["pad"]
        w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(k * k * cin)
        sc, sh = _affine(case["affine"], cout, g)
        Ho, Wo = R.out_size(H, W, k, case["stride"], pad)
        m.update(w=w, sc=sc, sh=sh, x_shape=(N, H, W, cin), out_shape=(N, Ho, Wo, cout))
        m["wd"] = _dev(w.reshape(cout, cin).contiguous() if fam == "c1x1" else packing.pack_conv2d_taps(w))
        m["ref_kw"] = dict(stride=case["stride"], pad=pad, relu_after=case["relu"])
    elif fam in ("stem7", "stem3"):
        k, cout, pad = (7, 64, 3) if fam == "stem7" else (3, 32, 1)
        w = torch.randn(cout, 3, k, k, generator=g) / np.sqrt(3.0 * k * k)
        sc, sh = packing.fold_bn_fp32(_bn(cout, g), list(range(cout)))
        m.update(w=w, sc=sc, sh=sh, x_shape=(N, H, W, 3), out_shape=(N,) + R.out_size(H, W, k, 2, pad) + (cout,))
        m["wd"] = _dev(packing.pack_stem7x7(w) if fam == "stem7" else w.contiguous())
        m["ref_kw"] = dict(stride=2, pad=pad, relu_after=True)
    elif fam == "small":
        cin, cout, k, s = case["cin"], case["cout"], case["k"], case["stride"]
        w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(k * k * cin)
        sc, sh = packing.fold_bn_fp32(_bn(cout, g), list(range(cout)))
        m.update(w=w, sc=sc, sh=sh, x_shape=(N, H, W, cin), out_shape=(N,) + R.out_size(H, W, k, s, k // 2) + (cout,))
        m["wd"] = _dev(packing.pack_conv2d_small(w))
        m["ref_kw"] = dict(stride=s, pad=k // 2, relu_after=case.get("relu", True))
    elif fam == "to16":
        cin, u = case["cin"], 2 if case["up"] else 1
        w = torch.randn(16, cin, 3, 3, generator=g) / np.sqrt(9.0 * cin)
        sc, sh = packing.fold_bn_fp32(_bn(16, g), list(range(16)))
        m.update(w=w, sc=sc, sh=sh, x_shape=(N, H, W, cin), out_shape=(N, u * H, u * W, 16))
        m["wd"] = _dev(packing.pack_conv2d_to16(w))
        m["ref_kw"] = dict(pad=1, relu_after=True, upsample=case["up"])
    elif fam == "disp":
        cin, u = case["cin"], case["up"]
        w = torch.randn(1, cin, 3, 3, generator=g) / np.sqrt(9.0 * cin) * 3.0
        m.update(w=w, b=torch.randn(1, generator=g), dm=10.0, x_shape=(N, H, W, cin), out_shape=(N, 1, u * H, u * W))
        m["wd"], m["bd"] = _dev(w.contiguous()), _dev(m["b"])
    m["scd"], m["shd"] = _dev(m.get("sc")), _dev(m.get("sh"))
    m["x"] = _rand_dev(m["x_shape"], seed + 1)
    m["res"] = _rand_dev(m["out_shape"], seed + 2) if case.get("res") else None
    return m


def _op(case, m, x, res):
    """the case's op through the public front end (ops.*) under the current binding"""
    from estdepth_amd import ops
    fam = case["fam"]
    if fam == "plan":
        return m["plan"].run(x, res)
    if fam == "c1x1":
        return ops.conv1x1_nhwc(x, m["wd"], m["scd"], m["shd"], case["stride"], case["relu"], res)
    if fam == "taps":
        return ops.conv2d_taps_nhwc(x, m["wd"], m["scd"], m["shd"], case["k"], case["stride"], case["pad"], case["relu"], res)
    if fam == "stem7":
        return ops.stem7x7s2_nhwc(x, m["wd"], m["scd"], m["shd"])
    if fam == "stem3":
        return ops.stem3x3s2_nhwc(x, m["wd"], m["scd"], m["shd"])
    if fam == "small":
        return ops.conv2d_small_nhwc(x, m["wd"], m["scd"], m["shd"], case["cout"], case["k"], case["stride"], case.get("relu", True))
    if fam == "to16":
        return ops.conv2d_k3_to16_nhwc(x, m["wd"], m["scd"], m["shd"], case["up"])
    return ops.disp_head_nhwc(x, m["wd"], m["bd"], m["dm"], case["up"])


def _raw(case, m, x, res, out):
    """the same launch through the C ABI directly, on caller-provided (guarded) buffers -> estd_status"""
    import ctypes
    from estdepth_amd import _native as NV
    lib, st = NV.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    fam = case["fam"]
    N, H, W = m["x_shape"][:3]
    if fam == "plan":
        plan, kern = m["plan"], case["kern"]
        d = NV.Conv2dDesc()
        d.N, d.H, d.W, d.cin, d.cout, d.dilation = N, H, W, plan.cin, plan.cout, plan.dil
        nt = plan.route(N, H, W)[1]
        d.group_tiles = nt
        d.in_, d.scale, d.shift, d.out = x.data_ptr(), plan.scale.data_ptr(), plan.shift.data_ptr(), out.data_ptr()
        d.relu_before_residual, d.relu_after_residual = plan.relu_before, plan.relu_after
        d.residual = res.data_ptr() if res is not None else None
        if kern.startswith("conv2d_wino2_kernel"):
            d.w_wino = plan.w_wino2.data_ptr()
            return lib.estd_conv2d_k3_wino2(ctypes.byref(d), st)
        if kern.startswith("conv2d_wino_kernel"):
            d.w_wino = getattr(plan, "w_wino_nt%d" % nt).data_ptr()
            return lib.estd_conv2d_k3_wino(ctypes.byref(d), st)
        d.w = getattr(plan, "w_nt%d" % nt).data_ptr()
        if kern.startswith("conv2d_k3_split_kernel"):
            d.w_split = plan.w_split.data_ptr()
            return lib.estd_conv2d_k3_split(ctypes.byref(d), st)
        return lib.estd_conv2d_k3(ctypes.byref(d), st)
    if fam in ("c1x1", "taps"):
        d = NV.Conv1x1Desc() if fam == "c1x1" else NV.Conv2dTapsDesc()
        d.N, d.H, d.W, d.cin, d.cout, d.stride, d.relu = N, H, W, m["x_shape"][3], m["out_shape"][3], case["stride"], int(case["relu"])
        if fam == "taps":
            d.ksize, d.pad = case["k"], case["pad"]
        d.in_, d.w, d.out = x.data_ptr(), m["wd"].data_ptr(), out.data_ptr()
        d.scale = m["scd"].data_ptr() if m["scd"] is not None else None
        d.shift = m["shd"].data_ptr() if m["shd"] is not None else None
        d.residual = res.data_ptr() if res is not None else None
        return (lib.estd_conv1x1_nhwc if fam == "c1x1" else lib.estd_conv2d_taps_nhwc)(ctypes.byref(d), st)
    if fam in ("stem7", "stem3"):
        fn = lib.estd_stem7x7s2_nhwc if fam == "stem7" else lib.estd_stem3x3s2_nhwc
        return fn(p(x), p(m["wd"]), p(m["scd"]), p(m["shd"]), p(out), N, H, W, st)
    if fam == "small":
        return lib.estd_conv2d_small_nhwc(p(x), p(m["wd"]), p(m["scd"]), p(m["shd"]), p(out), N, H, W, case["cin"], case["cout"], case["k"],
                                          case["stride"], int(case.get("relu", True)), st)
    if fam == "to16":
        u = 2 if case["up"] else 1
        return lib.estd_conv2d_k3_to16_nhwc(p(x), p(m["wd"]), p(m["scd"]), p(m["shd"]), p(out), N, u * H, u * W, case["cin"], int(case["up"]), st)
    return lib.estd_disp_head_nhwc(p(x), p(m["wd"]), p(m["bd"]), float(m["dm"]), p(out), N, H, W, case["cin"], case["up"], st)


def _ref(case, m, x, res, points):
    if case["fam"] == "disp":
        return R.disp_head_ref(x, m["w"], m["b"], m["dm"], case["up"], points=points)
    return R.conv2d_ref(x, m["w"], m.get("sc"), m.get("sh"), residual=res, points=points, **m["ref_kw"])


# ------------------------------------------------------------------------------------------------------------------ guard bands
SENT32 = 0x7FC0DEAD                    # a quiet-NaN payload no kernel computes
BAND = 4096                            # sentinel elements before and after each tensor (16 KiB: several whole tiles of records)


def _guarded(shape, fill=None):
    """a contiguous view of `shape` inside a buffer filled with the sentinel -> (buffer, view, (lo, hi))"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BAND,), SENT32, dtype=torch.int32, device=DEV).view(torch.float32)
    view = buf[BAND:BAND + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view, (BAND, BAND + n)


def _untouched(buf, lo, hi):
    b = buf.view(torch.int32)
    return int((b[:lo] != SENT32).sum()) + int((b[hi:] != SENT32).sum())


class _Switches:
    KEYS = ("CONV2D_ALGO", "CONV2D_NT", "C2W2_DIL2", "CONV2D_ARITH", "BINDING")

    def __init__(self, sw, binding):
        self.sw = dict(sw or {}, BINDING=binding)

    def __enter__(self):
        from estdepth_amd import ops
        self.old = {k: getattr(ops, k) for k in self.KEYS}
        for k, v in self.sw.items():
            setattr(ops, k, v)

    def __exit__(self, *exc):
        from estdepth_amd import ops
        for k, v in self.old.items():
            setattr(ops, k, v)
        return False


KERNEL_RE = re.compile(r"\b(conv1x1_\w+_kernel|conv2d_\w+_kernel|stem\w+_kernel|disp_head_nhwc_kernel)(<[^>()]*>)?")


def _sample_points(N, Ho, Wo, g, n=2000):
    """n random output pixels + the last image's last row and last column (up to 512 pixels each) + its four corners, as (n, y, x)"""
    rnd = torch.stack([torch.randint(0, s, (n,), generator=g) for s in (N, Ho, Wo)], 1)
    ys, xs = torch.arange(max(0, Ho - 512), Ho), torch.arange(max(0, Wo - 512), Wo)
    row = torch.stack([torch.full_like(xs, N - 1), torch.full_like(xs, Ho - 1), xs], 1)
    col = torch.stack([torch.full_like(ys, N - 1), ys, torch.full_like(ys, Wo - 1)], 1)
    corners = torch.tensor([[N - 1, y, x] for y in (0, Ho - 1) for x in (0, Wo - 1)])
    return torch.cat([rnd, row, col, corners])


def _expected_kernel(case, shape):
    if case.get("kern"):
        from estdepth_amd import _native
        return case["kern_ab"] if case.get("kern_ab") and _native.has_ab() else case["kern"]
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    N, H, W, cin, cout = shape
    if case["fam"] == "c1x1":
        return c1x1_kernel(int(os.environ.get("ESTD_C1X1_CFG", "0")), int(os.environ.get("ESTD_C1X1_LDS", "1")), N, H, W, cin, cout,
                           case["stride"], cus)
    return taps_kernel(int(os.environ.get("ESTD_CTAPS_CFG", "0")), N, H, W, cin, cout, case["k"], case["stride"], case["pad"], cus)


def _three_runs(case, m, want, what):
    """steps 1-3 of a case on one shape -> the op's output, the kernel instances that ran"""
    # 1. the torch binding, under the profiler
    with _Switches(case.get("sw"), "torch"):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            out_t = _op(case, m, m["x"], m["res"])
            torch.cuda.synchronize()
    ran = {mm.group(1) + (mm.group(2) or "") for e in prof.key_averages() for mm in [KERNEL_RE.search(e.key)] if mm}
    assert ran == {want}, "%s: ran %s, expected %s" % (what, sorted(ran), want)
    assert tuple(out_t.shape) == tuple(m["out_shape"]), (what, tuple(out_t.shape))
    # 2. the ctypes binding: bit-identical
    with _Switches(case.get("sw"), "ctypes"):
        out_c = _op(case, m, m["x"], m["res"])
        torch.cuda.synchronize()
    assert torch.equal(out_t.view(torch.int32), out_c.view(torch.int32)), "%s: the bindings differ" % what
    del out_c
    # 3. the C ABI on guarded buffers: nothing written outside the output, nothing read outside the input / residual
    xb, xg, _ = _guarded(m["x_shape"], m["x"])
    rg = _guarded(m["out_shape"], m["res"])[1] if m["res"] is not None else None
    ob, og, (lo, hi) = _guarded(m["out_shape"])
    with _Switches(case.get("sw"), "ctypes"):
        status = _raw(case, m, xg, rg, og)
        torch.cuda.synchronize()
    assert status == 0, "%s: estd status %d" % (what, status)
    assert _untouched(ob, lo, hi) == 0, "%s: written outside the output" % what
    assert torch.equal(og.view(torch.int32), out_t.view(torch.int32)), "%s: the guarded launch differs from the op" % what
    return out_t, ran


def run_case(case, shapes=None, reserves=(None,)):
    """all shapes of one case -> (worst ratio, the kernel instances that ran).  ``reserves``: run steps 1-3 once per
    ops.set_reserved_cus value (None: the setting as it is); the outputs of all of them must be bit-identical."""
    from estdepth_amd import ops
    worst, seen = 0.0, set()
    seed = sum(map(ord, case["id"]))
    big = case["id"].startswith(BIG_IDS) or case["id"].startswith("full-")
    for shape in case["shapes"] if shapes is None else shapes:
        shape = tuple(shape)
        m = _make(case, shape, seed + sum(shape))
        want = _expected_kernel(case, shape)
        what = "%s %s" % (case["id"], shape)
        out_t = None
        prev = ops.get_reserved_cus()
        try:
            for r in reserves:
                if r is not None:
                    assert ops.set_reserved_cus(r) == r
                out_r, ran = _three_runs(case, m, want, what if r is None else "%s reserve %d" % (what, r))
                seen |= ran
                if out_t is None:
                    out_t = out_r
                else:
                    assert torch.equal(out_t.view(torch.int32), out_r.view(torch.int32)), "%s: reserve %s changes the result" % (what, r)
                del out_r
        finally:
            ops.set_reserved_cus(prev)
        # 4. the fp64 reference
        os_ = m["out_shape"]
        points = _sample_points(os_[0], *(os_[2:] if case["fam"] == "disp" else os_[1:3]), torch.Generator().manual_seed(seed)) if big else None
        ref, A = _ref(case, m, m["x"], m["res"], points)
        if points is None:
            got = out_t
        elif case["fam"] == "disp":
            pd = points.to(DEV)
            got = out_t[pd[:, 0], 0, pd[:, 1], pd[:, 2]]
        else:
            pd = points.to(DEV)
            got = out_t[pd[:, 0], pd[:, 1], pd[:, 2]]
        worst = max(worst, R.check_bound(got, ref, A, C_ROUTE[_route(want)], what))
        del m, out_t, got, ref, A
        torch.cuda.empty_cache()
    return worst, sorted(seen)


ROUTES = (("conv2d_wino2_kernel", "wino2"), ("conv2d_wino_kernel", "wino"), ("conv2d_k3_split_kernel", "k3_split"), ("conv2d_k3_kernel", "k3"),
          ("conv1x1_lds_kernel", "conv1x1_lds"), ("conv1x1_nhwc_kernel", "conv1x1"), ("conv2d_taps_kernel", "taps"), ("stem7x7", "stem7x7"),
          ("stem3x3", "stem3x3"), ("conv2d_small_kernel", "small"), ("conv2d_k3_to16_kernel", "to16"), ("disp_head", "disp_head"))


def _route(kern):
    """the C_ROUTE entry of a kernel instance"""
    return next(r for prefix, r in ROUTES if kern.startswith(prefix))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


@pytest.mark.parametrize("case", PLAN_CASES + OTHER_CASES, ids=lambda c: c["id"])
def test_conv2d_route_against_fp64(case):
    from estdepth_amd import _native
    if case.get("ab") and not _native.has_ab():
        pytest.skip("ESTD_BUILD_AB=1 kernels are not in this build")
    ratio, kernels = run_case(case)
    print("ROUTE-RATIO %s %s %.3f %s" % (_route(kernels[0]), case["id"], ratio, " ".join(kernels)))


@pytest.mark.parametrize("case", [c for c in PLAN_CASES if "many" in c] + RANGE_CASES, ids=lambda c: c["id"])
def test_conv2d_plan_over_multi_item_ranges(case):
    """every instance of conv2d_wino2 / conv2d_k3 on its many-item shape, all elements against the fp64 reference, under the full grid and
    under set_reserved_cus(128): the same protocol per grid, and the two grids bit-identical"""
    import tile_ranges_ref as TR
    shape = (case["many"],) + MANY_HW
    ratio, kernels = run_case(case, shapes=[shape], reserves=TR.RESERVES)
    print("ROUTE-RATIO %s %s-ranges %.3f %s" % (_route(kernels[0]), case["id"], ratio, " ".join(kernels)))
    if kernels[0].startswith(("conv2d_wino2_kernel", "conv2d_k3_kernel")):      # (ESTD_BUILD_AB=1: conv2d_wino_kernel takes plan-k3-nt2-d2-res)
        cus = torch.cuda.get_device_properties(DEV).multi_processor_count
        fam = TR.family2d(kernels[0], case["cout"])
        counts = [TR.classes2d(fam, shape, case["cout"], cus, r) for r in TR.RESERVES]
        print("TILE-RANGES %s %s" % (case["id"], " | ".join("G=%d len %d-%d same=%d image=%d group=%d" % (
            c["G"], c["len_min"], c["len_max"], c["same_image"], c["next_image"], c["next_group"]) for c in counts)))


# ------------------------------------------------------------------------------------------- forced configurations (child processes)
def _child(env, cases):
    """run `cases` in a fresh process with `env` (the latched switches) -> {case id: (ratio, kernels)}; failures are reported per case"""
    code = ("import json, sys, traceback\n"
            "sys.path.insert(0, 'tests')\n"
            "import test_gpu_conv2d_routes as T\n"
            "for c in json.loads(sys.argv[1]):\n"
            "    try:\n"
            "        r, k = T.run_case(c)\n"
            "        print('CASE ' + json.dumps([c['id'], r, k]), flush=True)\n"
            "    except Exception:\n"
            "        print('FAIL ' + json.dumps([c['id'], traceback.format_exc()[-1500:]]), flush=True)\n")
    r = subprocess.run([sys.executable, "-c", code, json.dumps(cases)], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    if r.returncode < 0 or r.returncode in (134, 139):          # a crashed GPU process: start nothing more on this device
        pytest.exit("child %s ended with status %d:\n%s" % (env, r.returncode, r.stderr[-3000:]), returncode=1)
    got, fails = {}, []
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            cid, ratio, kern = json.loads(line[5:])
            got[cid] = (ratio, kern)
        elif line.startswith("FAIL "):
            fails.append(json.loads(line[5:]))
    assert r.returncode == 0, (env, r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert not fails, "%s: %s" % (env, "\n".join("%s: %s" % f for f in fails))
    assert sorted(got) == sorted(c["id"] for c in cases), (env, sorted(got))
    return got


@pytest.mark.parametrize("cfg", C1X1_CFGS + ["lds0"])
def test_conv1x1_forced_configuration(cfg):
    """every instance of estd_conv1x1_nhwc (ESTD_C1X1_CFG; "lds0": ESTD_C1X1_LDS=0, the direct form's heuristic on the full-size layers)
    on the tile-edge shapes, the fall-backs of the forced configuration included (asserted instance by instance)"""
    if cfg == "lds0":
        env, cases = dict(ESTD_C1X1_LDS="0"), _c1("full-lds0", C1X1_FULL)
    else:
        env, cases = dict(ESTD_C1X1_CFG=str(cfg)), _c1("c1x1-%d" % cfg, C1X1_EDGE)
    got = _child(env, cases)
    kerns = sorted({k for _, ks in got.values() for k in ks})
    if cfg != "lds0":
        forced = _inst("conv1x1_lds_kernel", C1X1_LDS[cfg]) if cfg in C1X1_LDS else _inst("conv1x1_nhwc_kernel", DIRECT[cfg])
        assert forced in kerns, (cfg, kerns)
    for cid, (ratio, ks) in sorted(got.items()):
        print("ROUTE-RATIO %s %s %.3f %s" % (_route(ks[0]), cid, ratio, " ".join(ks)))


@pytest.mark.parametrize("cfg", TAPS_CFGS)
def test_conv2d_taps_forced_configuration(cfg):
    """every instance of estd_conv2d_taps_nhwc (ESTD_CTAPS_CFG) x k 1 / 3 / 5 x stride 1 / 2 x pad 0 / k // 2 at the tile edges"""
    got = _child(dict(ESTD_CTAPS_CFG=str(cfg)), _tp("taps-%d" % cfg, TAPS_EDGE))
    kerns = sorted({k for _, ks in got.values() for k in ks})
    assert _inst("conv2d_taps_kernel", DIRECT[cfg]) in kerns, (cfg, kerns)
    for cid, (ratio, ks) in sorted(got.items()):
        print("ROUTE-RATIO taps %s %.3f %s" % (cid, ratio, " ".join(ks)))


# -------------------------------------------------------------------------------------------------------------- limits and arguments
@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_whole_batch_descriptors_refuse_past_the_32bit_limit(binding):
    """conv1x1 / taps address the whole batch through one 32-bit buffer descriptor: at / past 0x7fffff00 bytes they refuse (no launch)"""
    from estdepth_amd import ops
    with _Switches(None, binding):
        for fam, s in (("c1x1", C1X1_AT), ("taps", TAPS_ABOVE)):
            N, H, W, cin, cout = s[:5]
            x = torch.empty(N, H, W, cin, device=DEV)
            w = torch.zeros(cout, cin, device=DEV) if fam == "c1x1" else torch.zeros(9, cout, cin, device=DEV)
            with pytest.raises(RuntimeError, match=r"estd_status -3\)"):
                if fam == "c1x1":
                    ops.conv1x1_nhwc(x, w, None, None)
                else:
                    ops.conv2d_taps_nhwc(x, w, None, None, 3)
            del x
            torch.cuda.empty_cache()


def _malformed():
    """(name, call) pairs with one wrong-sized argument each"""
    from estdepth_amd import ops, packing
    x32, x64 = torch.randn(1, 8, 8, 32, device=DEV), torch.randn(1, 8, 8, 64, device=DEV)
    v = lambda n: torch.ones(n, device=DEV)                                    # noqa: E731
    w1 = torch.randn(64, 32, device=DEV)
    wt = packing.pack_conv2d_taps(torch.randn(64, 32, 3, 3)).to(DEV)
    ws = packing.pack_conv2d_small(torch.randn(64, 32, 1, 1)).to(DEV)
    return [
        ("conv1x1 w cin", lambda: ops.conv1x1_nhwc(x64, w1, v(64), v(64))),
        ("conv1x1 short scale", lambda: ops.conv1x1_nhwc(x32, w1, v(32), v(64))),
        ("conv1x1 short shift", lambda: ops.conv1x1_nhwc(x32, w1, None, v(32))),
        ("conv1x1 residual", lambda: ops.conv1x1_nhwc(x32, w1, v(64), v(64), residual=torch.zeros(1, 8, 8, 32, device=DEV))),
        ("taps w cin", lambda: ops.conv2d_taps_nhwc(x64, wt, v(64), v(64), 3)),
        ("taps short scale", lambda: ops.conv2d_taps_nhwc(x32, wt, v(32), v(64), 3)),
        ("taps short shift", lambda: ops.conv2d_taps_nhwc(x32, wt, None, v(16), 3)),
        ("taps residual", lambda: ops.conv2d_taps_nhwc(x32, wt, v(64), v(64), 3, residual=torch.zeros(1, 4, 4, 64, device=DEV))),
        ("small packed size", lambda: ops.conv2d_small_nhwc(x32, ws[:2].contiguous(), v(64), v(64), 64, 1, 1, True)),
        ("small packed cin", lambda: ops.conv2d_small_nhwc(x64, ws, v(64), v(64), 64, 1, 1, True)),
        ("small short scale", lambda: ops.conv2d_small_nhwc(x32, ws, v(32), v(64), 64, 1, 1, True)),
        ("small short shift", lambda: ops.conv2d_small_nhwc(x32, ws, v(64), v(48), 64, 1, 1, True)),
    ]


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_arguments_raise_before_any_launch(binding):
    """the ctypes front end checks what the torch binding checks: weight shape / packed size, scale / shift sizes, residual shape -- and
    raises before anything is launched"""
    for name, call in _malformed():
        with _Switches(None, binding):
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                with pytest.raises(RuntimeError):
                    call()
                torch.cuda.synchronize()
        ran = [e.key for e in prof.key_averages() if KERNEL_RE.search(e.key)]
        assert not ran, "%s / %s launched %s" % (binding, name, ran)
