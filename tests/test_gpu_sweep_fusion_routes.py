"""Every kernel instance of csrc/plane_sweep.hip and csrc/est_fusion.hip (stage B of a step: the cost volume, the EST fusion, the ConvGRU
elementwise stages, soft-argmin) against the fp64 reference of tests/sweep_fusion_ref.py.

A route is one kernel instance.  Each case
  * asserts WHICH instance ran, template arguments included (torch.profiler's demangled names); the instances of
    homo_warp_costvol / warp_attention / gru_* are predicted by Python copies of their dispatchers (``costvol_kernel``, ``wa_kernel``,
    ``gru_kernel``) from the source count, the 2 GiB test, H % 8 and the switches;
  * compares every output element (every sampled voxel at full size) with the reference:
    |gpu - ref| <= C_ROUTE[route] * 2^-24 * A + pos (pos: the position tolerance of a sample times the texel differences around it), an
    ambiguous sample (within its tolerance of a mask edge) passing on either side of the mask; at most 1e-3 of the samples may be ambiguous
    (one in a case of fewer than 1000 samples);
  * runs the op under both bindings and once more through the C ABI directly, with every input and output carved out of buffers filled
    with a NaN sentinel: the three results are bit-identical and nothing outside the written region changes -- for gru_blend
    (out_stride = 32) and cdhw_to_vol (dst_off 0 / 16) that includes the other half of every record.
ESTD_WA_BUF, ESTD_WA_OCC and ESTD_GRU_FAST are latched at the first call: those cases run in child processes, one at a time.
ESTD_SWEEP_LINEAR is read at every call."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sweep_fusion_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMB_CAP = 1e-3                  # ambiguous samples per case: at most this share of the samples (one in a case of fewer than 1000)

# per-element bound constants, in units of 2^-24 A: at least 3 x the worst ratio measured on an MI355X over every case of the route
# (in the comments).  0.000: the position term covers every difference of the route's cases.
C_ROUTE = {
    "homo_warping": 3.0,          # measured 0.948 (sweep-ident)
    "mix1x1": 14.0,               # measured 4.511 (mix-64-64)
    "costvol": 3.0,               # measured 0.992 (costvol-ident)
    "warp_volume": 5.0,           # measured 1.345 (wvol-ident)
    "warp_volume_ex": 1.0,        # measured 0.000
    "warp_attention": 2.0,        # measured 0.530 (every NS / BUF instance, the 2 GiB cases and the full-size volumes included)
    "attention_prewarped": 2.0,   # measured 0.360 (pre-n16)
    "groupnorm_finalize": 3.0,    # measured 0.971 (gn-1023)
    "gru_reset": 7.0,             # measured 2.320 (full-reset-cfg2)
    "gru_blend": 4.0,             # measured 1.029 (full-blend-cfg5); FAST instances 0.783
    "softargmin": 2.0,            # measured 0.387
    "cam": 3.0,                   # measured 0.798
    "layout": 0.0,                # exact copies
}

# ---------------------------------------------------------------------------------------------------------------- expected instances
WA_NS = (2, 3, 4, 8, 16)
INSTANCES = {
    # route: the kernel instances of csrc/plane_sweep.hip and csrc/est_fusion.hip that reach it
    "cam": ["cam_pair_proj_kernel", "cam_sweep_proj_kernel", "cam_volume_mats_kernel"],
    "homo_warping": ["homo_warping_kernel"],
    "mix1x1": ["mix1x1_kernel"],
    "costvol": ["homo_warp_costvol_kernel<true>", "homo_warp_costvol_kernel<false>"],
    "warp_volume": ["warp_volume_kernel"],
    "warp_volume_ex": ["warp_volume_ex_kernel"],
    "warp_attention": ["warp_attention_kernel<%d, %s>" % (ns, b) for ns in WA_NS for b in ("true", "false")],
    "attention_prewarped": ["attention_prewarped_kernel"],
    "groupnorm_finalize": ["groupnorm_finalize_kernel"],
    "gru_reset": ["gru_reset_kernel<true>", "gru_reset_kernel<false>"],
    "gru_blend": ["gru_blend_kernel<true>", "gru_blend_kernel<false>"],
    "softargmin": ["softargmin_up_kernel"],
    "layout": ["cdhw_to_vol_kernel", "vol_to_cdhw_kernel"],
}
# kernels of the two files that are no routes of any suite (the 2D glue kernels that share est_fusion.hip -- bn_act_nhwc_kernel,
# spp_upsample_cat_kernel -- are routes of tests/test_gpu_glue2d_routes.py)
NOT_ROUTES = {
    "estd_mark_kernel": "profiler marker (estd_profile_mark), computes nothing",
}
KERNEL_RE = re.compile(r"\b(cam_\w+_kernel|homo_warp\w*_kernel|mix1x1_kernel|warp_\w+_kernel|attention_prewarped_kernel|groupnorm_finalize_kernel|"
                       r"gru_\w+_kernel|softargmin_up_kernel|cdhw_to_vol_kernel|vol_to_cdhw_kernel)(<[^>()]*>)?")


def costvol_kernel(H, linear):
    """the instance estd_homo_warp_costvol launches"""
    return "homo_warp_costvol_kernel<%s>" % ("true" if H % 8 == 0 and not linear else "false")


def wa_kernel(n_src, D, H, W, buf_env=-1):
    """the instance estd_warp_attention launches (ESTD_WA_BUF = buf_env, -1 unset)"""
    buf = (buf_env != 0 if buf_env >= 0 else n_src == 3) and D * H * W * 128 < 0x7FFFFFFF
    ns = n_src if n_src in (2, 3, 4) else (8 if n_src <= 8 else 16)
    return "warp_attention_kernel<%d, %s>" % (ns, "true" if buf else "false")


def gru_kernel(which, fast):
    return "gru_%s_kernel<%s>" % (which, "true" if fast else "false")


def _env_int(name, default):
    v = os.environ.get(name)
    return int(v) if v is not None else default


# ---------------------------------------------------------------------------------------------------------------------- geometry
def _K(H, W):
    from estdepth_amd import synth
    K = synth.intrinsics(H * 4, W * 4).copy()
    K[:2] *= 0.25
    return torch.from_numpy(K)


def _pose(v, motion=1.0, tz=0.0):
    from estdepth_amd import synth
    p = synth.camera_pose(v, motion=motion).copy()
    p[2, 3] += tz
    return torch.from_numpy(p)


def _proj12(geom, D, H, W):
    """-> (proj12 [12] fp32 on the device, depth planes [D] on the device)"""
    if geom == "ident":                      # exact positions: n = +-1 exactly where x * dv = W - 1 or y * dv = H - 1
        return R.exact_sweep_proj().to(DEV), (torch.arange(D, dtype=torch.float32) % 3 + 1.0).to(DEV)
    if geom == "den0":                       # projected depth exactly -eps on every plane: x is 0 / 0 (NaN), y is +-inf
        return R.den0_sweep_proj().to(DEV), torch.linspace(0.5, 4.0, D).to(DEV)
    from estdepth_amd import ops
    motion, tz = {"small": (1.0, 0.0), "large": (6.0, 0.0), "behind": (1.0, 2.5)}[geom]
    K = _K(H, W).to(DEV)
    P = ops.cam_sweep_proj(_pose(0).to(DEV), _pose(1, motion, tz).to(DEV), K)
    return P, torch.linspace(0.5, 4.0, D).to(DEV)


def _mats(geom, n, D, H, W):
    """-> (mats [n,30] fp32 on the device, depth planes [D], depth_min, depth_interval)"""
    if geom == "ident":                      # exact positions: n = +-1 exactly on the border columns / rows, n_z = -1
        M, zmin = R.exact_volume_mats()
        return M.repeat(n, 1).to(DEV), torch.ones(D).to(DEV), zmin, 1.0
    dv = torch.linspace(0.5, 4.0, D)
    dmin, dint = 0.5, float(dv[1] - dv[0])
    if geom == "den0":                       # q2 = -eps exactly: X = 0 / 0, Y = +-inf
        return R.den0_volume_mats().repeat(n, 1).to(DEV), dv.to(DEV), dmin, dint
    from estdepth_amd import ops
    motion, tz = {"small": (0.7, 0.0), "large": (6.0, 0.0), "behind": (1.0, 2.0), "tiny": (0.05, 0.0)}[geom]
    K = _K(H, W).to(DEV)
    M = torch.stack([ops.cam_volume_mats(_pose(j + 1, motion, tz).to(DEV), _pose(0).to(DEV), K) for j in range(n)])
    return M, dv.to(DEV), dmin, dint


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def _ramp_hw(H, W, C):
    """channels 0, 1 = x + 1, y + 1 (the rest 0), [H,W,C]"""
    t = torch.zeros(H, W, C, device=DEV)
    t[..., 0] = torch.arange(W, device=DEV, dtype=torch.float32)[None, :] + 1
    t[..., 1] = torch.arange(H, device=DEV, dtype=torch.float32)[:, None] + 1
    return t


def _ramp_dhw(D, H, W, C):
    """channels 0, 1, 2 = x + 1, y + 1, z + 1, [D,H,W,C]"""
    t = torch.zeros(D, H, W, C, device=DEV)
    t[..., 0] = torch.arange(W, device=DEV, dtype=torch.float32) + 1
    t[..., 1] = (torch.arange(H, device=DEV, dtype=torch.float32) + 1)[:, None]
    t[..., 2] = (torch.arange(D, device=DEV, dtype=torch.float32) + 1)[:, None, None]
    return t


# ------------------------------------------------------------------------------------------------ closed-form volumes (2 GiB cases)
def hash_values(idx, seed):
    """element index (int64, any device) -> float32 in [-1, 1) with 24 significant bits: exact in fp32, evaluated alike on CPU / GPU"""
    h = (idx * 2654435761 + seed) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x45D9F3B) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    return ((h >> 8) - 8388608).to(torch.float32) / 8388608.0


def hash_volume(shape, seed):
    n = int(np.prod(shape))
    out = torch.empty(n, device=DEV)
    step = 1 << 26
    for s in range(0, n, step):
        e = min(n, s + step)
        out[s:e] = hash_values(torch.arange(s, e, device=DEV, dtype=torch.int64), seed)
    return out.view(*shape)


def hash_getter(seed, C=32):
    return lambda f: hash_values(f.reshape(-1, 1) * C + torch.arange(C), seed).double().reshape(*f.shape, C)


# ------------------------------------------------------------------------------------------------------------------ guard bands
SENT32 = 0x7FC0DEAD                    # a quiet-NaN payload no kernel computes
BAND = 4096


def _guarded(shape, fill=None, dtype=torch.float32):
    n = int(np.prod(shape))
    if dtype == torch.float64:
        buf = torch.full((n + 2 * BAND,), SENT32, dtype=torch.int64, device=DEV).view(torch.float64)
    else:
        buf = torch.full((n + 2 * BAND,), SENT32, dtype=torch.int32, device=DEV).view(torch.float32)
    view = buf[BAND:BAND + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _band_intact(buf):
    b = buf.view(torch.int64 if buf.dtype == torch.float64 else torch.int32)
    return bool((b[:BAND] == SENT32).all()) and bool((b[-BAND:] == SENT32).all())


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class _Binding:
    def __init__(self, binding, env=None):
        self.binding, self.env = binding, env or {}

    def __enter__(self):
        from estdepth_amd import ops
        self.old = ops.BINDING
        ops.BINDING = self.binding
        self.old_env = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        from estdepth_amd import ops
        ops.BINDING = self.old
        for k, v in self.old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


# ------------------------------------------------------------------------------------------------------------------------ cases
def K_(cid, fam, **kw):
    return dict(id=cid, fam=fam, **kw)


WA_EDGE = [(2, 4, 8), (3, 5, 9), (4, 8, 16), (5, 3, 7), (2, 2, 2), (7, 6, 13)]      # whole / partial bricks, D odd, W < 8, H < 4, minimum 2
CASES = [
    # plane sweep, level 1
    K_("sweep-small", "sweep", dims=(5, 9, 13), C=6, geom="small"),
    K_("sweep-large", "sweep", dims=(4, 11, 7), C=3, geom="large"),
    K_("sweep-behind", "sweep", dims=(6, 8, 10), C=4, geom="behind"),
    K_("sweep-ident", "sweep", dims=(3, 7, 9), C=2, geom="ident"),
    K_("sweep-den0", "sweep", dims=(3, 5, 6), C=2, geom="den0"),
    K_("sweep-px", "sweep", dims=(4, 9, 12), C=4, geom="small", px=True),
    K_("sweep-min", "sweep", dims=(1, 2, 2), C=1, geom="small"),
    K_("sweep-probe", "sweep", dims=(3, 12, 16), C=2, geom="small", probe=True),
    K_("mix-64-32", "mix", dims=(7, 9), cin=64, cout=32, bias=True),
    K_("mix-3-4", "mix", dims=(1, 1), cin=3, cout=4, bias=False),
    K_("mix-64-64", "mix", dims=(13, 21), cin=64, cout=64, bias=True),
    # fused cost volume
    K_("costvol-h8-256", "costvol", dims=(4, 8, 8), geom="small"),          # 256 voxels per plane band multiple
    K_("costvol-h8-ragged", "costvol", dims=(3, 16, 7), geom="large"),
    K_("costvol-h7", "costvol", dims=(5, 7, 9), geom="small"),
    K_("costvol-h7-256", "costvol", dims=(4, 7, 64), geom="behind"),        # 1792 = 7 x 256 voxels
    K_("costvol-ident", "costvol", dims=(3, 8, 11), geom="ident"),
    K_("costvol-den0", "costvol", dims=(2, 8, 6), geom="den0"),
    K_("costvol-linear", "costvol", dims=(5, 16, 12), geom="small", linear=True),
    K_("costvol-probe", "costvol", dims=(3, 16, 20), geom="small", probe=True),
    K_("full-costvol-cfg2", "costvol", dims=(64, 120, 160), geom="small", full=True),
    # volume warp, level 1
    K_("wvol-small", "wvol", dims=(5, 6, 9), C=5, geom="small"),
    K_("wvol-large", "wvol", dims=(4, 7, 6), C=3, geom="large"),
    K_("wvol-behind", "wvol", dims=(6, 5, 8), C=2, geom="behind"),
    K_("wvol-ident", "wvol", dims=(4, 5, 6), C=2, geom="ident"),
    K_("wvol-den0", "wvol", dims=(3, 4, 5), C=2, geom="den0"),
    K_("wvol-min", "wvol", dims=(2, 2, 2), C=3, geom="small"),
    K_("wvol-probe", "wvol", dims=(8, 9, 12), C=3, geom="tiny", probe=True),
    K_("wvolex-voxel", "wvolex", dims=(6, 7, 9), C=3, geom="small", per_voxel=True),
    K_("wvolex-border", "wvolex", dims=(5, 6, 8), C=3, geom="large", border=True, pad=0.5),
    K_("wvolex-border-voxel", "wvolex", dims=(5, 6, 7), C=2, geom="small", per_voxel=True, border=True, pad=-1.25),
    K_("wvolex-disp", "wvolex", dims=(6, 6, 8), C=2, geom="small", disp=True),
    K_("wvolex-min", "wvolex", dims=(2, 2, 2), C=2, geom="small", border=True, pad=2.0),
    # fused warp + attention: every NS instance, tile edges, geometry
] + [K_("wa-n%d-%dx%dx%d" % ((n,) + d), "wa", dims=d, n=n, geom="small") for n in (1, 2, 3, 4, 5, 9, 16) for d in WA_EDGE[:3]] + [
] + [K_("wa-n3-%dx%dx%d" % d, "wa", dims=d, n=3, geom="small") for d in WA_EDGE[3:]] + [
    K_("wa-n2-large", "wa", dims=(7, 6, 13), n=2, geom="large"),
    K_("wa-n3-behind", "wa", dims=(6, 5, 9), n=3, geom="behind"),
    K_("wa-n2-ident", "wa", dims=(4, 4, 8), n=2, geom="ident"),
    K_("wa-n3-den0", "wa", dims=(2, 4, 8), n=3, geom="den0"),
    K_("wa-n3-xcd-on", "wa", dims=(2, 8, 64), n=3, geom="small"),           # 16 bricks: grid % 8 == 0
    K_("wa-n3-xcd-off", "wa", dims=(2, 4, 56), n=3, geom="small"),          # 7 bricks
    K_("wa-n1-probe", "wa", dims=(8, 8, 16), n=1, geom="tiny", probe=True),
    K_("wa-n3-softmax-range", "wa", dims=(4, 4, 8), n=3, geom="tiny", kscale=6.0),   # |corr| up to ~ 600: expf overflows without the max
] + [K_("full-wa-cfg2-n%d" % n, "wa", dims=(64, 120, 160), n=n, geom="small", full=True) for n in (1, 2, 3, 4)] + [
    K_("full-wa-cfg5-n%d" % n, "wa", dims=(128, 240, 320), n=n, geom="small", full=True) for n in (1, 2, 3, 4)] + [
    K_("pre-n1", "pre", dims=(3, 5, 7), n=1),
    K_("pre-n5", "pre", dims=(2, 4, 9), n=5),
    K_("pre-n16", "pre", dims=(2, 3, 5), n=16),
    # GroupNorm statistics
] + [K_("gn-%d" % nb, "gn", n_blocks=nb, ratio=1.0) for nb in (1, 1023, 1024, 1025, 8192, 8193)] + [
    K_("gn-edge-8193", "gn", n_blocks=8193, ratio=R.GN_RANGE),
    K_("gn-edge-1", "gn", n_blocks=1, ratio=R.GN_RANGE),
    K_("full-gn-cfg2", "gn", n_blocks="cfg2", ratio=1.0),
    # ConvGRU elementwise stages
    K_("reset-small", "reset", n_vox=3 * 5 * 7),
    K_("reset-one", "reset", n_vox=1),
    K_("blend-small", "blend", n_vox=3 * 5 * 7, stride=32),
    K_("blend-stride16", "blend", n_vox=2 * 4 * 9, stride=16),
    K_("blend-stride20", "blend", n_vox=67, stride=20),
    K_("blend-one", "blend", n_vox=1, stride=32),
    K_("full-reset-cfg2", "reset", n_vox=64 * 120 * 160, full=True),
    K_("full-blend-cfg2", "blend", n_vox=64 * 120 * 160, stride=32, full=True),
    K_("full-blend-cfg5", "blend", n_vox=128 * 240 * 320, stride=32, full=True),
] + [K_("sam-w%d-d%d-s%d-n%d" % (w, d, s, n), "sam", dims=(n, d, 3, w), scale=s)
     for (w, d, s, n) in [(1, 1, 1, 1), (31, 7, 2, 3), (32, 8, 3, 1), (33, 9, 4, 3), (31, 64, 4, 1), (33, 65, 1, 3), (32, 1, 4, 3),
                          (1, 65, 3, 1), (33, 8, 2, 1), (32, 9, 1, 3)]] + [
    K_("sam-extreme", "sam", dims=(2, 9, 4, 33), scale=4, extreme=True),
    K_("full-sam-cfg2", "sam", dims=(1, 64, 120, 160), scale=4),
    K_("full-sam-cfg5", "sam", dims=(1, 128, 240, 320), scale=4),
    K_("cam-small", "cam", motion=1.0),
    K_("cam-large", "cam", motion=6.0),
    K_("layout-c16-off0", "layout", C=16, dims=(3, 5, 7), off=0),
    K_("layout-c16-off16", "layout", C=16, dims=(3, 5, 7), off=16),
    K_("layout-c32", "layout", C=32, dims=(2, 3, 11), off=0),
    K_("layout-c5-off3", "layout", C=5, dims=(1, 1, 65), off=3),
]


# ------------------------------------------------------------------------------------------------------------------- families
def _make(case):
    """-> dict of device inputs for the case"""
    fam, seed = case["fam"], sum(map(ord, case["id"]))
    m = {}
    if fam in ("sweep", "costvol"):
        D, H, W = case["dims"]
        m["P"], m["dv"] = _proj12(case["geom"], D, H, W)
        C = case.get("C", 32)
        if case.get("probe"):
            src = _ramp_hw(H, W, C)
        else:
            src = _rand((H, W, C), seed)
        m["src"] = src.permute(2, 0, 1).contiguous() if fam == "sweep" else src.contiguous()
        if fam == "costvol":
            m["ref"] = torch.zeros(H, W, 32, device=DEV) if case.get("probe") else _rand((H, W, 32), seed + 1)
        if case.get("px"):
            m["dv"] = (m["dv"].view(D, 1, 1) * (1.0 + 0.05 * torch.tanh(_rand((D, H, W), seed + 2)))).contiguous()
    elif fam == "mix":
        H, W = case["dims"]
        m["x"] = _rand((case["cin"], H, W), seed)
        m["w"] = _rand((case["cout"], case["cin"]), seed + 1, 1.0 / np.sqrt(case["cin"]))
        m["b"] = _rand((case["cout"],), seed + 2) if case["bias"] else None
    elif fam in ("wvol", "wvolex"):
        D, H, W = case["dims"]
        m["M"], m["dv"], m["dmin"], m["dint"] = _mats(case["geom"], 1, D, H, W)
        m["M"] = m["M"][0].contiguous()
        C = case["C"]
        m["vol"] = (_ramp_dhw(D, H, W, C).permute(3, 0, 1, 2).contiguous() if case.get("probe") else _rand((C, D, H, W), seed))
        if case.get("per_voxel"):
            m["dv"] = (m["dv"].view(D, 1, 1) * (1.0 + 0.03 * torch.tanh(_rand((D, H, W), seed + 2)))).contiguous()
        if case.get("disp"):
            dmin, dmax = 1.0 / 4.0, 1.0 / 0.5
            m["disp"] = (dmin, (dmax - dmin) / (D - 1))
            m["dv"] = (1.0 / (torch.arange(D, dtype=torch.float32) * m["disp"][1] + dmin)).to(DEV)
    elif fam == "wa":
        D, H, W = case["dims"]
        n = case["n"]
        m["M"], m["dv"], m["dmin"], m["dint"] = _mats(case["geom"], n, D, H, W)
        if case.get("hash"):
            m["t"] = hash_volume((D, H, W, 32), seed)
            m["s"] = [hash_volume((D, H, W, 32), seed + 1 + j) for j in range(n)]
        elif case.get("probe"):
            m["t"] = torch.zeros(D, H, W, 32, device=DEV)
            m["s"] = [_ramp_dhw(D, H, W, 32)]
        else:
            ks = case.get("kscale", 1.0)
            m["t"] = _rand((D, H, W, 32), seed)
            m["t"][..., 16:] *= ks
            m["s"] = [_rand((D, H, W, 32), seed + 1 + j) for j in range(n)]
            for s in m["s"]:
                s[..., 16:] *= ks
    elif fam == "pre":
        D, H, W = case["dims"]
        m["t"] = _rand((D, H, W, 32), seed)
        m["s"] = [_rand((D, H, W, 32), seed + 1 + j) for j in range(case["n"])]
    elif fam == "gn":
        from estdepth_amd import ops
        nb = case["n_blocks"]
        if nb == "cfg2":
            nb = ops.conv3d_grid(1, 64, 120, 160)
        g = np.random.default_rng(seed)
        k = 64                                                    # values per block and group
        std = 1.0
        mean = case["ratio"] * std
        x = g.standard_normal((nb, 2, k)) * std + mean * np.array([1.0, -0.5])[None, :, None]
        part = np.stack([x[:, 0].sum(1), (x[:, 0] ** 2).sum(1), x[:, 1].sum(1), (x[:, 1] ** 2).sum(1)], 1)
        m["part"], m["nb"], m["count"], m["eps"] = torch.from_numpy(part).to(DEV), nb, float(nb * k), 1e-5
    elif fam in ("reset", "blend"):
        n = case["n_vox"]
        m["xh"], m["ru"] = _rand((n, 32), seed), _rand((n, 32), seed + 1, 1.5)
        m["st"] = torch.tensor([0.1, 0.9, -0.2, 1.1], device=DEV)
        m["g"], m["b"] = _rand((16,), seed + 2, 0.5) + 1.0, _rand((16,), seed + 3, 0.3)
        if fam == "blend":
            m["o"], m["st_o"] = _rand((n, 16), seed + 4, 2.0), torch.tensor([0.3, 0.7, 0.0, 0.0], device=DEV)
            m["go"], m["bo"] = _rand((16,), seed + 5, 0.5) + 1.0, _rand((16,), seed + 6, 0.3)
    elif fam == "sam":
        N_, D, H, W = case["dims"]
        lg = _rand((N_, D, H, W), seed, 3.0)
        if case.get("extreme"):
            lg[:, 0, 0] = -float("inf")
            lg[:, 1, 1] = 80.0
            lg[:, 2, 2] = -1e30
            lg[0, :, 3, :] = 1e4 * torch.tanh(lg[0, :, 3, :])
        m["l"] = lg.contiguous()
        m["dv"] = (torch.arange(D, dtype=torch.float32) * 0.157 + 0.5).to(DEV)
    elif fam == "cam":
        K = _K(120, 160)
        m["K"] = K.to(DEV)
        m["pi"], m["pj"] = _pose(1, case["motion"]).to(DEV), _pose(3, case["motion"]).to(DEV)
        m["sp"] = torch.linalg.inv(m["pj"]).contiguous()
        m["rp"] = torch.linalg.inv(m["pi"]).contiguous()
    elif fam == "layout":
        D, H, W = case["dims"]
        m["src"] = _rand((case["C"], D, H, W), seed)
    return m


def _op(case, m, outs=None):
    """the case's op through ops.* under the current binding -> tuple of outputs"""
    from estdepth_amd import ops
    fam = case["fam"]
    if fam == "sweep":
        if case.get("px"):
            return (ops.homo_warping_px_chw(m["src"], m["P"], m["dv"]),)
        return (ops.homo_warping_chw(m["src"], m["P"], m["dv"], case["dims"][0]),)
    if fam == "mix":
        return (ops.mix1x1(m["x"], m["w"], m["b"]),)
    if fam == "costvol":
        return (ops.homo_warp_costvol(m["src"], m["ref"], m["P"], m["dv"], case["dims"][0]),)
    if fam == "wvol":
        return (ops.warp_volume_cdhw(m["vol"], m["M"], m["dv"], m["dmin"], m["dint"]),)
    if fam == "wvolex":
        d = m.get("disp")
        return (ops.warp_volume_ex_cdhw(m["vol"], m["M"], m["dv"], case.get("per_voxel", False), m["dmin"], m["dint"],
                                        d[0] if d else None, d[1] if d else None, case.get("border", False), case.get("pad", 0.0)),)
    if fam == "wa":
        return (ops.warp_attention(m["t"], m["s"], m["M"], m["dv"], m["dmin"], m["dint"]),)
    if fam == "pre":
        return (ops.attention_prewarped(m["t"], m["s"]),)
    if fam == "gn":
        return (ops.groupnorm_finalize(m["part"], m["nb"], m["count"], m["eps"]),)
    if fam == "reset":
        return (ops.gru_reset_apply(m["xh"], m["ru"], m["st"], m["g"], m["b"]),)
    if fam == "blend":
        out = outs[0] if outs is not None else _guarded((case["n_vox"], 32))[1]
        ops.gru_blend(m["xh"], m["ru"], m["o"], m["st"], m["st_o"], m["g"], m["b"], m["go"], m["bo"], out, case["stride"])
        return (out,)
    if fam == "sam":
        return ops.softargmin_up(m["l"], m["dv"], case["scale"])
    if fam == "cam":
        return (ops.cam_pair_proj(m["sp"], m["rp"]), ops.cam_sweep_proj(m["pi"], m["pj"], m["K"]),
                ops.cam_volume_mats(m["pj"], m["pi"], m["K"]), ops.cam_volume_mats(m["pj"], None, m["K"]))
    if fam == "layout":
        C, (D, H, W), off = case["C"], case["dims"], case["off"]
        dst = outs[0] if outs is not None else _guarded((D * H * W, 32))[1]
        ops.cdhw_to_vol(m["src"], dst, 32, off)
        back = ops.vol_to_cdhw(dst, C, (D, H, W), 32, off)
        return dst, back


def _blend_out_shape(case):
    return (case["n_vox"], 32) if case["stride"] == 32 else ((case["n_vox"] - 1) * case["stride"] + 16,)


def _raw(case, g, o):
    """the same launches through the C ABI on guarded buffers ``g`` (inputs) / ``o`` (outputs) -> list of statuses"""
    import ctypes
    from estdepth_amd import _native as NV
    lib, st = NV.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    fam = case["fam"]
    if fam == "sweep":
        C, H, W = g["src"].shape
        D = case["dims"][0]
        fn = lib.estd_homo_warping_px if case.get("px") else lib.estd_homo_warping
        return [fn(p(g["src"]), p(g["P"]), p(g["dv"]), p(o[0]), C, D, H, W, st)]
    if fam == "mix":
        Cin, H, W = g["x"].shape
        return [lib.estd_mix1x1_chw_to_hwc(p(g["x"]), p(g["w"]), p(g.get("b")), p(o[0]), Cin, g["w"].shape[0], H * W, st)]
    if fam == "costvol":
        D, H, W = case["dims"]
        return [lib.estd_homo_warp_costvol(p(g["src"]), p(g["ref"]), p(g["P"]), p(g["dv"]), p(o[0]), D, H, W, st)]
    if fam == "wvol":
        C, D, H, W = g["vol"].shape
        return [lib.estd_warp_volume(p(g["vol"]), p(g["M"]), p(g["dv"]), ctypes.c_float(g["dmin"]), ctypes.c_float(g["dint"]), p(o[0]),
                                     C, D, H, W, st)]
    if fam == "wvolex":
        C, D, H, W = g["vol"].shape
        d = g.get("disp")
        opts = NV.WarpVolumeOpts(int(case.get("per_voxel", False)), int(d is not None), int(case.get("border", False)), g["dmin"], g["dint"],
                                 d[0] if d else 0.0, d[1] if d else 1.0, case.get("pad", 0.0))
        return [lib.estd_warp_volume_ex(p(g["vol"]), p(g["M"]), p(g["dv"]), ctypes.byref(opts), p(o[0]), C, D, H, W, st)]
    if fam == "wa":
        D, H, W = case["dims"]
        arr = (ctypes.c_void_p * len(g["s"]))(*[s.data_ptr() for s in g["s"]])
        return [lib.estd_warp_attention(p(g["t"]), arr, p(g["M"]), len(g["s"]), p(g["dv"]), ctypes.c_float(g["dmin"]),
                                        ctypes.c_float(g["dint"]), p(o[0]), D, H, W, st)]
    if fam == "pre":
        arr = (ctypes.c_void_p * len(g["s"]))(*[s.data_ptr() for s in g["s"]])
        return [lib.estd_attention_prewarped(p(g["t"]), arr, len(g["s"]), p(o[0]), g["t"].numel() // 32, st)]
    if fam == "gn":
        return [lib.estd_groupnorm_finalize(p(g["part"]), g["nb"], ctypes.c_double(g["count"]), ctypes.c_float(g["eps"]), p(o[0]), st)]
    if fam == "reset":
        return [lib.estd_gru_reset_apply(p(g["xh"]), p(g["ru"]), p(g["st"]), p(g["g"]), p(g["b"]), p(o[0]), case["n_vox"], st)]
    if fam == "blend":
        return [lib.estd_gru_blend(p(g["xh"]), p(g["ru"]), p(g["o"]), p(g["st"]), p(g["st_o"]), p(g["g"]), p(g["b"]), p(g["go"]), p(g["bo"]),
                                   p(o[0]), case["stride"], case["n_vox"], st)]
    if fam == "sam":
        N_, D, H, W = g["l"].shape
        return [lib.estd_softargmin_up(p(g["l"]), p(g["dv"]), p(o[0]), p(o[1]), N_, D, H, W, case["scale"], st)]
    if fam == "cam":
        return [lib.estd_cam_pair_proj(p(g["sp"]), p(g["rp"]), p(o[0]), st), lib.estd_cam_sweep_proj(p(g["pi"]), p(g["pj"]), p(g["K"]), p(o[1]), st),
                lib.estd_cam_volume_mats(p(g["pj"]), p(g["pi"]), p(g["K"]), p(o[2]), st),
                lib.estd_cam_volume_mats(p(g["pj"]), None, p(g["K"]), p(o[3]), st)]
    if fam == "layout":
        C, (D, H, W), off = case["C"], case["dims"], case["off"]
        S = D * H * W
        return [lib.estd_cdhw_to_vol(p(g["src"]), p(o[0]), C, S, 32, off, st), lib.estd_vol_to_cdhw(p(o[0]), p(o[1]), C, S, 32, off, st)]


def _expected(case):
    fam = case["fam"]
    if fam == "costvol":
        return {costvol_kernel(case["dims"][1], case.get("linear", False))}
    if fam == "wa":
        D, H, W = case["dims"]
        return {wa_kernel(case["n"], D, H, W, _env_int("ESTD_WA_BUF", -1))}
    if fam in ("reset", "blend"):
        return {gru_kernel(fam, _env_int("ESTD_GRU_FAST", 0) == 1)}
    return set(INSTANCES[ROUTE_OF[fam]])


ROUTE_OF = {"sweep": "homo_warping", "mix": "mix1x1", "costvol": "costvol", "wvol": "warp_volume", "wvolex": "warp_volume_ex", "wa": "warp_attention",
            "pre": "attention_prewarped", "gn": "groupnorm_finalize", "reset": "gru_reset", "blend": "gru_blend", "sam": "softargmin", "cam": "cam",
            "layout": "layout"}


def _points(D, H, W, seed, n=3000):
    """n random voxels + the last brick (2 x 4 x 8) + the last two planes' last rows + the volume's corners -> flat (d, y, x) indices"""
    g = torch.Generator().manual_seed(seed)
    S = D * H * W
    rnd = torch.randint(0, S, (n,), generator=g)
    last = [((D - 1 - dd) * H + (H - 1 - yy)) * W + (W - 1 - xx) for dd in range(min(D, 2)) for yy in range(min(H, 4)) for xx in range(min(W, 8))]
    rows = [((D - 1 - dd) * H + (H - 1)) * W + x for dd in range(min(D, 2)) for x in range(0, W, max(1, W // 64))]
    corners = [(d * H + y) * W + x for d in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    return torch.unique(torch.cat([rnd, torch.tensor(last + rows + corners)]))


def _checks(case, m, outs):
    """-> list of (what, got, Ref) for the case's outputs"""
    fam = case["fam"]
    full = case.get("full", False)
    seed = sum(map(ord, case["id"]))
    if fam == "sweep":
        D, H, W = case["dims"]
        return [("out", outs[0], R.homo_warping_ref(m["src"], m["P"], m["dv"], D))]
    if fam == "mix":
        return [("out", outs[0], R.mix1x1_ref(m["x"], m["w"], m["b"]))]
    if fam == "costvol":
        D, H, W = case["dims"]
        if full:
            pts = _points(D, H, W, seed)
            return [("out", outs[0].view(-1, 32)[pts.to(DEV)], R.costvol_ref(m["src"], m["ref"], m["P"], m["dv"], D, points=pts))]
        return [("out", outs[0], R.costvol_ref(m["src"], m["ref"], m["P"], m["dv"], D))]
    if fam in ("wvol", "wvolex"):
        return [("out", outs[0], R.warp_volume_ref(m["vol"], m["M"], m["dv"], m["dmin"], m["dint"], disp=m.get("disp"),
                                                   border=case.get("border", False), padding_value=case.get("pad", 0.0)))]
    if fam == "wa":
        D, H, W = case["dims"]
        srcs = [hash_getter(seed + 1 + j) for j in range(case["n"])] if case.get("hash") else m["s"]
        tgt = hash_getter(seed) if case.get("hash") else m["t"]
        if full or case.get("hash"):
            pts = _points(D, H, W, seed)
            return [("xh", outs[0].view(-1, 32)[pts.to(DEV)],
                     R.warp_attention_ref(tgt, srcs, m["M"], m["dv"], m["dmin"], m["dint"], points=pts, dims=(D, H, W)))]
        return [("xh", outs[0], R.warp_attention_ref(m["t"], m["s"], m["M"], m["dv"], m["dmin"], m["dint"]))]
    if fam == "pre":
        return [("xh", outs[0], R.attention_prewarped_ref(m["t"], m["s"]))]
    if fam == "gn":
        return [("stats", outs[0], R.groupnorm_finalize_ref(m["part"], m["count"], m["eps"]))]
    fast = _env_int("ESTD_GRU_FAST", 0) == 1
    if fam == "reset":
        pts = _points(1, 1, case["n_vox"], seed) if full else None
        got = outs[0].view(-1, 32)
        return [("xrh", got[pts.to(DEV)] if full else got, R.gru_reset_ref(m["xh"], m["ru"], m["st"], m["g"], m["b"], fast=fast, points=pts))]
    if fam == "blend":
        pts = _points(1, 1, case["n_vox"], seed) if full else None
        s = case["stride"]
        idx = torch.arange(case["n_vox"], device=DEV) * s
        got = outs[0].view(-1)[(idx[:, None] + torch.arange(16, device=DEV))]
        got = got[pts.to(DEV)] if full else got
        return [("out", got, R.gru_blend_ref(m["xh"], m["ru"], m["o"], m["st"], m["st_o"], m["g"], m["b"], m["go"], m["bo"], fast=fast, points=pts))]
    if fam == "sam":
        rd, rp = R.softargmin_ref(m["l"], m["dv"], case["scale"])
        return [("depth", outs[0], rd), ("prob", outs[1], rp)]
    if fam == "cam":
        return [("pair", outs[0], R.cam_pair_proj_ref(m["sp"], m["rp"])), ("sweep", outs[1], R.cam_sweep_proj_ref(m["pi"], m["pj"], m["K"])),
                ("volume", outs[2], R.cam_volume_mats_ref(m["pj"], m["pi"], m["K"])), ("volume-rel", outs[3], R.cam_volume_mats_ref(m["pj"], None, m["K"]))]
    if fam == "layout":
        C, off = case["C"], case["off"]
        src = m["src"].reshape(C, -1).t().double().cpu()
        z = torch.zeros_like(src)
        return [("vol", outs[0].view(-1, 32)[:, off:off + C], R.Ref(src, z)), ("cdhw", outs[1], R.Ref(m["src"].double().cpu(), torch.zeros_like(m["src"].double().cpu())))]


def _outside_written(case, out_bufs):
    """number of changed sentinel words inside the output views that the op must not write (the other half of strided records)"""
    fam = case["fam"]
    if fam == "blend" and case["stride"] > 16:
        v = out_bufs[0].view(-1)
        s = case["stride"]
        keep = torch.ones(v.numel(), dtype=torch.bool, device=DEV)
        idx = torch.arange(case["n_vox"], device=DEV) * s
        keep[(idx[:, None] + torch.arange(16, device=DEV)).reshape(-1)] = False
        return int((_bits(v)[keep] != SENT32).sum())
    if fam == "layout":
        v = out_bufs[0]
        C, off = case["C"], case["off"]
        keep = torch.ones(32, dtype=torch.bool, device=DEV)
        keep[off:off + C] = False
        return int((_bits(v)[:, keep] != SENT32).sum())
    return 0


def _out_shapes(case, outs):
    if case["fam"] == "blend":
        return [_blend_out_shape(case)]
    if case["fam"] == "layout":
        return [(int(np.prod(case["dims"])), 32), tuple(outs[1].shape)]
    return [tuple(o.shape) for o in outs]


def run_case(case):
    """-> (worst ratio, the instances that ran, ambiguous samples, hash of the outputs)"""
    m = _make(case)
    want = _expected(case)
    what = case["id"]
    env = {"ESTD_SWEEP_LINEAR": "1" if case.get("linear") else None}
    # 1. torch binding under the profiler (strided outputs go into sentinel-filled buffers)
    pre = [_guarded(s)[1] for s in ([_blend_out_shape(case)] if case["fam"] == "blend" else
                                     [(int(np.prod(case["dims"])), 32)] if case["fam"] == "layout" else [])]
    with _Binding("torch", env):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            outs_t = _op(case, m, pre or None)
            torch.cuda.synchronize()
    ran = {mm.group(1) + (mm.group(2) or "") for e in prof.key_averages() for mm in [KERNEL_RE.search(e.key)] if mm}
    assert ran == want, "%s: ran %s, expected %s" % (what, sorted(ran), sorted(want))
    assert _outside_written(case, outs_t) == 0, "%s: the torch binding wrote outside its channels" % what
    # 2. ctypes binding: bit-identical
    pre_c = [_guarded(o.shape)[1] for o in pre]
    with _Binding("ctypes", env):
        outs_c = _op(case, m, pre_c or None)
        torch.cuda.synchronize()
    for a, b in zip(outs_t, outs_c):
        assert torch.equal(_bits(a), _bits(b)), "%s: the bindings differ" % what
    del outs_c, pre_c
    # 3. the C ABI on guarded buffers: nothing written outside the outputs, nothing read outside the inputs
    g, in_bufs = {}, []
    for k, v in m.items():
        if isinstance(v, torch.Tensor):
            b, view = _guarded(v.shape, v, v.dtype)
            g[k], in_bufs = view, in_bufs + [b]
        elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            g[k] = []
            for t in v:
                b, view = _guarded(t.shape, t)
                g[k].append(view)
                in_bufs.append(b)
        else:
            g[k] = v
    ob = [_guarded(s, dtype=o.dtype) for s, o in zip(_out_shapes(case, outs_t), outs_t)]
    with _Binding("ctypes", env):
        status = _raw(case, g, [v for _, v in ob])
        torch.cuda.synchronize()
    assert all(s == 0 for s in status), "%s: estd status %s" % (what, status)
    for b, v in ob:
        assert _band_intact(b), "%s: written outside an output" % what
    for b in in_bufs:
        assert _band_intact(b), "%s: written into an input's guard band" % what
    for (b, v), o in zip(ob, outs_t):
        assert torch.equal(_bits(v.reshape(o.shape)), _bits(o)), "%s: the guarded launch differs from the op" % what
    del g, in_bufs, ob
    # 4. the fp64 reference
    worst, amb = 0.0, 0
    c = C_ROUTE[ROUTE_OF[case["fam"]]]
    for name, got, ref in _checks(case, m, outs_t):
        r, n_amb = R.check_bound(got, ref, c, "%s %s" % (what, name))
        assert n_amb <= max(1.0, AMB_CAP * ref.n_samples), "%s %s: %d of %d samples ambiguous" % (what, name, n_amb, ref.n_samples)
        worst, amb = max(worst, r), max(amb, n_amb)
    if case.get("probe"):
        _probe(case, m, outs_t)
    digest = hashlib.sha256(b"".join(_bits(o).cpu().numpy().tobytes() for o in outs_t)).hexdigest()[:16]
    del m, outs_t
    torch.cuda.empty_cache()
    return worst, sorted(ran), amb, digest


def _probe(case, m, outs):
    """affine source ramps: wherever every corner is inside and no axis is masked, the output is the kernel's own sample position + 1;
    it must lie within delta of the fp64 position"""
    fam = case["fam"]
    D, H, W = case["dims"]
    S = D * H * W
    pts = torch.arange(S)
    d, y, x = R._dhw(pts, D, H, W)
    if fam in ("sweep", "costvol"):
        axes, amb_den = R._sweep_pos(m["P"], m["dv"].double().cpu()[d], x, y, H, W)
        got = outs[0].double().cpu()
        got = got.reshape(-1, D, H, W).reshape(got.shape[0], -1).t()[:, :2] if fam == "sweep" else got.reshape(S, 32)[:, :2]
        got = got[:, [1, 0]]                                   # (y + 1, x + 1)
        dims = (H, W)
    else:
        axes, amb_den = R._volume_pos(m["M"].reshape(-1, 30)[0], m["dv"].double().cpu()[d], x, y, D, H, W, m["dmin"], m["dint"])
        o = outs[0].double().cpu()
        got = o.reshape(3, S).t() if fam == "wvol" else o.reshape(S, 32)[:, 16:19]
        got = got[:, [2, 1, 0]]                                # (z + 1, y + 1, x + 1)
        dims = (D, H, W)
    inside = ~amb_den
    for (i, masked, amb, _), n in zip(axes, dims):
        inside &= ~masked & ~amb & (i.v >= 0) & (i.v <= n - 1)
    assert int(inside.sum()) >= S // 4, "%s: too few samples inside the source (%d of %d)" % (case["id"], int(inside.sum()), S)
    for a, ((i, _, _, _), n) in enumerate(zip(axes, dims)):
        err = (got[:, a] - (i.v + 1.0)).abs()
        tol = R.C_POS * i.e + 8 * R.U * (i.v.abs() + 1.0)
        bad = inside & (err > tol)
        assert not bool(bad.any()), "%s: axis %d position off by %.3g (tolerance %.3g)" % (case["id"], a, float(err[bad].max()), float(tol[bad].max()))


# -------------------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_sweep_fusion_route_against_fp64(case):
    ratio, kernels, amb, _ = run_case(case)
    print("ROUTE-RATIO %s %s %.3f amb=%d %s" % (ROUTE_OF[case["fam"]], case["id"], ratio, amb, " ".join(kernels)))


def test_costvol_banded_and_linear_instances_agree_bit_for_bit():
    """ESTD_SWEEP_LINEAR is read at every call: the XCD-banded and the linear block mappings must write the same volume"""
    case = K_("costvol-ab", "costvol", dims=(6, 16, 23), geom="large")
    m = _make(case)
    outs = []
    for lin in (None, "1"):
        with _Binding("torch", {"ESTD_SWEEP_LINEAR": lin}):
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                outs.append(_op(case, m)[0])
                torch.cuda.synchronize()
        ran = {mm.group(1) + (mm.group(2) or "") for e in prof.key_averages() for mm in [KERNEL_RE.search(e.key)] if mm}
        assert ran == {costvol_kernel(16, lin is not None)}, ran
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


# ------------------------------------------------------------------------------------------------------------------ limits
def _wa_limit_case(D):
    return K_("wa-limit-%d" % D, "wa", dims=(D, 256, 256), n=3, geom="tiny", hash=True)


@pytest.mark.parametrize("D,buf", [(255, True), (256, False)])
def test_warp_attention_around_2GiB_per_source(D, buf):
    """3 sources of 255 x 256 x 256 records (2 139 095 040 bytes: the buffer-load form) and 256 x 256 x 256 (2^31 bytes: the pointer
    form), filled on the device from a closed form; the reference reads that form at the corners it needs, among them those of the
    final planes, where a short num_records would read zeros"""
    case = _wa_limit_case(D)
    assert wa_kernel(3, D, 256, 256) == "warp_attention_kernel<3, %s>" % ("true" if buf else "false")
    ratio, kernels, amb, _ = run_case(case)
    print("ROUTE-RATIO warp_attention %s %.3f amb=%d %s" % (case["id"], ratio, amb, " ".join(kernels)))


def test_costvol_refuses_2_pow_31_voxels_before_launch():
    """D * H * W >= 2^31 - 1 (32-bit voxel indices): estd_homo_warp_costvol returns ESTD_ERR_UNSUPPORTED before launching (tiny buffers)"""
    import ctypes
    from estdepth_amd import _native as NV
    lib, st = NV.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = torch.zeros(64, device=DEV)
    p = ctypes.c_void_p(t.data_ptr())
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for D, H, W in ((1 << 25, 8, 8), (0x7FFFFFFF, 1, 1), (1 << 23, 16, 16)):
            assert lib.estd_homo_warp_costvol(p, p, p, p, p, D, H, W, st) == -3, (D, H, W)
        torch.cuda.synchronize()
    assert not [e.key for e in prof.key_averages() if KERNEL_RE.search(e.key)]


# ------------------------------------------------------------------------------------------- latched switches (child processes)
def _child(env, cases):
    """run ``cases`` in a fresh process with ``env`` -> {case id: (ratio, kernels, ambiguous, digest)}"""
    code = ("import json, sys, traceback\n"
            "sys.path.insert(0, 'tests')\n"
            "import test_gpu_sweep_fusion_routes as T\n"
            "for c in json.loads(sys.argv[1]):\n"
            "    try:\n"
            "        print('CASE ' + json.dumps([c['id']] + list(T.run_case(c))), flush=True)\n"
            "    except Exception:\n"
            "        print('FAIL ' + json.dumps([c['id'], traceback.format_exc()[-1500:]]), flush=True)\n")
    r = subprocess.run([sys.executable, "-c", code, json.dumps(cases)], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    if r.returncode < 0 or r.returncode in (134, 139):          # a crashed GPU process: start nothing more on this device
        pytest.exit("child %s ended with status %d:\n%s" % (env, r.returncode, r.stderr[-3000:]), returncode=1)
    got, fails = {}, []
    for line in r.stdout.splitlines():
        if line.startswith("CASE "):
            cid, ratio, kern, amb, digest = json.loads(line[5:])
            got[cid] = (ratio, kern, amb, digest)
        elif line.startswith("FAIL "):
            fails.append(json.loads(line[5:]))
    assert r.returncode == 0, (env, r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert not fails, "%s: %s" % (env, "\n".join("%s: %s" % tuple(f) for f in fails))
    assert sorted(got) == sorted(c["id"] for c in cases), (env, sorted(got))
    return got


WA_FORCED = [K_("wa-forced-n%d" % n, "wa", dims=(5, 6, 13), n=n, geom="small") for n in (1, 2, 3, 4, 5, 9, 16)]


@pytest.mark.parametrize("buf", [0, 1])
def test_warp_attention_forced_form(buf):
    """ESTD_WA_BUF = 0 | 1 forces the pointer / buffer-load form for every source count: all ten warp_attention instances"""
    got = _child(dict(ESTD_WA_BUF=str(buf)), WA_FORCED)
    kerns = sorted({k for v in got.values() for k in v[1]})
    assert kerns == sorted("warp_attention_kernel<%d, %s>" % (ns, "true" if buf else "false") for ns in WA_NS), kerns
    for cid, (ratio, ks, amb, _) in sorted(got.items()):
        print("ROUTE-RATIO warp_attention %s-buf%d %.3f amb=%d %s" % (cid, buf, ratio, amb, " ".join(ks)))


def test_warp_attention_occupancy_cap_reproduces_the_default():
    """ESTD_WA_OCC = 2 requests 80 KB of LDS (the dynamic-LDS opt-in path): same instance, bit-identical result"""
    cases = [K_("wa-occ-n3", "wa", dims=(6, 9, 21), n=3, geom="small"), K_("wa-occ-n2", "wa", dims=(4, 8, 16), n=2, geom="large")]
    got = _child(dict(ESTD_WA_OCC="2"), cases)
    for c in cases:
        _, kern, _, digest = run_case(c)
        assert got[c["id"]][1] == kern and got[c["id"]][3] == digest, (c["id"], got[c["id"]], kern, digest)


def test_gru_fast_transcendentals():
    """ESTD_GRU_FAST = 1: gru_reset_kernel<true> / gru_blend_kernel<true> under the bound with the absolute transcendental term"""
    cases = [c for c in CASES if c["fam"] in ("reset", "blend") and not c["id"].startswith("full-blend-cfg5")]
    got = _child(dict(ESTD_GRU_FAST="1"), cases)
    kerns = sorted({k for v in got.values() for k in v[1]})
    assert kerns == ["gru_blend_kernel<true>", "gru_reset_kernel<true>"], kerns
    for cid, (ratio, ks, amb, _) in sorted(got.items()):
        print("ROUTE-RATIO %s %s-fast %.3f amb=%d %s" % (ks[0].split("_kernel")[0], cid, ratio, amb, " ".join(ks)))


# ----------------------------------------------------------------------------------------------------------- malformed arguments
def _sent(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device=DEV).view(torch.float32)


def _short(t, n):
    """the first n elements of a full-sized tensor: were it wrongly accepted, the kernel would still read and write memory the test owns"""
    return t.reshape(-1)[:n]


def _arg_table():
    """One entry per operator: (the operator's name in messages, call(**args) -> outputs, valid() -> its arguments by name, the argument
    it writes or None, [(label, the argument replaced, its malformed value[, the name the message gives it])]).  Every malformed call
    differs from the valid one in that one argument.  Volumes are D x H x W = 2 x 3 x 5 (the smallest the warps accept, no two sizes
    equal, 30 voxels)."""
    from estdepth_amd import ops
    r = lambda *s: _rand(s, 7 + sum(s))                                         # noqa: E731
    eye = torch.eye(4, device=DEV)
    K = torch.tensor([[50.0, 0.0, 2.5], [0.0, 50.0, 1.5], [0.0, 0.0, 1.0]], device=DEV)
    dv = torch.tensor([1.0, 2.0], device=DEV)
    P, M30, st, aff = r(12), r(30), torch.tensor([0.1, 0.9, -0.2, 1.1], device=DEV), r(16)
    kv, kv16, vol, mix = r(2, 3, 5, 32), r(2, 3, 5, 16), r(4, 2, 3, 5), r(3, 5, 32)
    f64 = lambda t: t.double()                                                  # noqa: E731
    blend = dict(xh=kv, ru=r(2, 3, 5, 32), o_raw=kv16, stats_ru=st, stats_o=st, gamma_u=aff, beta_u=aff, gamma_o=aff, beta_o=aff, out_stride=32)

    def void(fn, dest):                                  # an operator that returns nothing: its output is the argument it writes
        return lambda **a: (fn(**a), a[dest])[1]
    return [
        ("cam_pair_proj", ops.cam_pair_proj, lambda: dict(src_proj=eye * 2, ref_proj=eye), None, [
            ("a 12-float src_proj", "src_proj", _short(eye, 12)), ("a 12-float ref_proj", "ref_proj", _short(eye, 12)),
            ("float64", "src_proj", f64(eye)), ("a list", "src_proj", [1.0] * 16), ("None", "ref_proj", None)]),
        ("cam_sweep_proj", ops.cam_sweep_proj, lambda: dict(ref_pose=eye, src_pose=eye * 2, intr=K), None, [
            ("a 12-float ref_pose", "ref_pose", _short(eye, 12)), ("a 12-float src_pose", "src_pose", _short(eye, 12)),
            ("6-float intrinsics", "intr", _short(K, 6)), ("float64 intrinsics", "intr", f64(K))]),
        ("cam_volume_mats", void(ops.cam_volume_mats, "out"), lambda: dict(pose_j=eye * 2, pose_i=eye, intr=K, out=_sent(30)), "out", [
            ("a 12-float pose_j", "pose_j", _short(eye, 12)), ("a 12-float pose_i", "pose_i", _short(eye, 12)),
            ("6-float intrinsics", "intr", _short(K, 6)), ("a 24-float out", "out", _short(_sent(30), 24))]),
        ("cam_volume_mats", void(ops.cam_volume_mats, "out"), lambda: dict(pose_j=eye * 2, pose_i=None, intr=K, out=_sent(30)), "out", []),
        ("homo_warping", ops.homo_warping_chw, lambda: dict(src_chw=r(4, 3, 5), proj12=P, depth_values=dv, D=2), None, [
            ("src_chw [C,HW]", "src_chw", r(4, 15)), ("src_chw [2,C,H,W]", "src_chw", r(2, 4, 3, 5)), ("9-float proj12", "proj12", _short(P, 9)),
            ("one depth for two planes", "depth_values", _short(dv, 1)), ("float64 depths", "depth_values", f64(dv))]),
        ("homo_warping_px", ops.homo_warping_px_chw, lambda: dict(src_chw=r(4, 3, 5), proj12=P, depth_dhw=r(2, 3, 5).abs() + 1), None, [
            ("depth_dhw [D,W,H]", "depth_dhw", r(2, 5, 3)), ("depth_dhw [D,HW]", "depth_dhw", r(2, 15)), ("9-float proj12", "proj12", _short(P, 9)),
            ("src_chw [C,HW]", "src_chw", r(4, 15))]),
        ("mix1x1", ops.mix1x1, lambda: dict(in_chw=r(8, 3, 5), w=r(4, 8), bias=r(4)), None, [
            ("w [Cin,Cout]", "w", r(8, 4)), ("w for another Cin", "w", r(4, 6)), ("a 3-float bias", "bias", _short(r(4), 3)),
            ("in_chw [Cin,HW]", "in_chw", r(8, 15))]),
        ("mix1x1", ops.mix1x1, lambda: dict(in_chw=r(8, 3, 5), w=r(4, 8), bias=None), None, []),
        ("homo_warp_costvol", ops.homo_warp_costvol, lambda: dict(src_mix=mix, ref_mix=r(3, 5, 32), proj12=P, depth_values=dv, D=2, out=_sent(2, 3, 5, 32)),
         "out", [
            ("16-channel src_mix", "src_mix", r(3, 5, 16)), ("ref_mix [W,H,32]", "ref_mix", r(5, 3, 32)), ("9-float proj12", "proj12", _short(P, 9)),
            ("one depth for two planes", "depth_values", _short(dv, 1)), ("out one plane short", "out", _short(_sent(2, 3, 5, 32), 3 * 5 * 32)),
            ("float64 ref_mix", "ref_mix", f64(mix)), ("None for src_mix", "src_mix", None)]),
        ("softargmin_up", ops.softargmin_up, lambda: dict(logits=r(1, 2, 3, 5), depth_values=dv, scale=4), None, [
            ("logits [D,H,W]", "logits", r(2, 3, 5)),
            ("one depth for two planes", "depth_values", _short(dv, 1)), ("a list of depths", "depth_values", [1.0, 2.0]), ("None", "logits", None)]),
        ("warp_volume", ops.warp_volume_cdhw, lambda: dict(vol=vol, mats30=M30, depth_values=dv, depth_min=0.5, depth_interval=0.1), None, [
            ("vol [C,D,HW]", "vol", r(4, 2, 15)), ("24-float mats30", "mats30", _short(M30, 24)),
            ("one depth for two planes", "depth_values", _short(dv, 1), "depth"), ("float64 vol", "vol", f64(vol))]),
        ("warp_volume_ex", ops.warp_volume_ex_cdhw, lambda: dict(vol=vol, mats30=M30, depth=r(2, 3, 5).abs() + 1, depth_per_voxel=True, depth_min=0.5,
                                                               depth_interval=0.1), None, [
            ("per-voxel depth one short", "depth", _short(r(2, 3, 5), 29)), ("per-plane depth for per-voxel", "depth", dv),
            ("24-float mats30", "mats30", _short(M30, 24)), ("vol [C,D,HW]", "vol", r(4, 2, 15))]),
        ("warp_attention", ops.warp_attention, lambda: dict(kv_target=kv, kv_sources=[r(2, 3, 5, 32), kv], mats=r(2, 30), depth_values=dv, depth_min=0.5,
                                                          depth_interval=0.1), None, [
            ("16-channel kv_target", "kv_target", kv16), ("a source [D,W,H,32]", "kv_sources", [kv, r(2, 5, 3, 32)]),
            ("a 16-channel source", "kv_sources", [kv16, kv]), ("no source", "kv_sources", []), ("17 sources", "kv_sources", [kv] * 17),
            ("a float64 source", "kv_sources", [kv, f64(kv)]),
            ("mats for one source", "mats", _short(r(2, 30), 30)), ("one depth for two planes", "depth_values", _short(dv, 1))]),
        ("attention_prewarped", ops.attention_prewarped, lambda: dict(kv_target=kv, kv_sources=[r(2, 3, 5, 32), kv]), None, [
            ("no source", "kv_sources", []), ("17 sources", "kv_sources", [kv] * 17), ("a source [D,W,H,32]", "kv_sources", [kv, r(2, 5, 3, 32)]),
            ("a source one voxel short", "kv_sources", [_short(kv, 29 * 32), kv]), ("a float64 source", "kv_sources", [f64(kv), kv]),
            ("a target of 29.97 voxels", "kv_target", _short(kv, 959))]),
        ("gru_reset_apply", ops.gru_reset_apply, lambda: dict(xh=kv, ru=r(2, 3, 5, 32), stats4=st, gamma_r=aff, beta_r=aff), None, [
            ("ru one voxel short", "ru", _short(kv, 29 * 32)), ("xh of 29.97 voxels", "xh", _short(kv, 959)), ("2-float stats", "stats4", _short(st, 2)),
            ("8-float gamma", "gamma_r", _short(aff, 8)), ("15-float beta", "beta_r", _short(aff, 15)), ("float64 ru", "ru", f64(kv))]),
        ("gru_blend", void(ops.gru_blend, "out_value"), lambda: dict(blend, out_value=_sent(2, 3, 5, 32)), "out_value", [
            ("ru one voxel short", "ru", _short(kv, 29 * 32)), ("o_raw one voxel short", "o_raw", _short(kv16, 29 * 16)),
            ("32-channel o_raw", "o_raw", kv), ("3-float stats_ru", "stats_ru", _short(st, 3)), ("3-float stats_o", "stats_o", _short(st, 3)),
            ("15-float gamma_u", "gamma_u", _short(aff, 15)), ("15-float beta_u", "beta_u", _short(aff, 15)),
            ("15-float gamma_o", "gamma_o", _short(aff, 15)), ("15-float beta_o", "beta_o", _short(aff, 15)),
            ("out_value one float short", "out_value", _short(_sent(2, 3, 5, 32), 29 * 32 + 15))]),
        ("groupnorm_finalize", ops.groupnorm_finalize, lambda: dict(partials=r(3, 4).double(), n_blocks=3, count=48.0), None, [
            ("float32 partials", "partials", r(3, 4)), ("partials one block short", "partials", r(2, 4).double())]),
        ("cdhw_to_vol", void(ops.cdhw_to_vol, "dst"), lambda: dict(src=r(16, 2, 3, 5), dst=_sent(31, 32)[1:], dst_stride=32, dst_off=16), "dst", [      # (dst, src below: views with a record in front)
            ("dst one record short", "dst", _short(_sent(31, 32)[1:], 29 * 32)), ("a negative offset", "dst_off", -16), ("src without channels", "src", r(480)),
            ("float64 src", "src", f64(r(16, 2, 3, 5)))]),
        ("vol_to_cdhw", ops.vol_to_cdhw, lambda: dict(src=r(31, 32)[1:], C=16, dims=(2, 3, 5), src_stride=32, src_off=16), None, [
            ("src one record short", "src", _short(r(31, 32)[1:], 29 * 32)), ("a negative offset", "src_off", -16), ("two dims", "dims", (6, 5)),
            ("float64 src", "src", f64(r(30, 32)))]),
    ]


def _malformed(table=None, fill_dest=False):
    """(label, operator's name in messages, argument's name in messages, call, the tensor the call would write or None) of every malformed
    call of ``table`` (_arg_table() unless given, whose destinations hold the sentinel already); ``fill_dest``: a copy of the tensor the
    operator writes is filled with the sentinel first.  No malformed argument is a CPU tensor: a kernel that got one would fault."""
    out = []
    for op, fn, valid, dest, bad in (_arg_table() if table is None else table):
        for label, arg, value, *msg_name in bad:
            args = dict(valid(), **{arg: value})
            if fill_dest and dest is not None and arg != dest:
                args[dest] = torch.full_like(args[dest].view(torch.int32), SENT32).view(torch.float32)
            out.append(("%s: %s" % (op, label), op, msg_name[0] if msg_name else arg, lambda fn=fn, args=args: fn(**args), args.get(dest)))
    return out


def _as_tuple(o):
    return tuple(o) if isinstance(o, (tuple, list)) else (o,)


def test_the_valid_call_of_every_operator_runs_alike_under_both_bindings():
    """the rule set refuses nothing it should accept: bit-identical outputs"""
    for op, fn, valid, _, _ in _arg_table():
        outs = []
        for binding in ("torch", "ctypes"):
            with _Binding(binding):
                outs.append(_as_tuple(fn(**valid())))
        torch.cuda.synchronize()
        assert len(outs[0]) == len(outs[1]) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*outs)), op


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_malformed_arguments_raise_before_any_launch(binding):
    """the ctypes front end checks what the torch binding checks -- and raises before anything is launched: RuntimeError under both bindings
    with the operator's and the argument's name in the message, no kernel of the suite in the trace, the destination of an operator that
    writes into a caller's buffer untouched"""
    cases = _malformed()
    assert len(cases) >= 80 and len({c[0] for c in cases}) == len(cases)
    with _Binding(binding):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            for label, op, arg, call, dest in cases:
                with pytest.raises(RuntimeError) as e:
                    call()
                assert op in str(e.value) and arg in str(e.value), "%s / %s: the message names neither %s nor %s: %s" % (binding, label, op, arg, e.value)
                if dest is not None and dest.is_cuda:
                    assert bool((dest.view(torch.int32) == SENT32).all()), "%s / %s wrote into its destination" % (binding, label)
            torch.cuda.synchronize()
    ran = [e.key for e in prof.key_averages() if KERNEL_RE.search(e.key)]
    assert not ran, "%s: a refused call launched %s" % (binding, ran)


def test_a_tensor_on_another_device_is_refused():
    """every operator runs on its first tensor's device: a later tensor on another one is refused with the same message under both bindings"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from estdepth_amd import ops
    other = torch.device("cuda:1")
    eye, dv = torch.eye(4, device=DEV), torch.tensor([1.0, 2.0], device=DEV)
    kv = _rand((2, 3, 5, 32), 3)
    for binding in ("torch", "ctypes"):
        with _Binding(binding):
            for arg, call in (("ref_proj", lambda: ops.cam_pair_proj(eye, eye.to(other))),
                              ("depth_values", lambda: ops.softargmin_up(_rand((1, 2, 3, 5), 4), dv.to(other), 4)),
                              ("kv_sources[1]", lambda: ops.attention_prewarped(kv, [kv, kv.to(other)])),
                              ("b", lambda: ops.planes_cat_nhwc(_rand((1, 2, 3, 5), 5), _rand((1, 4, 3, 5), 6).to(other)))):
                with pytest.raises(RuntimeError, match=r"%s is on cuda:1 but the operator runs on cuda:0" % re.escape(arg)):
                    call()
            # ... and an operator whose tensors all live on the other device runs there, whatever device is current
            out = ops.cam_pair_proj((eye * 2).to(other), eye.to(other))
            assert out.device == other and torch.equal(out.cpu(), ops.cam_pair_proj(eye * 2, eye).cpu())

