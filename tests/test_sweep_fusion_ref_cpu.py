"""The fp64 reference of tests/sweep_fusion_ref.py (the bound tests/test_gpu_sweep_fusion_routes.py holds every plane-sweep and EST-fusion
kernel to) on the CPU:
  * its sampling is torch.nn.functional.grid_sample in float64 (4D and 5D, align_corners=False, zeros and border) with the masks applied on
    top; its softmax, GroupNorm, sigmoid and tanh are torch's float64 modules;
  * it agrees with the goldens G1, G3, G5, G12 and with oracle.ref_ops within the bound it states;
  * each plausible kernel mistake of sweep_fusion_ref.MISTAKES, evaluated by the same reference on whole small volumes, fails the bound at
    the loosest route constant, while the correct result rounded to fp32 passes it;
  * every kernel instance the compiler emits for csrc/plane_sweep.hip and csrc/est_fusion.hip is named in the GPU test's instance table
    (or excluded there by name)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fixtures_spec as S
import sweep_fusion_ref as R
from test_gpu_sweep_fusion_routes import C_ROUTE, INSTANCES, NOT_ROUTES

C_MAX = max(C_ROUTE.values())
C_GOLDEN = 16.0                 # the reference's own fp32 rounding order differs from the kernels': a few ulp of A


def _synth_K(H, W):
    from estdepth_amd import synth
    K = synth.intrinsics(H * 4, W * 4).copy()
    K[:2] *= 0.25
    return torch.from_numpy(K)


def _pose(v, motion=1.0):
    from estdepth_amd import synth
    return torch.from_numpy(synth.camera_pose(v, motion=motion))


def _sweep_P(H, W, motion=1.0):
    from oracle import ref_ops as O
    K = _synth_K(H, W).numpy()

    def proj(v):
        e = np.linalg.inv(_pose(v, motion).numpy().astype(np.float64)).astype(np.float32)
        p = e.copy()
        p[:3, :4] = K @ e[:3, :4]
        return p[None]
    P = O.matmul(proj(1), O.inv(proj(0)))[0]
    return torch.from_numpy(np.concatenate([P[:3, :3].reshape(-1), P[:3, 3]]).astype(np.float32))


def _vol_M(H, W, motion=0.7):
    from estdepth_amd import camera
    return camera.relative_volume_matrix((_pose(2, motion) @ torch.linalg.inv(_pose(0)))[None], _synth_K(H, W)[None], "cpu").reshape(30)


def _grid(i, n):
    """un-normalised position -> grid_sample coordinate (align_corners=False)"""
    return (2.0 * i + 1.0) / n - 1.0


# --------------------------------------------------------------------------------------------------------- sampling = grid_sample
@pytest.mark.parametrize("motion", [1.0, 6.0])
def test_plane_sweep_sampling_is_grid_sample_4d(motion):
    C, D, H, W = 3, 4, 9, 13
    g = torch.Generator().manual_seed(1)
    src = torch.randn(C, H, W, generator=g)
    P = _sweep_P(H, W, motion)
    dv = torch.linspace(0.5, 4.0, D)
    ref = R.homo_warping_ref(src, P, dv, D)
    pts = torch.arange(D * H * W)
    d, y, x = R._dhw(pts, D, H, W)
    axes, _ = R._sweep_pos(P, dv.double()[d], x, y, H, W)
    pos = [torch.where(m, torch.full_like(i.v, im), i.v) for (i, m, _, im) in axes]
    grid = torch.stack([_grid(pos[1], W), _grid(pos[0], H)], -1).view(1, D, H * W, 2)
    gs = F.grid_sample(src.double()[None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0].view(C, D, H, W)
    assert torch.allclose(ref.val, gs, atol=1e-12, rtol=0), float((ref.val - gs).abs().max())
    assert (ref.val != 0).float().mean() > 0.3


@pytest.mark.parametrize("border,disp,per_voxel", [(False, False, False), (True, False, False), (False, True, False), (True, False, True)])
def test_volume_sampling_is_grid_sample_5d(border, disp, per_voxel):
    C, D, H, W = 2, 6, 7, 9
    g = torch.Generator().manual_seed(2)
    vol = torch.randn(C, D, H, W, generator=g)
    M = _vol_M(H, W, 2.0)
    dv = torch.linspace(0.5, 4.0, D)
    dmin, dint = 0.5, float(dv[1] - dv[0])
    dsp = (0.25, (2.0 - 0.25) / (D - 1)) if disp else None
    dep = dv.view(D, 1, 1) * (1.0 + 0.03 * torch.randn(D, H, W, generator=g)) if per_voxel else dv
    pad = 0.75
    ref = R.warp_volume_ref(vol, M, dep, dmin, dint, disp=dsp, border=border, padding_value=pad)
    pts = torch.arange(D * H * W)
    d, y, x = R._dhw(pts, D, H, W)
    dd = dep.double().reshape(-1)[pts] if per_voxel else dep.double()[d]
    axes, _ = R._volume_pos(M, dd, x, y, D, H, W, dmin, dint, dsp)
    pos = [torch.where(m, torch.full_like(i.v, im), i.v) for (i, m, _, im) in axes]
    grid = torch.stack([_grid(pos[2], W), _grid(pos[1], H), _grid(pos[0], D)], -1).view(1, D, H, W, 3)
    src = vol.double()[None].clone()
    if border:                                      # the reference pads the outer voxel layer with padding_value
        src[..., 0, :, :] = src[..., -1, :, :] = pad
        src[..., :, 0, :] = src[..., :, -1, :] = pad
        src[..., :, :, 0] = src[..., :, :, -1] = pad
    gs = F.grid_sample(src, grid, mode="bilinear", padding_mode="border" if border else "zeros", align_corners=False)[0]
    assert torch.allclose(ref.val, gs, atol=1e-12, rtol=0), float((ref.val - gs).abs().max())


def test_attention_softmax_and_gru_are_the_float64_modules():
    g = torch.Generator().manual_seed(3)
    n_vox, n = 50, 3
    t = torch.randn(n_vox, 32, generator=g)
    srcs = [torch.randn(n_vox, 32, generator=g) for _ in range(n)]
    r = R.attention_prewarped_ref(t, srcs)
    corr = torch.stack([(t[:, 16:].double() * s[:, 16:].double()).sum(1) for s in srcs], 1)
    a = torch.nn.Softmax(dim=1)(corr)
    h = sum(a[:, j:j + 1] * srcs[j][:, :16].double() for j in range(n)) / n
    assert torch.allclose(r.val[:, 16:], h, atol=1e-13) and torch.equal(r.val[:, :16], t[:, :16].double())
    # GroupNorm(1, 16) in float64 with the statistics groupnorm_finalize computes from the partials
    xh, ru, o = torch.randn(n_vox, 32, generator=g), torch.randn(n_vox, 32, generator=g) * 2 + 0.3, torch.randn(n_vox, 16, generator=g)
    gam, bet = [torch.randn(16, generator=g) for _ in range(4)], [torch.randn(16, generator=g) for _ in range(4)]

    def stats(v):                              # one "block" per voxel: (sum, sum of squares) of each 16-channel group
        p = torch.stack([v[:, :16].sum(1), (v[:, :16] ** 2).sum(1), v[:, 16:].sum(1), (v[:, 16:] ** 2).sum(1)], 1) if v.shape[1] == 32 else \
            torch.stack([v.sum(1), (v ** 2).sum(1), v.sum(1), (v ** 2).sum(1)], 1)
        return R.groupnorm_finalize_ref(p.double(), 16.0 * v.shape[0], 1e-5).val

    def gn(v, w, b):
        m = torch.nn.GroupNorm(1, 16, eps=float(np.float32(1e-5))).double()
        with torch.no_grad():
            m.weight.copy_(w.double())
            m.bias.copy_(b.double())
        return m(v.double().t()[None])[0].t()
    st_ru, st_o = stats(ru), stats(o)
    rr = R.gru_reset_ref(xh, ru, st_ru, gam[0], bet[0])
    want = torch.nn.Sigmoid()(gn(ru[:, :16], gam[0], bet[0])) * xh[:, 16:].double()
    assert torch.allclose(rr.val[:, 16:], want, atol=1e-12), float((rr.val[:, 16:] - want).abs().max())
    rb = R.gru_blend_ref(xh, ru, o, st_ru, st_o, gam[1], bet[1], gam[2], bet[2])
    u = torch.nn.Sigmoid()(gn(ru[:, 16:], gam[1], bet[1]))
    want = u * xh[:, 16:].double() + (1 - u) * torch.nn.Tanh()(gn(o, gam[2], bet[2]))
    assert torch.allclose(rb.val, want, atol=1e-12), float((rb.val - want).abs().max())


def test_groupnorm_finalize_reference_is_exact():
    """mean and rstd from exact sums against float64 numpy on the samples themselves, inside and at the edge of GN_RANGE"""
    g = np.random.default_rng(4)
    for ratio in (0.0, 1.0, R.GN_RANGE):
        x = g.standard_normal((1025, 2, 64)) + ratio * np.array([1.0, -0.5])[None, :, None]
        part = np.stack([x[:, 0].sum(1), (x[:, 0] ** 2).sum(1), x[:, 1].sum(1), (x[:, 1] ** 2).sum(1)], 1)
        r = R.groupnorm_finalize_ref(torch.from_numpy(part), x[:, 0].size, 1e-5)
        for grp in range(2):
            v = x[:, grp].astype(np.longdouble)
            mean = v.mean()
            var = ((v - mean) ** 2).mean()
            rstd = 1.0 / np.sqrt(var + np.longdouble(np.float32(1e-5)))
            assert abs(float(r.val[2 * grp]) - float(mean)) <= 1e-9 * max(1.0, abs(float(mean)))
            # the partial sums of squares themselves carry fp64 rounding: cancellation at ratio^2 ~ 4e6 leaves ~1e-9 relative
            assert abs(float(r.val[2 * grp + 1]) / float(rstd) - 1.0) <= 1e-15 * (1 + 2 * ratio ** 2) * 64
            assert float(r.A[2 * grp + 1]) <= 3.0 * float(r.val[2 * grp + 1])          # a few ulp over the whole stated range


# ------------------------------------------------------------------------------------------------------------ goldens and oracle
def _passes(got, ref, c=C_GOLDEN):
    ratio, n_amb = R.bound_ratio(torch.as_tensor(np.asarray(got)), ref)
    assert ratio <= c, ratio
    assert n_amb <= 1e-3 * ref.n_samples + 2, (n_amb, ref.n_samples)
    return ratio


def _proj_of(sp, rp):
    from oracle import ref_ops as O
    P = O.matmul(sp.numpy(), O.inv(rp.numpy()))[0]
    return torch.from_numpy(np.concatenate([P[:3, :3].reshape(-1), P[:3, 3]]).astype(np.float32))


def test_reference_agrees_with_golden_g1_g12_homo_warping(golden_dir):
    g = np.load(os.path.join(golden_dir, "g1_homo_warping.npz"))
    for name, src, sp, rp, dv in S.g1_cases():
        D = dv.shape[1]
        _passes(g[name][0], R.homo_warping_ref(src[0], _proj_of(sp, rp), dv.reshape(-1), D))
    g12 = np.load(os.path.join(golden_dir, "g12_level1_signatures.npz"))
    src, sp, rp, depth = S.g12_homo_case()
    _passes(g12["homo_per_pixel"][0], R.homo_warping_ref(src[0], _proj_of(sp, rp), depth[0]))


def test_reference_agrees_with_golden_g3_g12_warp_volume(golden_dir):
    from estdepth_amd import camera
    g = np.load(os.path.join(golden_dir, "g3_warp_volume.npz"))
    vol, depth, rel, K, dmin, dint = S.g3_case()
    M = camera.relative_volume_matrix(rel, K, "cpu").reshape(30)
    D = vol.shape[2]
    _passes(g["out"][0], R.warp_volume_ref(vol[0], M, depth.reshape(D, -1)[:, 0], dmin, dint))
    g12 = np.load(os.path.join(golden_dir, "g12_level1_signatures.npz"))
    for name, kw in S.g12_volume_cases().items():
        v = kw["feat_volume"][0]
        C, D, H, W = v.shape
        M = camera.relative_volume_matrix(kw["pose"], kw["cam_intr"], "cpu").reshape(30)
        dep = kw["depth"].reshape(D, H, W)
        per_voxel = "per_voxel" in name
        dsp = (kw["disp_min"], kw["disp_interval"]) if "disp_min" in kw else None
        ref = R.warp_volume_ref(v, M, dep if per_voxel else dep[:, 0, 0], kw["depth_min"], kw["depth_interval"], disp=dsp,
                                border=kw.get("padding_mode") == "border", padding_value=kw.get("padding_value", 0.0))
        _passes(g12["vol_" + name][0], ref)


def test_reference_agrees_with_golden_g5_softargmin(golden_dir):
    g = np.load(os.path.join(golden_dir, "g5_depthlayer.npz"))
    dv, cases = S.g5_cases()
    for name, lg in cases.items():
        rd, rp = R.softargmin_ref(lg, dv.reshape(-1), 4)
        _passes(g[name + "_depth"], rd)
        _passes(g[name + "_prob"], rp)


def test_reference_agrees_with_the_oracle():
    from oracle import ref_ops as O
    g = torch.Generator().manual_seed(5)
    # attention over pre-warped volumes: the oracle's epipolar_attention (channels-first)
    n_vox, n = 40, 4
    t = torch.randn(n_vox, 32, generator=g)
    srcs = [torch.randn(n_vox, 32, generator=g) for _ in range(n)]
    h = O.epipolar_attention(t[:, 16:].t().numpy()[None], [s[:, 16:].t().numpy()[None] for s in srcs],
                             [s[:, :16].t().numpy()[None] for s in srcs])[0].T
    ref = R.attention_prewarped_ref(t, srcs)
    _passes(np.concatenate([t[:, :16].numpy(), h], 1), ref)
    # soft-argmin with its upsampling
    lg = torch.randn(2, 9, 3, 5, generator=g) * 4
    dv = torch.linspace(0.5, 3.0, 9)
    d, p = O.depthlayer_upsampled(lg.numpy(), np.broadcast_to(dv.numpy(), (2, 9)).reshape(2, 9, 1, 1), 2)
    rd, rp = R.softargmin_ref(lg, dv, 2)
    _passes(d, rd)
    _passes(p, rp)
    # the fused warp + attention: oracle warp_volume of K and V, then its attention
    D, H, W = 4, 6, 9
    kv_t, kvs = torch.randn(D, H, W, 32, generator=g), [torch.randn(D, H, W, 32, generator=g) for _ in range(2)]
    K = _synth_K(H, W)
    dvv = torch.linspace(0.5, 4.0, D)
    dint = float(dvv[1] - dvv[0])
    from estdepth_amd import camera
    mats = camera.volume_matrices([_pose(0)[None], _pose(1, 0.7)[None], _pose(2, 0.7)[None]], 1, K[None], "cpu")[0]
    depth = np.broadcast_to(dvv.numpy().reshape(1, 1, D, 1), (1, 1, D, H * W))
    to_c = lambda kv, sl: np.ascontiguousarray(np.moveaxis(kv.numpy()[..., sl], -1, 0))[None]     # noqa: E731
    wk, wv = [], []
    for j in range(2):
        rel = O.matmul(_pose(j + 1, 0.7).numpy()[None], O.inv(_pose(0).numpy()[None]))
        wv.append(O.warp_volume(to_c(kvs[j], slice(0, 16)), depth, rel, K.numpy()[None], None, 0.5, dint))
        wk.append(O.warp_volume(to_c(kvs[j], slice(16, 32)), depth, rel, K.numpy()[None], None, 0.5, dint))
    h = np.moveaxis(O.epipolar_attention(to_c(kv_t, slice(16, 32)), wk, wv)[0], 0, -1)
    ref = R.warp_attention_ref(kv_t, kvs, mats, dvv, 0.5, dint)
    _passes(np.concatenate([kv_t[..., :16].numpy(), h], -1), ref)


def test_camera_references_agree_with_the_host_algebra():
    """the cam_* references against the project's torch-fp32 host composition of the same matrices (estdepth_amd/camera.py)"""
    from estdepth_amd import camera
    K = _synth_K(120, 160)
    pi, pj = _pose(1, 2.0), _pose(3, 2.0)
    host = camera.volume_matrices([pi[None], pj[None]], 1, K[None], "cpu")[0, 0]
    _passes(host, R.cam_volume_mats_ref(pj, pi, K))
    sp, rp = torch.linalg.inv(pj), torch.linalg.inv(pi)
    P = torch.matmul(sp[None], torch.inverse(rp[None]))[0]
    _passes(torch.cat([P[:3, :3].reshape(-1), P[:3, 3]]), R.cam_pair_proj_ref(sp, rp))


# ------------------------------------------------------------------------------------------------------------ planted mistakes
def _m_sweep(mistake):
    """whole small volumes: plane sweep (costvol form) -> (good, bad) Refs"""
    D, H, W = 4, 8, 11
    g = torch.Generator().manual_seed(7)
    src, ref = torch.randn(H, W, 32, generator=g), torch.randn(H, W, 32, generator=g)
    if mistake == "mask_ge_1":
        P, dv = R.exact_sweep_proj(), torch.arange(D, dtype=torch.float32) % 3 + 1.0
    elif mistake == "den_no_eps":
        P, dv = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float32), torch.linspace(2e-8, 8e-8, D)
    elif mistake == "far_corner_dropped":       # near-identity: the last voxels sample the last record
        P, dv = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.3, 0.2, 0], dtype=torch.float32), torch.linspace(1.0, 2.0, D)
    else:
        P, dv = _sweep_P(H, W, 1.0), torch.linspace(0.5, 4.0, D)
    return (R.costvol_ref(src, ref, P, dv, D), R.costvol_ref(src, ref, P, dv, D, mistake=mistake))


def _m_volume(mistake):
    D, H, W = 5, 6, 9
    g = torch.Generator().manual_seed(8)
    kv_t = torch.randn(D, H, W, 32, generator=g)
    kvs = [torch.randn(D, H, W, 32, generator=g) for _ in range(3)]
    dv = torch.linspace(0.5, 4.0, D)
    dmin, dint = 0.5, float(dv[1] - dv[0])
    if mistake == "mask_ge_1":
        M, dmin = R.exact_volume_mats()
        M, dv, dint = M.repeat(3, 1), torch.ones(D), 1.0
    elif mistake == "den_no_eps":
        M = torch.zeros(30)
        M[[0, 4, 8, 9, 14, 19, 21, 25, 29]] = 1.0
        M, dv, dmin, dint = M.repeat(3, 1), torch.linspace(2e-10, 6e-10, D), 0.0, 1e-10
    elif mistake == "far_corner_dropped":
        from estdepth_amd import camera
        K = _synth_K(H, W)
        M = camera.volume_matrices([_pose(0)[None]] + [_pose(j + 1, 0.02)[None] for j in range(3)], 1, K[None], "cpu")[0]
    elif mistake == "softmax_no_max":
        from estdepth_amd import camera
        M = camera.volume_matrices([_pose(0)[None]] + [_pose(j + 1, 0.05)[None] for j in range(3)], 1, _synth_K(H, W)[None], "cpu")[0]
        kv_t[..., 16:] *= 6.0
        for s in kvs:
            s[..., 16:] *= 6.0
    else:
        from estdepth_amd import camera
        M = camera.volume_matrices([_pose(0)[None]] + [_pose(j + 1, 0.7)[None] for j in range(3)], 1, _synth_K(H, W)[None], "cpu")[0]
    return (R.warp_attention_ref(kv_t, kvs, M, dv, dmin, dint), R.warp_attention_ref(kv_t, kvs, M, dv, dmin, dint, mistake=mistake))


def _m_gru(mistake):
    g = torch.Generator().manual_seed(9)
    n = 200
    xh, ru, o = torch.randn(n, 32, generator=g), torch.randn(n, 32, generator=g) * 1.5, torch.randn(n, 16, generator=g) * 2
    st, st_o = torch.tensor([0.1, 0.9, -0.2, 1.1]), torch.tensor([0.3, 0.7, 0.0, 0.0])
    gm, bt = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g) * 0.3
    if mistake == "reset_on_x" or (mistake == "neighbour_gamma"):
        refs = [(R.gru_reset_ref(xh, ru, st, gm, bt), R.gru_reset_ref(xh, ru, st, gm, bt, mistake=mistake))]
        if mistake == "reset_on_x":
            return refs
    else:
        refs = []
    return refs + [(R.gru_blend_ref(xh, ru, o, st, st_o, gm, bt, gm.flip(0), bt, fast=False),
                    R.gru_blend_ref(xh, ru, o, st, st_o, gm, bt, gm.flip(0), bt, mistake=mistake))]


def _m_sam(mistake):
    g = torch.Generator().manual_seed(10)
    lg = torch.randn(2, 9, 3, 33, generator=g) * 3
    dv = torch.linspace(0.5, 4.0, 9)
    rd, _ = R.softargmin_ref(lg, dv, 2)
    bd, _ = R.softargmin_ref(lg, dv, 2, mistake=mistake)
    return [(rd, bd)]                           # (the probability map does not read depth_values)


def _pairs(mistake):
    if mistake in ("align_corners_true", "corner_xy_swapped", "far_corner_dropped", "mask_ge_1", "den_no_eps"):
        return [_m_sweep(mistake), _m_volume(mistake)]
    if mistake in ("softmax_no_max", "no_mean_over_views"):
        return [_m_volume(mistake)]
    if mistake in ("blend_u_swapped", "reset_on_x", "neighbour_gamma"):
        return _m_gru(mistake)
    return _m_sam(mistake)


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_bound_rejects_each_plausible_kernel_mistake(mistake):
    for good, bad in _pairs(mistake):
        r, n_amb = R.bound_ratio(good.val.float(), good)
        assert r <= 1.0, (mistake, r, n_amb)
        ratio, _ = R.bound_ratio(bad.val.float(), good)
        assert ratio > C_MAX, "%s slips under the bound (worst ratio %.1f <= %g)" % (mistake, ratio, C_MAX)


# ------------------------------------------------------------------------------------------------------------ instance table
def test_every_emitted_instance_is_named_in_the_route_table():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is not installed")
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    from test_gpu_glue2d_routes import INSTANCES as GLUE          # the 2D glue kernels of est_fusion.hip are that suite's routes
    glue_routes = {k for ks in GLUE.values() for k in ks}
    named = {k for ks in INSTANCES.values() for k in ks}
    emitted = set()
    for f in ("plane_sweep.hip", "est_fusion.hip"):
        rec, _ = kr.resource_usage(os.path.join(kr.CSRC, f), isa=False)
        for name in kr.demangle(list(rec)).values():
            m = re.search(r"(\w+_kernel)(<[^>()]*>)?\(", name)
            assert m, name
            emitted.add(m.group(1) + (m.group(2) or ""))
    glue = emitted & glue_routes                   # whatever of these two files the glue suite claims (tests/test_kernel_ledger_cpu.py
    assert glue and not glue & named               # holds every claim to exactly one suite)
    assert emitted - set(NOT_ROUTES) - glue == named, (sorted(emitted - set(NOT_ROUTES) - glue - named), sorted(named - emitted))
    assert set(NOT_ROUTES) <= emitted
