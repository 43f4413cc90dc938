"""CPU-only checks of the TSDF reference (tests/tsdf_ref.py) and of everything of the TSDF feature that needs no device: the reference
against closed forms, the ambiguous share of every GPU case's fixture, a numpy-fp32 evaluation through the very comparison the GPU test
applies, the extraction reference on an analytic sphere, TSDFVolume's argument checks and the ESTD_ERR_ARG returns of both entry points."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_ref as R
from helpers import check_desc_layout


def _mats(case):
    from estdepth_amd import camera
    m = camera.tsdf_matrices(torch.from_numpy(case["poses"]), torch.from_numpy(case["K"]), case["origin"], case["voxel"])
    return m.numpy().reshape(-1, 3, 4)


def test_plane_head_on_closed_form():
    """a plane seen head-on by an axis-aligned camera: D = (plane_z - voxel_z) / trunc inside the band, 1 in front of it, untouched behind"""
    H, W, vox, trunc, plane_z = 60, 80, 0.05, 0.2, 2.0
    K = R.intrinsics(H, W)
    mats = R.tsdf_matrices64(np.eye(4)[None], K, (-0.4, -0.3, 1.0), vox)
    depth = np.full((1, H, W), plane_z, dtype=np.float32)
    Z0 = np.zeros((40, 12, 16), np.float32)
    ref = R.integrate(Z0, Z0, mats, depth, trunc=trunc)
    vz = 1.0 + (np.arange(40) + 0.5) * vox
    assert ref["updated"].any()
    for iz in range(40):
        upd = ref["updated"][iz]
        sdf = plane_z - vz[iz]
        if sdf < -trunc - 1e-6:
            assert not upd.any()
        elif sdf > -trunc + 1e-6:
            assert upd.all()
            np.testing.assert_allclose(ref["D"][iz], min(1.0, sdf / trunc), atol=1e-6)
            assert (ref["Wt"][iz] == 1).all()
    assert (ref["D"][~ref["updated"]] == 0).all() and (ref["Wt"][~ref["updated"]] == 0).all()


def test_matrices_match_reference_helper():
    """estdepth_amd.camera.tsdf_matrices (torch, float64) == the helper's numpy float64 form up to the fp32 rounding of the result"""
    c = R.build_case("t3")
    a, b = _mats(c), R.tsdf_matrices64(c["poses"], c["K"], c["origin"], c["voxel"])
    assert a.shape == b.shape == (3, 3, 4)
    assert np.abs(a.astype(np.float64) - b).max() <= 2.0 ** -23 * np.abs(b).max()
    # a voxel centre projects where the pinhole model puts it
    idx = np.array([17.0, 40.0, 55.0, 1.0])
    world = np.asarray(c["origin"]) + (idx[:3] + 0.5) * c["voxel"]
    cam = np.linalg.inv(c["poses"][1]) @ np.append(world, 1.0)
    pix = c["K"] @ cam[:3]
    np.testing.assert_allclose(a[1].astype(np.float64) @ idx, pix, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_ambiguous_share_and_fp32_evaluation(name):
    """every GPU case's fixture: the reference leaves out at most 3 % of the updated voxels, and a numpy-fp32 evaluation of the contract
    passes the comparison the GPU test applies (fp32 arithmetic can reach the bar)"""
    c = R.build_case(name)
    mats = _mats(c)
    D0 = np.zeros(c["dims"], np.float32)
    W0 = np.zeros(c["dims"], np.float32)
    for _ in range(c["calls"]):
        ref = R.integrate(D0, W0, mats, c["depths"], c["confs"], **c["params"])
        got = R.integrate(D0, W0, mats, c["depths"], c["confs"], dtype=np.float32, **c["params"])
        fig = R.compare(got["D"], got["Wt"], ref, weighted=c["params"]["weighted"], D_before=D0, W_before=W0)
        assert fig["amb_share"] <= R.AMB_CAP
        if name == "away":
            assert fig["updated"] == 0
        else:
            assert fig["updated"] > 1000
        D0, W0 = got["D"], got["Wt"]
    if name == "second":
        assert W0.max() == 4.0           # the clamp at w_max was reached


def test_comparison_rejects_a_wrong_kernel():
    """the bar is not vacuous: pixel centres on half-integers (a plausible mistake) fail it"""
    c = R.build_case("t3")
    mats = _mats(c)
    Z0 = np.zeros(c["dims"], np.float32)
    ref = R.integrate(Z0, Z0, mats, c["depths"], None, **c["params"])
    wrong = mats.copy()
    wrong[:, 0] += 0.5 * wrong[:, 2]
    got = R.integrate(Z0, Z0, wrong, c["depths"], None, dtype=np.float32, **c["params"])
    with pytest.raises(AssertionError):
        R.compare(got["D"], got["Wt"], ref)


@pytest.mark.parametrize("name", sorted(R.ROUTE_CASES))
def test_route_cases_ambiguous_share_and_fp32_evaluation(name):
    """the small cases of tests/test_gpu_recon3d_routes.py: the same two properties under the same cap"""
    c = R.build_case(name)
    mats = _mats(c)
    Z0 = np.zeros(c["dims"], np.float32)
    ref = R.integrate(Z0, Z0, mats, c["depths"], None, **c["params"])
    got = R.integrate(Z0, Z0, mats, c["depths"], None, dtype=np.float32, **c["params"])
    fig = R.compare(got["D"], got["Wt"], ref, D_before=Z0, W_before=Z0)
    assert fig["amb_share"] <= R.AMB_CAP and fig["updated"] >= 4
    # the brick form: any sub-range of the volume evaluates to the same values at the volume's own indices
    Z, Y, X = c["dims"]
    rng = ((Z // 2, Z), (Y // 3, Y), (4 * (X // 8), X))
    sl = tuple(slice(a, b) for a, b in rng)
    brick = R.integrate(Z0[sl], Z0[sl], mats, c["depths"], None, voxel_range=rng, **c["params"])
    for k in ("D", "Wt", "A", "updated", "amb"):
        assert np.array_equal(brick[k], ref[k][sl]), k


def test_big_volume_bricks_ambiguous_share_and_brick_forms():
    """the bricks of the 520 x 1024 x 1024 case of tests/test_gpu_recon3d_routes.py: each within the cap on its own, the fp32 evaluation
    passes; and the brick form of the extraction gives the whole volume's records (ids, positions, normals) away from the brick's faces"""
    import test_gpu_recon3d_routes as G
    case = G.big_case()
    mats = _mats(case)
    Z0 = np.zeros((8, 16, 64), np.float32)
    for b in G.BIG_BRICKS:
        rng = G.big_brick_range(b)
        assert all(lo % s == 0 and hi <= d for (lo, hi), s, d in zip(rng, (8, 16, 64), G.BIG_DIMS))
        ref = R.integrate(Z0, Z0, mats, case["depths"], None, voxel_range=rng, **case["params"])
        got = R.integrate(Z0, Z0, mats, case["depths"], None, voxel_range=rng, dtype=np.float32, **case["params"])
        fig = R.compare(got["D"], got["Wt"], ref, D_before=Z0, W_before=Z0)
        assert fig["amb_share"] <= R.AMB_CAP and (fig["updated"] > 1000) == (b != (0, 0, 0))
    assert tuple(b + s for b, s in zip(G.BIG_BRICKS[3], (8, 16, 64))) == G.BIG_DIMS            # the last brick of the volume
    D, W, vox, origin, _ = _sphere_volume(n=24)
    whole = R.extract(D, W, 1.0, vox, origin)
    rng = ((6, 24), (0, 20), (4, 24))
    part = R.extract(D[6:, :20, 4:], W[6:, :20, 4:], 1.0, vox, origin, voxel_range=rng, dims=D.shape)
    idx = part["edge"] // 3
    keep = (idx // (24 * 24) >= 8) & ((idx // 24) % 24 < 17) & (idx % 24 >= 6)
    sel = np.isin(whole["edge"], part["edge"][keep])
    assert keep.sum() > 100 and sel.sum() == keep.sum()
    for k in ("xyz", "normal", "weight", "tol_xyz"):
        assert np.array_equal(part[k][keep], whole[k][sel]), k


@pytest.mark.parametrize("mistake", R.INTEGRATE_MISTAKES)
def test_compare_rejects_each_integrate_mistake(mistake):
    """each plausible mistake of the integrate kernel, evaluated in fp32 as the kernel would, fails the comparison the GPU suites apply
    (eight frames into a volume whose weight is capped at 4, so that the cap is reached)"""
    c = R.build_case("r8x16x64-t8-120x160")
    mats, params = _mats(c), dict(c["params"], w_max=4.0)
    Z0 = np.zeros(c["dims"], np.float32)
    ref = R.integrate(Z0, Z0, mats, c["depths"], None, **params)
    good = R.integrate(Z0, Z0, mats, c["depths"], None, dtype=np.float32, **params)
    assert R.compare(good["D"], good["Wt"], ref)["updated"] > 1000 and good["Wt"].max() == 4.0
    bad = R.integrate(Z0, Z0, mats, c["depths"], None, dtype=np.float32, mistake=mistake, **params)
    with pytest.raises(AssertionError):
        R.compare(bad["D"], bad["Wt"], ref)


def _sphere_volume(n=48, vox=0.05, radius=0.8, trunc=0.2):
    origin = (-n * vox / 2,) * 3
    c = (np.arange(n) + 0.5) * vox + origin[0]
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    sdf = np.sqrt(x * x + y * y + z * z) - radius             # outside positive: D increases away from the centre
    D = np.clip(sdf / trunc, -1, 1).astype(np.float32)
    W = (np.abs(sdf) < 3 * trunc).astype(np.float32) * 2.0
    return D, W, vox, origin, radius


def test_extraction_reference_on_a_sphere():
    D, W, vox, origin, radius = _sphere_volume()
    ref = R.extract(D, W, 1.0, vox, origin)
    # the crossing count equals a direct count
    obs = W >= 1.0
    n = 0
    for axis in range(3):
        a = np.moveaxis(D, axis, 0)
        o = np.moveaxis(obs, axis, 0)
        n += int((o[:-1] & o[1:] & (((a[:-1] < 0) & (0 <= a[1:])) | ((a[1:] < 0) & (0 <= a[:-1])))).sum())
    assert len(ref["edge"]) == n > 1000
    assert len(np.unique(ref["edge"])) == n
    # points within a voxel of the surface
    r = np.linalg.norm(ref["xyz"], axis=1)
    assert np.abs(r - radius).max() < vox
    # normals point outward (towards increasing D): the gradient of a sampled sphere deviates from the radial direction by O(voxel / radius)
    radial = ref["xyz"] / r[:, None]
    cos = (ref["normal"] * radial).sum(1)
    assert cos.min() > 1.0 - 2.0 * (vox / radius), cos.min()
    np.testing.assert_allclose(np.linalg.norm(ref["normal"], axis=1), 1.0, atol=1e-12)
    assert (ref["weight"] == 2.0).all()


@pytest.mark.parametrize("mistake", R.EXTRACT_MISTAKES)
def test_compare_points_rejects_each_extraction_mistake(mistake):
    """each plausible mistake of the extraction, evaluated by the reference itself, fails compare_points: on a sphere (curved, so a
    one-sided difference tilts the normal), and for the double count on a ramp through a voxel that is exactly zero"""
    if mistake == "cross_counted_twice":
        x = np.arange(8, dtype=np.float32)
        D = np.broadcast_to(0.25 * (x - 3.0), (4, 4, 8)).astype(np.float32).copy()
        W, vox, origin = np.full((4, 4, 8), 2.0, np.float32), 0.1, (0.0, 0.0, 0.0)
        assert (D[..., 3] == 0).all()
    else:
        D, W, vox, origin, _ = _sphere_volume(n=24)
    ref = R.extract(D, W, 1.0, vox, origin)
    bad = R.extract(D, W, 1.0, vox, origin, mistake=mistake)
    as_got = lambda r: {k: r[k].astype(np.float32) if k != "edge" else r[k] for k in ("edge", "xyz", "normal", "weight")}       # noqa: E731
    R.compare_points(as_got(ref), ref)
    if mistake == "cross_counted_twice":
        assert len(bad["edge"]) == 2 * len(ref["edge"]) == 32
    with pytest.raises(AssertionError):
        R.compare_points(as_got(bad), ref)


def test_extraction_one_sided_and_unobserved_neighbours():
    """a crossing next to the border and next to an unobserved voxel uses one-sided differences; an isolated pair has only its own edge"""
    D = np.ones((4, 4, 8), np.float32)
    W = np.zeros((4, 4, 8), np.float32)
    D[1, 1, 0], D[1, 1, 1] = -0.5, 0.5
    W[1, 1, 0] = W[1, 1, 1] = 3.0
    ref = R.extract(D, W, 1.0, 0.1, (0.0, 0.0, 0.0))
    assert list(ref["edge"]) == [3 * ((1 * 4 + 1) * 8 + 0) + 0]
    np.testing.assert_allclose(ref["xyz"][0], [0.1, 0.15, 0.15])
    np.testing.assert_allclose(ref["normal"][0], [1.0, 0.0, 0.0])
    assert ref["weight"][0] == 3.0


def test_volume_argument_checks_without_device():
    from estdepth_amd import fusion3d
    with pytest.raises(RuntimeError, match="multiple of 4"):
        fusion3d.TSDFVolume((8, 8, 10), 0.05, (0, 0, 0), device="cpu")
    with pytest.raises(RuntimeError, match="three positive"):
        fusion3d.TSDFVolume((8, 8), 0.05, (0, 0, 0), device="cpu")
    with pytest.raises(RuntimeError, match="voxel_size"):
        fusion3d.TSDFVolume((8, 8, 8), 0.0, (0, 0, 0), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion3d.TSDFVolume((8, 8, 8), 0.05, (0, 0, 0), device="cpu")
    chk = fusion3d.TSDFVolume.check_frames
    d, K, P = torch.ones(3, 1, 6, 8), torch.eye(3), torch.eye(4).repeat(3, 1, 1)
    depths, confs, poses, n = chk(d, P, K)
    assert n == 3 and len(depths) == 3 and confs == [] and tuple(depths[0].shape) == (6, 8)
    with pytest.raises(RuntimeError, match="poses"):
        chk(d, P[:2], K)
    with pytest.raises(RuntimeError, match="confidence"):
        chk(d, P, K, conf=torch.ones(3, 6, 9))
    with pytest.raises(RuntimeError, match="confidence maps"):
        chk(d, P, K, conf=torch.ones(2, 6, 8))
    with pytest.raises(RuntimeError, match="weighted"):
        chk(d, P, K, weighted=True)
    with pytest.raises(RuntimeError, match="T,H,W"):
        chk(torch.ones(6, 8), P, K)
    assert fusion3d.frame_groups(3) == [(0, 3)]
    assert fusion3d.frame_groups(8) == [(0, 8)]
    assert fusion3d.frame_groups(19) == [(0, 8), (8, 16), (16, 19)]


def test_frustum_volume_is_centred():
    from estdepth_amd import fusion3d
    K = torch.tensor(R.intrinsics(120, 160))
    org = fusion3d.frustum_volume(torch.eye(4), K, (120, 160), 0.5, 4.0, (64, 32, 128), 0.1)
    centre = np.asarray(org) + 0.5 * 0.1 * np.array([128, 32, 64])
    np.testing.assert_allclose(centre, [0.0, 0.0, 2.25], atol=1e-9)


def test_entry_points_validate_without_gpu():
    """null pointers, T outside 1..8, a misaligned X, bad sizes: ESTD_ERR_ARG (-1) before any launch"""
    from estdepth_amd import _native
    lib = _native.lib()
    assert lib.estd_tsdf_integrate(None, None) == -1
    good = dict(Z=8, Y=8, X=8, T=1, H=4, W=4, trunc=0.1, z_near=0.0, conf_min=0.0, w_max=8.0, tsdf=1 << 20, weight=1 << 21)

    def desc(**kw):
        d = _native.TsdfIntegrateDesc()
        for k, v in dict(good, **kw).items():
            setattr(d, k, v)
        return d
    for bad in (dict(), dict(T=0, depth0=1), dict(T=9, depth0=1), dict(X=10, depth0=1), dict(tsdf=None, depth0=1), dict(trunc=0.0, depth0=1),
                dict(H=0, depth0=1), dict(weighted=1, depth0=1), dict(w_max=float("nan"), depth0=1), dict(Z=0, depth0=1)):
        bad = dict(bad)
        has_depth = bad.pop("depth0", 0)
        d = desc(**bad)
        if has_depth:
            for t in range(8):
                d.depth[t] = 1 << 22
        assert lib.estd_tsdf_integrate(ctypes.byref(d), None) == -1, bad
    d = desc(Z=70000)
    d.depth[0] = 1 << 22
    assert lib.estd_tsdf_integrate(ctypes.byref(d), None) == -3           # ESTD_ERR_UNSUPPORTED: beyond the launch grid
    org = (ctypes.c_float * 3)(0, 0, 0)
    fake = ctypes.c_void_p(1 << 20)
    ext = lib.estd_tsdf_extract_points
    assert ext(None, None, 8, 8, 8, 0.1, org, 1.0, None, 0, None, None, None, None, None) == -1
    assert ext(fake, fake, 8, 8, 10, 0.1, org, 1.0, fake, 0, None, None, None, None, None) == -1       # X % 4
    assert ext(fake, fake, 8, 8, 8, 0.0, org, 1.0, fake, 0, None, None, None, None, None) == -1        # voxel size
    assert ext(fake, fake, 8, 8, 8, 0.1, org, 1.0, fake, -1, None, None, None, None, None) == -1       # capacity
    assert ext(fake, fake, 8, 8, 8, 0.1, org, 1.0, fake, 4, None, None, None, None, None) == -1        # capacity without outputs
    assert ext(fake, fake, 8, 8, 8, 0.1, None, 1.0, fake, 0, None, None, None, None, None) == -1       # origin
    assert ext(fake, fake, 8, 8, 8, 0.1, org, 1.0, None, 0, None, None, None, None, None) == -1        # counter


def test_tsdf_desc_struct_layout(tmp_path):
    """sizeof/offsetof of estd_tsdf_integrate_desc as the C compiler sees it == the ctypes mirror."""
    from estdepth_amd import _native, ops
    frames, = check_desc_layout(tmp_path, "estd_tsdf_integrate_desc", _native.TsdfIntegrateDesc, macros=["ESTD_TSDF_MAX_FRAMES"])
    assert frames == ops.TSDF_MAX_FRAMES == _native.TSDF_MAX_FRAMES
    assert ctypes.sizeof(_native.TsdfIntegrateDesc) == 48 + 16 + 128 + 384
