"""CPU-only checks of the ray-casting reference (tests/tsdf_raycast_ref.py) and of everything of the render feature that needs no device: the
reference against closed forms (a plane seen head-on, a sphere), camera.tsdf_ray_matrix against the helper's float64 form and as the inverse of
camera.tsdf_matrices, the ambiguous share of every input of the GPU suite with a numpy-fp32 evaluation through the very comparison the GPU
test applies, a plausible wrong kernel that the comparison rejects, render's argument checks, the ESTD_ERR_* returns of estd_tsdf_raycast and
the layout of its descriptor."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tsdf_ref as R
import tsdf_raycast_ref as RR
from helpers import check_desc_layout


@functools.lru_cache(maxsize=3)
def _fused(name):
    """(case, D, Wt): the case's frames fused by the numpy-fp32 evaluation of the integrate contract (the CPU stand-in for the device volume)"""
    c = R.build_case(name)
    mats = R.tsdf_matrices64(c["poses"], c["K"], c["origin"], c["voxel"])
    D, Wt = np.zeros(c["dims"], np.float32), np.zeros(c["dims"], np.float32)
    for _ in range(c["calls"]):
        o = R.integrate(D, Wt, mats, c["depths"], c["confs"], dtype=np.float32, **c["params"])
        D, Wt = o["D"], o["Wt"]
    return c, D, Wt


def _both(c, D, Wt, pose, w_min, t_min=RR.T_MIN):
    v = RR.view(c, pose)
    args = (D, Wt, v["M"], v["H"], v["W"], t_min, v["dt"], v["n_steps"], w_min)
    return RR.raycast(*args), RR.raycast(*args, dtype=np.float32)


def test_plane_head_on_closed_form():
    """an axis-aligned camera in front of the plane z = 2.02: every pixel renders that z-depth, normal (0, 0, -1), the volume's weight"""
    vox, trunc, plane_z, dims, origin = 0.05, 0.2, 2.02, (40, 24, 32), (-0.83, -0.61, 1.0)
    z = origin[2] + (np.arange(dims[0]) + 0.5) * vox
    D = np.broadcast_to(np.clip((plane_z - z) / trunc, -1, 1)[:, None, None], dims).astype(np.float32)
    Wt = np.full(dims, 2.0, np.float32)
    H, W = 30, 40
    K = R.intrinsics(H, W, fov_scale=2.3)
    M = RR.ray_matrix(np.eye(4), K, origin, vox)
    ref = RR.raycast(D, Wt, M, H, W, 0.5, vox, 60, 1.0)
    assert ref["hit"].all() and ref["amb"].mean() <= RR.AMB_CAP
    np.testing.assert_allclose(ref["depth"], plane_z, atol=1e-6)
    np.testing.assert_allclose(ref["normal"], np.broadcast_to([0.0, 0.0, -1.0], (H, W, 3)), atol=1e-6)
    assert (ref["weight"] == 2.0).all()
    got = RR.raycast(D, Wt, M, H, W, 0.5, vox, 60, 1.0, dtype=np.float32)
    RR.compare(got, ref, "plane")
    # w_min above the volume's weight: nothing is observed, nothing hits; a ray that starts behind the plane never finds a front face
    assert not RR.raycast(D, Wt, M, H, W, 0.5, vox, 60, 3.0)["hit"].any()
    assert not RR.raycast(D, Wt, M, H, W, 2.1, vox, 60, 1.0)["hit"].any()


def _sphere_volume(n=48, vox=0.05, radius=0.8, trunc=0.2):
    origin = (-n * vox / 2,) * 3
    c = (np.arange(n) + 0.5) * vox + origin[0]
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    sdf = np.sqrt(x * x + y * y + z * z) - radius             # outside positive: D increases away from the centre
    D = np.clip(sdf / trunc, -1, 1).astype(np.float32)
    W = (np.abs(sdf) < 3 * trunc).astype(np.float32) * 2.0
    return D, W, vox, origin, radius


def test_sphere_depths_and_normals():
    """a sphere seen from outside: depths within a voxel of the analytic ones, normals within O(voxel / radius) of radial, towards the camera"""
    D, Wt, vox, origin, radius = _sphere_volume()
    H, W = 48, 64
    K = R.intrinsics(H, W, fov_scale=1.2)
    pose = R.look_at((0.3, -0.2, -2.5), (0.0, 0.0, 0.0))
    M = RR.ray_matrix(pose, K, origin, vox)
    ref = RR.raycast(D, Wt, M, H, W, 0.5, vox, 80, 1.0)
    ana = R.raycast_scene(pose, K, H, W, plane_z=1e9, centre=(0.0, 0.0, 0.0), radius=radius)
    ana = np.where(ana < 100.0, ana, 0.0)
    hit = ref["hit"]
    assert hit.sum() > 500 and not (hit & (ana == 0)).any()
    assert np.abs(ref["depth"] - ana)[hit].max() < vox
    pts = RR.backproject(ref["depth"], pose, K)[hit]
    radial = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    cos = (ref["normal"][hit] * radial).sum(1)
    assert cos.min() > 1.0 - 2.0 * (vox / radius), cos.min()
    np.testing.assert_allclose(np.linalg.norm(ref["normal"][hit], axis=1), 1.0, atol=1e-12)
    assert (ref["weight"][hit] == 2.0).all() and (ref["depth"][~hit] == 0).all()
    # a camera at the sphere's centre sees only back faces: no hit (front faces only)
    inside = R.look_at((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    assert not RR.raycast(D, Wt, RR.ray_matrix(inside, K, origin, vox), H, W, 0.0, vox, 80, 1.0)["hit"].any()


def test_ray_matrix_matches_helper_and_inverts_tsdf_matrices():
    from estdepth_amd import camera
    c = R.build_case("t3")
    poses = np.concatenate([c["poses"], RR.HELD_OUT_POSE[None]])
    m = camera.tsdf_ray_matrix(torch.from_numpy(poses), torch.from_numpy(c["K"]), c["origin"], c["voxel"])
    assert tuple(m.shape) == (4, 12) and m.dtype == torch.float32 and not m.is_cuda
    for i, P in enumerate(poses):
        a, b = m[i].numpy().reshape(3, 4), RR.ray_matrix(P, c["K"], c["origin"], c["voxel"])
        assert np.abs(a.astype(np.float64) - b).max() <= 2.0 ** -23 * np.abs(b).max()
    one = camera.tsdf_ray_matrix(torch.from_numpy(poses[1]), torch.from_numpy(c["K"]), c["origin"], c["voxel"])
    assert tuple(one.shape) == (1, 12) and torch.equal(one[0], m[1])
    # the inverse of camera.tsdf_matrices: the voxel-index position of pixel (u, v) at z-depth t projects back to (u t, v t, t)
    A = camera.tsdf_matrices(torch.from_numpy(poses), torch.from_numpy(c["K"]), c["origin"], c["voxel"]).numpy().reshape(-1, 3, 4).astype(np.float64)
    for i in range(4):
        Mi = m[i].numpy().reshape(3, 4).astype(np.float64)
        for u, v, t in ((0.0, 0.0, 0.7), (159.0, 119.0, 2.9), (41.0, 97.0, 1.3)):
            p = Mi[:, :3] @ np.array([u, v, 1.0]) * t + Mi[:, 3]
            np.testing.assert_allclose(A[i] @ np.append(p, 1.0), [u * t, v * t, t], rtol=1e-5, atol=2e-4)
    with pytest.raises(RuntimeError, match="cam_intr"):
        camera.tsdf_ray_matrix(torch.from_numpy(poses), torch.eye(3).repeat(2, 1, 1), c["origin"], c["voxel"])


@pytest.mark.parametrize("which", ["held_out", "fused"])
@pytest.mark.parametrize("name,w_min", RR.VALUE_CASES)
def test_ambiguous_share_and_fp32_evaluation(name, w_min, which):
    """every input of the GPU suite: the reference leaves out at most 3 % of the hit pixels, and a numpy-fp32 evaluation of the contract passes
    the comparison the GPU test applies (fp32 arithmetic can reach the bar)"""
    c, D, Wt = _fused(name)
    pose = RR.HELD_OUT_POSE if which == "held_out" else c["poses"][-1]
    ref, got = _both(c, D, Wt, pose, w_min)
    fig = RR.compare(got, ref, "%s w_min %g %s" % (name, w_min, which))
    assert fig["hit"] > 1000 and fig["amb_share"] <= RR.AMB_CAP


def test_full_size_case():
    c, D, Wt = _fused(RR.FULL_CASE[0])
    ref, got = _both(c, D, Wt, RR.HELD_OUT_POSE, RR.FULL_CASE[1])
    fig = RR.compare(got, ref, "full")
    assert fig["hit"] > 100000
    ana = R.raycast_scene(RR.HELD_OUT_POSE, c["K"], *ref["depth"].shape)
    err = np.abs(ref["depth"] - ana)[ref["hit"] & (ana > 0)] / c["voxel"]
    assert np.median(err) <= 0.1 and np.percentile(err, 95) <= 0.5


@pytest.mark.parametrize("name", ["t3", "t8"])
def test_geometry_of_the_reference(name):
    """the bar of the GPU suite's geometry test holds for the float64 reference with a wide margin, and fails a half-voxel convention error"""
    c, D, Wt = _fused(name)
    v = RR.view(c)
    ana = R.raycast_scene(RR.HELD_OUT_POSE, c["K"], v["H"], v["W"])
    ref = RR.raycast(D, Wt, v["M"], v["H"], v["W"], v["t_min"], v["dt"], v["n_steps"], 1.0)
    sel = ref["hit"] & (ana > 0)
    err = np.abs(ref["depth"] - ana)[sel] / c["voxel"]
    assert sel.sum() > 10000 and np.median(err) <= 0.1 / 10 and np.percentile(err, 95) <= 0.5 / 3
    wrong = v["M"].copy()
    wrong[:, 3] += 0.5
    bad = RR.raycast(D, Wt, wrong, v["H"], v["W"], v["t_min"], v["dt"], v["n_steps"], 1.0)
    sel = bad["hit"] & (ana > 0)
    assert np.median(np.abs(bad["depth"] - ana)[sel] / c["voxel"]) > 0.1


def test_comparison_rejects_a_wrong_kernel():
    """the bar is not vacuous: voxel centres at idx instead of idx + 0.5 (a plausible mistake, a 15 mm shift) fail it"""
    c, D, Wt = _fused("t3")
    v = RR.view(c)
    ref = RR.raycast(D, Wt, v["M"], v["H"], v["W"], v["t_min"], v["dt"], v["n_steps"], 1.0)
    wrong = v["M"].copy()
    wrong[:, 3] += 0.5
    got = RR.raycast(D, Wt, wrong, v["H"], v["W"], v["t_min"], v["dt"], v["n_steps"], 1.0, dtype=np.float32)
    with pytest.raises(AssertionError):
        RR.compare(got, ref, "wrong")
    good = RR.raycast(D, Wt, v["M"], v["H"], v["W"], v["t_min"], v["dt"], v["n_steps"], 1.0, dtype=np.float32)
    RR.compare(good, ref, "right")


def test_brick_form_equals_the_whole_volume():
    """raycast on a brick with index_offset (positions in the whole volume's voxel coordinates) == raycast on the whole volume whose
    weights are zero outside the brick"""
    vox, trunc, plane_z, dims, origin = 0.05, 0.2, 2.02, (40, 24, 32), (-0.83, -0.61, 1.0)
    z = origin[2] + (np.arange(dims[0]) + 0.5) * vox
    D = np.broadcast_to(np.clip((plane_z - z) / trunc, -1, 1)[:, None, None], dims).astype(np.float32)
    Wt = np.zeros(dims, np.float32)
    Wt[12:, 4:, 8:] = 2.0
    M = RR.ray_matrix(np.eye(4), R.intrinsics(30, 40, fov_scale=2.3), origin, vox)
    whole = RR.raycast(D, Wt, M, 30, 40, 0.5, vox, 60, 1.0)
    brick = RR.raycast(D[12:, 4:, 8:], Wt[12:, 4:, 8:], M, 30, 40, 0.5, vox, 60, 1.0, index_offset=(8, 4, 12))
    assert whole["hit"].sum() > 100
    for k in ("depth", "normal", "weight", "hit", "amb", "tol_depth"):
        assert np.array_equal(whole[k], brick[k]), k


def _route_views():
    import test_gpu_recon3d_routes as G
    return [("%dx%d" % hw, hw) for hw in G.RAY_SIZES] + [(label, None) for label, _ in G.special_views()]


@pytest.mark.parametrize("label,hw", _route_views())
def test_route_views_ambiguous_share_and_fp32_evaluation(label, hw):
    """the views of tests/test_gpu_recon3d_routes.py on its slab volume: the reference alone stays within the cap (depth and colour), and
    the numpy-fp32 evaluation passes the comparison"""
    import test_gpu_recon3d_routes as G
    import tsdf_color_ref as CR
    s = G._fused_slab()
    view = G.slab_view(*hw) if hw else dict(G.special_views())[label]
    args = (s["D"], s["W"], view["M"], view["H"], view["W"], view["t_min"], view["dt"], view["n_steps"], 1.0)
    ref = RR.raycast(*args)
    fig = RR.compare(RR.raycast(*args, dtype=np.float32), ref, label)
    cref = CR.render_colors(s["D"], s["W"], s["C"], view, 1.0, ray=ref)
    assert fig["amb_share"] <= RR.AMB_CAP and int(cref["amb"].sum()) <= RR.AMB_CAP * fig["hit"]
    assert fig["hit"] >= (max(1, hw[0] * hw[1] // 16) if hw else 0)


@pytest.mark.parametrize("mistake", RR.MISTAKES)
def test_compare_rejects_each_plausible_kernel_mistake(mistake):
    """each plausible mistake of the ray caster, evaluated in fp32 as the kernel would, fails the comparison: a back face from a ray that
    starts inside the sphere, a hit whose first sample lies in an unobserved cell and w > w_min where the observed voxels hold exactly
    w_min (w_min = 3 after three frames)"""
    c, D, Wt = _fused("t3")
    v = RR.view(c)
    t_min, w_min = (1.7, 1.0) if mistake == "back_face" else (v["t_min"], 3.0)
    args = (D, Wt, v["M"], v["H"], v["W"], t_min, v["dt"], v["n_steps"], w_min)
    ref = RR.raycast(*args)
    assert RR.compare(RR.raycast(*args, dtype=np.float32), ref, "right")["hit"] > 1000
    with pytest.raises(AssertionError):
        RR.compare(RR.raycast(*args, dtype=np.float32, mistake=mistake), ref, mistake)


def test_special_views_of_the_gpu_suite():
    """the inputs the GPU suite asserts fixed outcomes on: looking away and from the side (no hit, no ambiguity), t_min inside the sphere
    (front faces only) and behind the plane (no hit at all)"""
    c, D, Wt = _fused("t3")
    flip = np.diag([-1.0, 1.0, -1.0, 1.0])
    for pose in (RR.HELD_OUT_POSE @ flip, R.look_at((30.0, 0.0, 0.0), (30.0, 0.0, 5.0))):
        ref, got = _both(c, D, Wt, pose, 1.0)
        assert not ref["hit"].any() and not ref["amb"].any() and (got["depth"] == 0).all()
    front = _both(c, D, Wt, None, 1.0)[0]
    ref, got = _both(c, D, Wt, None, 1.0, t_min=1.7)
    fig = RR.compare(got, ref, "t3 from t_min 1.7")
    inside_sphere = front["hit"] & (front["depth"] < 1.6)
    assert fig["hit"] > 1000 and inside_sphere.sum() > 1000 and not (ref["hit"] & (ref["depth"] < 2.3) & inside_sphere).any()
    ref, got = _both(c, D, Wt, None, 1.0, t_min=2.72)
    assert ref["hit"].sum() == 0 and (got["depth"][~ref["amb"]] == 0).all()


def test_render_argument_checks_without_device():
    from estdepth_amd import fusion3d
    K, P = torch.tensor(R.intrinsics(120, 160)), torch.eye(4, dtype=torch.float64)
    plan = functools.partial(fusion3d.render_plan, (96, 128, 128), 0.03, (-1.92, -1.92, 0.2), 1e-3)
    mats, hw, t_min, dt, n_steps, stacked = plan(P, K, (120, 160))
    assert tuple(mats.shape) == (1, 12) and hw == (120, 160) and t_min == 1e-3 and dt == 0.03 and not stacked
    far = 0.2 + 96 * 0.03                                              # the volume's far face: every ray has left it there
    assert len(n_steps) == 1 and t_min + (n_steps[0] - 1) * dt >= far > t_min + (n_steps[0] - 3) * dt
    mats, _, _, _, n_steps, stacked = plan(torch.stack([P, torch.from_numpy(RR.HELD_OUT_POSE)]), K, (120, 160), depth_min=0.3, depth_max=3.6, step=0.03)
    assert tuple(mats.shape) == (2, 12) and stacked and n_steps[0] == n_steps[1] and n_steps[0] in (111, 112)
    for bad, match in ((dict(cam_pose=torch.eye(3)), "cam_pose"), (dict(cam_intr=torch.eye(4)), "cam_intr"), (dict(image_hw=(0, 160)), "image_hw"),
                       (dict(image_hw=(120,)), "image_hw"), (dict(depth_min=-1.0), "depth_min"), (dict(step=0.0), "step"),
                       (dict(depth_min=2.0, depth_max=1.0), "depth_max"), (dict(w_min=float("nan")), "w_min"), (dict(step=1e-9), "samples"),
                       (dict(cam_pose=torch.zeros(0, 4, 4)), "at least one"), (dict(cam_intr=torch.zeros(3, 3)), "singular")):
        kw = dict(dict(cam_pose=P, cam_intr=K, image_hw=(120, 160)), **bad)
        with pytest.raises(RuntimeError, match=match):
            plan(kw.pop("cam_pose"), kw.pop("cam_intr"), kw.pop("image_hw"), **kw)


def test_entry_point_validates_without_gpu():
    """null pointers, sizes, step and range: ESTD_ERR_ARG (-1) before any launch; beyond the launch grid: ESTD_ERR_UNSUPPORTED (-3)"""
    from estdepth_amd import _native
    lib = _native.lib()
    assert lib.estd_tsdf_raycast(None, None) == -1
    good = dict(Z=8, Y=8, X=8, H=4, W=4, n_steps=4, t_min=0.0, dt=0.1, w_min=1.0, tsdf=1 << 20, weight=1 << 21, depth=1 << 22, normal=1 << 23,
                out_weight=1 << 24)

    def status(mat0=1.0, **kw):
        d = _native.TsdfRaycastDesc()
        for k, v in dict(good, **kw).items():
            setattr(d, k, v)
        d.mat[0], d.mat[5], d.mat[10] = mat0, 1.0, 1.0
        return lib.estd_tsdf_raycast(ctypes.byref(d), None)
    for bad in (dict(tsdf=None), dict(weight=None), dict(depth=None), dict(normal=None), dict(out_weight=None), dict(H=0), dict(W=0), dict(n_steps=0),
                dict(H=-3), dict(dt=0.0), dict(dt=-0.1), dict(dt=float("inf")), dict(dt=float("nan")), dict(t_min=-0.5), dict(t_min=float("inf")),
                dict(t_min=float("nan")), dict(w_min=float("nan")), dict(X=10), dict(Z=0), dict(mat0=float("nan"))):
        assert status(**bad) == -1, bad
    for big in (dict(Z=70000), dict(X=1 << 21), dict(H=1 << 16, W=1 << 16), dict(n_steps=(1 << 24) + 1)):
        assert status(**big) == -3, big


def test_raycast_desc_struct_layout(tmp_path):
    """sizeof / offsetof of estd_tsdf_raycast_desc as the C compiler sees it == the ctypes mirror"""
    from estdepth_amd import _native
    check_desc_layout(tmp_path, "estd_tsdf_raycast_desc", _native.TsdfRaycastDesc)
    assert ctypes.sizeof(_native.TsdfRaycastDesc) == 40 + 48 + 48
