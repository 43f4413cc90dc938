"""The host layer over the mesh rasteriser (estdepth_amd/mesh_render.py: render_mesh, mesh_visibility, visible_points, visible_mask;
cloud_metrics.compare_meshes(visible=); TSDFVolume.compare(visible=)) on the device.

Geometry, at the ray-cast's bars (README, TSDF row: |depth - analytic| at most 0.1 voxel in the median and 0.5 voxel at the 95th
percentile of the hit pixels).  The float64 chain -- tsdf_mesh_ref.mesh of the volume, then the reference rasteriser of
tests/mesh_raster_ref.py -- has to meet the bars on the CPU first; figures in voxels, median / p95:

    the fused 0.37 m sphere, 120 x 160 from 1.3 m         chain 0.0414 / 0.1153    device 0.0414 / 0.1153
    the eight-view analytic scene at the held-out pose    chain 0.0018 / 0.1167    device 0.0018 / 0.1168

Facing: the triangles of extract_mesh run counter-clockwise seen from the free side, so every covered pixel of the sphere's render has
facing = +1, the chain's and the device's.  The scene's render cannot say the same, and the float64 chain shows it: 3 of its 18626
covered pixels at the held-out pose (1 to 3 at each of the fusion poses tried) have facing = -1.  They look at the walls that TSDF
fusion raises along the rays grazing a silhouette, which tests/test_gpu_tsdf_mesh.py documents (21 of the reference mesh's 16686
triangles face none of the eight eyes): a property of the fused volume, not of the mesher or the rasteriser.  There the check is that
every covered pixel has facing +1 or -1 and that the share of -1 stays below that documented share of the triangles, 21 / 16686.

Attributes: colours and vertex normals interpolated with bary, against mesh_sample_ref.interpolate on the device's own face and bary
maps, within that module's bound (one fp32 rounding per operation of a + b1 (b - a) + b2 (c - a)), held to 2 x; for a normalised
normal n = p / |p| a perturbation d of p moves n by at most 2 |d| / |p|, and the fp32 normalisation adds at most 4 roundings."""
import numpy as np
import pytest
import torch

from estdepth_amd.cloud_metrics import compare_meshes
from estdepth_amd.fusion3d import sample_mesh
from estdepth_amd.mesh_render import mesh_visibility, render_mesh, visible_mask, visible_points

import mesh_raster_ref as R
import mesh_sample_ref as MS
import track_ref as T
import tsdf_mesh_ref as M
import tsdf_raycast_ref as RR
import tsdf_ref as TR
from test_gpu_mesh_raster_routes import WITHOUT_LOAD as RASTER, profiled
from test_gpu_recon3d_routes import _cpu, _dev

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MEDIAN_BAR, P95_BAR = 0.1, 0.5                                     # voxels: the ray-cast's bars
HW = (120, 160)
U32 = MS.U32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _np(out):
    return {k: (_cpu(v) if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _figures(depth, analytic, voxel):
    hit = (depth > 0) & (analytic > 0)
    err = np.abs(depth.astype(np.float64) - analytic)[hit] / voxel
    return int(hit.sum()), float(np.median(err)), float(np.percentile(err, 95))


def sphere_depth(centre, radius, pose, K, H, W):
    """z-depth of the near intersection of every pixel's ray with the sphere, 0 without one, float64"""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = (np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T) @ pose[:3, :3].T
    oc = pose[:3, 3] - np.asarray(centre)
    a, b, c = (d * d).sum(-1), d @ oc, oc @ oc - radius * radius
    disc = b * b - a * c
    return np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, 0.0)


def sphere_case():
    D, W, origin, centre = M.sphere_volume()
    pose = R.look_at(centre + np.asarray([0.35, -0.25, -1.2]), centre)
    K = R.intrinsics(*HW, f=260.0)
    return D, W, origin, pose, K, sphere_depth(centre, M.SPHERE_R, pose, K, *HW), M.VOXEL


def scene_case():
    """eight views of the three-body scene fused in float64 on the host (tests/test_gpu_tsdf_mesh.py's set-up), seen from the held-out pose"""
    dims, origin = (96, 128, 128), (-1.92, -1.92, 0.2)
    K = TR.intrinsics(*HW)
    poses = TR.scene_poses(8, seed=2)
    depths = np.stack([T.scene_maps(P, K, *HW)[0] for P in poses]).astype(np.float32)
    return dims, origin, poses, K, depths, RR.HELD_OUT_POSE, T.scene_maps(RR.HELD_OUT_POSE, K, *HW)[0], TR.VOXEL


def chain_render(D, W, origin, voxel, pose, K):
    ref = M.mesh(D, W, 1.0, voxel, origin)
    xyz, faces = ref["xyz"].astype(np.float32), ref["faces"].astype(np.int32)
    return xyz, faces, R.raster(xyz, faces, R.raster_matrix(pose, K), *HW, 1e-3, box=True)


WALL_SHARE = 21.0 / 16686.0          # tests/test_gpu_tsdf_mesh.py: the reference mesh's triangles that face none of the eyes


def _render_volume(vol, pose, K, what, analytic, voxel, chain, closed):
    mesh = vol.extract_mesh()
    out = profiled(RASTER, lambda: render_mesh(mesh, torch.from_numpy(pose), torch.from_numpy(K), HW))
    got = _np(out)
    n, med, p95 = _figures(got["depth"], analytic, voxel)
    n_c, med_c, p95_c = _figures(chain["depth"], analytic, voxel)
    print("MESH-RENDER %s: %d triangles, %d hit pixels; |depth - analytic| in voxels, median / p95: device %.4f / %.4f, float64 chain %.4f / %.4f"
          % (what, mesh["faces"].shape[0], n, med, p95, med_c, p95_c))
    assert n_c > 3000 and med_c <= MEDIAN_BAR and p95_c <= P95_BAR, "the float64 chain misses the bars"
    assert n > 3000 and med <= MEDIAN_BAR and p95 <= P95_BAR
    covered = got["face"] >= 0
    away, away_c = int((got["facing"] == -1).sum()), int((chain["facing"] == -1).sum())
    print("MESH-RENDER %s: facing -1 on %d of %d covered pixels (float64 chain: %d of %d)" % (what, away, covered.sum(), away_c, (chain["face"] >= 0).sum()))
    assert covered.sum() >= n and np.all(np.abs(got["facing"][covered]) == 1) and np.all(got["facing"][~covered] == 0)
    if closed:
        assert away == 0 == away_c
    else:
        assert away <= WALL_SHARE * covered.sum() and away_c <= WALL_SHARE * (chain["face"] >= 0).sum()
    assert np.all((got["depth"] > 0) == covered) and got["invalid"] == 0
    # face normals: the triangle's, from mesh_area's kernel; towards the camera on every covered pixel
    from estdepth_amd import ops
    fn = _cpu(ops.mesh_face_area(mesh["xyz"], mesh["faces"])[1])
    assert np.array_equal(got["normal"][covered], fn[got["face"][covered]]) and np.all(got["normal"][~covered] == 0)
    return mesh, got


@pytest.mark.parametrize("where", ["d64", "d64-rotated", "d512"])
def test_the_rasteriser_away_from_the_origin(where):
    """three crossing triangles and their camera 64 m and 512 m out, and 64 m out in a turned world (tests/placement.py), against the
    float64 reference TO THE BIT, as everywhere in this family: the kernel projects the fp32 vertices in float64 in the contract's order,
    so the large M_j3 cancels against the large coordinates exactly as it does in numpy"""
    import placement as PL
    from estdepth_amd import ops
    from test_gpu_mesh_raster_routes import as_got
    case = R.placed_case(PL.PLACES[where])
    xyz, faces, mat, H, W, zn = case
    got = as_got(ops.mesh_raster(_dev(xyz), _dev(faces), torch.from_numpy(np.ascontiguousarray(mat)), H, W, zn))
    fig = R.compare(got, R.raster(*case), "interpenetrating@%s" % where)
    print("PLACEMENT mesh_raster interpenetrating@%s: %d pixels covered by %d faces, equal to the reference's bits" % (where, fig["covered"], fig["seen"]))
    assert fig["seen"] == 3 and fig["covered"] > 300


def test_render_of_the_fused_sphere():
    from estdepth_amd.fusion3d import TSDFVolume
    D, W, origin, pose, K, analytic, voxel = sphere_case()
    vol = TSDFVolume(D.shape, voxel, origin, device=DEV)
    vol.volume.copy_(_dev(np.stack([D, W])))
    _render_volume(vol, pose, K, "sphere", analytic, voxel, chain_render(D, W, origin, voxel, pose, K)[2], closed=True)


@pytest.fixture(scope="module")
def scene():
    from estdepth_amd.fusion3d import TSDFVolume
    dims, origin, poses, K, depths, pose, analytic, voxel = scene_case()
    vol = TSDFVolume(dims, voxel, origin, device=DEV)
    vol.integrate(_dev(depths), torch.from_numpy(poses), torch.from_numpy(K))
    torch.cuda.synchronize()
    return vol, poses, K, pose, analytic, voxel, origin


def test_render_of_the_eight_view_scene(scene):
    vol, poses, K, pose, analytic, voxel, origin = scene
    host = vol.volume.cpu().numpy()
    _render_volume(vol, pose, K, "scene", analytic, voxel, chain_render(host[0], host[1], origin, voxel, pose, K)[2], closed=False)


def test_colour_and_vertex_normals_are_interpolated_with_bary(scene):
    vol, poses, K, pose, _, _, _ = scene
    mesh = dict(vol.extract_mesh())
    xyz = _cpu(mesh["xyz"])
    mesh["color"] = _dev((127.5 + 100.0 * np.sin(3.0 * xyz + np.asarray([0.0, 1.0, 2.0]))).astype(np.float32))
    out = _np(render_mesh(mesh, torch.from_numpy(pose), torch.from_numpy(K), HW, normals="vertex"))
    hit = out["face"] >= 0
    faces, face, bary = _cpu(mesh["faces"]), out["face"][hit], out["bary"][hit]
    want, bound = MS.interpolate(_cpu(mesh["color"]), faces, face, bary)
    worst_c = MS._worst(out["color"][hit].astype(np.float64) - want, bound)
    p, pb = MS.interpolate(_cpu(mesh["normal"]), faces, face, bary)
    length = np.linalg.norm(p, axis=1, keepdims=True)
    ok = length[:, 0] > 1e-3
    n_bound = 2.0 * np.linalg.norm(pb, axis=1, keepdims=True) / length + 4.0 * U32
    worst_n = MS._worst((out["normal"][hit].astype(np.float64) - p / length)[ok], np.repeat(n_bound, 3, 1)[ok])
    print("MESH-RENDER attributes: %d pixels; of the bounds (2 allowed): colour %.3f, vertex normal %.3f" % (hit.sum(), worst_c, worst_n))
    assert hit.sum() > 3000 and ok.mean() > 0.999 and worst_c <= 2.0 and worst_n <= 2.0
    assert np.all(out["color"][~hit] == 0) and np.all(out["normal"][~hit] == 0)
    # the point a + b1 (b - a) + b2 (c - a) lies on its pixel's ray at the rendered depth
    pts, m = R.points_of(out, xyz, faces)
    q = R.project(R.raster_matrix(pose, K), pts.astype(np.float32))
    v, u = np.nonzero(m)
    assert np.abs(q[:, 0] / q[:, 2] - u).max() < 2e-3 and np.abs(q[:, 1] / q[:, 2] - v).max() < 2e-3
    assert np.abs(q[:, 2] - out["depth"][m]).max() < 1e-5
    # no normals, no colour: the keys are left out; uint8 rgb counts as colour; a host mesh is moved to the device
    bare = render_mesh(dict(xyz=xyz, faces=faces, rgb=np.full((xyz.shape[0], 3), 200, np.uint8)), pose, K, HW, normals=None)
    assert "normal" not in bare and np.array_equal(_cpu(bare["depth"]), out["depth"])
    assert set(np.unique(_cpu(bare["color"]).round())) == {0.0, 200.0}
    assert "color" not in render_mesh(mesh, pose, K, HW, normals=None, color=False)
    for bad, text in ((dict(normals="smooth"), "normals must be"), (dict(image_hw=(0, 4)), "image_hw")):
        kw = dict(image_hw=HW)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="render_mesh: " + text):
            render_mesh(mesh, pose, K, **kw)
    with pytest.raises(RuntimeError, match="normals='vertex' needs"):
        render_mesh(dict(xyz=xyz, faces=faces), pose, K, HW, normals="vertex")


def test_visibility_counts_sum_to_the_covered_pixels(scene):
    vol, poses, K, pose, _, _, _ = scene
    mesh = vol.extract_mesh()
    vis = mesh_visibility(mesh, torch.from_numpy(poses[:3]), torch.from_numpy(K), HW)
    assert vis["pixels"].dtype == torch.int64 and vis["pixels"].shape[0] == mesh["faces"].shape[0] and tuple(vis["depth"].shape) == (3, *HW)
    assert int(vis["pixels"].sum()) == int(vis["covered"].sum()) == int((vis["depth"] > 0).sum()) and vis["invalid"] == 0
    one = render_mesh(mesh, poses[1], K, HW, normals=None, color=False)
    assert torch.equal(one["depth"], vis["depth"][1])
    assert 0 < int((vis["pixels"] > 0).sum()) < mesh["faces"].shape[0]           # some triangles own no pixel


def _wall_and_box():
    """a 4 m x 3 m wall at z = 2.6 (two triangles) and a box 0.8 x 0.6 x 0.3 m in front of it, seen from two cameras"""
    wall = np.asarray([(-2, -1.5, 2.6), (2, -1.5, 2.6), (2, 1.5, 2.6), (-2, 1.5, 2.6)], np.float64)
    lo, hi = np.asarray([-0.4, -0.3, 1.5]), np.asarray([0.4, 0.3, 1.8])
    corners = np.asarray([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [(0, 1, 2), (0, 2, 3)] + [t for a, b, c, d in quads for t in ((a + 4, b + 4, c + 4), (a + 4, c + 4, d + 4))]
    xyz = np.concatenate([wall, corners]).astype(np.float32)
    poses = np.stack([np.eye(4), R.look_at((0.8, 0.0, 0.0), (0.0, 0.0, 2.6))])
    return xyz, np.asarray(faces, np.int32), poses, R.intrinsics(*HW, f=90.0), lo, hi


def _ray_hits_box(eye, pts, lo, hi):
    """slab test of the segments eye -> pts against the box [lo, hi]"""
    d = pts - eye
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - eye) / d, (hi - eye) / d
    near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    return (near <= far) & (far > 0) & (near < 1)


def test_samples_in_a_shadow_are_dropped():
    xyz, faces, poses, K, lo, hi = _wall_and_box()
    mesh = dict(xyz=xyz, faces=faces)
    wall = sample_mesh(dict(xyz=xyz[:4], faces=faces[:2]), n=20000, seed=4)
    pts = _cpu(wall["xyz"])
    tol = 0.05
    for view in (slice(0, 1), slice(1, 2), slice(0, 2)):
        P = poses[view]
        vis = mesh_visibility(mesh, torch.from_numpy(P), torch.from_numpy(K), HW)
        views = visible_points(wall["xyz"], vis["depth"], torch.from_numpy(P), torch.from_numpy(K), tol)
        mats = [R.raster_matrix(p, K) for p in P]
        want_depth = [R.raster(xyz, faces, m, *HW, 1e-3)["depth"] for m in mats]
        assert all(np.array_equal(_cpu(vis["depth"][i]).view(np.uint32), want_depth[i].view(np.uint32)) for i in range(len(mats)))
        want = R.visible_points(pts, want_depth, mats, tol)
        got = _cpu(views)
        assert got.dtype == np.int32 and np.array_equal(got, want)               # the counts equal the float64 reference's exactly
        keep, again = visible_mask(mesh, wall["xyz"], P, K, HW, min_views=len(mats), tol=tol)
        assert torch.equal(again, views) and np.array_equal(_cpu(keep), want >= len(mats))
    # one camera at the origin: what lies in the box's shadow is dropped, the rest of the wall inside the image is kept (the box grown
    # and shrunk by the footprint of a pixel at its distance keeps the test off the shadow's border)
    P, m = poses[:1], R.raster_matrix(poses[0], K)
    got = _cpu(visible_points(wall["xyz"], mesh_visibility(mesh, torch.from_numpy(P), torch.from_numpy(K), HW)["depth"], P, K, tol))
    q = R.project(m, pts)
    in_image = (np.abs(q[:, 0] / q[:, 2] - (HW[1] - 1) / 2) < HW[1] / 2 - 2) & (np.abs(q[:, 1] / q[:, 2] - (HW[0] - 1) / 2) < HW[0] / 2 - 2)
    pad = 2.0 * hi[2] / K[0, 0] * np.asarray([1, 1, 0])
    shadow, near_shadow = _ray_hits_box(np.zeros(3), pts.astype(np.float64), lo + pad, hi - pad), _ray_hits_box(np.zeros(3), pts.astype(np.float64), lo - pad, hi + pad)
    # (a sample within a pixel's footprint of the wall's border may have its nearest pixel centre beside the wall)
    foot = 2.6 / K[0, 0]
    interior = (np.abs(pts[:, 0]) < 2.0 - foot) & (np.abs(pts[:, 1]) < 1.5 - foot)
    assert shadow.sum() > 500 and np.all(got[shadow] == 0) and np.all(got[in_image & interior & ~near_shadow] == 1)
    print("MESH-RENDER shadow: %d of %d wall samples seen, %d in the box's shadow, %d outside the image" % (got.sum(), got.size, shadow.sum(), (~in_image).sum()))


def test_compare_meshes_with_and_without_visible():
    xyz, faces, poses, K, lo, hi = _wall_and_box()
    gt = dict(xyz=xyz, faces=faces)
    pred = dict(xyz=xyz[:4] + np.asarray([0, 0, 0.01], np.float32), faces=faces[:2])
    before = profiled(set(), lambda: compare_meshes(pred, gt, 2500.0, threshold=0.05, max_dist=1.0))
    same = profiled(set(), lambda: compare_meshes(pred, gt, 2500.0, threshold=0.05, max_dist=1.0, visible=None))
    assert before == same and "n_gt_visible" not in before["sampled"]            # nothing new is launched, the previous output's bits
    vis = dict(cam_poses=torch.from_numpy(poses[:1]), cam_intr=torch.from_numpy(K), image_hw=HW)
    got = profiled(RASTER, lambda: compare_meshes(pred, gt, 2500.0, threshold=0.05, max_dist=1.0, visible=vis))
    blk = got["sampled"]
    assert blk["n_gt"] == before["sampled"]["n_gt"] and 0 < blk["n_gt_visible"] == got["n_gt"] < blk["n_gt"]
    assert blk["visible_share"] == blk["n_gt_visible"] / blk["n_gt"]
    # the box's hidden sides and the wall behind it leave: what is left of the ground truth is matched better; the predicted samples are
    # the same, and those behind the box have lost the ground truth they lay on
    assert got["recall"] > before["recall"] and got["n_pred"] == before["n_pred"] and got["accuracy"] >= before["accuracy"]
    with pytest.raises(RuntimeError, match="compare_meshes: visible= needs a ground truth with faces"):
        compare_meshes(pred, dict(xyz=xyz), 2500.0, visible=vis)
    with pytest.raises(RuntimeError, match="compare_meshes: visible must be a dict"):
        compare_meshes(pred, gt, 2500.0, visible=dict(cam_poses=poses))


def test_volume_compare_passes_visible_on(scene):
    vol, poses, K, pose, _, voxel, _ = scene
    gt = {k: v for k, v in vol.extract_mesh().items() if k in ("xyz", "faces")}
    plain = vol.compare(gt, sample=1.0 / voxel ** 2)
    assert plain == vol.compare(gt, sample=1.0 / voxel ** 2, visible=None)
    vis = dict(cam_poses=torch.from_numpy(poses), cam_intr=torch.from_numpy(K), image_hw=HW, min_views=1)
    got = vol.compare(gt, sample=1.0 / voxel ** 2, visible=vis)
    assert 0.5 * plain["n_gt"] < got["n_gt_visible"] <= plain["n_gt"] and got["n_pred"] == plain["n_pred"]
    with pytest.raises(RuntimeError, match="compare: visible= needs sample"):
        vol.compare(gt, visible=vis)
