"""Scene writer and float64 chain for the end-to-end tests of tools/run_stream.py (tests/test_run_stream_cpu.py, tests/test_gpu_run_stream.py).
A plain helper module of the test suite (not a conftest); host only.

The scene is track_ref's analytic three-body scene (the plane z = 2.6 and two spheres) seen from ``track_ref.scene_poses(n, seed=2)`` at
640 x 480 WITH THE READER'S OWN INTRINSICS (``eval_io.scaled_intrinsics``: the reader hard-codes them, so a scene it is to read must be made
with them), stored through ``eval_io.write_synthetic_scene`` (ScanNet layout, uint16 millimetres).  ``read_back`` returns what the tool is
fed -- the millimetre depths, the float32 poses and K of ``SequenceReader`` -- and every reference of the suites is evaluated FROM THOSE
VALUES, not from the analytic ones; the analytic surface only enters through ``surface_distance``.

The tool's targets under ``--lwindow 3`` are frames 1 .. n - 2, in order; its volume is centred on the frustum of frame 0 between
``--depth_min`` and ``--depth_max`` (``frustum_volume``).  ``fuse64`` = tsdf_ref.integrate of the targets + tsdf_ref.extract.

Figures of the scene (tests/test_run_stream_cpu.py asserts them): 10 frames, 8 targets, volume 96 x 128 x 128 at 3 cm, depths 0.5 .. 3.1 m:
depths 1.46 .. 2.96 m without a hole; every sample of all 10 frames at least a truncation distance inside the volume; millimetre storage
error <= 0.5 mm; the float64 integration of the 8 targets updates 227 406 voxels with an ambiguous share of 0.0217 (cap 0.03) and the
extraction gives 9 848 points whose distance to the analytic surface has median 0.0034 voxel and 95th percentile 0.151 voxel.
"""
import importlib.util
import os

import numpy as np
import torch

import track_ref as T
import tsdf_ref as R

IMAGE_SIZE = (640, 480)                      # (W, H) of the stored frames
N_FRAMES, LWINDOW = 10, 3
DIMS, VOXEL, DEPTH_MIN, DEPTH_MAX = (96, 128, 128), 0.03, 0.5, 3.1
TRUNC = 4 * VOXEL                            # TSDFVolume's default
MARGIN = 1.25                                # the project's semantic bar (test_gpu_track.MARGIN, tsdf_color_ref.MEDIAN_FACTOR)
POSE_SEED = 2
VOLUME_ARGS = ["--volume-dims"] + [str(d) for d in DIMS] + ["--voxel-size", str(VOXEL), "--depth_min", str(DEPTH_MIN), "--depth_max", str(DEPTH_MAX)]


def load_tool():
    """tools/run_stream.py imported from its path (it is a script, not part of the package)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_stream.py")
    spec = importlib.util.spec_from_file_location("run_stream_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reader_intrinsics(image_size=IMAGE_SIZE):
    """the reader's K for ``image_size`` = (W, H): float32 values as float64 [3,3]"""
    from estdepth_amd.eval_io import scaled_intrinsics
    return scaled_intrinsics(tuple(image_size)).double().numpy()


def smooth_rgb(n, h, w):
    """any smooth image: three low-frequency waves that move with the frame index, uint8 [n,h,w,3]"""
    v, u = np.meshgrid(np.linspace(0.0, 1.0, h), np.linspace(0.0, 1.0, w), indexing="ij")
    out = []
    for i in range(n):
        chans = [127.5 + 100.0 * np.sin(2 * np.pi * (fu * u + fv * v) + 0.3 * i + ph) for fu, fv, ph in ((1.0, 0.5, 0.0), (0.5, 1.5, 1.0), (1.5, 1.0, 2.0))]
        out.append(np.clip(np.rint(np.stack(chans, -1)), 0, 255).astype(np.uint8))
    return np.stack(out)


def write_scene(dir, n_frames, *, corrupt=0.0, drift_from=None, seed):
    """Render and store the scene -> dict(poses [n,4,4] f64: the TRUE poses, written [n,4,4] f64: the poses on disk, clean [n,H,W] f64: the
    analytic depths, depths [n,H,W] f64: the depths handed to the writer, bad [n,H,W] bool, K [3,3] f64, rgb).  ``corrupt``: that share of
    each frame's pixels is replaced by a depth drawn uniformly in the scene's own depth range (RandomState(seed), in the style of
    consistency_ref.corrupted_stack).  ``drift_from=k``: the poses of frames >= k are written as track_ref.perturbed(pose)."""
    from estdepth_amd.eval_io import write_synthetic_scene
    w, h = IMAGE_SIZE
    K = reader_intrinsics()
    poses = T.scene_poses(n_frames, seed=POSE_SEED)
    clean = np.stack([T.scene_maps(P, K, h, w)[0] for P in poses])
    rng = np.random.RandomState(seed)
    bad = rng.uniform(size=clean.shape) < corrupt
    lo, hi = float(clean[clean > 0].min()), float(clean.max())
    depths = np.where(bad, rng.uniform(lo, hi, size=clean.shape), clean)
    written = np.stack([T.perturbed(P) if (drift_from is not None and i >= drift_from) else P for i, P in enumerate(poses)])
    rgb = smooth_rgb(n_frames, h, w)
    write_synthetic_scene(str(dir), list(rgb), list(depths), list(written))
    return dict(poses=poses, written=written, clean=clean, depths=depths, bad=bad, K=K, rgb=rgb)


def read_back(dir, image_size=IMAGE_SIZE):
    """what the tool is fed -> dict(depths [n,h,w] f32 (native size, invalid = 0), poses [n,4,4] f32, K [3,3] f32 (of ``image_size``), imgs
    [n,3,H,W] f32 at ``image_size``, names)"""
    from estdepth_amd.eval_io import SequenceReader
    reader = SequenceReader(str(dir), image_size=tuple(image_size), depth_min=DEPTH_MIN, depth_max=DEPTH_MAX, frame_interval=1)
    frames = [reader[i] for i in range(len(reader))]
    return dict(depths=np.stack([f["dmap"][0, 0].numpy() for f in frames]), poses=np.stack([f["cam_pose"][0].numpy() for f in frames]),
                K=frames[0]["cam_intr"][0].numpy(), imgs=np.stack([f["img"][0].numpy() for f in frames]), names=[f["img_path"] for f in frames])


def nearest_index64(n_out, n_in):
    """the index formula of nearest neighbour on pixel centres, exact: output sample i has its centre at (i + 0.5) n_in / n_out in input
    pixels (edges on integers) and reads the input sample that holds it, floor((2 i + 1) n_in / (2 n_out)) in integer arithmetic"""
    i = np.arange(n_out, dtype=np.int64)
    return np.minimum(((2 * i + 1) * int(n_in)) // (2 * int(n_out)), n_in - 1)


def resample(a, hw):
    """[..., h, w] -> [..., H, W] by nearest neighbour on pixel centres (the tool's maps at another --image-size)"""
    ys, xs = nearest_index64(hw[0], a.shape[-2]), nearest_index64(hw[1], a.shape[-1])
    return a[..., ys, :][..., xs]


def targets_of(n_frames, lwindow=LWINDOW):
    """the frames the tool fuses, in order: the window's middle frame once ``lwindow`` frames are in"""
    return [i - (lwindow - 1) + lwindow // 2 for i in range(lwindow - 1, n_frames)]


def volume_origin(pose0, K, hw):
    """the tool's origin: the volume centred on the first frame's frustum; rounded to fp32 as TSDFVolume stores it"""
    from estdepth_amd.fusion3d import frustum_volume
    org = frustum_volume(torch.as_tensor(pose0), torch.as_tensor(K), hw, DEPTH_MIN, DEPTH_MAX, DIMS, VOXEL)
    return tuple(float(np.float32(v)) for v in org)


def matrices(poses, K, origin):
    """the fp32 matrices the integrate kernel receives for these (fp32) poses and K: the library's own host arithmetic"""
    from estdepth_amd import camera
    return camera.tsdf_matrices(torch.as_tensor(poses), torch.as_tensor(K), torch.tensor(origin, dtype=torch.float32), VOXEL).numpy().reshape(-1, 3, 4)


def integrate_targets(depths, poses, K, origin, dtype=np.float64, D0=None, W0=None):
    """tsdf_ref.integrate of the maps ``depths`` [T,H,W] f32 at ``poses`` [T,4,4], in order, into an empty volume (or D0 / W0)"""
    Z0 = np.zeros(DIMS, np.float32)
    return R.integrate(Z0 if D0 is None else D0, Z0 if W0 is None else W0, matrices(poses, K, origin), depths, None, trunc=TRUNC,
                       z_near=1e-3, dtype=dtype)


def fuse64(depths, poses, K, origin, dtype=np.float64):
    """the chain: integrate the targets, extract the surface -> (integrate's dict, extract's dict)"""
    ref = integrate_targets(depths, poses, K, origin, dtype)
    pts = R.extract(ref["D"].astype(np.float32), ref["Wt"].astype(np.float32), 1.0, VOXEL, origin)
    return ref, pts


def surface_distance(xyz):
    """[N,3] world points -> [N] distance in metres to the analytic surface: min(|z - 2.6|, ||p - c| - r| over the spheres)"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    d = np.abs(p[:, 2] - T.PLANE_Z)
    for centre, radius in T.SPHERES:
        d = np.minimum(d, np.abs(np.linalg.norm(p - np.asarray(centre, np.float64), axis=1) - radius))
    return d


def distance_figures(xyz):
    """(median, 95th percentile) of the distance to the analytic surface, in voxels"""
    d = surface_distance(xyz) / VOXEL
    return float(np.median(d)), float(np.percentile(d, 95))


def backproject(depth, pose, K):
    """[H,W] z-depth (pixel centres on integers) -> [N,3] world points of the valid pixels, float64"""
    depth = np.asarray(depth, np.float64)
    h, w = depth.shape
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ok = depth > 0
    pc = (np.stack([u[ok], v[ok], np.ones(int(ok.sum()))], -1) @ np.linalg.inv(np.asarray(K, np.float64)).T) * depth[ok][:, None]
    P = np.asarray(pose, np.float64)
    return pc @ P[:3, :3].T + P[:3, 3]


# ------------------------------------------------------------------------------------------------------------ CPU stand-ins of the chain
def filter_standin(depths, poses, K, radius=2, min_views=2, dtype=np.float32):
    """consistency_ref.evaluate of every map of the stack against its up-to-``radius`` neighbours on either side (the stream's window and
    its flush see exactly these) -> the maps that are fused: the averaged depth where at least ``min_views`` neighbours agree, else 0"""
    import consistency_ref as C
    n, kept = depths.shape[0], []
    for t in range(n):
        nb = sorted(C.window_sources(t, n, radius))
        out = C.evaluate(depths[t], depths[nb], C.matrices64(poses[t], K, poses[nb], K), dtype=dtype)
        kept.append(np.where(out["views"] >= min_views, out["depth"], 0).astype(np.float32))
    return np.stack(kept)


def track_standin(depths, poses, K, origin, track=True, dtype=np.float32, t_min=1.2):
    """The tool's --track loop with the references in ``dtype``: from the second map on, the model is ray-cast from the volume fused so far
    at the map's own (written) pose (tsdf_raycast_ref.raycast, sampled from ``t_min`` -- in front of the scene -- to the volume's farthest
    corner), the pose refined against it (track_ref.refine, 10 iterations about the volume's centre, dist_max = the truncation distance),
    and the map fused at the refined pose (tsdf_ref.integrate).  -> (the poses fused at [T,4,4] f64, extract's dict of the final volume)"""
    import math
    import tsdf_raycast_ref as RC
    h, w = depths.shape[-2:]
    D, W, used = np.zeros(DIMS, np.float32), np.zeros(DIMS, np.float32), []
    ext = VOXEL * np.array(DIMS[::-1], np.float64)
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64) * ext + np.asarray(origin, np.float64)
    for k in range(depths.shape[0]):
        P = np.asarray(poses[k], np.float64)
        if track and k > 0:
            far = float(((corners - P[:3, 3]) @ P[:3, 2]).max())
            n_steps = int(math.ceil(max(far - t_min, 0.0) / VOXEL)) + 1
            m = RC.raycast(D, W, RC.ray_matrix(P, K, origin, VOXEL), h, w, t_min, VOXEL, n_steps, 1.0, dtype=dtype)
            model = dict(depth=m["depth"].astype(np.float32), normal=m["normal"].astype(np.float32), pose=P, K=K)
            P, _ = T.refine(depths[k], K, P, model, iters=10, pivot=np.asarray(origin, np.float64) + 0.5 * ext, dist_max=TRUNC, z_near=1e-3, dtype=dtype)
        used.append(P)
        ref = integrate_targets(depths[k:k + 1], P[None], K, origin, dtype, D, W)
        D, W = ref["D"].astype(np.float32), ref["Wt"].astype(np.float32)
    return np.stack(used), R.extract(D, W, 1.0, VOXEL, origin)
