"""Stand-alone timing of csrc/tsdf.hip on an MI355X (device events, warm-up, many repetitions; not part of bench.py).

    python tools/tsdf_bench.py [--reps 200] [--out profiles/tsdf_bench.txt]

Three 640 x 480 depth maps of the analytic plane-plus-sphere scene of tests/tsdf_ref.py, fused into a 256^3 and a 512 x 512 x 256 volume at
3 cm, each centred on the first camera's frustum between depth_min and depth_max the way tools/run_stream.py --fuse places it:
  (a) one T = 3 integrate call               (b) three T = 1 calls on the same data (the plain design (a) exists to beat)
  (c) (a) with the frustum skip compiled out (every voxel loaded and stored)          (d) the point extraction (count + records)
For (a): bytes moved per voxel touched and the share of the 6.3 TB/s streaming rate an MI355X reaches (a roofline, not a pass bar), and the
fuse time beside the 15 ms Joint step it follows.  A 1 GiB buffer is rewritten (untimed) in front of every timed call, so the volume is
read from HBM as it is behind a model step, not from the Infinity Cache.

    python tools/tsdf_bench.py --raycast [--reps 200] [--out profiles/tsdf_raycast_bench.txt]

times csrc/tsdf_raycast.hip instead: one 640 x 480 render (TSDFVolume.render, default range and step) of the 256^3 volume above after the
T = 3 fuse, from the first fused camera and from the held-out pose of tests/tsdf_raycast_ref.py, with the kernel's own counters (samples
whose weights / whose D values were read per ray), beside the fuse + extract pass and the Joint step.

    python tools/tsdf_bench.py --color [--reps 200] [--out profiles/tsdf_color_bench.txt]

times the colour path beside the plain one on the 256^3 volume: the T = 3 fuse with and without colour (estd_tsdf_integrate_color: five
planes per touched group instead of two), the edge colours of the extracted points, and the 640 x 480 render with and without a colour map
from the held-out pose.  The two plain figures are the ones to hold against another commit's.

    python tools/tsdf_bench.py --mesh [--reps 200] [--out profiles/tsdf_mesh_bench.txt]

times TSDFVolume.extract_mesh (csrc/mesh/tsdf_mesh.hip: surface nets) on the 256^3 volume after the T = 3 fuse, beside extract_points:
the four kernel launches (cells and faces, each counting and then filling) and the host ordering behind them (two sorts, the binary
search of the cell ids, the triangle split) separately, each between device events, and the whole call with its two count read-backs.

    python tools/tsdf_bench.py --mesh-components [--reps 100] [--out profiles/mesh_components_bench.txt]

times the connected components of that mesh (csrc/mesh/mesh_components.hip) and fusion3d.filter_mesh: the operator (its four launches)
and the whole filter between device events, each call behind the cache flush, the four kernels one by one from the profiler's device
times over the same calls, beside the yardstick -- the same labels by scipy.sparse.csgraph.connected_components on the host, the copies
included, or where scipy is missing a min-label propagation loop in torch on the device.

    python tools/tsdf_bench.py --mesh-sample [--reps 100] [--out profiles/mesh_sample_bench.txt]

times the mesh sampling (csrc/mesh/mesh_sample.hip) on that mesh and on the 204 800-triangle grid of tests/mesh_components_ref.py: the
area kernel, the sample kernel at 10^5 and 10^6 samples and the whole fusion3d.sample_mesh, between device events, behind the cache flush
and back to back, beside the same sampling formed with torch operators on the same prefix sums.

    python tools/tsdf_bench.py --mesh-raster [--reps 100] [--out profiles/mesh_raster_bench.txt]

times the mesh rasteriser (csrc/mesh/mesh_raster.hip) at 640 x 480: the raster kernel with and without the load in front of its atomic,
the resolve kernel and the whole mesh_render.render_mesh, between device events, behind the cache flush and back to back -- for that
mesh from the held-out pose of the ray-cast bench, for a 204 800-triangle grid that fills the image, for a two-triangle wall that fills
it (the large-box regime) and for 4096 coincident small triangles (the contention regime) -- beside TSDFVolume.render of the same volume
from the same pose.

    python tools/tsdf_bench.py --mesh-distance [--reps 20] [--out profiles/mesh_distance_bench.txt]

times the point-to-mesh distance (csrc/mesh/mesh_distance.hip): the two binning kernels, the whole TriangleGrid build and the search at
10^5 and 10^6 queries against that mesh and a 204 800-triangle height field, the 170-triangle ground truth of the run-stream tests on the big
list alone, and cloud_metrics.compare_meshes with and without exact=True -- medians between device events after a warm-up -- beside the
same minimum formed with torch operators (a chunked brute force over all triangles).

    python tools/tsdf_bench.py --register [--reps 20] [--out profiles/rigid_align_bench.txt]

times the rigid registration (csrc/track/rigid_align.hip) on 10^5 and 10^6 samples of that mesh against the mesh moved by a fixed twist:
the apply, system and reduce kernels apart, one whole iteration split into search and system, and the same sums formed with torch
operators (gathers, einsum, .sum() in float64) on the same device.

    python tools/tsdf_bench.py --mesh-simplify [--reps 50] [--parent-tree DIR] [--out profiles/mesh_simplify_bench.txt]

times the mesh simplification (csrc/mesh/mesh_simplify.hip) on that mesh and on the 204 800-triangle height field: the two kernels apart
and the whole fusion3d.simplify_mesh -- medians of warm calls between device events -- beside the same sums formed with torch operators
(gathers and index_add_ in float64).  --parent-tree DIR (a built checkout of the parent commit) adds the gate: the default extract_mesh of
both trees in alternating pairs of fresh processes.

    python tools/tsdf_bench.py --cloud-knn [--reps 30] [--parent-tree DIR] [--out profiles/cloud_knn_bench.txt]

times the k-nearest-neighbour search and the PCA normals (csrc/cloud/cloud_knn.hip) at k = 8, 16, 32 on the cloud extracted from that
volume and on a 200 704-point height field: the two kernels apart, the whole cloud_metrics.estimate_normals and the candidates examined
per query, beside the same result with torch operators (cdist + topk, gathers, batched linalg.eigh) where the distance matrix fits.
--parent-tree DIR adds compare_clouds with default arguments in both trees, in alternating pairs of fresh processes.

    python tools/tsdf_bench.py --global-register [--reps 30] [--parent-tree DIR] [--out profiles/global_register_bench.txt]

times the four kernels of the global registration (csrc/register/global_register.hip) and the whole register_global on that volume's
cloud against itself moved and on the 200 704-point height field thinned to 2 cm and to 5 cm, the matcher beside torch.cdist + argmin on
the same descriptors and the hypothesis scoring beside the same sums with torch operators.  --parent-tree DIR adds compare_clouds and
register with default arguments in both trees, in alternating pairs of fresh processes.

    python tools/tsdf_bench.py --cloud-cluster [--reps 30] [--parent-tree DIR] [--out profiles/cloud_cluster_bench.txt]

times the density-based clustering (csrc/cloud/cloud_cluster.hip) on that volume's cloud and on the 200 704-point height field at eps of 2
and 4 point spacings: the four kernels apart (the profiler's device times), the entry point and the whole cloud_metrics.cluster_dbscan --
medians of warm calls -- beside the same partition from torch operators (cdist, masks, argmin) and scipy's connected_components on the
first 16 384 points.  --parent-tree DIR adds compare_clouds with default arguments and mesh_components in both trees, in alternating pairs
of fresh processes."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_BPS = 6.3e12          # achievable HBM streaming rate of an MI355X
JOINT_STEP_MS = 15.5         # the Joint step a T = 3 fuse follows (README: 15.43-15.58 ms)


def timed(fn, reps, flush=None, warmup=10):
    """mean ms per call over ``reps`` calls, each between its own pair of device events; ``flush``: a buffer larger than the 256 MB
    Infinity Cache that is rewritten (untimed) in front of every call, so the call finds the volume in HBM as it does behind a model step"""
    for _ in range(warmup):
        fn()
    pairs = []
    for i in range(reps):
        if flush is not None:
            flush.fill_(float(i))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return float(np.mean([a.elapsed_time(b) for a, b in pairs]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--raycast", action="store_true", help="time the ray caster (csrc/tsdf_raycast.hip) instead of integrate / extract")
    ap.add_argument("--mesh", action="store_true", help="time extract_mesh (kernels and host ordering apart) beside extract_points")
    ap.add_argument("--mesh-components", action="store_true", help="time the mesh components and filter_mesh beside a host / torch yardstick")
    ap.add_argument("--mesh-sample", action="store_true", help="time the mesh sampling (csrc/mesh/mesh_sample.hip) beside the same sampling with torch operators")
    ap.add_argument("--mesh-raster", action="store_true", help="time the mesh rasteriser (csrc/mesh/mesh_raster.hip) beside TSDFVolume.render")
    ap.add_argument("--mesh-distance", action="store_true", help="time the point-to-mesh distance (csrc/mesh/mesh_distance.hip) beside a torch "
                    "brute force; writes profiles/mesh_distance_bench.txt unless --out says otherwise")
    ap.add_argument("--register", action="store_true", help="time the rigid registration (csrc/track/rigid_align.hip): its kernels, one whole "
                    "iteration and the same sums with torch operators; writes profiles/rigid_align_bench.txt unless --out says otherwise")
    ap.add_argument("--mesh-simplify", action="store_true", help="time the mesh simplification (csrc/mesh/mesh_simplify.hip): its kernels, the whole "
                    "simplify_mesh and the same sums with torch operators; writes profiles/mesh_simplify_bench.txt unless --out says otherwise")
    ap.add_argument("--cloud-knn", action="store_true", help="time the k-nearest-neighbour search and the PCA normals (csrc/cloud/cloud_knn.hip): its "
                    "kernels, the whole estimate_normals and the same result with torch operators; writes profiles/cloud_knn_bench.txt unless --out "
                    "says otherwise")
    ap.add_argument("--global-register", action="store_true", help="time the global registration (csrc/register/global_register.hip): its four "
                    "kernels, the whole register_global, the matcher beside torch.cdist + argmin and the hypothesis scoring beside torch operators; "
                    "writes profiles/global_register_bench.txt unless --out says otherwise")
    ap.add_argument("--cloud-cluster", action="store_true", help="time the density-based clustering (csrc/cloud/cloud_cluster.hip): its four kernels, "
                    "the entry point, the whole cluster_dbscan and the same partition with torch operators and scipy; writes "
                    "profiles/cloud_cluster_bench.txt unless --out says otherwise")
    ap.add_argument("--parent-tree", metavar="DIR", help="with --mesh-simplify: a built checkout of the parent commit; the default extract_mesh of both "
                    "trees is timed in alternating pairs of fresh processes (with --cloud-knn: the default compare_clouds; with --global-register: "
                    "the default compare_clouds and register)")
    ap.add_argument("--color", action="store_true", help="time the colour fuse, the edge colours and the colour render beside the plain figures")
    args = ap.parse_args()
    if args.register:
        args.out = args.out or os.path.join(ROOT, "profiles", "rigid_align_bench.txt")
        return register_main(args)
    if args.mesh_simplify:
        args.out = args.out or os.path.join(ROOT, "profiles", "mesh_simplify_bench.txt")
        return simplify_main(args)
    if args.cloud_knn:
        args.out = args.out or os.path.join(ROOT, "profiles", "cloud_knn_bench.txt")
        return knn_main(args)
    if args.global_register:
        args.out = args.out or os.path.join(ROOT, "profiles", "global_register_bench.txt")
        return global_register_main(args)
    if args.cloud_cluster:
        args.out = args.out or os.path.join(ROOT, "profiles", "cloud_cluster_bench.txt")
        return cluster_main(args)
    if args.raycast:
        return raycast_main(args)
    if args.mesh:
        return mesh_main(args)
    if args.mesh_components:
        return components_main(args)
    if args.mesh_sample:
        return sample_main(args)
    if args.mesh_raster:
        return raster_main(args)
    if args.mesh_distance:
        args.out = args.out or os.path.join(ROOT, "profiles", "mesh_distance_bench.txt")
        return distance_main(args)
    if args.color:
        return color_main(args)
    import tsdf_ref as R
    from estdepth_amd import camera, ops
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax = 480, 640, 3, 0.03, 0.1, 10.0
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    dl = [depths[t] for t in range(T)]
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB
    lines = ["tsdf_bench: %d x %d maps, T = %d, voxel %.3f m, %d repetitions per figure, %s" % (W, H, T, vox, args.reps, torch.cuda.get_device_name(0))]
    for dims in ((256, 256, 256), (256, 512, 512)):
        origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
        vol = TSDFVolume(dims, vox, origin, device=dev)
        mats = camera.tsdf_matrices(torch.from_numpy(poses), torch.from_numpy(K), vol.origin, vox)
        n_vox = dims[0] * dims[1] * dims[2]

        def fuse(group, no_skip=False):
            ops.tsdf_integrate_(vol.volume, dl[group], [], mats[group].contiguous(), vol.trunc, vol.z_near, 0.0, False, vol.w_max, no_skip)

        # steady state of a stream: the volume already holds earlier frames of the same neighbourhood.  Which voxels a call reads and
        # writes depends on the maps and matrices alone, not on the volume's state, so every repetition does the same work.
        fuse(slice(0, T))
        torch.cuda.synchronize()
        touched = int((vol.volume[1] > 0).sum().item())
        groups16 = int((vol.volume[1].reshape(-1, 4) > 0).any(1).sum().item())          # 16-byte groups the kernel reads and writes
        t_a = timed(lambda: fuse(slice(0, T)), args.reps, flush)
        t_b = timed(lambda: [fuse(slice(t, t + 1)) for t in range(T)], args.reps, flush)
        t_c = timed(lambda: fuse(slice(0, T), no_skip=True), args.reps, flush)
        t_a_warm = timed(lambda: fuse(slice(0, T)), args.reps)
        pts = vol.extract_points()
        t_d_count = timed(lambda: ops.tsdf_extract_points(vol.volume, vox, vol.origin, 1.0, 0), args.reps, flush)
        t_d = timed(lambda: ops.tsdf_extract_points(vol.volume, vox, vol.origin, 1.0, pts["count"]), args.reps, flush)
        vol_bytes = groups16 * 4 * 16.0                    # D and Wt groups, read and written once
        map_bytes = T * H * W * 4.0
        floor_ms = (vol_bytes + map_bytes) / STREAM_BPS * 1e3
        lines += [
            "volume %d x %d x %d (Z Y X), origin (%.2f, %.2f, %.2f): %d voxels, %d updated (%.1f %%), %d of %d 16-byte groups (%.1f %%)"
            % (dims + origin + (n_vox, touched, 100.0 * touched / n_vox, groups16, n_vox // 4, 400.0 * groups16 / n_vox)),
            "  (a) one T=3 call           %8.3f ms" % t_a,
            "  (b) three T=1 calls        %8.3f ms   (a)/(b) = %.2f" % (t_b, t_a / t_b),
            "  (c) (a) without the skip   %8.3f ms   (a)/(c) = %.2f" % (t_c, t_a / t_c),
            "  (d) extraction             %8.3f ms count only, %.3f ms with %d records" % (t_d_count, t_d, pts["count"]),
            "  (a) volume traffic %.1f MB = %.1f bytes per voxel touched (+ %.1f MB of depth maps); at %.1f TB/s that is %.3f ms: (a) runs at %.1f %% "
            "of the streaming rate" % (vol_bytes / 1e6, vol_bytes / max(touched, 1), map_bytes / 1e6, STREAM_BPS / 1e12, floor_ms, 100.0 * floor_ms / t_a),
            "  (a) beside the %.1f ms Joint step it follows: %.1f %% of the step" % (JOINT_STEP_MS, 100.0 * t_a / JOINT_STEP_MS),
            "  (a) back to back, no cache flush between calls: %.3f ms" % t_a_warm,
        ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def mesh_main(args):
    import tsdf_ref as R
    from estdepth_amd import ops
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume, mesh_edge_stats
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    m = vol.extract_mesh()
    pts = vol.extract_points()
    n_v, n_q = m["count"], int(m["edge"].shape[0])
    stats = mesh_edge_stats(m["faces"])
    v, o = vol.volume, vol.origin
    t_pts = timed(lambda: ops.tsdf_extract_points(v, vox, o, 1.0, pts["count"]), args.reps, flush)
    t_vc = timed(lambda: ops.tsdf_mesh_vertices(v, None, vox, o, 1.0, 0), args.reps, flush)
    t_vf = timed(lambda: ops.tsdf_mesh_vertices(v, None, vox, o, 1.0, n_v), args.reps, flush)
    t_fc = timed(lambda: ops.tsdf_mesh_faces(v, 1.0, 0), args.reps, flush)
    t_ff = timed(lambda: ops.tsdf_mesh_faces(v, 1.0, n_q), args.reps, flush)
    _, cell, xyz, normal, weight, _ = ops.tsdf_mesh_vertices(v, None, vox, o, 1.0, n_v)
    _, edge, quad = ops.tsdf_mesh_faces(v, 1.0, n_q)

    def order():
        c, perm = torch.sort(cell)
        e, q_perm = torch.sort(edge)
        index = torch.searchsorted(c, quad[q_perm].to(torch.int64))
        return xyz[perm], normal[perm], weight[perm], index[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3).to(torch.int32), e

    t_order = timed(order, args.reps)
    t_all = timed(lambda: vol.extract_mesh(), args.reps, flush)
    t_all_warm = timed(lambda: vol.extract_mesh(), args.reps)
    lines = ["tsdf_bench --mesh: %d x %d maps, T = %d, voxel %.3f m, %d repetitions per figure, %s" % (W, H, T, vox, args.reps, torch.cuda.get_device_name(0)),
             "volume %d x %d x %d (Z Y X), origin (%.2f, %.2f, %.2f): %d vertices, %d triangles; mesh edges shared by 1 / 2 / more triangles: %d / %d / %d"
             % (dims + origin + (n_v, 2 * n_q, stats["boundary"], stats["manifold"], stats["non_manifold"])),
             "  extract_points kernel (the parent's read-out)      %8.3f ms with %d records" % (t_pts, pts["count"]),
             "  cell kernel                                        %8.3f ms count only, %.3f ms with %d records" % (t_vc, t_vf, n_v),
             "  face kernel                                        %8.3f ms count only, %.3f ms with %d records" % (t_fc, t_ff, n_q),
             "  the four launches of extract_mesh                  %8.3f ms (sum of the above)" % (t_vc + t_vf + t_fc + t_ff),
             "  host ordering (2 sorts, searchsorted, split)       %8.3f ms, volume-independent, inputs in cache" % t_order,
             "  extract_mesh, whole call                           %8.3f ms after a cache flush, %.3f ms back to back (two count read-backs included)"
             % (t_all, t_all_warm),
             "  every kernel figure: a 1 GiB buffer is rewritten (untimed) in front of the call, so the volume comes from HBM"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def components_main(args):
    import re
    import time
    import tsdf_ref as R
    from estdepth_amd import ops
    from estdepth_amd.fusion3d import TSDFVolume, filter_mesh, frustum_volume
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps = min(args.reps, 100)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    m = vol.extract_mesh()
    faces, n_v = m["faces"].contiguous(), m["count"]
    label, triangles, _ = ops.mesh_components(faces, n_v)
    roots = torch.nonzero(label == torch.arange(n_v, device=dev, dtype=torch.int32)).reshape(-1)
    sizes = torch.sort(triangles[roots], descending=True)[0]
    n_big = int((sizes >= 100).sum().item())
    t_op = timed(lambda: ops.mesh_components(faces, n_v), reps, flush)
    t_op_warm = timed(lambda: ops.mesh_components(faces, n_v), reps)
    t_filter = timed(lambda: filter_mesh(m, min_triangles=100), reps, flush)
    t_extract = timed(lambda: vol.extract_mesh(), reps, flush)
    # the four kernels one by one: the profiler's device time over the same flushed calls (one entry point launches all four)
    def kernel_times(f, v):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            for i in range(reps):
                flush.fill_(float(i))
                ops.mesh_components(f, v)
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            k = re.search(r"mesh_cc_\w+_kernel", e.key)
            if k:
                out[k.group(0)] = (getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) / max(e.count, 1) / 1e3
        return out
    per_kernel = kernel_times(faces, n_v)
    # a mesh large enough to fill the device: the 204 800-triangle grid of the tests, five islands, vertex ids permuted, faces shuffled
    import mesh_components_ref as C
    grid_np, grid_v = C.build_case("grid-320")
    grid = torch.from_numpy(grid_np.copy()).to(dev)
    assert np.array_equal(ops.mesh_components(grid, grid_v)[0].cpu().numpy(), C.reference("grid-320")["label"])
    t_grid = timed(lambda: ops.mesh_components(grid, grid_v), reps, flush)
    grid_kernels = kernel_times(grid, grid_v)
    # the yardstick
    want = label.cpu().numpy()
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        def yard():
            f = faces.cpu().numpy().astype(np.int64)
            g = coo_matrix((np.ones(2 * f.shape[0], np.int8), (np.r_[f[:, 0], f[:, 0]], np.r_[f[:, 1], f[:, 2]])), shape=(n_v, n_v))
            lab = connected_components(g, directed=False)[1]
            smallest = np.full(int(lab.max()) + 1 if n_v else 0, n_v, np.int64)
            np.minimum.at(smallest, lab, np.arange(n_v))
            return torch.from_numpy(smallest[lab].astype(np.int32)).to(dev)
        yard_name = "scipy.sparse.csgraph.connected_components on the host, with the copy of the faces down and of the labels up"
    except ImportError:
        def yard():
            f = faces.to(torch.int64)
            lab = torch.arange(n_v, device=dev)
            while True:
                best = lab[f].min(1).values
                new = lab.clone()
                for k in range(3):
                    new.scatter_reduce_(0, f[:, k], best, "amin")
                new = new[new]
                if torch.equal(new, lab):
                    return lab.to(torch.int32)
                lab = new
        yard_name = "a min-label propagation loop in torch on the device (scipy is not installed)"
    assert np.array_equal(yard().cpu().numpy(), want), "the yardstick and the kernels disagree"
    torch.cuda.synchronize()
    n_yard = 5
    t0 = time.perf_counter()
    for _ in range(n_yard):
        yard()
        torch.cuda.synchronize()
    t_yard = (time.perf_counter() - t0) / n_yard * 1e3
    lines = ["tsdf_bench --mesh-components: %d x %d maps, T = %d, voxel %.3f m, mean of %d calls per figure, %s" % (W, H, T, vox, reps, torch.cuda.get_device_name(0)),
             "volume %d x %d x %d (Z Y X): mesh of %d vertices, %d triangles; %d components with faces (largest: %s triangles), %d of them with at "
             "least 100 triangles, %d vertices no face uses" % (dims + (n_v, faces.shape[0], int((sizes > 0).sum().item()),
                                                                " / ".join(str(int(x)) for x in sizes[:4].tolist()), n_big, int((sizes == 0).sum().item())))]
    for k in ("mesh_cc_init_kernel", "mesh_cc_hook_kernel", "mesh_cc_flatten_kernel", "mesh_cc_count_kernel"):
        lines.append("  %-26s %8.4f ms (profiler device time, mean of %d)" % (k, per_kernel.get(k, float("nan")), reps))
    lines += ["  mesh_components operator   %8.4f ms between device events after a cache flush (four launches, three allocations), %.4f ms back to back"
              % (t_op, t_op_warm),
              "  filter_mesh, whole call    %8.4f ms after a cache flush (operator + torch glue: roots, bincount, masks, cumsum, re-indexing; read-backs included)" % t_filter,
              "  extract_mesh beside it     %8.4f ms after a cache flush (the call the filter follows)" % t_extract,
              "  yardstick                  %8.3f ms: %s (wall clock, mean of %d); operator / yardstick = 1 / %.0f"
              % (t_yard, yard_name, n_yard, t_yard / t_op),
              "  a larger mesh, the permuted and shuffled grid of tests/mesh_components_ref.py (%d triangles, %d vertices, 5 components): operator "
              "%.4f ms after a cache flush; %s" % (grid.shape[0], grid_v, t_grid, ", ".join(
                  "%s %.4f" % (k[8:-7], grid_kernels.get(k, float("nan"))) for k in ("mesh_cc_init_kernel", "mesh_cc_hook_kernel",
                                                                                    "mesh_cc_flatten_kernel", "mesh_cc_count_kernel"))),
              "  the labels of the yardstick and of the kernels are equal; no bar is set (the parent has nothing comparable)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def sample_main(args):
    import ctypes
    import tsdf_ref as R
    import mesh_components_ref as C
    from estdepth_amd import _native, ops
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume, sample_mesh
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps = min(args.reps, 100)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    m = vol.extract_mesh()
    grid_np, grid_v = C.build_case("grid-320")
    grid_xyz = torch.from_numpy(np.random.default_rng(0).uniform(0.0, 4.0, (grid_v, 3)).astype(np.float32)).to(dev)
    meshes = [("the mesh of the %d x %d x %d volume" % dims, m["xyz"].contiguous(), m["faces"].contiguous()),
              ("the grid of tests/mesh_components_ref.py (permuted ids, vertices uniform in a 4 m box)", grid_xyz, torch.from_numpy(grid_np.copy()).to(dev))]
    lib = _native.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["tsdf_bench --mesh-sample: mean of %d calls per figure between device events, 'cold' = behind a 1 GiB cache flush, 'warm' = back to back, %s"
             % (reps, torch.cuda.get_device_name(0))]
    for name, xyz, faces in meshes:
        V, F = xyz.shape[0], faces.shape[0]
        area, fnormal, invalid = ops.mesh_face_area(xyz, faces)
        cum = torch.cumsum(torch.floor(area * 2.0 ** ops.mesh_sample_scale(F, float(area.max().item()))).to(torch.int64), 0)
        total = int(cum[-1].item())

        def kernel_a():
            assert lib.estd_mesh_face_area(p(xyz), V, p(faces), F, p(area), p(fnormal), p(invalid), stream()) == 0
        lines.append("%s: %d vertices, %d triangles, %.3f m2" % (name, V, F, float(area.sum().item())))
        lines.append("  mesh_face_area_kernel (+ the 8-byte memset)    %8.4f ms cold  %8.4f ms warm" % (timed(kernel_a, reps, flush), timed(kernel_a, reps)))
        for n in (10 ** 5, 10 ** 6):
            w = ops.mesh_sample_stratum(total, n)
            out = [torch.empty((n, 3), device=dev), torch.empty(n, device=dev, dtype=torch.int32), torch.empty((n, 2), device=dev), torch.empty((n, 3), device=dev)]

            def kernel_b():
                assert lib.estd_mesh_sample(p(xyz), V, p(faces), F, None, 0, p(cum), p(fnormal), n, 0, w, 7, p(out[0]), p(out[1]), p(out[2]), p(out[3]),
                                            None, stream()) == 0

            def yard():
                # the same sampling with torch operators on the same prefix sums: three random draws, the search, the gathers, the arithmetic
                t = torch.arange(n, device=dev, dtype=torch.int64) * w + torch.randint(0, w, (n,), device=dev, dtype=torch.int64)
                f = torch.searchsorted(cum, t, right=True)
                uv = torch.rand((n, 2), device=dev)
                uv = torch.where((uv.sum(1) > 1.0)[:, None], 1.0 - uv, uv)
                tri = faces[f].to(torch.int64)
                a, b, c = xyz[tri[:, 0]], xyz[tri[:, 1]], xyz[tri[:, 2]]
                return torch.addcmul(torch.addcmul(a, uv[:, :1], b - a), uv[:, 1:], c - a), f, uv, fnormal[f]
            kernel_b()
            got, ref = torch.bincount(out[1].to(torch.int64), minlength=F), torch.bincount(yard()[1], minlength=F)
            assert int((got - ref).abs().max().item()) <= 4, "the yardstick and the kernel spread the samples differently"
            whole = lambda: sample_mesh(dict(xyz=xyz, faces=faces), n=n, seed=7)
            t_b, t_bw, t_y, t_yw, t_all, t_allw = (timed(kernel_b, reps, flush), timed(kernel_b, reps), timed(yard, reps, flush), timed(yard, reps),
                                                   timed(whole, reps, flush), timed(whole, reps))
            lines += ["  N = %d (stratum %d units, about %d dependent 8-byte loads per lane):" % (n, w, max(1, F).bit_length()),
                      "    mesh_sample_kernel, plain upper-bound search %8.4f ms cold  %8.4f ms warm  (%.2f G samples/s warm)" % (t_b, t_bw, n / t_bw / 1e6),
                      "    yardstick: torch randint / rand / searchsorted / gathers / addcmul %8.4f ms cold  %8.4f ms warm  (kernel / yardstick = 1 / %.1f cold)"
                      % (t_y, t_yw, t_y / t_b),
                      "    sample_mesh, whole call (finite check, area kernel, max and total read-backs, cumsum, sample kernel) %8.4f ms cold  %8.4f ms warm"
                      % (t_all, t_allw)]
    lines.append("  no bar is set (the parent has nothing comparable); a search narrowed per wave was not built and is not measured")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def median_ms(fn, reps, warmup=5):
    """median ms per call over ``reps`` calls, each between its own pair of device events, after ``warmup`` untimed calls"""
    for _ in range(warmup):
        fn()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in pairs]))


def distance_main(args):
    """--mesh-distance: the binning kernels, the build and the search of csrc/mesh/mesh_distance.hip for 10^5 and 10^6 queries against
    the mesh of the 256^3 bench volume and a 204 800-triangle height field, the 170-triangle ground truth of the run-stream tests on the big
    list alone, and compare_meshes with and without exact=True; the yardstick is the same minimum by torch operators (chunked brute
    force over all triangles, the closest point by clamped barycentric projection and the three edges)."""
    import tempfile
    import mesh_sample_ref as MS
    import run_stream_ref as RS
    import tsdf_ref as R
    from estdepth_amd import cloud_metrics, ops
    from estdepth_amd.cloud_metrics import TriangleGrid
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps = min(args.reps, 20)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    m = vol.extract_mesh()
    # 204 800 triangles as a surface: a 320 x 320 grid of quads over a 4 m square, a gentle height field (the grid of
    # tests/mesh_components_ref.py has that many triangles too, but no geometry: its bench scatters the vertices)
    u = np.linspace(0.0, 4.0, 321)
    gx, gy = np.meshgrid(u, u, indexing="xy")
    grid_xyz = torch.from_numpy(np.stack([gx, gy, 0.2 * np.sin(1.7 * gx) * np.cos(1.3 * gy)], -1).reshape(-1, 3).astype(np.float32)).to(dev)
    i, j = np.meshgrid(np.arange(320), np.arange(320), indexing="xy")
    v00 = (j * 321 + i).reshape(-1)
    grid_np = np.concatenate([np.stack([v00, v00 + 1, v00 + 322], 1), np.stack([v00, v00 + 322, v00 + 321], 1)]).astype(np.int32)
    with tempfile.TemporaryDirectory() as d:
        RS.write_scene(d, RS.N_FRAMES, seed=5)
        rb = RS.read_back(d)
    tg = RS.targets_of(RS.N_FRAMES)
    gt_xyz, gt_faces = MS.scene_mesh(rb["depths"][tg], rb["poses"][tg], rb["K"])
    max_dist = 1.0

    def edge_d2(q, a, b):
        ab, aq = b - a, q - a
        t = ((aq * ab).sum(-1) / (ab * ab).sum(-1).clamp_min(1e-30)).clamp(0, 1)
        return ((aq - t[..., None] * ab) ** 2).sum(-1)

    def yard(q, tri, chunk):
        """torch operators only: per chunk of queries the distance to every triangle -- the plane distance where the projection falls
        inside, else the nearest of the three edges -- and the minimum"""
        a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
        n = torch.linalg.cross(b - a, c - a)
        nn = (n * n).sum(-1)
        out = []
        for i in range(0, q.shape[0], chunk):
            p = q[i:i + chunk, None, :]
            ap = p - a
            inside = ((torch.linalg.cross(b - a, ap) * n).sum(-1) >= 0) & ((torch.linalg.cross(c - b, p - b) * n).sum(-1) >= 0) & \
                     ((torch.linalg.cross(a - c, p - c) * n).sum(-1) >= 0)
            plane = (ap * n).sum(-1) ** 2 / nn
            edges = torch.minimum(torch.minimum(edge_d2(p, a, b), edge_d2(p, b, c)), edge_d2(p, c, a))
            out.append(torch.where(inside, plane, edges).min(1)[0])
        return torch.cat(out).sqrt().clamp(max=max_dist)

    lines = ["tsdf_bench --mesh-distance: median of %d calls per figure between device events after 5 warm-up calls, max_dist %.1f m, %s"
             % (reps, max_dist, torch.cuda.get_device_name(0))]
    meshes = [("the mesh of the %d x %d x %d volume" % dims, m["xyz"].contiguous(), m["faces"].contiguous(), None),
              ("a 320 x 320 grid of quads over a 4 m square, a gentle height field", grid_xyz, torch.from_numpy(grid_np).to(dev), None),
              ("the 170-triangle ground truth of the run-stream tests, big list only", torch.from_numpy(gt_xyz).to(dev), torch.from_numpy(gt_faces).to(dev), float("inf"))]
    for name, xyz, faces, cell in meshes:
        mesh = dict(xyz=xyz, faces=faces)
        grid = TriangleGrid(mesh, max_dist, cell)
        big = grid.big_cells
        lines.append("%s: %d vertices, %d triangles (%d invalid); cell %.4g, dims %s, %d pairs + %d on the big list"
                     % (name, xyz.shape[0], faces.shape[0], grid.invalid, grid.cell, grid.dims, grid.n_pairs, grid.n_big))
        bins = lambda: ops.mesh_tri_bins(xyz, faces, grid.lo, grid.cell, grid.dims, big)
        lines.append("  mesh_tri_bins (kernel + the 8-byte memset + three allocations) %8.4f ms" % median_ms(bins, reps))
        if grid.n_pairs:
            count = bins()[0]
            offset = (torch.cumsum(count.long(), 0) - count).contiguous()
            lines.append("  mesh_tri_fill (kernel + two allocations)                      %8.4f ms" % median_ms(lambda: ops.mesh_tri_fill(xyz, faces, grid.lo, grid.cell, grid.dims, big, offset, grid.n_pairs), reps))
        lines.append("  TriangleGrid, whole build (box and median area by torch, bins, cumsum, fill, stable sort, searchsorted, record gather) %8.4f ms"
                     % median_ms(lambda: TriangleGrid(mesh, max_dist, cell), reps))
        tri = xyz[faces.long()]
        for n in (10 ** 5, 10 ** 6):
            # queries near the surface, as the samples of a reconstruction are: points of the triangles, moved by up to 5 cm
            g = torch.Generator(device=dev).manual_seed(n)
            f = torch.randint(0, faces.shape[0], (n,), device=dev, generator=g)
            uv = torch.rand((n, 2), device=dev, generator=g)
            uv = torch.where((uv.sum(1) > 1)[:, None], 1 - uv, uv)
            q = tri[f, 0] + uv[:, :1] * (tri[f, 1] - tri[f, 0]) + uv[:, 1:] * (tri[f, 2] - tri[f, 0]) + (torch.rand((n, 3), device=dev, generator=g) - 0.5) * 0.1
            q = q.contiguous()
            order = torch.sort(ops.cloud_cell_keys(q, grid.lo, grid.cell, grid.dims), stable=True)[1] if grid.n_pairs else torch.arange(n, device=dev)
            search = lambda: ops.mesh_nearest(q, order, grid.big_records, grid.records, grid.cell_start, grid.lo, grid.cell, grid.dims, max_dist)
            t_s, t_q = median_ms(search, reps), median_ms(lambda: grid.query(q), reps)
            ny = min(n, 20000)                                 # the yardstick on the first ny queries, scaled: its cost is linear in them
            chunk = max(1, min(ny, (1 << 24) // max(1, faces.shape[0])))
            t_y = median_ms(lambda: yard(q[:ny], tri, chunk), 3, warmup=1) * (n / ny)
            worst = float((grid.query(q[:ny])[0] - yard(q[:ny], tri, chunk)).abs().max().item())
            lines += ["  M = %d queries within 5 cm of the surface:" % n,
                      "    mesh_nearest_kernel                     %9.4f ms  (%.1f M queries/s)" % (t_s, n / t_s / 1e3),
                      "    TriangleGrid.query (finite check, keys, sort, search) %9.4f ms" % t_q,
                      "    yardstick: torch brute force over all triangles, %d queries timed and scaled to M: %9.1f ms (search / yardstick = 1 / %.0f); "
                      "largest |difference| on those queries %.2g m" % (ny, t_y, t_y / t_s, worst)]
    # compare_meshes on the run-stream ground truth against a copy moved by 2 mm, with and without exact
    gt = dict(xyz=torch.from_numpy(gt_xyz).to(dev), faces=torch.from_numpy(gt_faces).to(dev))
    pred = dict(xyz=gt["xyz"] + 0.002, faces=gt["faces"])
    for density in (1111.0, 2500.0):
        t_a = median_ms(lambda: cloud_metrics.compare_meshes(pred, gt, density), reps)
        t_b = median_ms(lambda: cloud_metrics.compare_meshes(pred, gt, density, exact=True), reps)
        a, b = cloud_metrics.compare_meshes(pred, gt, density), cloud_metrics.compare_meshes(pred, gt, density, exact=True)
        lines.append("compare_meshes, the 170-triangle ground truth against itself moved by (2, 2, 2) mm, density %g (%d + %d samples): sampled %8.3f ms "
                     "(accuracy %.5f m), exact %8.3f ms (accuracy %.5f m)" % (density, a["n_pred"], a["n_gt"], t_a, a["accuracy"], t_b, b["accuracy"]))
    lines.append("  no bar is set in advance; not measured: an indirection (face index -> vertices) at search time instead of the gathered 48-byte records, "
                 "an LDS broadcast instead of scalar loads in phase A, other big_cells than 64, queries far from the surface")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


EXTRACT_SNIPPET = """
import sys, numpy as np, torch
sys.path.insert(0, 'tests')
import tsdf_ref as R
from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
dev = torch.device('cuda:0')
H, W, T, vox, dims = 480, 640, 3, 0.03, (256, 256, 256)
K = R.intrinsics(H, W)
poses = R.scene_poses(T, seed=1)
depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
vol = TSDFVolume(dims, vox, frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), 0.1, 10.0, dims, vox), device=dev)
vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
for _ in range(5):
    vol.extract_mesh()
torch.cuda.synchronize()
ms = []
for _ in range(%d):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); vol.extract_mesh(); e1.record(); torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
print('EXTRACT_MS %%.4f' %% float(np.median(ms)))
"""


def extract_pairs(parent, reps, pairs=5):
    """the default extract_mesh of the parent's tree and of this one, in alternating fresh processes -> [(parent ms, this ms), ...]"""
    import subprocess
    out = []
    for _ in range(pairs):
        row = []
        for tree in (parent, ROOT):
            r = subprocess.run([sys.executable, "-c", EXTRACT_SNIPPET % reps], cwd=tree, env=dict(os.environ, PYTHONPATH=tree), capture_output=True,
                               text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError("the extract_mesh timing failed in %s (exit %d):\n%s" % (tree, r.returncode, r.stderr[-2000:]))
            row.append(float(r.stdout.split("EXTRACT_MS")[1].split()[0]))
        out.append(tuple(row))
    return out


def simplify_main(args):
    """--mesh-simplify: the two kernels of csrc/mesh/mesh_simplify.hip apart (through the C ABI, on prepared glue), the whole
    fusion3d.simplify_mesh, and the quadric sums formed with torch operators (gathers, index_add_ in float64), on the mesh of the 256^3
    bench volume and on the 204 800-triangle height field of --mesh-distance; medians of warm calls between device events."""
    import ctypes
    import tsdf_ref as R
    from estdepth_amd import _native, cloud_metrics
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume, simplify_mesh
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps = min(args.reps, 50)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    m = vol.extract_mesh()
    u = np.linspace(0.0, 4.0, 321)
    gx, gy = np.meshgrid(u, u, indexing="xy")
    grid_xyz = torch.from_numpy(np.stack([gx, gy, 0.2 * np.sin(1.7 * gx) * np.cos(1.3 * gy)], -1).reshape(-1, 3).astype(np.float32)).to(dev)
    i, j = np.meshgrid(np.arange(320), np.arange(320), indexing="xy")
    v00 = (j * 321 + i).reshape(-1)
    grid_faces = torch.from_numpy(np.concatenate([np.stack([v00, v00 + 1, v00 + 322], 1), np.stack([v00, v00 + 322, v00 + 321], 1)]).astype(np.int32)).to(dev)
    lib = _native.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["tsdf_bench --mesh-simplify: median of %d warm calls per figure between device events, %s" % (reps, torch.cuda.get_device_name(0)),
             "nobody has measured these before: the parent commit has nothing comparable, so the times are recorded, not gated"]
    for name, xyz, faces, cell in (("the mesh of the %d x %d x %d volume" % dims, m["xyz"].contiguous(), m["faces"].contiguous(), 2 * vox),
                                   ("the 320 x 320 height field over a 4 m square", grid_xyz, grid_faces, 0.05)):
        V, F = xyz.shape[0], faces.shape[0]
        out = simplify_mesh(dict(xyz=xyz, faces=faces), cell)
        Kc, cluster, cell_key = out["count"], out["cluster"], out["cell_key"]
        lo = xyz.amin(0).cpu().contiguous()
        d3 = list(cloud_metrics._dims((xyz.amax(0).cpu().double() - lo.double()).tolist(), float(np.float32(cell))))
        mean = cloud_metrics.voxel_downsample(xyz, cell)[0]                   # the same grid: simplify_mesh's default origin is the bounding box's minimum
        corner, triple = torch.empty(3 * F, device=dev, dtype=torch.int32), torch.empty((F, 3), device=dev, dtype=torch.int32)
        counts = torch.empty(2, device=dev, dtype=torch.int64)

        def kernel_faces():
            assert lib.estd_mesh_cluster_faces(p(faces), F, V, p(cluster), Kc, p(corner), p(triple), p(counts), stream()) == 0
        kernel_faces()
        rec_cluster, order = torch.sort(corner, stable=True)
        segments = torch.searchsorted(rec_cluster, torch.arange(Kc + 1, device=dev, dtype=torch.int32)).contiguous()
        o_xyz, o_n, o_p = torch.empty((Kc, 3), device=dev), torch.empty((Kc, 3), device=dev), torch.empty(Kc, device=dev, dtype=torch.bool)
        lo3, dd = (ctypes.c_float * 3)(*lo.tolist()), (ctypes.c_int * 3)(*d3)

        def kernel_quadrics():
            assert lib.estd_mesh_cluster_quadrics(p(xyz), V, p(faces), F, p(order), p(segments), p(cell_key), Kc, p(mean), lo3, float(np.float32(cell)), dd,
                                                  2.0 ** -12, p(o_xyz), p(o_n), p(o_p), stream()) == 0
        kernel_quadrics()
        assert torch.equal(o_xyz, out["xyz"]) and torch.equal(o_p, out["placed"]), "the prepared glue is not simplify_mesh's"
        plane = d3[0] * d3[1]
        g = torch.stack([cell_key % d3[0], (cell_key % plane) // d3[0], cell_key // plane], 1).double()
        centre = lo.double().to(dev) + (g + 0.5) * float(np.float32(cell))

        def yard():
            # the same twelve sums with torch operators: gathers, elementwise float64, one index_add_ per cluster table
            tri = xyz[faces.long()].double()                                  # [F,3,3]
            a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
            mm = torch.linalg.cross(b - a, c - a)
            k = corner.long().reshape(F, 3)
            sums = torch.zeros((Kc + 1, 12), device=dev, dtype=torch.float64)
            outer = (mm[:, :, None] * mm[:, None, :]).reshape(F, 9)[:, [0, 1, 2, 4, 5, 8]]
            for jj in range(3):
                delta = (mm * (a - centre[k[:, jj].clamp(max=Kc - 1)])).sum(1, keepdim=True)
                sums.index_add_(0, k[:, jj], torch.cat([outer, delta * mm, mm], 1))
            return sums
        ref = yard()[:Kc, 9:]
        nn = torch.nn.functional.normalize(ref, dim=1).float()
        assert float((nn - o_n).abs().max().item()) < 1e-5, "the yardstick and the kernel disagree on the normals"
        whole = lambda: simplify_mesh(dict(xyz=xyz, faces=faces), cell)
        t_f, t_q, t_y, t_all = median_ms(kernel_faces, reps), median_ms(kernel_quadrics, reps), median_ms(yard, reps), median_ms(whole, reps)
        lines += ["%s, cell %.3f m: %d vertices %d triangles -> %d vertices %d triangles (%s)" % (name, cell, V, F, Kc, out["faces"].shape[0], out["stats"]),
                  "  mesh_cluster_faces_kernel (+ the 16-byte memset)              %8.4f ms  (%.2f G faces/s)" % (t_f, F / t_f / 1e6),
                  "  mesh_cluster_quadric_kernel, 8 lanes per cluster, %5.1f records per cluster  %8.4f ms  (%.2f G records/s)"
                  % (3.0 * F / max(Kc, 1), t_q, 3 * F / t_q / 1e6),
                  "  yardstick: the twelve sums by torch gathers and index_add_ in float64 (no solve)  %8.4f ms  (kernel / yardstick = 1 / %.1f)" % (t_y, t_y / t_q),
                  "  simplify_mesh, whole call (finite check, keys, two stable sorts, centroids, both kernels, the face glue, read-backs)  %8.4f ms" % t_all]
    lines.append("  not built and not measured: a lane per cluster, a wave per cluster for very long segments, gathered 16-byte vertex records")
    if args.parent_tree:
        pairs = extract_pairs(os.path.abspath(args.parent_tree), reps)
        lines.append("the gate: the default extract_mesh() of the 256^3 volume, median of %d calls per process, parent commit / this tree in alternating fresh processes:" % reps)
        lines += ["  pair %d: parent %8.4f ms   this tree %8.4f ms" % (n, a, b) for n, (a, b) in enumerate(pairs)]
        pa, pb = float(np.median([a for a, _ in pairs])), float(np.median([b for _, b in pairs]))
        spread = max(max(a for a, _ in pairs) - min(a for a, _ in pairs), max(b for _, b in pairs) - min(b for _, b in pairs))
        lines.append("  medians: parent %.4f ms, this tree %.4f ms (difference %+.4f ms; the pairs spread over %.4f ms)" % (pa, pb, pb - pa, spread))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


COMPARE_SNIPPET = """
import numpy as np, torch
from estdepth_amd.cloud_metrics import compare_clouds
rng = np.random.RandomState(0)
u = rng.uniform(0.0, 4.0, size=(2, 200000, 2))
f = lambda p, dz: np.stack([p[:, 0], p[:, 1], 0.2 * np.sin(1.7 * p[:, 0]) * np.cos(1.3 * p[:, 1]) + dz], 1).astype(np.float32)
a, b = torch.from_numpy(f(u[0], 0.0)).cuda(), torch.from_numpy(f(u[1], 0.01)).cuda()
ts = []
for i in range(%d + 3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); compare_clouds(a, b, threshold=0.05, downsample=0.02); e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
print("COMPARE_MS", float(np.median(ts[3:])))
"""


REGISTER_SNIPPET = """
import numpy as np, torch
from estdepth_amd.registration import register
rng = np.random.RandomState(0)
u = rng.uniform(0.0, 4.0, size=(2, 50000, 2))
f = lambda p: np.stack([p[:, 0], p[:, 1], 0.2 * np.sin(1.7 * p[:, 0]) * np.cos(1.3 * p[:, 1])], 1)
g = lambda p: np.stack([-0.34 * np.cos(1.7 * p[:, 0]) * np.cos(1.3 * p[:, 1]), 0.26 * np.sin(1.7 * p[:, 0]) * np.sin(1.3 * p[:, 1]), np.ones(len(p))], 1)
n = g(u[1]); n /= np.linalg.norm(n, axis=1, keepdims=True)
a = torch.from_numpy((f(u[0]) + (0.004, -0.003, 0.005)).astype(np.float32)).cuda()
tgt = dict(xyz=torch.from_numpy(f(u[1]).astype(np.float32)).cuda(), normal=torch.from_numpy(n.astype(np.float32)).cuda())
ts = []
for i in range(%d + 3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); register(a, tgt); e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
print("COMPARE_MS", float(np.median(ts[3:])))
"""


def compare_pairs(parent, reps, pairs=5, snippet=COMPARE_SNIPPET):
    """compare_clouds with default arguments (or another ``snippet`` that prints COMPARE_MS) in the parent's tree and in this one, in
    alternating fresh processes -> [(parent ms, this ms), ...]"""
    import subprocess
    out = []
    for _ in range(pairs):
        row = []
        for tree in (parent, ROOT):
            r = subprocess.run([sys.executable, "-c", snippet % reps], cwd=tree, env=dict(os.environ, PYTHONPATH=tree), capture_output=True,
                               text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError("the compare_clouds timing failed in %s (exit %d):\n%s" % (tree, r.returncode, r.stderr[-2000:]))
            row.append(float(r.stdout.split("COMPARE_MS")[1].split()[0]))
        out.append(tuple(row))
    return out


def knn_main(args):
    """--cloud-knn: the search kernel and the normals kernel of csrc/cloud/cloud_knn.hip apart (through the C ABI, on a prepared grid),
    the whole cloud_metrics.estimate_normals and the candidates examined per query, at k = 8, 16, 32, on the cloud extracted from the
    256^3 bench volume and on a 200 704-point height field; the yardstick is the same result by torch operators (cdist + topk, gathers,
    float64 covariances, batched linalg.eigh) on the first 16 384 points, where the distance matrix fits; medians of warm calls."""
    import ctypes
    import tsdf_ref as R
    from estdepth_amd import _native, cloud_metrics, ops
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps = min(args.reps, 30)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    cloud_a = vol.extract_points()["xyz"].contiguous()
    u = np.linspace(0.0, 4.0, 448)
    gx, gy = np.meshgrid(u, u, indexing="xy")
    cloud_b = torch.from_numpy(np.stack([gx, gy, 0.2 * np.sin(1.7 * gx) * np.cos(1.3 * gy)], -1).reshape(-1, 3).astype(np.float32)).to(dev)
    lib = _native.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["tsdf_bench --cloud-knn: median of %d warm calls per figure between device events, %s" % (reps, torch.cuda.get_device_name(0)),
             "nobody has measured these before: the parent commit has nothing comparable, so the times are recorded, not gated"]
    for name, pts, radius in (("the cloud of the %d x %d x %d volume (voxel %.2f m)" % (dims + (vox,)), cloud_a, 0.12),
                              ("the 448 x 448 height field over a 4 m square", cloud_b, 0.04)):
        n = int(pts.shape[0])
        grid = cloud_metrics.PointGrid(pts, radius)
        order = torch.sort(ops.cloud_cell_keys(pts, grid.lo, grid.cell, grid.dims), stable=True)[1].contiguous()
        lines.append("%s: %d points, neighbours within %.2f m, cell %.4f m, %d x %d x %d cells" % ((name, n, radius, grid.cell) + tuple(grid.dims)))
        for k in (8, 16, 32):
            dist, index = torch.empty((n, k), device=dev), torch.empty((n, k), device=dev, dtype=torch.int32)
            count, st = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
            d = _native.CloudKnnDesc()
            d.M, d.N, d.k = n, n, k
            d.query, d.order, d.records, d.cell_start = pts.data_ptr(), order.data_ptr(), grid.records.data_ptr(), grid.cell_start.data_ptr()
            d.dist, d.index, d.count, d.stats = dist.data_ptr(), index.data_ptr(), count.data_ptr(), None
            d.cell, d.max_dist = grid.cell, radius
            d.lo[:], d.dims[:] = grid.lo.tolist(), grid.dims

            def search():
                assert lib.estd_cloud_knn(ctypes.byref(d), stream()) == 0
            normal, eig = torch.empty((n, 3), device=dev), torch.empty((n, 3), device=dev)
            valid, invalid = torch.empty(n, device=dev, dtype=torch.uint8), torch.zeros(1, device=dev, dtype=torch.int64)

            def fit():
                assert lib.estd_cloud_normals(p(pts), n, p(pts), n, p(index), p(count), k, None, 0, p(normal), p(eig), p(valid), p(invalid), None, stream()) == 0
            search()
            fit()
            whole = lambda: cloud_metrics.estimate_normals(pts, k, radius)
            out = whole()
            assert torch.equal(out["normal"], normal) and torch.equal(out["count"], count), "the prepared grid is not estimate_normals'"
            t_s, t_f, t_all = median_ms(search, reps), median_ms(fit, reps), median_ms(whole, reps)
            d.stats = st.data_ptr()
            search()
            torch.cuda.synchronize()
            d.stats = None
            lines.append("  k = %2d: knn_search_kernel %8.4f ms (%.1f M queries/s, %.1f candidates examined per query, %.2f neighbours found)   "
                         "knn_normals_kernel %8.4f ms   estimate_normals, whole call (finite check, grid build, two sorts, both kernels, curvature, one "
                         "read-back) %8.4f ms   %d rows not valid" % (k, t_s, n / t_s / 1e3, float(st.double().mean()), float(count.double().mean()), t_f,
                                                                      t_all, int(invalid.item())))
        # the yardstick on a subset: the distance matrix of 16 384 points is 1 GiB in fp32
        m, k = min(n, 16384), 16
        sub = pts[:m].contiguous()

        def yard():
            dd, ii = torch.cdist(sub, sub).topk(k, dim=1, largest=False)
            nb = sub[ii].double()                                             # [m,k,3]
            inside = (dd <= radius)[..., None].double()
            cnt = inside.sum(1).clamp(min=1.0)
            x = (nb - (nb * inside).sum(1, keepdim=True) / cnt[:, None]) * inside
            w, v = torch.linalg.eigh(x.transpose(1, 2) @ x)
            return w, v[:, :, 0]
        sub_out = cloud_metrics.estimate_normals(sub, k, radius)
        w, v = yard()
        ok = sub_out["valid"].bool()
        agree = float(((v[ok].float() * sub_out["normal"][ok]).sum(1).abs() > 1 - 1e-4).double().mean()) if bool(ok.any()) else 1.0
        t_y, t_k = median_ms(yard, max(reps // 3, 3)), median_ms(lambda: cloud_metrics.estimate_normals(sub, k, radius), reps)
        lines.append("  yardstick on the first %d points, k = 16: cdist + topk, gathers, float64 covariances, batched linalg.eigh %8.4f ms;  "
                     "estimate_normals on the same points %8.4f ms (1 / %.1f); %.2f %% of the valid normals agree to 1e-4"
                     % (m, t_y, t_k, t_y / t_k, 100.0 * agree))
    lines.append("  not built and not measured: a list kept sorted by insertion, instances by k range, a multi-lane covariance (it changes the order of the sums)")
    if args.parent_tree:
        pairs = compare_pairs(os.path.abspath(args.parent_tree), reps)
        lines.append("the default path: compare_clouds(threshold=0.05, downsample=0.02) on two 200 000-point clouds, median of %d calls per process, "
                     "parent commit / this tree in alternating fresh processes:" % reps)
        lines += ["  pair %d: parent %8.4f ms   this tree %8.4f ms" % (i, a, b) for i, (a, b) in enumerate(pairs)]
        pa, pb = float(np.median([a for a, _ in pairs])), float(np.median([b for _, b in pairs]))
        spread = max(max(a for a, _ in pairs) - min(a for a, _ in pairs), max(b for _, b in pairs) - min(b for _, b in pairs))
        lines.append("  medians: parent %.4f ms, this tree %.4f ms (difference %+.4f ms; the pairs spread over %.4f ms)" % (pa, pb, pb - pa, spread))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


COMPONENTS_SNIPPET = """
import numpy as np, torch
from estdepth_amd.fusion3d import mesh_components
n = 321
idx = np.arange(n * n).reshape(n, n)
a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
faces = torch.from_numpy(np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)).cuda()
ts = []
for i in range(%d + 3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); mesh_components(faces, n * n); e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
print("COMPARE_MS", float(np.median(ts[3:])))
"""


def cluster_main(args):
    """--cloud-cluster: the four kernels of csrc/cloud/cloud_cluster.hip apart (the profiler's device time of every launch of the entry
    point, through the C ABI on a prepared grid), the entry point and the whole cloud_metrics.cluster_dbscan, at eps of 2 and 4 point
    spacings with min_points = 6, on the cloud extracted from the 256^3 bench volume and on a 200 704-point height field; the yardstick is
    the same partition by torch operators (cdist, masks, argmin) and scipy.sparse.csgraph.connected_components on the first 16 384
    points, where the distance matrix fits; medians of warm calls."""
    import ctypes
    import re
    import time
    import tsdf_ref as R
    from estdepth_amd import _native, cloud_metrics
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps, min_points = min(args.reps, 30), 6
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    cloud_a = vol.extract_points()["xyz"].contiguous()
    u = np.linspace(0.0, 4.0, 448)
    gx, gy = np.meshgrid(u, u, indexing="xy")
    cloud_b = torch.from_numpy(np.stack([gx, gy, 0.2 * np.sin(1.7 * gx) * np.cos(1.3 * gy)], -1).reshape(-1, 3).astype(np.float32)).to(dev)
    lib = _native.lib()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    kernels = ("dbscan_count_kernel", "dbscan_hook_kernel", "dbscan_flatten_kernel", "dbscan_border_kernel")
    lines = ["tsdf_bench --cloud-cluster: median of %d warm calls per figure, %s; min_points = %d" % (reps, torch.cuda.get_device_name(0), min_points),
             "nobody has measured these before: the parent commit has nothing comparable, so the times are recorded, not gated"]
    for name, pts, spacing in (("the cloud of the %d x %d x %d volume (voxel %.2f m)" % (dims + (vox,)), cloud_a, vox),
                               ("the 448 x 448 height field over a 4 m square", cloud_b, 4.0 / 447.0)):
        n = int(pts.shape[0])
        lines.append("%s: %d points, point spacing %.5f m" % (name, n, spacing))
        for mult in (2, 4):
            eps = mult * spacing
            grid = cloud_metrics.PointGrid(pts, eps, eps)
            count, parent, label, size = (torch.empty(n, device=dev, dtype=torch.int32) for _ in range(4))
            noise = torch.empty(1, device=dev, dtype=torch.int32)
            d = _native.CloudDbscanDesc()
            d.N, d.min_points = n, min_points
            d.records, d.cell_start = grid.records.data_ptr(), grid.cell_start.data_ptr()
            d.count, d.parent, d.label, d.size, d.noise = count.data_ptr(), parent.data_ptr(), label.data_ptr(), size.data_ptr(), noise.data_ptr()
            d.cell, d.eps = grid.cell, eps
            d.lo[:], d.dims[:] = grid.lo.tolist(), grid.dims

            def call():
                assert lib.estd_cloud_dbscan(ctypes.byref(d), stream()) == 0
            call()
            whole = lambda: cloud_metrics.cluster_dbscan(pts, eps, min_points)
            out = whole()
            assert torch.equal(out["label"], label) and torch.equal(out["count"], count), "the prepared grid is not cluster_dbscan's"
            t_call, t_all = median_ms(call, reps), median_ms(whole, reps)
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    call()
                torch.cuda.synchronize()
            per = {k: [] for k in kernels}
            for e in prof.events():
                m = re.search(r"dbscan_\w+_kernel", e.name)
                if m and m.group(0) in per:
                    per[m.group(0)].append(float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0)) / 1e3)
            t_k = "   ".join("%s %8.4f ms" % (k, float(np.median(per[k])) if per[k] else float("nan")) for k in kernels)
            lines.append("  eps = %d spacings = %.5f m, cell %.5f m, %d x %d x %d cells: %.1f neighbours per point, %d core, %d clusters, %d noise"
                         % ((mult, eps, grid.cell) + tuple(grid.dims) + (float(count.double().mean()), int(out["core"].sum()), out["n_clusters"], out["noise"])))
            lines.append("    %s" % t_k)
            lines.append("    estd_cloud_dbscan, the four launches %8.4f ms (%.1f M points/s)   cluster_dbscan, whole call (finite check, grid build, one sort, "
                         "the kernels, dense ids, one read-back) %8.4f ms" % (t_call, n / t_call / 1e3, t_all))
        # the yardstick on a subset: the distance matrix of 16 384 points is 1 GiB in fp32
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        m, eps = min(n, 16384), 2 * spacing
        sub = pts[:m].contiguous()

        def yard():
            dist = torch.cdist(sub, sub)
            nb = dist <= eps
            core = nb.sum(1) >= min_points
            ij = (nb & core[:, None] & core[None, :]).nonzero().cpu().numpy()
            n_comp, lab = connected_components(coo_matrix((np.ones(ij.shape[0], np.int8), (ij[:, 0], ij[:, 1])), shape=(m, m)), directed=False)
            near = torch.where(nb & core[None, :], dist, torch.full((), float("inf"), device=dev)).min(1)
            return core, lab, near
        core, lab, near = yard()
        sub_out = cloud_metrics.cluster_dbscan(sub, eps, min_points)
        n_yard = int(np.unique(lab[core.cpu().numpy()]).shape[0])

        def wall(fn, k):
            ts = []
            for _ in range(k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            return float(np.median(ts))
        t_y, t_c = wall(yard, max(reps // 6, 3)), wall(lambda: cloud_metrics.cluster_dbscan(sub, eps, min_points), reps)
        lines.append("  yardstick on the first %d points, eps = 2 spacings: cdist, masks, scipy connected_components, argmin %9.3f ms wall;  cluster_dbscan on "
                     "the same points %8.3f ms wall (1 / %.1f); %d clusters against %d, core points agree on %.2f %%"
                     % (m, t_y, t_c, t_y / t_c, n_yard, sub_out["n_clusters"], 100.0 * float((core == sub_out["core"]).double().mean())))
    lines.append("  not built and not measured: a core flag in record order (count[index] is gathered instead), a cell edge of eps / 2, an early test of "
                 "equal roots before unite, a cell-level union for cells whose diagonal is below eps")
    if args.parent_tree:
        for what, snippet in (("compare_clouds(threshold=0.05, downsample=0.02) on two 200 000-point clouds", COMPARE_SNIPPET),
                              ("mesh_components on the 204 800-triangle height field", COMPONENTS_SNIPPET)):
            pairs = compare_pairs(os.path.abspath(args.parent_tree), reps, snippet=snippet)
            lines.append("the default path: %s, median of %d calls per process, parent commit / this tree in alternating fresh processes:" % (what, reps))
            lines += ["  pair %d: parent %8.4f ms   this tree %8.4f ms" % (i, a, b) for i, (a, b) in enumerate(pairs)]
            pa, pb = float(np.median([a for a, _ in pairs])), float(np.median([b for _, b in pairs]))
            spread = max(max(a for a, _ in pairs) - min(a for a, _ in pairs), max(b for _, b in pairs) - min(b for _, b in pairs))
            lines.append("  medians: parent %.4f ms, this tree %.4f ms (difference %+.4f ms; the pairs spread over %.4f ms)" % (pa, pb, pb - pa, spread))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def global_register_main(args):
    """--global-register: the four kernels of csrc/register/global_register.hip apart (through the C ABI, on prepared lists) and the whole
    registration.register_global, on the cloud extracted from the 256^3 bench volume against itself moved and on the 200 704-point
    height field thinned to 2 cm and to 5 cm against itself moved; the matcher beside torch.cdist + argmin on the same descriptors, the
    hypothesis scoring beside the same sums with torch operators; medians of warm calls.  --parent-tree DIR adds compare_clouds and
    register with default arguments in both trees, in alternating pairs of fresh processes."""
    import ctypes
    import tsdf_ref as R
    from estdepth_amd import _native, cloud_metrics, registration
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps = min(args.reps, 30)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    cloud_a = vol.extract_points()["xyz"].contiguous()
    u = np.linspace(0.0, 4.0, 448)
    gx, gy = np.meshgrid(u, u, indexing="xy")
    cloud_b = torch.from_numpy(np.stack([gx, gy, 0.2 * np.sin(1.7 * gx) * np.cos(1.3 * gy)], -1).reshape(-1, 3).astype(np.float32)).to(dev)
    M = np.eye(4)                                                             # the motion of the second side: 100 degrees about a skew axis, 2 m
    ax, th = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.radians(100.0)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M[:3, :3], M[:3, 3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx), (1.0, -1.0, 1.5)
    lib = _native.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hyp, k = 65536, 32
    lines = ["tsdf_bench --global-register: median of %d warm calls per figure between device events, %s" % (reps, torch.cuda.get_device_name(0)),
             "first measurements: the parent commit has nothing comparable, so the times are recorded, not gated; k = %d, %d hypotheses" % (k, hyp)]
    for name, raw, voxel in (("the cloud of the %d x %d x %d volume (voxel %.2f m), thinned to 6 cm" % (dims + (vox,)), cloud_a, 0.06),
                             ("the 448 x 448 height field over a 4 m square, thinned to 5 cm", cloud_b, 0.05),
                             ("the 448 x 448 height field over a 4 m square, thinned to 2 cm", cloud_b, 0.02)):
        moved = registration.transform(raw, M)
        sides = []
        for pts_raw in (raw, moved):
            pts = cloud_metrics.voxel_downsample(pts_raw, voxel)[0].contiguous()
            nrm = cloud_metrics.estimate_normals(pts, 16, 2.0 * voxel)["normal"].contiguous()
            _, index, count = cloud_metrics.PointGrid(pts, 5.0 * voxel).knn(pts, k)
            sides.append((pts, nrm, index.contiguous(), count.contiguous()))
        pts, nrm, index, count = sides[0]
        n = int(pts.shape[0])
        hist, pairs_n = torch.empty((n, 33), device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
        desc, valid = torch.empty((n, 33), device=dev), torch.empty(n, device=dev, dtype=torch.uint8)
        invalid = torch.zeros(1, device=dev, dtype=torch.int64)

        def spfh():
            assert lib.estd_cloud_spfh(p(pts), p(nrm), n, p(index), p(count), k, 0, p(hist), p(pairs_n), stream()) == 0

        def fpfh():
            assert lib.estd_cloud_fpfh(p(pts), p(nrm), n, p(index), p(count), k, p(hist), p(pairs_n), p(desc), p(valid), p(invalid), stream()) == 0
        spfh()
        fpfh()
        fa = registration.fpfh(pts, nrm, k, 5.0 * voxel, oriented=False)
        fb = registration.fpfh(sides[1][0], sides[1][1], k, 5.0 * voxel, oriented=False)
        assert torch.equal(fa["desc"], desc), "the prepared lists are not fpfh's"
        a, b, m = fa["desc"], fb["desc"], int(fb["desc"].shape[0])
        mi, md, ms2 = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev), torch.empty(n, device=dev)

        def match():
            assert lib.estd_feature_match(p(a), n, p(b), m, None, None, p(mi), p(md), p(ms2), stream()) == 0

        def yard_match():
            return torch.cdist(a, b).argmin(1)
        match()
        agree = float((yard_match() == mi.long()).double().mean())
        pr, _ = registration.match_features(a, b, fa["valid"], fb["valid"])
        C = int(pr.shape[0])
        P, Q = pts[pr[:, 0]].contiguous(), sides[1][0][pr[:, 1]].contiguous()
        dist_max = 1.5 * voxel
        cnt, status = torch.empty(hyp, device=dev, dtype=torch.int32), torch.empty(hyp, device=dev, dtype=torch.uint8)
        ssq, Tm = torch.empty(hyp, device=dev, dtype=torch.float64), torch.empty((hyp, 12), device=dev, dtype=torch.float64)
        best = torch.zeros(1, device=dev, dtype=torch.int64)

        def ransac():
            assert lib.estd_ransac_pairs(p(P), p(Q), C, hyp, 0, dist_max, 0.9, p(cnt), p(status), p(ssq), p(Tm), p(best), stream()) == 0
        ransac()
        torch.cuda.synchronize()
        scored = torch.nonzero(status == 0)[:, 0][:4096]
        Ts = Tm[scored].reshape(-1, 3, 4)
        P64, Q64 = P.double(), Q.double()

        def yard_score():                                                     # the same sums for the first 4 096 scored hypotheses
            e = torch.einsum("hij,cj->hci", Ts[:, :, :3], P64) + Ts[:, None, :, 3] - Q64[None]
            r2 = (e * e).sum(-1)
            inl = r2 <= dist_max * dist_max
            return inl.sum(1), (r2 * inl).sum(1)
        same = bool(torch.equal(yard_score()[0].int(), cnt[scored])) if scored.numel() else True
        whole = lambda: registration.register_global(raw, moved, voxel, hypotheses=hyp)
        out = whole()
        t = {f.__name__: median_ms(f, reps) for f in (spfh, fpfh, match, ransac)}
        t_ym, t_ys, t_all = median_ms(yard_match, max(reps // 3, 3)), median_ms(yard_score, max(reps // 3, 3)) if scored.numel() else 0.0, median_ms(whole, max(reps // 3, 3))
        n_scored = int((status == 0).sum().item())
        lines += ["%s: %d and %d points, normals estimated (k = 16), folded descriptors" % (name, n, m),
                  "  greg_spfh_kernel<false> %8.4f ms   greg_fpfh_kernel %8.4f ms   (%.1f M points/s together)" % (t["spfh"], t["fpfh"], n / (t["spfh"] + t["fpfh"]) / 1e3),
                  "  greg_match_kernel %d x %d  %8.4f ms (%.1f G fma/s)   yardstick torch.cdist + argmin %8.4f ms (kernel / yardstick = %.2f; %.2f %% of the "
                  "rows name the same partner)" % (n, m, t["match"], 33.0 * n * m / t["match"] / 1e6, t_ym, t["match"] / t_ym, 100.0 * agree),
                  "  greg_ransac_kernel, %d correspondences, %d of %d hypotheses scored  %8.4f ms (%.1f G rows/s)   yardstick: the sums of the first %d "
                  "scored hypotheses with torch operators (einsum, float64) %8.4f ms, the same counts: %s (per scored hypothesis: kernel %.3f us, yardstick %.3f us)"
                  % (C, n_scored, hyp, t["ransac"], n_scored * C / max(t["ransac"], 1e-9) / 1e6, int(scored.numel()), t_ys, same,
                     1e3 * t["ransac"] / max(n_scored, 1), 1e3 * t_ys / max(int(scored.numel()), 1)),
                  "  register_global, whole call (two thinnings, two normal fits, four searches, descriptors, two matches, hypotheses, read-backs) "
                  "%8.4f ms: %d pairs, winner %d with %d inliers (%s)" % (t_all, out["pairs"], out["hypothesis"], out["count"], out["reason"])]
    lines.append("  not built and not measured: a matcher whose workgroups split b between them (it launches ceil(M / 64) workgroups, each over all of "
                 "b), FPFH with fewer accumulators per lane, hypotheses scored in fp32")
    if args.parent_tree:
        for what, snippet in (("compare_clouds(threshold=0.05, downsample=0.02) on two 200 000-point clouds", COMPARE_SNIPPET),
                              ("register() with default arguments, 50 000 points onto 50 000 with normals", REGISTER_SNIPPET)):
            pairs = compare_pairs(os.path.abspath(args.parent_tree), reps, snippet=snippet)
            lines.append("the default path: %s, median of %d calls per process, parent commit / this tree in alternating fresh processes:" % (what, reps))
            lines += ["  pair %d: parent %8.4f ms   this tree %8.4f ms" % (i, x, y) for i, (x, y) in enumerate(pairs)]
            pa, pb = float(np.median([x for x, _ in pairs])), float(np.median([y for _, y in pairs]))
            spread = max(max(x for x, _ in pairs) - min(x for x, _ in pairs), max(y for _, y in pairs) - min(y for _, y in pairs))
            lines.append("  medians: parent %.4f ms, this tree %.4f ms (difference %+.4f ms; the pairs spread over %.4f ms)" % (pa, pb, pb - pa, spread))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def register_main(args):
    """--register: the three kernels of csrc/track/rigid_align.hip apart (device times from torch.profiler), one whole iteration of
    registration.rigid_system split into search and system, and the same 29 sums formed with torch operators (gathers, einsum, .sum() in
    float64) on the same device -- for 10^5 and 10^6 samples of the 256^3 bench volume's mesh against that mesh moved by a fixed twist."""
    import time
    import tsdf_ref as R
    from estdepth_amd import ops, registration, tracking
    from estdepth_amd.cloud_metrics import TriangleGrid
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume, sample_mesh
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps = min(args.reps, 20)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    m = vol.extract_mesh()
    twist = np.array([0.006, -0.005, 0.006, 0.005, -0.004, 0.006])                       # about 1 cm and 0.5 degrees (tests/track_ref.py TWIST)
    G = tracking.exp_se3(twist)
    moved_mesh = dict(xyz=registration.transform(m["xyz"].contiguous(), G), faces=m["faces"].contiguous())
    dist_max = 0.1
    grid = TriangleGrid(moved_mesh, dist_max)
    normal = ops.mesh_face_area(grid.xyz, grid.faces)[1]
    T12 = torch.from_numpy(np.ascontiguousarray(np.eye(4)[:3, :4].astype(np.float32)))
    lines = ["tsdf_bench --register: median of %d calls per figure between device events after 5 warm-up calls; kernel times: the mean device time "
             "torch.profiler reports over the same calls; dist_max %.2f m, plane metric, %s" % (reps, dist_max, torch.cuda.get_device_name(0)),
             "the mesh of the %d x %d x %d volume: %d vertices, %d triangles; the target is that mesh moved by Exp(%s)" % (dims + (m["xyz"].shape[0], m["faces"].shape[0], twist.tolist()))]

    def kernel_us(fn, names):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for n in names:
                if n in e.key:
                    total = getattr(e, "self_device_time_total", None)
                    out[n] = (total if total is not None else e.self_cuda_time_total) / max(e.count, 1)
        return [out.get(n, float("nan")) for n in names]

    def yard(moved, index, target, nrm, d2):
        """torch operators only: the gates, J and the 29 sums (as A, b, sum r^2, count) in float64"""
        ok = index >= 0
        n = nrm[index.clamp(min=0)]
        e = target - moved
        ok = ok & ((e * e).sum(1) <= d2)
        r = torch.where(ok, (n * e).sum(1), torch.zeros((), device=dev)).double()
        J = torch.where(ok[:, None], torch.cat([n, torch.linalg.cross(target, n)], 1), torch.zeros((), device=dev)).double()
        return torch.einsum("ni,nj->ij", J, J), (J * r[:, None]).sum(0), (r * r).sum(), ok.sum()

    for n in (10 ** 5, 10 ** 6):
        s = sample_mesh(dict(xyz=m["xyz"], faces=m["faces"]), n=n, seed=0)
        src, sn = s["xyz"].contiguous(), s["normal"].contiguous()
        for _ in range(5):
            ops.rigid_apply(src, sn, T12)
        moved, mn = ops.rigid_apply(src, sn, T12)
        _, face, closest = grid.query(moved, closest=True)
        index = face.long()
        system = lambda: ops.rigid_system(moved, None, index, closest, normal, False, "plane", dist_max)                         # noqa: E731
        for _ in range(5):
            system()
        k_apply, = kernel_us(lambda: ops.rigid_apply(src, sn, T12), ["rigid_apply_kernel"])
        k_sys, k_red = kernel_us(system, ["rigid_system_kernel", "rigid_reduce_kernel"])
        t_apply = median_ms(lambda: ops.rigid_apply(src, sn, T12), reps)
        t_search = median_ms(lambda: grid.query(moved, closest=True), reps)
        t_system = median_ms(system, reps)
        d2 = float(np.float32(dist_max) * np.float32(dist_max))
        t_yard = median_ms(lambda: yard(moved, index, closest, normal, d2), reps)
        tgt = registration._Target(grid, dist_max, None, "tsdf_bench")
        whole = []
        for _ in range(reps + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = registration.rigid_system(src, np.eye(4), tgt, metric="plane", dist_max=dist_max)
            whole.append(1e3 * (time.perf_counter() - t0))
        t_whole = float(np.median(whole[3:]))
        A, b, rr, cnt = yard(moved, index, closest, normal, d2)
        sums = system()[2].cpu().numpy()
        Ad, bd, rrd, cntd = tracking.unpack_sums(sums)
        gap = max(float(np.abs(Ad - A.cpu().numpy()).max() / np.abs(Ad).max()), float(np.abs(bd - b.cpu().numpy()).max() / max(np.abs(bd).max(), 1e-300)))
        lines += ["  N = %d samples (with normals); %d matched, rmse %.5f m:" % (n, out["count"], out["rmse"]),
                  "    rigid_apply_kernel  %9.2f us   (points and normals: %d bytes moved, %.0f GB/s -- back to back, the arrays warm in the caches)" % (k_apply, 48 * n, 48 * n / k_apply / 1e3),
                  "    rigid_system_kernel %9.2f us   rigid_reduce_kernel %9.2f us   (%d workgroups, %d bytes read per point)" % (k_sys, k_red, (n + 255) // 256, 44),
                  "    ops.rigid_apply (kernel + two allocations) %9.4f ms;  ops.rigid_system (two kernels + four allocations) %9.4f ms" % (t_apply, t_system),
                  "    one iteration, registration.rigid_system, host wall time with the 29-double read-back: %9.4f ms; of it the search "
                  "(TriangleGrid.query with closest: finite check, keys, sort, mesh_nearest) %9.4f ms, apply + system %9.4f ms"
                  % (t_whole, t_search, t_apply + t_system),
                  "    yardstick: the same gates and sums with torch operators (gathers, cross, einsum, .sum() in float64): %9.4f ms "
                  "(ops.rigid_system / yardstick = 1 / %.1f); count %d against %d, largest relative difference of A and b %.2g"
                  % (t_yard, t_yard / t_system, int(cnt.item()), cntd, gap)]
    lines.append("  no bar is set in advance; not measured: the search fused with the system kernel (one pass over the moved cloud instead of "
                 "two, no closest / face arrays), and a device-side 6 x 6 solve that would spare the read-back of 29 doubles per iteration")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def raster_main(args):
    import ctypes
    import tsdf_ref as R
    import tsdf_raycast_ref as RR
    from estdepth_amd import _native, camera, ops
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    from estdepth_amd.mesh_render import render_mesh
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    reps = min(args.reps, 100)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    m = vol.extract_mesh()
    pose = RR.HELD_OUT_POSE
    eye = np.eye(4)
    Ki = np.linalg.inv(K)
    corner = lambda u, v, z: tuple((Ki @ np.asarray([u, v, 1.0])) * z)                     # the point of pixel (u, v) at depth z, camera at the origin
    n = 320                                                                                 # 2 n^2 = 204 800 triangles over the whole image
    gu, gv = np.meshgrid(np.linspace(-2.0, W + 1.0, n + 1), np.linspace(-2.0, H + 1.0, n + 1))
    grid_xyz = np.stack([np.asarray(corner(u, v, 2.5 + 0.3 * np.sin(0.01 * u + 0.02 * v))) for u, v in zip(gu.ravel(), gv.ravel())]).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    a = (j * (n + 1) + i).ravel()
    grid_faces = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)]).astype(np.int32)
    grid_faces = grid_faces[np.random.default_rng(0).permutation(grid_faces.shape[0])]      # no order in memory or on the screen
    wall_xyz = np.asarray([corner(-8, -8, 2.0), corner(W + 8, -8, 2.0), corner(W + 8, H + 8, 2.5), corner(-8, H + 8, 2.5)], np.float32)
    small = np.asarray([corner(300, 200, 2.0), corner(306, 201, 2.0), corner(302, 207, 2.0)], np.float32)     # about 20 pixels
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cases = [("the mesh of the %d x %d x %d volume from the held-out pose" % dims, m["xyz"].contiguous(), m["faces"].contiguous(), pose),
             ("a 320 x 320 grid of quads over the whole image, triangles in shuffled order (about 1.5 pixels each)", t(grid_xyz), t(grid_faces), eye),
             ("a wall of two triangles that fills the image (4800 blocks of 8 x 8 pixels each, dealt to 64 waves)", t(wall_xyz),
              t(np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)), eye),
             ("4096 coincident triangles of about 20 pixels (every wave wants the same keys)", t(small), t(np.asarray([(0, 1, 2)] * 4096, np.int32)), eye)]
    lib = _native.lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["tsdf_bench --mesh-raster: %d x %d, mean of %d calls per figure between device events, 'cold' = behind a 1 GiB cache flush, 'warm' = back to "
             "back, %s" % (W, H, reps, torch.cuda.get_device_name(0))]
    keys = torch.empty((H, W), device=dev, dtype=torch.int64)
    invalid = torch.empty(1, device=dev, dtype=torch.int64)
    out = [torch.empty((H, W), device=dev), torch.empty((H, W), device=dev, dtype=torch.int32), torch.empty((H, W, 2), device=dev),
           torch.empty((H, W), device=dev, dtype=torch.int32)]
    for name, xyz, faces, P in cases:
        V, F = xyz.shape[0], faces.shape[0]
        mat = camera.mesh_raster_matrix(torch.from_numpy(P), torch.from_numpy(K))
        cm = (ctypes.c_double * 12)(*mat.tolist())

        def raster(flags):
            assert lib.estd_mesh_raster(p(xyz), V, p(faces), F, 0, F, cm, H, W, 1e-3, flags | ops.MESH_RASTER_CLEAR, p(keys), p(invalid), stream()) == 0

        def resolve():
            assert lib.estd_mesh_raster_resolve(p(xyz), V, p(faces), F, cm, H, W, p(keys), p(out[0]), p(out[1]), p(out[2]), p(out[3]), stream()) == 0
        clear = lambda: keys.fill_(-1)
        whole = lambda: render_mesh(dict(xyz=xyz, faces=faces), P, K, (H, W))
        bare = lambda: render_mesh(dict(xyz=xyz, faces=faces), P, K, (H, W), normals=None, color=False)
        raster(0)
        resolve()
        covered = int((out[1] >= 0).sum().item())
        figs = [timed(lambda: raster(ops.MESH_RASTER_PRELOAD), reps, flush), timed(lambda: raster(ops.MESH_RASTER_PRELOAD), reps), timed(lambda: raster(0), reps, flush),
                timed(lambda: raster(0), reps), timed(resolve, reps, flush), timed(resolve, reps), timed(clear, reps),
                timed(whole, reps, flush), timed(whole, reps), timed(bare, reps, flush), timed(bare, reps)]
        lines += ["%s: %d vertices, %d triangles, %d of %d pixels covered" % (name, V, F, covered, H * W),
                  "  mesh_raster_kernel<1>, load in front of the atomic (+ the two memsets)  %8.4f ms cold  %8.4f ms warm" % (figs[0], figs[1]),
                  "  mesh_raster_kernel<0>, atomic alone, the default (+ the two memsets)    %8.4f ms cold  %8.4f ms warm" % (figs[2], figs[3]),
                  "  mesh_resolve_kernel                                                    %8.4f ms cold  %8.4f ms warm" % (figs[4], figs[5]),
                  "  (a fill of the 2.4 MB key buffer alone, warm: %.4f ms)" % figs[6],
                  "  render_mesh, whole call with face normals (matrix on the host, area kernel, gathers, one read-back) %8.4f ms cold  %8.4f ms warm"
                  % (figs[7], figs[8]),
                  "  render_mesh(normals=None, color=False): depth, face, bary, facing alone %8.4f ms cold  %8.4f ms warm" % (figs[9], figs[10])]
    cast = lambda: vol.render(torch.from_numpy(pose), torch.from_numpy(K), (H, W))
    lines += ["yardstick: TSDFVolume.render of the same volume from the held-out pose (ray casting, csrc/tsdf_raycast.hip), whole call  %8.4f ms cold  "
              "%8.4f ms warm" % (timed(cast, reps, flush), timed(cast, reps)),
              "no bar is set (the parent has nothing comparable)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def raycast_main(args):
    import tsdf_ref as R
    import tsdf_raycast_ref as RR
    from estdepth_amd import ops
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume, render_plan
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB
    reps = max(args.reps, 100)
    lines = ["tsdf_bench --raycast: one %d x %d render of the %d x %d x %d volume (voxel %.3f m, origin (%.2f, %.2f, %.2f), T = %d fused), "
             "%d repetitions per figure after 10 warm-up calls, %s" % ((W, H) + dims + (vox,) + origin + (T, reps, torch.cuda.get_device_name(0)))]
    fuse_extract_ms = 0.15 + 0.05                       # profiles/tsdf_bench.txt: (a) + (d) of this volume
    for label, pose in (("first fused camera", poses[0]), ("held-out pose", RR.HELD_OUT_POSE)):
        mats, _, t_min, dt, n_steps, _ = render_plan(vol.dims, vox, vol.origin, vol.z_near, torch.from_numpy(pose), torch.from_numpy(K), (H, W))
        mat = mats[0].contiguous()

        def cast(stats=False):
            return ops.tsdf_raycast(vol.volume, mat, H, W, t_min, dt, n_steps[0], 1.0, stats)
        depth, _, _, st = cast(stats=True)
        torch.cuda.synchronize()
        st = st.cpu().numpy().astype(np.int64)
        probed, gathered = st[..., 0], st[..., 1]
        hit = int((depth > 0).sum().item())
        t_cold = timed(cast, reps, flush)
        t_warm = timed(cast, reps)
        bytes_ray = 32.0 * (probed + gathered)
        lines += [
            "%s: t = %.3f .. %.2f m in %d steps of %.3f m, %d of %d pixels hit" % (label, t_min, t_min + (n_steps[0] - 1) * dt, n_steps[0], dt, hit, H * W),
            "  render, volume in HBM (1 GiB rewritten before every call)   %8.3f ms" % t_cold,
            "  render, back to back                                        %8.3f ms" % t_warm,
            "  samples per ray whose weights were read: mean %.1f, max %d of %d; whose D values were read: mean %.1f, max %d"
            % (probed.mean(), probed.max(), n_steps[0], gathered.mean(), gathered.max()),
            "  gathered bytes per ray: mean %.0f, max %d (8 x 4 bytes per weight probe + 8 x 4 per D gather); %.1f MB per render, %.2f TB/s of "
            "gathers back to back" % (bytes_ray.mean(), bytes_ray.max(), bytes_ray.sum() / 1e6, bytes_ray.sum() / (t_warm * 1e-3) / 1e12),
            "  beside the %.1f ms Joint step: %.1f %% of the step; beside the T = 3 integrate + extract pass (%.2f ms): %.1f x"
            % (JOINT_STEP_MS, 100.0 * t_cold / JOINT_STEP_MS, fuse_extract_ms, t_cold / fuse_extract_ms),
        ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


def color_main(args):
    import tsdf_color_ref as CR
    import tsdf_raycast_ref as RR
    import tsdf_ref as R
    from estdepth_amd import camera, ops
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume, render_plan
    assert torch.cuda.is_available(), "tools/tsdf_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    K = R.intrinsics(H, W)
    poses = R.scene_poses(T, seed=1)
    depths_np = np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)
    images = torch.from_numpy(CR.case_images(dict(depths=depths_np, poses=poses, K=K))).to(dev)
    depths = torch.from_numpy(depths_np).to(dev)
    dl, il = [depths[t] for t in range(T)], [images[t] for t in range(T)]
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev, color=True)
    mats = camera.tsdf_matrices(torch.from_numpy(poses), torch.from_numpy(K), vol.origin, vox).contiguous()
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB
    reps = args.reps

    def fuse():
        ops.tsdf_integrate_(vol.volume, dl, [], mats, vol.trunc, vol.z_near, 0.0, False, vol.w_max)

    def fuse_color():
        ops.tsdf_integrate_color_(vol.volume, vol.color, dl, [], il, mats, vol.trunc, vol.z_near, 0.0, False, vol.w_max)
    fuse_color()
    torch.cuda.synchronize()
    groups16 = int((vol.volume[1].reshape(-1, 4) > 0).any(1).sum().item())
    pts = vol.extract_points()
    edge = pts["edge"].contiguous()
    rmats, _, t_min, dt, n_steps, _ = render_plan(vol.dims, vox, vol.origin, vol.z_near, torch.from_numpy(RR.HELD_OUT_POSE), torch.from_numpy(K), (H, W))
    mat = rmats[0].contiguous()

    def cast():
        return ops.tsdf_raycast(vol.volume, mat, H, W, t_min, dt, n_steps[0], 1.0)

    def cast_color():
        return ops.tsdf_raycast_color(vol.volume, vol.color, mat, H, W, t_min, dt, n_steps[0], 1.0)
    # alternating rounds, so that a drift of the clock or of the box falls on both members of a pair alike
    rounds, per = 4, max(reps // 4, 1)
    fig = {k: [] for k in ("fuse", "fuse_color", "cast", "cast_color")}
    for _ in range(rounds):
        fig["fuse"].append(timed(fuse, per, flush))
        fig["fuse_color"].append(timed(fuse_color, per, flush))
        fig["cast"].append(timed(cast, per, flush))
        fig["cast_color"].append(timed(cast_color, per, flush))
    t_edge = timed(lambda: ops.tsdf_edge_colors(vol.volume, vol.color, edge), reps, flush)
    med = {k: float(np.median(v)) for k, v in fig.items()}
    lines = [
        "tsdf_bench --color: %d x %d maps and renders, T = %d, volume %d x %d x %d at %.3f m, %d rounds of %d repetitions per figure (median of the "
        "rounds; every call behind a 1 GiB cache flush), %s" % ((W, H, T) + dims + (vox, rounds, per, torch.cuda.get_device_name(0))),
        "  plain T=3 fuse              %8.3f ms   (rounds: %s)" % (med["fuse"], " ".join("%.3f" % v for v in fig["fuse"])),
        "  colour T=3 fuse             %8.3f ms   (rounds: %s)   colour / plain = %.2f" % (med["fuse_color"], " ".join("%.3f" % v for v in fig["fuse_color"]),
                                                                                       med["fuse_color"] / med["fuse"]),
        "    %d 16-byte groups touched: %.1f MB of volume traffic with colour (160 bytes per group), %.1f MB without (64)"
        % (groups16, groups16 * 160.0 / 1e6, groups16 * 64.0 / 1e6),
        "  edge colours                %8.3f ms   for %d records" % (t_edge, pts["count"]),
        "  plain render, held-out pose %8.3f ms   (rounds: %s)" % (med["cast"], " ".join("%.3f" % v for v in fig["cast"])),
        "  colour render               %8.3f ms   (rounds: %s)   colour / plain = %.2f" % (med["cast_color"], " ".join("%.3f" % v for v in fig["cast_color"]),
                                                                                       med["cast_color"] / med["cast"]),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
