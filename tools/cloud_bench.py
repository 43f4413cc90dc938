"""Stand-alone timing of the point-cloud scores (csrc/cloud_nn.hip, estdepth_amd/cloud_metrics.py) on an MI355X: device events, warm-up, the
median of repeated launches; not part of bench.py -- nothing here runs inside the timed step.

    python tools/cloud_bench.py [--reps 20] [--out profiles/cloud_metrics_bench.txt]

Workloads (max_dist = 1 m, what compare_clouds uses at a 5 cm threshold):
  8k    the cloud extracted from the 256^3 volume of tools/tsdf_bench.py (three 640 x 480 maps of the analytic scene of tests/tsdf_ref.py)
        against itself with 5 mm of Gaussian noise added
  200k  the analytic surface seen from one camera (400 x 500 pixels back-projected) against the same surface seen from another
  1M    the same at 1000 x 1000 pixels
Per workload and cell edge (the default of cloud_metrics.grid_plan, x 0.5 and x 2):
  build    PointGrid construction of both clouds (bounding box, keys, stable sort, cell table, records; includes one host synchronisation each)
  search   both directions of PointGrid.query with the grids built: the queries' keys, their sort and estd_cloud_nearest
  kernel   estd_cloud_nearest alone, both directions, the queries' order precomputed
  examined candidates whose distance was evaluated per query (the STATS instance): what explains the kernel's time
The yardstick is not the code under test: torch.cdist + min on the same device, both directions, chunked to 8192 query rows, at 8k and 200k."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAX_DIST = 1.0


def median_ms(fn, reps, warmup=3):
    """median ms of ``reps`` calls, each between its own pair of device events"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def brute(query, target, chunk=8192):
    """torch.cdist + min, chunked over the queries -> (dist, index)"""
    d, i = [], []
    for a in range(0, query.shape[0], chunk):
        v, k = torch.cdist(query[a:a + chunk], target).min(1)
        d.append(v)
        i.append(k)
    return torch.cat(d), torch.cat(i)


def fused_cloud(dev):
    """the 256^3 case of tools/tsdf_bench.py -> the extracted points"""
    import tsdf_ref as R
    from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
    H, W, T, vox, dmin, dmax, dims = 480, 640, 3, 0.03, 0.1, 10.0, (256, 256, 256)
    K, poses = R.intrinsics(H, W), R.scene_poses(T, seed=1)
    depths = torch.from_numpy(np.stack([R.raycast_scene(P, K, H, W) for P in poses]).astype(np.float32)).to(dev)
    origin = frustum_volume(torch.from_numpy(poses[0]), torch.from_numpy(K), (H, W), dmin, dmax, dims, vox)
    vol = TSDFVolume(dims, vox, origin, device=dev)
    vol.integrate(depths, torch.from_numpy(poses), torch.from_numpy(K))
    return vol.extract_points()["xyz"].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    reps = max(args.reps, 5)
    import cloud_metrics_ref as C
    import tsdf_ref as R
    from estdepth_amd import cloud_metrics as M
    from estdepth_amd import ops
    assert torch.cuda.is_available(), "tools/cloud_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    poses = R.scene_poses(2, seed=5)
    work = []
    a = fused_cloud(dev)
    gen = torch.Generator().manual_seed(3)
    work.append(("8k", a, (a + 0.005 * torch.randn(a.shape, generator=gen).to(dev)).contiguous(), True))
    for name, (H, W), with_brute in (("200k", (400, 500), True), ("1M", (1000, 1000), False)):
        K = R.intrinsics(H, W)
        work.append((name, torch.from_numpy(C.surface_points(poses[0], K, H, W)).to(dev), torch.from_numpy(C.surface_points(poses[1], K, H, W)).to(dev), with_brute))
    lines = ["cloud_bench: both directions between two clouds, max_dist %.1f m, median of %d calls after 3 warm-up calls, %s" % (MAX_DIST, reps, torch.cuda.get_device_name(0))]
    for name, p, q, with_brute in work:
        lines.append("%s: %d and %d points" % (name, p.shape[0], q.shape[0]))
        base = None
        for factor in (1.0, 0.5, 2.0):
            cells = []
            for cloud in (p, q):
                c64 = cloud.double()
                default = M.grid_plan(c64.amin(0).cpu().numpy(), c64.amax(0).cpu().numpy(), cloud.shape[0], MAX_DIST)[0]
                cells.append(None if factor == 1.0 else factor * default)
            build = median_ms(lambda: (M.PointGrid(p, MAX_DIST, cells[0]), M.PointGrid(q, MAX_DIST, cells[1])), reps)
            gp, gq = M.PointGrid(p, MAX_DIST, cells[0]), M.PointGrid(q, MAX_DIST, cells[1])
            search = median_ms(lambda: (gp.query(q), gq.query(p)), reps)
            oq = torch.sort(ops.cloud_cell_keys(q, gp.lo, gp.cell, gp.dims), stable=True)[1]
            op_ = torch.sort(ops.cloud_cell_keys(p, gq.lo, gq.cell, gq.dims), stable=True)[1]

            def kernel(stats=False):
                return (ops.cloud_nearest(q, oq, gp.records, gp.cell_start, gp.lo, gp.cell, gp.dims, MAX_DIST, stats=stats),
                        ops.cloud_nearest(p, op_, gq.records, gq.cell_start, gq.lo, gq.cell, gq.dims, MAX_DIST, stats=stats))
            t_kernel = median_ms(kernel, reps)
            r0, r1 = kernel(stats=True)
            ex = torch.cat([r0[2], r1[2]]).double()
            if base is None:
                base = (r0[0].clone(), r0[1].clone(), r1[0].clone(), r1[1].clone())
            same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                       for x, y in zip(base, (r0[0], r0[1], r1[0], r1[1])))
            lines.append("  cell x %.1f (%.4f m, %d x %d x %d cells; %.4f m, %d x %d x %d): build %8.3f ms   search %8.3f ms   kernel %8.3f ms   "
                         "examined %8.1f per query (max %d)   bits as the default cell's: %s"
                         % ((factor, gp.cell) + tuple(gp.dims) + (gq.cell,) + tuple(gq.dims) + (build, search, t_kernel, ex.mean().item(), int(ex.max().item()), same)))
        if with_brute:
            t_brute = median_ms(lambda: (brute(q, p), brute(p, q)), max(reps // 4, 3), warmup=1)
            gp, gq = M.PointGrid(p, MAX_DIST), M.PointGrid(q, MAX_DIST)
            t_all = median_ms(lambda: (M.PointGrid(p, MAX_DIST).query(q), M.PointGrid(q, MAX_DIST).query(p)), reps)
            d_b, _ = brute(q, p)
            d_g, _ = gp.query(q)
            lines.append("  torch.cdist + min, both directions, chunks of 8192 queries: %8.3f ms;  grid build + search (default cell): %8.3f ms;  ratio %.1f;  "
                         "largest |dist difference| %.2e m (cdist's fp32 arithmetic is not the contract's)"
                         % (t_brute, t_all, t_brute / t_all, float((d_b.clamp(max=MAX_DIST) - d_g).abs().max().item())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
