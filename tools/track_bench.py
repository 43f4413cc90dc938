"""Stand-alone timing of csrc/track/frame_align.hip on an MI355X (device events, warm-up, medians; not part of bench.py).

    python tools/track_bench.py [--reps 100] [--out profiles/track_bench.txt]

Three 640 x 480 frames of the three-body scene of tests/track_ref.py are fused into a 256^3 volume at 3 cm; the model is rendered once at a
guess 9.8 mm and 0.50 degrees off the held-out pose, and the held-out frame is aligned against it:
  (a) one align_step launch pair (the alignment kernel and its reduction) between its own pair of device events, the matrices formed once
      outside the timed region, maps wherever the previous launch left them;
  (b) the same behind a 1 GiB buffer rewritten (untimed) in front of every launch: the maps come from HBM, as behind a model step;
  (c) the YARDSTICK: the same 29 sums formed with torch operators on the device (projection, rounding, gathers, gates, the products in
      fp32, the sums in float64) -- not the code under test -- timed as (a) and (b); its sums are printed beside the kernel's;
  (d) TSDFVolume.track with max_iter = 10 (one render, then per iteration one launch pair, one 29-double read-back and the 6 x 6 solve
      on the host), wall clock around a synchronised call, and the same through tracking.refine_pose on the rendered model alone.
No bar is set.  The algorithmic traffic of (a) is the depth map and the matched model pixels read (depth + normal) and two maps written."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def per_launch(fn, reps, flush=None, warmup=10):
    """ms of every one of ``reps`` calls, each between its own pair of device events"""
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
    return np.array([a.elapsed_time(b) for a, b in pairs])


def wall(fn, reps, warmup=3):
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    return np.array(out)


def torch_sums(depth, m_depth, m_normal, mats, dist_max, z_near):
    """the 29 sums of estd_frame_align with torch operators (no fused multiply-adds: the last bits of a decision may differ)"""
    H, W = depth.shape
    Hm, Wm = m_depth.shape
    L, F, B = (mats[i].reshape(3, 4) for i in range(3))                    # ``mats`` on the device already
    v, u = torch.meshgrid(torch.arange(H, device=depth.device, dtype=torch.float32), torch.arange(W, device=depth.device, dtype=torch.float32), indexing="ij")
    ok = torch.isfinite(depth) & (depth > z_near)
    d = torch.where(ok, depth, torch.ones_like(depth))
    p = [d * (L[j, 0] * u + (L[j, 1] * v + L[j, 2])) + L[j, 3] for j in range(3)]
    a, b, c = (F[j, 0] * p[0] + (F[j, 1] * p[1] + (F[j, 2] * p[2] + F[j, 3])) for j in range(3))
    ok &= c > z_near
    c = torch.where(ok, c, torch.ones_like(c))
    um, vm = torch.floor(a / c + 0.5), torch.floor(b / c + 0.5)
    ok &= (um >= 0) & (um < Wm) & (vm >= 0) & (vm < Hm)
    idx = torch.where(ok, vm * Wm + um, torch.zeros_like(um)).long()
    dm = m_depth.reshape(-1)[idx]
    ok &= dm > 0
    n = m_normal.reshape(-1, 3)[idx]
    umf, vmf = torch.where(ok, um, torch.zeros_like(um)), torch.where(ok, vm, torch.zeros_like(vm))
    e = [dm * (B[j, 0] * umf + (B[j, 1] * vmf + B[j, 2])) + B[j, 3] - p[j] for j in range(3)]
    ok &= (e[0] * e[0] + (e[1] * e[1] + e[2] * e[2])) <= float(np.float32(dist_max) * np.float32(dist_max))
    r = n[..., 0] * e[0] + (n[..., 1] * e[1] + n[..., 2] * e[2])
    w = [p[1] * n[..., 2] - p[2] * n[..., 1], p[2] * n[..., 0] - p[0] * n[..., 2], p[0] * n[..., 1] - p[1] * n[..., 0]]
    zero = torch.zeros_like(r)
    J = torch.stack([torch.where(ok, t, zero) for t in (n[..., 0], n[..., 1], n[..., 2], w[0], w[1], w[2])], -1).reshape(-1, 6)
    r = torch.where(ok, r, zero).reshape(-1)
    iu = torch.triu_indices(6, 6, device=depth.device)
    A = (J[:, iu[0]] * J[:, iu[1]]).double().sum(0)
    return torch.cat([A, (J * r[:, None]).double().sum(0), (r * r).double().sum()[None], ok.double().sum()[None]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out")
    args = ap.parse_args()
    reps = max(args.reps, 10)
    import track_ref as T
    import tsdf_ref as R
    from estdepth_amd import camera, ops, tracking
    from estdepth_amd.fusion3d import TSDFVolume
    assert torch.cuda.is_available(), "tools/track_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W = 480, 640
    K = R.intrinsics(H, W)
    poses = R.scene_poses(3, seed=4)
    vol = TSDFVolume((256, 256, 256), R.VOXEL, (-3.84, -3.84, -0.5), device=dev)
    depths = np.stack([T.scene_maps(P, K, H, W)[0] for P in poses]).astype(np.float32)
    vol.integrate(torch.from_numpy(depths).to(dev), torch.from_numpy(poses), torch.from_numpy(K))
    depth = torch.from_numpy(T.scene_maps(T.HELD_OUT_POSE, K, H, W)[0].astype(np.float32)).to(dev)
    guess, Kt = torch.from_numpy(T.perturbed(T.HELD_OUT_POSE)), torch.from_numpy(K)
    maps = vol.render(guess, Kt, (H, W))
    model = dict(depth=maps["depth"], normal=maps["normal"], pose=guess, K=Kt)
    mats = camera.frame_align_matrices(guess, Kt, guess, Kt)
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB

    def kernel():
        return ops.frame_align(depth, None, model["depth"], model["normal"], mats, vol.trunc, vol.z_near, 0.0)

    mats_dev = mats.to(dev)

    def yardstick():
        return torch_sums(depth, model["depth"], model["normal"], mats_dev, vol.trunc, vol.z_near)
    got, want = kernel()[2].cpu().numpy(), yardstick().cpu().numpy()
    scale = np.maximum(np.abs(want), 1e-300)
    warm, cold = per_launch(kernel, reps), per_launch(kernel, reps, flush)
    y_warm, y_cold = per_launch(yardstick, reps), per_launch(yardstick, reps, flush)
    out = vol.track(depth, guess, Kt)
    t_track = wall(lambda: vol.track(depth, guess, Kt), max(reps // 5, 5))
    t_refine = wall(lambda: tracking.refine_pose(depth, Kt, guess, model, dist_max=vol.trunc, z_near=vol.z_near), max(reps // 5, 5))
    n = int(got[28])
    traffic = (H * W + n * 4) * 4.0 + 2 * H * W * 4.0
    fmt = lambda t: "median %8.2f us   (min %.2f, 10th / 90th percentile %.2f / %.2f)" % (1e3 * np.median(t), 1e3 * t.min(), 1e3 * np.percentile(t, 10),  # noqa: E731
                                                                                        1e3 * np.percentile(t, 90))
    te, ae = T.pose_error(out["pose"].numpy(), T.HELD_OUT_POSE)
    lines = [
        "track_bench: one %d x %d frame against a render of the 256^3 volume, %d launches per figure after 10 warm-up launches, %s" % (W, H, reps, torch.cuda.get_device_name(0)),
        "matched pixels %d of %d; %.1f MB of algorithmic traffic; the kernel's sums against the torch yardstick's: largest relative difference %.2e, counts %d / %d"
        % (n, H * W, traffic / 1e6, float(np.max(np.abs(got - want) / scale)), n, int(want[28])),
        "  (a) align_step launches (kernel + reduction), own event pair  " + fmt(warm),
        "  (b) the same behind a 1 GiB cache flush                       " + fmt(cold),
        "  (c) yardstick: the 29 sums with torch operators               " + fmt(y_warm),
        "      the same behind a 1 GiB cache flush                       " + fmt(y_cold),
        "  (d) TSDFVolume.track, max_iter = 10: %d iterations (%s), render included    wall clock " % (out["iterations"], out["reason"]) + fmt(t_track),
        "      tracking.refine_pose on the rendered model alone                         wall clock " + fmt(t_refine),
        "      pose error %.2f mm %.3f deg -> %.3f mm %.4f deg; rmse %.2f -> %.2f mm"
        % (1e3 * T.pose_error(guess.numpy(), T.HELD_OUT_POSE)[0], np.degrees(T.pose_error(guess.numpy(), T.HELD_OUT_POSE)[1]), 1e3 * te, np.degrees(ae),
           1e3 * out["trace"][0]["rmse"], 1e3 * out["trace"][-1]["rmse"]),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
