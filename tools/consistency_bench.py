"""Stand-alone timing of csrc/depth_consistency.hip on an MI355X (device events, warm-up, the median of many launches; not part of bench.py).

    python tools/consistency_bench.py [--reps 200] [--out profiles/consistency_bench.txt]

One 640 x 480 target of the analytic plane-plus-sphere scene of tests/tsdf_ref.py (0.4 % noise, the "full" geometry of tests/consistency_ref.py)
checked against 2, 4 and 8 sources through ops.depth_consistency, the matrices formed once outside the timed region:
  (a) one launch between its own pair of device events, maps wherever the previous launch left them (the median and the spread of the launches)
  (b) the same behind a 1 GiB buffer rewritten (untimed) in front of every launch: the maps come from HBM, as behind a model step
  (c) 100 launches back to back between ONE pair of events, per launch: what a launch costs once the queue hides the launch latency
The algorithmic traffic is (1 + S) maps read and 4 written; its time at the 6.3 TB/s streaming rate of an MI355X is printed beside the figures
(a roofline, not a pass bar: a kernel this small is expected to be bound by its launch)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_BPS = 6.3e12          # achievable HBM streaming rate of an MI355X


def per_launch(fn, reps, flush=None, warmup=10):
    """ms of every one of ``reps`` launches, each between its own pair of device events"""
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


def back_to_back(fn, n, rounds=5):
    """ms per launch of ``n`` launches between one pair of events; the median of ``rounds``"""
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    reps = max(args.reps, 20)
    import consistency_ref as C
    from estdepth_amd import camera, ops
    assert torch.cuda.is_available(), "tools/consistency_bench.py needs a ROCm device"
    dev = torch.device("cuda:0")
    H, W = 480, 640
    flush = torch.empty(256 << 20, device=dev)          # 1 GiB
    lines = ["consistency_bench: one %d x %d target against S sources, %d launches per figure after 10 warm-up launches, %s"
             % (W, H, reps, torch.cuda.get_device_name(0))]
    for S in (2, 4, 8):
        c = C.make_case((H, W), S, seed=4)
        target = torch.from_numpy(c["target"]).to(dev)
        sources = [torch.from_numpy(s).to(dev) for s in c["sources"]]
        mats = camera.consistency_matrices(torch.from_numpy(c["pose_t"]), torch.from_numpy(c["K_t"]), torch.from_numpy(c["poses_s"]), torch.from_numpy(c["K_s"]))

        def check():
            return ops.depth_consistency(target, sources, mats, C.PX_MAX, C.REL_MAX, C.Z_NEAR)
        views, visible, _, _ = check()
        torch.cuda.synchronize()
        share = float(views.sum().item()) / max(float(visible.sum().item()), 1.0)
        warm, cold, b2b = per_launch(check, reps), per_launch(check, reps, flush), back_to_back(check, 100)
        traffic = (1 + S + 4) * H * W * 4.0
        floor_us = traffic / STREAM_BPS * 1e6
        lines += [
            "S = %d: %.1f MB of algorithmic traffic ((1 + S) maps read, 4 written) = %.2f us at %.1f TB/s; consistent share of the visible sources %.3f"
            % (S, traffic / 1e6, floor_us, STREAM_BPS / 1e12, share),
            "  (a) one launch, own event pair          median %7.2f us   (min %.2f, 10th / 90th percentile %.2f / %.2f)"
            % (1e3 * np.median(warm), 1e3 * warm.min(), 1e3 * np.percentile(warm, 10), 1e3 * np.percentile(warm, 90)),
            "  (b) the same behind a 1 GiB cache flush median %7.2f us   (min %.2f, 10th / 90th percentile %.2f / %.2f)"
            % (1e3 * np.median(cold), 1e3 * cold.min(), 1e3 * np.percentile(cold, 10), 1e3 * np.percentile(cold, 90)),
            "  (c) 100 launches back to back, per launch      %7.2f us   = %.2f TB/s of algorithmic traffic, %.1f %% of the streaming rate"
            % (1e3 * b2b, traffic / (b2b * 1e-3) / 1e12, 100.0 * floor_us / (1e3 * b2b)),
        ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
