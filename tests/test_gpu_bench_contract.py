"""GPU: bench.py contract -- one JSON line with the required keys at N=1 (a plain run: the headline alone; --full: everything
else beside it), and the N=2 code path (two ranks sharing the single test GPU, gloo instead of RCCL) including the memory-bank
all-gather and the max-over-ranks timing."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_bench_plain_line_is_the_headline_alone():
    """a plain run (no --full): set-up, warm-up, the timed steps, one line -- the headline fields, nothing measured beside them"""
    out = subprocess.run([sys.executable, "bench.py", "--workload", "cfg1", "--steps", "3", "--warmup", "1"], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert REQUIRED <= set(d) and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "depth frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["config"]["workload"].startswith("cfg1")
    assert abs(d["config"]["depth_frames_per_step"] * 1e3 / d["value"] - d["ms_per_step"]) <= 1e-3          # value = frames per step / step time
    assert d["config"]["full"] is False and d["roofline"] is None and d["config"]["sustained"] is None and d["config"]["dump_outputs"] is None
    assert not {"cpu_baseline", "parity", "other_workloads", "alt_arith"} & set(d)


def test_bench_single_gpu_line():
    out = subprocess.run([sys.executable, "bench.py", "--full", "--workload", "cfg1", "--steps", "3", "--warmup", "1", "--sustained-s", "1", "--sustained-bucket", "50", "--no-replay-profile"], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    d = _last_json(out.stdout)
    assert REQUIRED <= set(d) and "cpu_baseline" in d and d["config"]["full"] is True
    assert d["parity"]["logits_within_tolerance"] and set(d["parity"]["logit_volumes_vs_oracle"]) == {"init", "fused"}
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["config"]["workload"].startswith("cfg1")
    assert d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] <= 1
    assert d["cpu_baseline"]["kind"] in ("port", "torch-ops") and d["cpu_baseline"]["cores"] >= 1
    runs = d["cpu_baseline"]["all_runs"]     # the C/OpenMP port at 8 threads, the torch-operator leg at 8 threads and at the box's default; headline = the fastest
    assert [(r["kind"], r["cores"] == 8) for r in runs[:2]] == [("port", True), ("torch-ops", True)] and runs[2]["kind"] == "torch-ops"
    assert len(runs) in (3, 5) and d["cpu_baseline"]["value"] == max(r["value"] for r in runs)
    if len(runs) == 5:     # a box with a >= 16-core socket: + the torch-operator leg at 32 and 64 threads pinned to the physical cores of one socket
        assert [(r["kind"], bool(r["pinned"])) for r in runs[3:]] == [("torch-ops", True)] * 2 and runs[3]["cores"] <= 32 < runs[4]["cores"] <= 64 \
            or runs[3]["cores"] == runs[4]["cores"]           # (a socket with <= 32 cores runs both legs on all of them)
    assert all(not r["pinned"] for r in runs[:3])
    assert d["parity"]["within_tolerance"] and max(d["parity"]["max_abs_depth_diff_vs_oracle_m"].values()) <= 1e-4
    # SURVEY section 8(d) "Metric": abs_rel(depth_gpu, depth_cpu) per output scale beside the max-abs figure, against both CPU arithmetics
    assert d["parity"]["oracle_kind"] == "port" and set(d["parity"]["abs_rel_vs_oracle"]) == set(d["parity"]["max_abs_depth_diff_vs_oracle_m"])
    assert all(0 <= v < 1e-4 for v in d["parity"]["abs_rel_vs_oracle"].values()), d["parity"]["abs_rel_vs_oracle"]
    assert max(d["parity"]["vs_torch_ops"]["max_abs_depth_diff_m"].values()) <= 2e-4 and all(v < 1e-4 for v in d["parity"]["vs_torch_ops"]["abs_rel"].values())
    assert {"homo_warp_costvol", "softargmin"} <= set(d["roofline"]["hbm_kernels"])
    assert "conv3d:32->32" in d["roofline"]["mfma_kernels"]
    assert d["dtype"] == "f32" and d["config"]["conv3d_arith"] == "f32"          # the headline is native fp32 MFMA
    from estdepth_amd import _native
    if _native.has_ab():                                      # the operand-split second opinion exists in ESTD_BUILD_AB=1 builds only
        assert d["alt_arith"]["conv3d_arith"] == "bf16x3" and d["alt_arith"]["value"] > 0
    else:
        assert "alt_arith" not in d


@pytest.mark.parametrize("workload", ["cfg1", "stream"])
def test_bench_dump_outputs_are_repeatable(tmp_path, workload):
    """--dump-outputs DIR: the last timed step's results as float32 / float64 .npy files within 64 MB, the depth maps among them, the
    same files from a second run of the same command (identical seeded inputs; within 1e-4, the parity bar, since bench.py lets the
    library pick its 2D convolution algorithms per process); --steps is the timed step count."""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, "bench.py", "--workload", workload, "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / run)],
                             cwd=ROOT, capture_output=True, text=True, timeout=900)
        d = _last_json(out.stdout)
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and set(d["config"]["dump_outputs"]) == {f[:-4] for f in os.listdir(tmp_path / run)}
        dumps.append({f: np.load(os.path.join(tmp_path, run, f)) for f in sorted(os.listdir(tmp_path / run))})
    a, b = dumps
    assert any(f.startswith("outputs_depth_") for f in a) and sorted(a) == sorted(b)
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in a) <= 64 * 2 ** 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and np.isfinite(a[f]).all(), f
        np.testing.assert_allclose(a[f], b[f], rtol=1e-4, atol=1e-4, err_msg=f)


def test_bench_headline_workload_roofline_fields_are_hardware_fractions():
    """BASELINE configs[1] (the workload `value` is quoted on): `frac` is the EXECUTED fraction of the fp32 MFMA peak
    (<= 1 -- the algorithmic rate of a Winograd kernel is above the peak and lives in its own field), the dominant kernel's
    launches fit inside the step, the stand-alone HBM-kernel figures are present.  The per-kernel in-step figures describe the
    hipGraph REPLAY that produced `value` (rocprofv3 kernel trace of a child run), the dominant kernel's live HIP-event brackets
    agree with it within 15 %, and every family whose eager bracket is further off is named.  The other single-GPU workloads
    (ESTM window, cfg5, stream) are timed in the same run."""
    out = subprocess.run([sys.executable, "bench.py", "--full", "--workload", "joint", "--steps", "5", "--warmup", "2", "--no-alt", "--no-cpu-baseline", "--sustained-s", "6"],
                         cwd=ROOT, capture_output=True, text=True, timeout=1500)
    d = _last_json(out.stdout)
    r = d["roofline"]
    assert r["replay_trace"] and "error" not in r["replay_trace"], r["replay_trace"]
    assert d["config"]["pipeline"] is False and d["config"]["serial_replay"] is None      # (the pipelined replay is opt-in: --pipeline on)
    assert abs(r["replay_trace"]["ms_per_step"] / d["ms_per_step"] - 1.0) < 0.10           # the traced child ran the same step
    fams = dict(r["mfma_kernels"], **r["hbm_kernels"])
    # (dres2 = 33 -> 33 runs as a 33 -> 32 launch of the three-axis kernel + its 33rd output channel as a pass of its own: round 6)
    assert {"conv3d:32->32", "conv3d:33->32", "conv3d:33->1", "conv3d:16->16", "conv3d:32->16", "warp_attention", "homo_warp_costvol",
            "softargmin", "gru_elementwise"} <= set(fams)
    for name, k in fams.items():
        assert k["source"] == "replay", (name, k)                                           # no family falls back to the eager brackets
        assert abs(k["launches_per_step"] - k["launches"] / d["steps"]) < 1e-6, (name, k)   # same launches in both passes
        off = abs(k["eager_over_replay"] - 1.0) > 0.15
        assert off == (name in r["families_perturbed_by_eager_brackets"]), (name, k)
    assert "conv3d:32->32" not in r["families_perturbed_by_eager_brackets"], r["replay"]   # the contract's live HIP-event figure holds
    assert abs(r["replay"]["eager_over_replay"] - 1.0) <= 0.15
    assert sum(k["launches_per_step"] * k["avg_launch_ms"] for k in r["mfma_kernels"].values()) <= d["ms_per_step"]
    ow = d["other_workloads"]
    assert set(ow) == {"estm", "cfg5", "stream", "joint_stream"} and all(v.get("value", 0) > 0 for v in ow.values()), ow
    assert ow["joint_stream"]["value"] > d["value"] and ow["stream"]["value"] > ow["estm"]["value"]     # the feature caches pay
    assert ow["estm"]["workload"].startswith("cfg3") and ow["cfg5"]["workload"].startswith("cfg5")
    assert REQUIRED <= set(d) and d["config"]["workload"].startswith("cfg2")
    assert 0 < r["frac"] <= 1 and r["achieved"] <= r["peak"] and abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-3
    assert r["algorithmic_tflops"] >= r["achieved"] and abs(r["achieved"] - r["algorithmic_tflops"] * r["executed_factor"]) < 0.05
    assert r["launches_per_step"] * r["avg_launch_ms"] <= d["ms_per_step"]
    for k in r["mfma_kernels"].values():
        assert 0 < k["frac"] <= 1 and k["achieved_tflops"] <= r["peak"]
    alone = r["hbm_kernels_standalone"]
    assert {"homo_warp_costvol", "warp_attention N=3", "gru_blend", "softargmin_up (T=3)"} <= set(alone)
    assert all(0 < v["frac"] <= 1 for v in alone.values())
    assert d["value"] > 50.0                               # north_star: >= 50 depth frames/s on one MI355X
    # the headline against seconds of the same step (round 6): per-bucket ms/step, the ratio timed / sustained, clocks and power beside it
    su = d["config"]["sustained"]
    assert su["steps"] == su["bucket_steps"] * len(su["ms_per_step_per_bucket"]) >= 2 * su["bucket_steps"] and su["seconds"] > 3
    assert d["config"]["sustained_ms_per_step"] == su["ms_per_step"] and d["config"]["sustained_over_timed"] == su["timed_over_sustained"]
    assert 0.9 < su["timed_over_sustained"] < 1.1, su                  # a 5-step figure on a cold box may be off by more than the 20-step one
    assert "error" in su["clocks"] or su["clocks"]["samples"] >= 3, su["clocks"]


def test_bench_world_size_one_rccl_communicator():
    """ESTD_FORCE_DIST=1: the N > 1 code against real RCCL on the one GPU of the test box -- nccl process group with device_id,
    channel cap, CU reserve, the asynchronous all-gather overlapped with the next step, the own-shard bit-equality check."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["ESTD_FORCE_DIST"] = "1"
    out = subprocess.run([sys.executable, "bench.py", "--full", "--workload", "cfg1", "--steps", "3", "--warmup", "1", "--sustained-s", "1", "--sustained-bucket", "50", "--no-alt", "--no-cpu-baseline"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    d = _last_json(out.stdout)
    ag = d["config"]["allgather"]
    assert d["n_gpus"] == 1 and ag["backend"].startswith("RCCL") and ag["own_shard_bit_equal"] is True
    assert ag["ms_alone"] > 0 and ag["ms_per_step_without_collective"] > 0 and "CUs left free" in d["config"]["parallelism"]
    assert "logit volume" in ag["record"] and ag["algo"] == "collective" and ag["algo_setting"] == "auto"
    # the CU reserve is held only where the exchange runs (a device-local copy here: stage A), and its cost is measured
    assert ag["reserve_scope"] == "A" and ag["reserved_cus"] == 8 and ag["reserve_scope_probe"]["exchange_alone_ms"] > 0
    assert ag["ms_per_step_without_collective_without_reserve"] > 0 and abs(ag["reserve_cost_ms"]) < 0.5 * d["ms_per_step"]
    assert ag["rccl"].get("debug_lines", 0) > 0, ag["rccl"]           # RCCL's own account of its set-up was captured and summarised


def test_bench_direct_exchange_world_size_one_rccl():
    """ESTD_AG_ALGO=direct on the world-size-1 RCCL communicator (the all-to-all send/recv list is empty there: own-shard copy only)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(ESTD_FORCE_DIST="1", ESTD_AG_ALGO="direct")
    out = subprocess.run([sys.executable, "bench.py", "--workload", "cfg1", "--steps", "3", "--warmup", "1", "--sustained-s", "1", "--sustained-bucket", "50", "--no-alt", "--no-cpu-baseline"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    d = _last_json(out.stdout)
    assert d["config"]["allgather"]["algo"] == "direct" and d["config"]["allgather"]["own_shard_bit_equal"] is True


def _check_two_ranks(d):
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["allgather"]["ms_per_step_without_collective"] > 0          # every N > 1 line carries the step time without the exchange
    assert d["config"]["allgather"]["auto"]["chosen"] in ("collective", "direct")   # ESTD_AG_ALGO=auto: both timed, every rank agreed
    assert "all-gather" in d["config"]["parallelism"]
    assert len(d["config"]["per_rank_ms_per_step"]) == 2
    ag = d["config"]["allgather"]
    assert ag["bytes_sent_per_rank"] == 4 * (2 * 16 * 16 * 32 * 40 + 16 + 16 * 32 * 40) and ag["bus_gbs_per_rank"] > 0      # K||V + pose + logits
    assert ag["other_algo"]["algo"] == "direct" and ag["other_algo"]["ms_alone"] > 0            # both exchange algorithms ran (gloo here)
    assert ag["own_shard_bit_equal"] is True             # the gathered bank equals the owner's tensors bit for bit


def test_bench_gpus_flag_launches_the_ranks_itself():
    """the driver's command line: `python bench.py --gpus N` with NO launcher and no WORLD_SIZE -> bench.py re-executes
    itself under torch.distributed.run with N ranks (here: 2 ranks sharing the single test GPU, gloo instead of RCCL)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, "bench.py", "--full", "--gpus", "2", "--workload", "cfg1", "--steps", "3", "--warmup", "1", "--sustained-s", "1", "--sustained-bucket", "50"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    d = _last_json(out.stdout)
    _check_two_ranks(d)
    assert any("share" in n for n in d["config"]["notes"])          # flagged as a code-path check on a 1-GPU box


def test_bench_two_ranks_under_an_external_launcher():
    env = dict(os.environ, ESTD_FORCE_DEVICE="0", ESTD_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "bench.py", "--full", "--gpus", "2", "--workload", "cfg1", "--steps", "3", "--warmup", "1", "--sustained-s", "1", "--sustained-bucket", "50"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    _check_two_ranks(_last_json(out.stdout))


def test_bench_line_survives_a_hanging_exchange_diagnostic():
    """the other exchange algorithm is timed last, under a watchdog: if it never returns (ESTD_AG_DIAG_TEST_HANG=1 = a sleep in its
    place on every rank) rank 0 still prints the complete line, says so in `other_algo`, and every rank exits with status 0"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(ESTD_AG_DIAG_TEST_HANG="1", ESTD_AG_DIAG_TIMEOUT="5")
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--workload", "cfg1", "--steps", "3", "--warmup", "1", "--sustained-s", "1", "--sustained-bucket", "50"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert d["n_gpus"] == 2 and d["value"] > 0 and len(d["config"]["per_rank_ms_per_step"]) == 2
    ag = d["config"]["allgather"]
    assert ag["own_shard_bit_equal"] is True and ag["bus_gbs_per_rank"] > 0
    assert ag["other_algo"]["algo"] == "direct" and "watchdog" in ag["other_algo"]["error"]
