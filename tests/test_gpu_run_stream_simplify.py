"""tools/run_stream.py --mesh M.ply --mesh-simplify CELL end to end on the device, on the scene, the 170-triangle ground-truth mesh and the
set-up of tests/test_gpu_run_stream_sample.py (its helpers are imported, not edited), with --score-3d GT.ply --score-sample 1111
--score-exact:
  * the ``mesh`` block of metrics.json carries the simplification's stats and describes the simplified mesh, which is the file that was
    written; without the flag the block, the cloud and the dumps are what they were;
  * the simplified mesh is the numpy reference's simplification of the device's surface nets, bit for bit;
  * the exact accuracy against the ground truth agrees with the float64 chain's figure for the same flags -- tests/tsdf_mesh_ref.py's
    float64 surface nets of the fused volume, simplified by tests/mesh_simplify_ref.py, carrying the device's sample records (as that
    test's chain measures the device's samples) and measured by the brute force of tests/mesh_distance_ref.py, clamped and averaged --
    within the margin tests/test_gpu_run_stream_exact.py grants the unsimplified run: 2 x the mean e_dist of the winners; and so does
    the host chain from the device's own surface nets with the reference sampler."""
import json
import sys

import numpy as np
import pytest
import torch

import mesh_distance_ref as D
import mesh_sample_ref as MS
import mesh_simplify_ref as R
import tsdf_mesh_ref as M
from test_gpu_run_stream_mesh import _argv, _dumps
from test_gpu_run_stream_sample import TOOL, scene  # noqa: F401 -- the scene fixture

pytestmark = pytest.mark.gpu
CELL, DENSITY = 0.08, 1111
STATS = ["collapsed", "duplicates", "faces", "faces_in", "fallback", "invalid", "placed", "vertices", "vertices_in"]


@pytest.fixture(scope="module")
def runs(scene, tmp_path_factory):
    """the command as a user gives it (main() = parse + run + metrics.json), and the same command without the flag in-process for its volume"""
    d, gt, _ = scene
    out = tmp_path_factory.mktemp("simplify")
    simp, plain = out / "simplified", out / "plain"
    score = ("--score-3d", gt, "--score-sample", DENSITY, "--score-exact")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(sys, "argv", ["run_stream.py"] + _argv(d, simp, "--fuse", simp / "scene.ply", "--mesh", simp / "mesh.ply", "--mesh-simplify", CELL, *score))
        TOOL.main()
    torch.cuda.synchronize()
    report = json.load(open(simp / "metrics.json"))
    base, state = TOOL.run(TOOL.parse(_argv(d, plain, "--fuse", plain / "scene.ply", "--mesh", plain / "mesh.ply", *score)))
    torch.cuda.synchronize()
    full = state.volume.extract_mesh()
    origin = np.asarray(state.volume.origin, np.float32)
    want = R.simplify(full["xyz"].cpu().numpy(), full["faces"].cpu().numpy(), CELL, origin)
    return dict(simp=simp, plain=plain, report=report, base=base, state=state, full=full, origin=origin, want=want, gt=gt)


def read_gt(gt):
    from estdepth_amd.fusion3d import read_ply
    return read_ply(gt, faces=True)


def _accuracy64(xyz, faces, n, gt, max_dist):
    """the host's end of the chain: the reference sampler (seed 0), the brute-force distance to the ground truth, clamped and averaged
    -> (accuracy, the margin of tests/test_gpu_run_stream_exact.py, the number of samples, the standard error of the mean over the draw)"""
    samples = MS.sample(xyz, faces, None, n, 0)["xyz"]
    gt_mesh = read_gt(gt)
    dmin, _, bf = D.nearest64(samples.astype(np.float32), gt_mesh["xyz"], gt_mesh["faces"])
    bound = D.C * float(np.take_along_axis(bf["e_dist"], np.argmin(bf["dist"], 1)[:, None], 1).mean())
    clamped = np.minimum(dmin, max_dist)
    return float(clamped.mean()), bound, samples.shape[0], float(clamped.std() / np.sqrt(clamped.shape[0]))


def test_the_mesh_block_and_the_file(runs):
    from estdepth_amd.fusion3d import mesh_edge_stats, read_ply
    block, got, base, state, full = runs["report"]["mesh"], runs["report"]["recon_3d"], runs["base"], runs["state"], runs["full"]
    simp, plain = runs["simp"], runs["plain"]
    # without the flag: today's block; with it: one more entry, and the cloud and the dumps are the same bytes
    assert sorted(set(block) - set(base["mesh"])) == ["simplify"] and "simplify" not in base["mesh"]
    assert sorted(block["simplify"]) == sorted(STATS + ["cell", "euler"]) and block["simplify"]["cell"] == CELL
    assert (plain / "scene.ply").read_bytes() == (simp / "scene.ply").read_bytes()
    a, b = _dumps(simp), _dumps(plain)
    assert a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    # the block and the file are the simplified mesh of the fused volume
    m = state.volume.extract_mesh(simplify=CELL)
    s = block["simplify"]
    assert {k: s[k] for k in STATS} == m["stats"] and s["invalid"] == 0
    assert (s["vertices_in"], s["faces_in"]) == (base["mesh"]["vertices"], base["mesh"]["faces"]) == (full["count"], full["faces"].shape[0])
    assert (block["vertices"], block["faces"]) == (s["vertices"], s["faces"]) and 0 < s["faces"] < s["faces_in"] / 4
    e = mesh_edge_stats(m["faces"])
    assert (block["boundary_edges"], block["manifold_edges"], block["non_manifold_edges"], s["euler"]) == (e["boundary"], e["manifold"], e["non_manifold"], e["euler"])
    back = read_ply(str(simp / "mesh.ply"), faces=True)
    assert np.array_equal(back["xyz"].view(np.int32), m["xyz"].cpu().numpy().view(np.int32)) and np.array_equal(back["faces"], m["faces"].cpu().numpy())
    assert got["exact"]["faces_pred"] == s["faces"] - got["exact"]["invalid_pred"]
    # the device's simplification of ITS mesh is the reference's, bit for bit
    R.compare({k: v.cpu().numpy() for k, v in m.items() if isinstance(v, torch.Tensor)}, runs["want"], "run_stream --mesh-simplify",
              keys=("faces", "xyz", "normal", "placed"))
    print("RUN-STREAM simplify %.2f: %s; edges %d / %d / %d; exact accuracy %.6f completeness %.6f; unsimplified accuracy %.6f completeness %.6f"
          % (CELL, s, e["boundary"], e["manifold"], e["non_manifold"], got["accuracy"], got["completeness"], base["recon_3d"]["accuracy"],
             base["recon_3d"]["completeness"]))


def test_exact_accuracy_against_the_host_chain_from_the_device_s_surface_nets(runs):
    """everything behind the surface nets on the host: the device's fp32 surface nets simplified by the numpy reference, sampled by the
    reference sampler and measured by the float64 brute force, within the margin of tests/test_gpu_run_stream_exact.py"""
    got, want = runs["report"]["recon_3d"], runs["want"]
    chain, bound, n, _ = _accuracy64(want["xyz"], want["faces"], got["n_pred"], runs["gt"], got["max_dist"])
    print("RUN-STREAM simplify, the host chain from the device's own surface nets: accuracy %.6f against the device's %.6f (bound %.3g, %d samples)"
          % (chain, got["accuracy"], bound, n))
    assert abs(got["accuracy"] - chain) <= bound


def test_exact_accuracy_against_the_float64_chain(runs):
    """The chain starts from the FLOAT64 surface nets (tests/tsdf_mesh_ref.py), simplified by the numpy reference; the margin is the one
    of tests/test_gpu_run_stream_exact.py, 2 x the mean e_dist of the winners.  As in that test, the chain measures the SAME samples as
    the device: that margin bounds the fp32 distance arithmetic between two measurements of the same points and nothing else.  Here the
    two surfaces are two meshes, so "the same samples" are the same (face, barycentric pair) records -- the device's, from
    sample_mesh(density, seed 0) on its simplified mesh, which is what the tool scored -- placed on the chain's vertices in float64;
    the two face lists must be equal for that, and are asserted to be.

    A first version of this test drew the chain's samples afresh with the reference sampler and missed the margin: 0.003546 m against
    the device's 0.003556 m, 1.0e-5 m apart where 6.0e-7 m are allowed, although all 1368 clusters and 2219 faces were the same and no
    vertex had moved by more than 9.8e-6 m.  The sampler places sample i at i w + (hash mod w) units of quantised area with
    w = total / n, so the last bit of the total area re-draws every sample inside its stratum: two draws of 7022 points, whose means no
    rounding margin relates (the standard error of such a mean over an independent draw, printed below, is 2.0e-4 m).  Both figures are
    still printed."""
    from estdepth_amd.fusion3d import sample_mesh
    got, state, want = runs["report"]["recon_3d"], runs["state"], runs["want"]
    host = state.volume.volume.cpu().numpy()
    ref = M.mesh(host[0], host[1], 1.0, state.volume.voxel_size, state.volume.origin.tolist())
    chain_mesh = R.simplify(ref["xyz"].astype(np.float32), ref["faces"].astype(np.int32), CELL, runs["origin"])
    # where the two chains part: the float64 surface nets against the device's fp32 ones, carried through the clustering
    both, ia, ib = np.intersect1d(want["cell_key"], chain_mesh["cell_key"], return_indices=True)
    moved = np.abs(want["xyz"][ia].astype(np.float64) - chain_mesh["xyz"][ib]).max(1)
    flips = int((want["placed"][ia] != chain_mesh["placed"][ib]).sum())
    print("RUN-STREAM simplify, float64 against fp32 surface nets: input vertices differ by at most %.3e m; %d of %d clusters in common, %d with another "
          "placed flag, output vertices moved by at most %.3e m (mean %.3e m), faces %d against %d"
          % (np.abs(ref["xyz"] - runs["full"]["xyz"].cpu().numpy()).max(), both.shape[0], want["cell_key"].shape[0], flips, moved.max(), moved.mean(),
             want["faces"].shape[0], chain_mesh["faces"].shape[0]))
    assert np.array_equal(want["cell_key"], chain_mesh["cell_key"]) and np.array_equal(want["faces"], chain_mesh["faces"])
    # the device's sample records on the chain's vertices
    dev = sample_mesh(state.volume.extract_mesh(simplify=CELL), density=DENSITY, seed=0)
    face, uv = dev["face"].cpu().numpy().astype(np.int64), dev["bary"].cpu().numpy().astype(np.float64)
    assert face.shape[0] == got["n_pred"]
    a, b, c = (chain_mesh["xyz"][chain_mesh["faces"][face, j]].astype(np.float64) for j in range(3))
    samples = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    gt_mesh = read_gt(runs["gt"])
    dmin, _, bf = D.nearest64(samples.astype(np.float32), gt_mesh["xyz"], gt_mesh["faces"])
    bound = D.C * float(np.take_along_axis(bf["e_dist"], np.argmin(bf["dist"], 1)[:, None], 1).mean())
    chain = float(np.minimum(dmin, got["max_dist"]).mean())
    area = MS.face_area(chain_mesh["xyz"], chain_mesh["faces"])["area"].sum()
    redrawn, _, n, stderr = _accuracy64(chain_mesh["xyz"], chain_mesh["faces"], MS.n_for_density(DENSITY, area), runs["gt"], got["max_dist"])
    print("RUN-STREAM simplify, the float64 chain on the device's sample records: accuracy %.6f against the device's %.6f (difference %.3e, bound %.3g, "
          "%d samples); with its samples drawn afresh by the reference sampler: %.6f (difference %.3e, %d samples; the standard error of the mean over "
          "an independent draw is %.3e)" % (chain, got["accuracy"], abs(got["accuracy"] - chain), bound, face.shape[0], redrawn,
                                            abs(got["accuracy"] - redrawn), n, stderr))
    assert abs(got["accuracy"] - chain) <= bound


def test_the_parse_time_refusals(scene, tmp_path, capsys):
    d, gt, _ = scene
    fuse = ("--fuse", tmp_path / "scene.ply")
    for bad in ((*fuse, "--mesh-simplify", CELL), (*fuse, "--mesh", tmp_path / "m.ply", "--mesh-simplify", 0), (*fuse, "--mesh", tmp_path / "m.ply", "--mesh-simplify", "nan"),
                (*fuse, "--mesh", tmp_path / "m.ply", "--mesh-simplify", -0.1)):
        with pytest.raises(SystemExit):
            TOOL.parse(_argv(d, tmp_path, *bad))
        assert "--mesh-simplify" in capsys.readouterr().err, bad
    TOOL.parse(_argv(d, tmp_path, *fuse, "--mesh", tmp_path / "m.ply", "--mesh-simplify", CELL, "--mesh-min-component", 100))
