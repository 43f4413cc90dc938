"""estdepth_amd/registration.py's ``register_global`` on the device against the float64 / integer reference chain of
tests/global_reg_ref.py, on the fixture of that module (a floor, two walls, three boxes and a sphere) moved by three motions: 90 degrees
about z and 1 m, 175 degrees about a skew axis and 3 m, one drawn from a seed.  The two sides are DISJOINT samples of the scene.

  * ``register`` from the identity does not land: its verdict and error are printed, and the error is asserted to lie outside the basin
    of 98 mm / 5 degrees.  This is the case the global stage exists for.
  * ``register_global(refine=None)`` returns the reference's hypothesis, inlier count, number of pairs and T_global TO THE BIT, the
    reference being given the very clouds and normals the device thinned (``out["clouds"]``).
  * with the staged refinement it lands within 2 x the reference chain's own error plus the stopping step: tests/test_gpu_registration.py's
    rule and reason (the partners may differ on ambiguous points).  The reference chain is global_reg_ref.chain followed by
    rigid_align_ref.refine with the same stages.
  * the same for a target given as a triangle mesh (sampled on the device first) and for bare clouds without normals on either side
    (estimated normals, the folded descriptor).
  * a winner below ``min_count`` comes back with reason "inliers" and the identity; ``compare_meshes(align=dict(metric="plane"))`` keeps
    today's keys and launches none of the new kernels; ``align=dict(init="global", voxel=V)`` brings a moved ground truth back.

The figures are printed (REGISTER-GLOBAL lines; recorded in profiles/global_register_gpu_tests.txt)."""
import numpy as np
import pytest
import torch

from estdepth_amd import registration

import global_reg_ref as G
import rigid_align_ref as RA
from test_gpu_recon3d_routes import _cpu, _dev, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ("cloud", "mesh", "bare")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def _call(fx, kind, **kw):
    raw = fx["raw"]
    src, sn = _dev(raw["src"]), _dev(raw["src_normal"])
    if kind == "mesh":
        return registration.register_global(src, dict(xyz=_dev(fx["mesh"]["xyz"]), faces=_dev(fx["mesh"]["faces"])), G.VOXEL, src_normal=sn,
                                            hypotheses=G.HYPOTHESES, **kw)
    if kind == "bare":
        return registration.register_global(src, _dev(raw["tgt"]), G.VOXEL, hypotheses=G.HYPOTHESES, **kw)
    return registration.register_global(src, dict(xyz=_dev(raw["tgt"]), normal=_dev(raw["tgt_normal"])), G.VOXEL, src_normal=sn,
                                        hypotheses=G.HYPOTHESES, **kw)


@pytest.mark.parametrize("name", G.MOTIONS)
def test_register_from_the_identity_does_not_land(name):
    fx = G.fixture(name)
    out = under("torch", lambda: registration.register(_dev(fx["src"]), dict(xyz=_dev(fx["tgt"]), normal=_dev(fx["tgt_normal"])), metric="plane",
                                                       dist_max=G.staged(), src_normal=_dev(fx["src_normal"])))
    et, er = G.error(out["T"], fx["T_true"])
    print("REGISTER-GLOBAL %s, register from the identity: %s after %d iterations, %.0f mm %.1f deg from the truth"
          % (name, out["reason"], out["iterations"], 1e3 * et, np.degrees(er)))
    assert et > G.BASIN_T or er > G.BASIN_R


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", G.MOTIONS)
def test_register_global_lands_where_the_reference_chain_lands(name, kind):
    fx = G.fixture(name)
    out = under("torch", lambda: _call(fx, kind))
    c = out["clouds"]
    assert c["oriented"] == (kind != "bare") and out["refine"] is None
    clouds = [_cpu(c[k]) for k in ("src", "src_normal", "target", "target_normal")]
    ref = G.chain(*clouds, oriented=c["oriented"])
    eg, rg = G.error(out["T_global"], fx["T_true"])
    print("REGISTER-GLOBAL %s %s: %d and %d points, %d pairs, winner %d with %d inliers (fitness %.3f), tallies %s; global stage %.1f mm %.2f deg"
          % (name, kind, clouds[0].shape[0], clouds[2].shape[0], out["pairs"], out["hypothesis"], out["count"], out["fitness"], out["status"],
             1e3 * eg, np.degrees(rg)))
    assert out["pairs"] == ref["pairs"] and out["hypothesis"] == ref["hypothesis"] and out["count"] == ref["count"]
    assert out["reason"] == ref["reason"] == "global" and out["converged"]
    assert out["T_global"].tobytes() == ref["T_global"].tobytes() and out["T"].tobytes() == ref["T_global"].tobytes()
    assert list(out["status"].values()) == np.bincount(ref["ransac"]["status"], minlength=4).tolist()
    assert out["fitness"] == ref["count"] / ref["pairs"]
    # the refinement: the device's against the float64 reference's, from the same start
    target = fx["mesh"] if kind == "mesh" else dict(xyz=clouds[2], normal=clouds[3])
    fine = G.refine(clouds[0], target, ref["T_global"])
    got = under("torch", lambda: _call(fx, kind, refine=dict(metric="plane")))
    assert got["T_global"].tobytes() == out["T_global"].tobytes() and got["refine"] is not None and got["refine"]["T"] is got["T"]
    tr, ar = G.error(fine["T"], fx["T_true"])
    td, ad = G.error(got["T"], fx["T_true"])
    print("REGISTER-GLOBAL %s %s refined: reference %.3g mm %.3g deg (%s, %d iterations); device %.3g mm %.3g deg (%s, %d iterations)"
          % (name, kind, 1e3 * tr, np.degrees(ar), fine["reason"], fine["iterations"], 1e3 * td, np.degrees(ad), got["reason"], got["refine"]["iterations"]))
    assert got["converged"] == fine["converged"] and got["reason"] == fine["reason"]
    assert td <= 2 * tr + RA.STEP_T and ad <= 2 * ar + RA.STEP_R


def test_a_winner_below_min_count_is_not_applied():
    fx = G.fixture("z90")
    out = under("torch", lambda: _call(fx, "cloud", min_count=100000, refine=dict(metric="plane")))
    assert out["reason"] == "inliers" and not out["converged"] and out["refine"] is None
    assert (out["T"] == np.eye(4)).all() and (out["T_global"] == np.eye(4)).all() and 0 < out["count"] < 100000 and out["hypothesis"] >= 0


def _moved_meshes():
    xyz, faces = G.scene_mesh()
    fine = RA.subdivided(xyz, faces)                                      # the same surface with other faces, hence other samples
    T = G.motion("skew175")
    Ti = np.linalg.inv(T)
    gt = dict(xyz=_dev(xyz), faces=_dev(faces))
    pred = dict(xyz=_dev(fine[0]), faces=_dev(fine[1]))
    moved = dict(xyz=_dev((fine[0].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)), faces=pred["faces"])
    return gt, pred, moved, T


def test_compare_meshes_keeps_its_bits_and_gains_the_global_start():
    from estdepth_amd.cloud_metrics import compare_meshes
    gt, pred, moved, T = _moved_meshes()
    density = 800.0
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        base = compare_meshes(pred, gt, density, align=dict(metric="plane"))
        torch.cuda.synchronize()
    # the evidence that the default path is untouched: none of the new kernels is launched, and the block has today's keys (two calls
    # agreeing shows repeatability only; the parent's bits are compared by tools/tsdf_bench.py --global-register --parent-tree)
    assert not [e.key for e in prof.key_averages() if "greg_" in e.key]
    assert sorted(base["alignment"]) == ["T", "converged", "correction", "iterations", "overlap", "reason", "rmse"]
    plain = compare_meshes(moved, gt, density)
    stuck = compare_meshes(moved, gt, density, align=dict(metric="plane"))
    got = compare_meshes(moved, gt, density, align=dict(metric="plane", init="global", voxel=G.VOXEL, hypotheses=G.HYPOTHESES))
    al = got["alignment"]
    et, er = G.error(np.asarray(al["T"]).reshape(4, 4), T)
    print("REGISTER-GLOBAL compare_meshes: accuracy unmoved %.6f, moved %.6f, aligned from the identity %.6f (%s), from the global start %.6f; "
          "T off by %.3g mm %.3g deg; global %s" % (base["accuracy"], plain["accuracy"], stuck["accuracy"], stuck["alignment"]["reason"], got["accuracy"],
                                                   1e3 * et, np.degrees(er), {k: v for k, v in al["global"].items() if k != "T_global"}))
    assert sorted(set(al) - set(base["alignment"])) == ["global"] and sorted(al["global"]) == ["T_global", "count", "fitness", "hypothesis", "pairs"]
    # the margin is measured as tests/test_gpu_registration.py measures it: the sampled score's own repeatability over three other seeds
    unmoved = compare_meshes(pred, gt, density)
    repeat = max(abs(compare_meshes(pred, gt, density, seed=s)["accuracy"] - unmoved["accuracy"]) for s in (1, 2, 3))
    print("REGISTER-GLOBAL compare_meshes: unaligned unmoved accuracy %.6f, repeatability %.3g" % (unmoved["accuracy"], repeat))
    assert al["converged"] and et <= G.BASIN_T and er <= G.BASIN_R
    assert plain["accuracy"] > unmoved["accuracy"] + repeat and abs(got["accuracy"] - unmoved["accuracy"]) <= repeat
    for bad in (dict(init="global"), dict(init="local", voxel=0.1), dict(voxel=0.1), dict(hypotheses=10)):
        with pytest.raises(RuntimeError, match="compare_meshes: align"):
            compare_meshes(moved, gt, density, align=dict(metric="plane", **bad))
    # a winner refused for its inliers (one hypothesis cannot gather 20): reported, not applied, the unmoved prediction is scored
    refused = compare_meshes(moved, gt, density, align=dict(metric="plane", init="global", voxel=G.VOXEL, hypotheses=1))
    ra = refused["alignment"]
    assert ra["reason"] == "inliers" and not ra["converged"] and ra["iterations"] == 0 and ra["T"] == [float(v) for v in np.eye(4).reshape(-1)]
    assert ra["global"]["count"] < 20 and ra["global"]["T_global"] == ra["T"]
    assert {k: v for k, v in refused.items() if k != "alignment"} == plain


def test_the_global_start_against_a_cloud_target():
    """``align=dict(init="global")`` where the target is a ``PointGrid``: compare_clouds, and compare_meshes with a ground truth without faces"""
    from estdepth_amd.cloud_metrics import compare_clouds, compare_meshes
    fx = G.fixture("skew175")
    raw = fx["raw"]
    src, sn, tgt, tn = (_dev(raw[k]) for k in ("src", "src_normal", "tgt", "tgt_normal"))
    align = dict(metric="plane", init="global", voxel=G.VOXEL, hypotheses=G.HYPOTHESES)
    plain = compare_clouds(src, tgt, pred_normal=sn, gt_normal=tn)
    for name, got in (("compare_clouds", compare_clouds(src, tgt, pred_normal=sn, gt_normal=tn, align=align)),
                      ("compare_meshes, a ground truth without faces",
                       compare_meshes(dict(xyz=src, normal=sn), dict(xyz=tgt, normal=tn), 800.0, align=align))):
        al = got["alignment"]
        et, er = G.error(np.asarray(al["T"]).reshape(4, 4), fx["T_true"])
        print("REGISTER-GLOBAL %s: %s, T off by %.3g mm %.3g deg, accuracy %.6f (unaligned %.6f); global %s"
              % (name, al["reason"], 1e3 * et, np.degrees(er), got["accuracy"], plain["accuracy"], {k: v for k, v in al["global"].items() if k != "T_global"}))
        assert sorted(al["global"]) == ["T_global", "count", "fitness", "hypothesis", "pairs"] and al["global"]["count"] >= 20
        assert al["converged"] and et <= G.BASIN_T and er <= G.BASIN_R and got["accuracy"] < plain["accuracy"]
