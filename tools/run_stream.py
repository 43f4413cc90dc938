#!/usr/bin/env python
"""Streaming (ESTM) evaluation of one scene directory: the role of the reference's eval_hybrid_seq.py
(test_scannet_seq, :123-258) on top of estdepth_amd.ESTMStream -- read frames, slide the 3-frame window with a
2-window memory, dump float16 .npy depth / confidence maps, report the depth-error suite against the scene's
ground-truth depth.  Needs an MI355X (the model has no CPU path).

    python tools/run_stream.py --scene-dir /data/scannet/scene0707_00 --out /tmp/eval --loadckpt model.ckpt
    python tools/run_stream.py --synthetic 8 --out /tmp/eval          # self-contained demo on a generated scene
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply      # + TSDF fusion of every target, point cloud
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --color --render-fused
        # + colour: every target's 0..255 RGB frame is fused beside its depth; scene.ply gets red / green / blue and --render-fused also
        # writes <out>/fused_rgb/<stem>.png
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --mesh /tmp/eval/scene_mesh.ply
        # + the fused surface as a triangle mesh (TSDFVolume.save_mesh: surface nets; red / green / blue with --color) and a "mesh" block in
        # metrics.json: vertices, faces and the mesh edges shared by one / two / more than two triangles
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --mesh /tmp/eval/scene_mesh.ply --mesh-min-component 100
        # + the mesh without its floaters: connected components of fewer than 100 triangles and the vertices no face uses are dropped
        # (fusion3d.filter_mesh over the GPU union-find of csrc/mesh/mesh_components.hip) before the file is written and the edges are
        # counted; the "mesh" block gains components, components_kept, vertices_dropped and faces_dropped
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --mesh /tmp/eval/scene_mesh.ply --mesh-simplify 0.08
        # + the mesh simplified: every vertex in one 8 cm cell of a grid anchored at the volume's origin becomes one vertex, placed where the
        # plane quadrics of the cell's triangles are smallest (fusion3d.simplify_mesh on csrc/mesh/mesh_simplify.hip), after
        # --mesh-min-component; the file, the edge counts and the --score-sample scores are the simplified mesh's, and the "mesh" block gains
        # simplify: cell, vertices_in, faces_in, vertices, faces, collapsed, duplicates, invalid, placed, fallback, euler
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --render-fused
        # + the fused volume ray-cast at every target's pose (TSDFVolume.render): <out>/fused_depth/*.npy beside refined_depth/ (float16,
        # same layout) and the fused depth scored against the same ground truth (errors_fused, fused_coverage, errors_on_covered)
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --geo-filter 2
        # + the cross-view consistency filter (estdepth_amd.consistency): every target's depth is checked against the 2 targets before and
        # after it; what is fused is the averaged depth on the pixels at least --geo-min-views neighbours agree on (fusion runs 2 targets
        # behind the stream); metrics.json gains consistency, errors_filtered and filtered_coverage
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --score-3d
        # + the 3D scores of the fused scene (estdepth_amd.cloud_metrics): the ground-truth depth maps of the same targets are fused into a
        # second volume of the same geometry and the two surfaces compared -- accuracy, completeness, chamfer, precision / recall / F-score;
        # --score-3d GT.ply compares against that cloud instead; metrics.json gains recon_3d
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --score-3d GT.ply --score-sample 2500
        # + surfaces instead of vertices: GT.ply is read with its faces and, like the fused side's own triangle mesh (after
        # --mesh-min-component when given), sampled by area at 2500 points per square metre (fusion3d.sample_mesh on
        # csrc/mesh/mesh_sample.hip) before the two are compared; recon_3d gains sampled: density, n_pred, n_gt, area_pred, area_gt,
        # invalid_pred, invalid_gt.  A GT.ply without faces is scored as the cloud it is (area_gt: null)
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --score-3d GT.ply --score-sample 2500 --score-visible
        # + only the ground truth the cameras saw: GT.ply's mesh is rendered at the pose, intrinsics and size of every fused target
        # (estdepth_amd.mesh_render on csrc/mesh/mesh_raster.hip) and its samples that no target (--score-visible N: fewer than N targets)
        # saw within --depth-max are dropped before the comparison; recon_3d.sampled gains n_gt_visible and visible_share
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --score-3d GT.ply --render-gt-mesh
        # + ground-truth depth from the mesh: the same renders go to <out>/gt_mesh_depth/<stem>.npy, and the predictions are scored against
        # them (errors_vs_gt_mesh, gt_mesh_coverage, errors_on_gt_mesh_covered): the 2D protocol of scenes that ship a mesh and no depth
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --score-3d SCAN.ply --score-align plane --score-normals
        # + a ground truth that comes WITHOUT normals (a laser scan, a PLY with x y z only): normals are estimated from its own points --
        # a plane fit over the 16 nearest neighbours within the threshold (cloud_metrics.estimate_normals, csrc/cloud/cloud_knn.hip) -- so
        # that normal_consistency and the plane metric are there; recon_3d gains normals: k, radius, estimated, invalid_pred, invalid_gt
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --score-3d --cloud-min-cluster 200
        # + the fused cloud without its floaters: the points are clustered by density (cloud_metrics.filter_clusters: DBSCAN with
        # --cloud-cluster-eps, default two voxel edges, and --cloud-cluster-min-points, default 6); the noise and every cluster of fewer than
        # 200 points are dropped before scene.ply is written and scored; a "cloud_clusters" block in metrics.json
    python tools/run_stream.py --synthetic 8 --out /tmp/eval --fuse /tmp/eval/scene.ply --track
        # + frame-to-model tracking (estdepth_amd.tracking): from the second fused target on, every target's pose is refined against the
        # volume (TSDFVolume.track: point-to-plane alignment of its depth map with the ray-cast model) before the target is fused -- the
        # filtered record too under --geo-filter; metrics.json gains tracking: per frame the correction, the rmse before and after, the
        # matched share and whether the refinement converged
    python tools/run_stream.py --scene-dir SCENE --frame-interval 1 --out /tmp/eval --depth-source gt --fuse /tmp/eval/scene.ply
        # the chain WITHOUT the network: no model is built; a stand-in with ESTMStream.push's contract (GroundTruthStream) hands every
        # target's ground-truth depth, brought to --image-size by nearest neighbour on pixel centres, with confidence 1 where it is valid,
        # to everything behind the stream.  For checking a scene's poses and intrinsics and the reconstruction chain (fusion, filter,
        # tracking, rendering, 3D scores) on their own: with true depths every error left is the scene's or the chain's, not the model's

parse(argv) and run(args) -> (report, state) drive the tool from a program (tests/test_gpu_run_stream.py); main() is parse + run + metrics.json.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def nearest_index(n_out, n_in):
    """nearest neighbour on pixel centres: the index in a row of ``n_in`` samples under each of ``n_out`` (the identity at n_out == n_in)"""
    return np.minimum(((np.arange(n_out) + 0.5) * n_in / n_out).astype(np.int64), n_in - 1)


def to_gt_grid(a, shape):
    """nearest neighbour on pixel centres: a map at the network's resolution on the ground truth's pixel grid (no new depth values)"""
    return a[nearest_index(shape[0], a.shape[0])][:, nearest_index(shape[1], a.shape[1])]


class GroundTruthStream:
    """--depth-source gt: ESTMStream.push's contract without a network.  None until ``lwindow`` frames are in, then per push the output
    dict of one target -- the window's frame ``lwindow // 2`` -- whose depths are that frame's ground-truth map on the ``image_hw`` grid
    (nearest neighbour on pixel centres, the identity at the native size) and whose confidences are 1 where that depth is valid, else 0.
    Works on whatever device the maps are on."""

    def __init__(self, lwindow=3, image_hw=None):
        if lwindow < 3:
            raise RuntimeError("a window needs at least 3 frames (model_hybrid.py:123)")
        self.lwindow, self.image_hw = lwindow, image_hw
        self._dmaps, self.windows = [], 0

    def push(self, img, cam_pose, cam_intr, dmap=None, dmask=None):
        if dmap is None:
            raise RuntimeError("GroundTruthStream.push: every frame needs its ground-truth depth map")
        self._dmaps = (self._dmaps + [dmap.reshape(dmap.shape[-2:])])[-self.lwindow:]
        if len(self._dmaps) < self.lwindow:
            return None
        gt = self._dmaps[self.lwindow // 2]
        h, w = self.image_hw if self.image_hw is not None else tuple(img.shape[-2:])
        ys = torch.from_numpy(nearest_index(h, gt.shape[0])).to(gt.device)
        xs = torch.from_numpy(nearest_index(w, gt.shape[1])).to(gt.device)
        depth = gt[ys][:, xs].to(torch.float32)
        depth = torch.where(torch.isfinite(depth) & (depth > 0), depth, torch.zeros_like(depth))[None, None].contiguous()
        conf = (depth > 0).to(torch.float32)
        self.windows += 1
        outputs = {("depth", 0, 0): depth, ("depth", 0, 2): depth.clone(), ("fused_prob", 0): conf, ("init_prob", 0): conf.clone()}
        return outputs, None, None


def ply_face_count(path):
    """the number of faces a PLY header announces (0 without a face element)"""
    with open(path, "rb") as f:
        for _ in range(200):
            line = f.readline().strip()
            if line.startswith(b"element face"):
                return int(line.split()[2])
            if not line or line == b"end_header":
                break
    return 0


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene-dir")
    ap.add_argument("--synthetic", type=int, default=0, help="generate a scene of this many frames instead")
    ap.add_argument("--out", required=True)
    ap.add_argument("--loadckpt")
    ap.add_argument("--resnet", type=int, default=50)
    ap.add_argument("--ndepths", type=int, default=64)
    ap.add_argument("--depth_min", type=float, default=0.1)
    ap.add_argument("--depth_max", type=float, default=10.0)
    ap.add_argument("--image-size", type=int, nargs=2, default=(320, 256), metavar=("W", "H"))
    ap.add_argument("--frame-interval", type=int, default=10)
    ap.add_argument("--lwindow", type=int, default=3)
    ap.add_argument("--memory_size", type=int, default=2)
    ap.add_argument("--layout", choices=("scannet", "7scenes"), default="scannet")
    ap.add_argument("--no-feature-cache", action="store_true")
    ap.add_argument("--fuse", metavar="PATH.ply", help="fuse every target's depth / fused_prob into a TSDF volume on the device "
                                                       "(estdepth_amd.fusion3d) and write its surface points here")
    ap.add_argument("--cloud-min-cluster", type=int, metavar="N", help="with --fuse: cluster the fused points by density (DBSCAN; "
                    "cloud_metrics.filter_clusters) and drop the noise and every cluster of fewer than N points before the cloud is written and "
                    "scored; metrics.json gains a cloud_clusters block")
    ap.add_argument("--cloud-cluster-eps", type=float, default=None, metavar="E", help="with --cloud-min-cluster: the neighbourhood radius in metres "
                    "(default: two voxel edges, which links the 26-neighbourhood of the extraction's one-point-per-voxel cloud; a default, not a tuned value)")
    ap.add_argument("--cloud-cluster-min-points", type=int, default=None, metavar="K", help="with --cloud-min-cluster: a point with K neighbours within E "
                    "(itself among them) is a core point (default: 6 of the roughly 12 a surface holds in that radius; a default, not a tuned value)")
    ap.add_argument("--mesh", metavar="MESH.ply", help="with --fuse: also write the fused surface as a triangle mesh (TSDFVolume.save_mesh; "
                    "with --color the vertices get red / green / blue) and report its size and edge statistics")
    ap.add_argument("--mesh-min-component", type=int, metavar="N", help="with --mesh: drop the connected components of fewer than N triangles "
                    "and the vertices no face uses (fusion3d.filter_mesh) before the mesh is written and its edges are counted")
    ap.add_argument("--mesh-simplify", type=float, metavar="CELL", help="with --mesh: simplify the mesh by vertex clustering with quadric placement "
                    "on a grid of CELL metres anchored at the volume's origin (fusion3d.simplify_mesh, after --mesh-min-component); the mesh that "
                    "is written, counted and scored with --score-sample is the simplified one, and the mesh block gains a simplify block")
    ap.add_argument("--render-fused", action="store_true", help="with --fuse: after the stream, render the volume at every target's pose, "
                    "write the fused depth maps to <out>/fused_depth and score them against the ground truth")
    ap.add_argument("--color", action="store_true", help="with --fuse: fuse every target's frame (the reader's 0..255 RGB, whatever the model is "
                    "fed) beside its depth; the PLY gets red / green / blue and --render-fused also writes <out>/fused_rgb/<stem>.png")
    ap.add_argument("--geo-filter", type=int, default=0, metavar="R", help="check every target's depth against the R targets before and after it "
                    "(estdepth_amd.consistency.ConsistencyWindow); with --fuse the filtered depth is what is fused, R targets behind the stream")
    ap.add_argument("--geo-px", type=float, default=1.0, help="with --geo-filter: largest reprojection error in pixels")
    ap.add_argument("--geo-rel", type=float, default=0.01, help="with --geo-filter: largest relative depth difference")
    ap.add_argument("--geo-min-views", type=int, default=2, help="with --geo-filter: a pixel is kept where at least this many neighbours agree")
    ap.add_argument("--score-3d", nargs="?", const=True, default=None, metavar="GT.ply", help="with --fuse: score the fused surface in 3D "
                    "(estdepth_amd.cloud_metrics.compare_clouds) against this ground-truth cloud, or without a path against the reader's "
                    "ground-truth depth maps of the same targets fused into a second volume of the same geometry (no confidence gating)")
    ap.add_argument("--score-threshold", type=float, default=0.05, help="with --score-3d: the precision / recall / F-score threshold in metres")
    ap.add_argument("--score-max-dist", type=float, default=None, help="with --score-3d: distances are clamped here (default: 20 thresholds)")
    ap.add_argument("--score-sample", type=float, default=None, metavar="DENSITY", help="with --score-3d: score surfaces instead of vertices -- the "
                    "fused side is its triangle mesh (after --mesh-min-component when given), a GT.ply with faces is read as a mesh, and both are "
                    "sampled by area at DENSITY points per square metre (fusion3d.sample_mesh); recon_3d gains a sampled block")
    ap.add_argument("--score-visible", type=int, nargs="?", const=1, default=None, metavar="MIN_VIEWS", help="with --score-3d GT.ply (a mesh) and "
                    "--score-sample: render the ground-truth mesh at every fused target's pose, intrinsics and size and drop its samples that "
                    "fewer than MIN_VIEWS (default 1) targets saw within --depth_max (mesh_render.visible_mask); recon_3d.sampled gains "
                    "n_gt_visible and visible_share")
    ap.add_argument("--score-exact", action="store_true", help="with --score-3d GT.ply (a mesh) and --score-sample: every distance is the distance "
                    "to the other SURFACE (cloud_metrics.compare_meshes(exact=True) on csrc/mesh/mesh_distance.hip), not to its nearest sample; "
                    "recon_3d gains an exact block: faces_pred, faces_gt, invalid_pred, invalid_gt")
    ap.add_argument("--score-align", nargs="?", const="plane", default=None, choices=("plane", "point"), metavar="plane|point", help="with "
                    "--score-3d GT.ply: register the fused surface to the ground truth first (estdepth_amd.registration: ICP with the "
                    "point-to-plane or point-to-point metric; against the ground truth's surface where the file has faces and --score-sample is "
                    "given) and score the moved surface -- for a ground truth in another frame of reference; recon_3d gains an alignment "
                    "block: T, correction, rmse, overlap, iterations, converged, reason.  A registration that does not converge is reported and "
                    "the unmoved surface is scored")
    ap.add_argument("--score-align-dist", type=float, nargs="+", default=None, metavar="D", help="with --score-align: partners farther than D "
                    "metres are left out; several decreasing values run as stages (default: 8, 4 and 2 score thresholds)")
    ap.add_argument("--score-align-iters", type=int, default=30, metavar="N", help="with --score-align: Gauss-Newton iterations per stage at most")
    ap.add_argument("--score-align-global", type=float, nargs="?", const=-1.0, default=None, metavar="VOXEL", help="with --score-align: start the "
                    "registration from a GLOBAL one (estdepth_amd.registration.register_global: FPFH descriptors, mutual matches and three-point "
                    "hypotheses on both sides thinned to VOXEL metres, default 1.5 score thresholds) -- for a ground truth metres and tens of "
                    "degrees away, where ICP alone refuses or lands on a wrong pose; the alignment block gains global: fitness, count, pairs, "
                    "hypothesis, T_global")
    ap.add_argument("--score-normals", type=int, nargs="?", const=16, default=None, metavar="K", help="with --score-3d GT.ply: a ground truth "
                    "without normals (a laser scan, a PLY without nx ny nz) gets them estimated from its own points -- a plane fit over the K "
                    "(default 16) nearest neighbours (cloud_metrics.estimate_normals; csrc/cloud/cloud_knn.hip) -- so that normal_consistency "
                    "and the plane metric of --score-align are there; recon_3d gains a normals block")
    ap.add_argument("--score-normals-radius", type=float, default=None, metavar="R", help="with --score-normals: neighbours within R metres "
                    "(default: --score-threshold)")
    ap.add_argument("--render-gt-mesh", action="store_true", help="with --score-3d GT.ply (a mesh): write its depth at every fused target's pose "
                    "to <out>/gt_mesh_depth and score the predictions against it: errors_vs_gt_mesh, gt_mesh_coverage, errors_on_gt_mesh_covered")
    ap.add_argument("--score-downsample", type=float, default=None, help="with --score-3d: voxel-grid down-sampling of both clouds first (metres)")
    ap.add_argument("--track", action="store_true", help="with --fuse: refine every target's pose against the fused volume before the target is "
                    "fused (TSDFVolume.track), from the second fused target on")
    ap.add_argument("--track-dist", type=float, default=None, metavar="D", help="with --track: matches farther than D metres from the model are "
                    "left out (default: the volume's truncation distance)")
    ap.add_argument("--track-iters", type=int, default=10, metavar="N", help="with --track: Gauss-Newton iterations per target at most")
    ap.add_argument("--voxel-size", type=float, default=0.04)
    ap.add_argument("--volume-dims", type=int, nargs=3, default=(256, 256, 256), metavar=("Z", "Y", "X"))
    ap.add_argument("--depth-source", choices=("net", "gt"), default="net", help="gt: no network is built; every target's depth is its own "
                    "ground-truth map at --image-size (nearest neighbour) with confidence 1 where valid -- checks a scene's poses and "
                    "intrinsics and the reconstruction chain without the model")
    args = ap.parse_args(argv)
    if args.render_fused and not args.fuse:
        ap.error("--render-fused needs --fuse PATH.ply")
    if args.mesh and not args.fuse:
        ap.error("--mesh needs --fuse PATH.ply")
    if args.cloud_min_cluster is not None and not args.fuse:
        ap.error("--cloud-min-cluster needs --fuse PATH.ply")
    if args.cloud_min_cluster is not None and args.cloud_min_cluster < 1:
        ap.error("--cloud-min-cluster must be at least 1")
    if args.cloud_min_cluster is None and (args.cloud_cluster_eps is not None or args.cloud_cluster_min_points is not None):
        ap.error("--cloud-cluster-eps and --cloud-cluster-min-points need --cloud-min-cluster N")
    if args.cloud_cluster_eps is not None and not 0 < args.cloud_cluster_eps < float("inf"):
        ap.error("--cloud-cluster-eps must be a positive radius in metres")
    if args.cloud_cluster_min_points is not None and args.cloud_cluster_min_points < 1:
        ap.error("--cloud-cluster-min-points must be at least 1")
    if args.cloud_min_cluster is not None and args.score_exact:
        ap.error("--cloud-min-cluster is not available with --score-exact (the surfaces themselves are scored there: --mesh-min-component cleans a mesh)")
    if args.mesh_min_component is not None and not args.mesh:
        ap.error("--mesh-min-component needs --mesh MESH.ply")
    if args.mesh_min_component is not None and args.mesh_min_component < 1:
        ap.error("--mesh-min-component must be at least 1")
    if args.mesh_simplify is not None and not args.mesh:
        ap.error("--mesh-simplify needs --mesh MESH.ply")
    if args.mesh_simplify is not None and not (args.mesh_simplify > 0 and args.mesh_simplify < float("inf")):
        ap.error("--mesh-simplify must be a positive cell edge in metres")
    if args.color and not args.fuse:
        ap.error("--color needs --fuse PATH.ply")
    if args.score_3d is not None and not args.fuse:
        ap.error("--score-3d needs --fuse PATH.ply")
    if args.score_sample is not None and args.score_3d is None:
        ap.error("--score-sample needs --score-3d")
    if args.score_sample is not None and not (args.score_sample > 0 and args.score_sample < float("inf")):
        ap.error("--score-sample must be a positive density in points per square metre")
    for flag, on in (("--score-visible", args.score_visible is not None), ("--render-gt-mesh", args.render_gt_mesh)):
        if on and not isinstance(args.score_3d, str):
            ap.error("%s needs --score-3d GT.ply (a triangle mesh to render)" % flag)
        if on and os.path.exists(args.score_3d) and ply_face_count(args.score_3d) == 0:
            ap.error("%s needs a GT.ply with faces: %s has none, and a point cloud cannot be rendered" % (flag, args.score_3d))
    if args.score_exact:
        if not isinstance(args.score_3d, str) or args.score_sample is None:
            ap.error("--score-exact needs --score-3d GT.ply (a triangle mesh) and --score-sample DENSITY")
        if os.path.exists(args.score_3d) and ply_face_count(args.score_3d) == 0:
            ap.error("--score-exact needs a GT.ply with faces: %s has none, and the distance to a point cloud is the sampled one" % args.score_3d)
    if args.score_align is not None and not isinstance(args.score_3d, str):
        ap.error("--score-align needs --score-3d GT.ply (a ground-truth file: the reader's own depth maps share the frame of the poses)")
    if args.score_align is None and (args.score_align_dist is not None or args.score_align_iters != 30):
        ap.error("--score-align-dist and --score-align-iters need --score-align")
    if args.score_align_dist is not None and not (all(0 < d < float("inf") for d in args.score_align_dist)
                                                  and all(a > b for a, b in zip(args.score_align_dist, args.score_align_dist[1:]))):
        ap.error("--score-align-dist takes positive distances in decreasing order")
    if args.score_align_iters < 0:
        ap.error("--score-align-iters must not be negative")
    if args.score_align_global is not None and args.score_align is None:
        ap.error("--score-align-global needs --score-align")
    if args.score_align_global is not None and args.score_align_global != -1.0 and not 0 < args.score_align_global < float("inf"):
        ap.error("--score-align-global takes a positive voxel edge in metres")
    if args.score_normals is not None and not isinstance(args.score_3d, str):
        ap.error("--score-normals needs --score-3d GT.ply (a ground-truth file: the reader's own depth maps give a volume with normals)")
    if args.score_normals is None and args.score_normals_radius is not None:
        ap.error("--score-normals-radius needs --score-normals")
    if args.score_normals is not None and not 3 <= args.score_normals <= 32:
        ap.error("--score-normals takes 3 to 32 neighbours")
    if args.score_normals is not None and args.score_exact:
        ap.error("--score-normals is not available with --score-exact")
    if args.score_normals_radius is not None and not 0 < args.score_normals_radius < float("inf"):
        ap.error("--score-normals-radius must be positive and finite")
    if args.score_visible is not None and args.score_sample is None:
        ap.error("--score-visible needs --score-sample DENSITY (the samples of the ground-truth surface are what is restricted)")
    if args.score_visible is not None and args.score_visible < 1:
        ap.error("--score-visible must be at least 1")
    if args.track and not args.fuse:
        ap.error("--track needs --fuse PATH.ply")
    if not args.scene_dir and not args.synthetic:
        ap.error("--scene-dir or --synthetic is required")
    return args


def run(args):
    """the whole evaluation -> (report, state): what main() writes to metrics.json, and the live objects behind it -- state.volume,
    state.volume_gt, state.geo (None without their flags), state.fused = [(frame name, the float64 pose the target was fused at)] in
    fusion order, state.targets (--render-fused: name, pose, intrinsics, size, prediction and ground truth of every target)"""
    from estdepth_amd import DepthNetHybrid, synth
    from estdepth_amd.streaming import ESTMStream
    from estdepth_amd.eval_io import SequenceReader, save_window_outputs, write_synthetic_scene
    from estdepth_amd.metrics import RunningErrors

    scene_dir, interval = args.scene_dir, args.frame_interval
    if args.synthetic:
        w, h = args.image_size
        _, poses, _, sample = synth.make_sequence(args.synthetic, h, w, seed=7)
        frames = synth.smooth_images(args.synthetic, h, w, seed=7)
        scene_dir = tempfile.mkdtemp(prefix="estd_scene_")
        imgs = [frames[0, i].permute(1, 2, 0).round().clamp(0, 255).byte().numpy() for i in range(args.synthetic)]
        dmaps = [sample["dmaps"][0, i, 0].numpy() for i in range(args.synthetic)]
        write_synthetic_scene(scene_dir, imgs, dmaps, [poses[0, i].numpy() for i in range(args.synthetic)])
        interval = 1

    dev = torch.device("cuda:0")
    if args.depth_source == "net":
        model = DepthNetHybrid(ndepths=args.ndepths, depth_min=args.depth_min, depth_max=args.depth_max,
                               resnet=args.resnet, IF_EST_transformer=True)
        if args.loadckpt:
            sd = torch.load(args.loadckpt, map_location="cpu")
            model.load_state_dict(sd.get("model", sd))
        else:
            synth.fill_state_dict(model, seed=2, head_gain=1.0)
        model = model.to(dev).eval()
        model.use_channels_last_2d()
        model.use_hip_psm()

    reader = SequenceReader(scene_dir, image_size=tuple(args.image_size), depth_min=args.depth_min,
                            depth_max=args.depth_max, frame_interval=interval,
                            scannet_layout=args.layout == "scannet")
    if args.depth_source == "net":
        stream = ESTMStream(model, lwindow=args.lwindow, memory_size=args.memory_size,
                            cache_features=not args.no_feature_cache)
    else:
        stream = GroundTruthStream(lwindow=args.lwindow, image_hw=(args.image_size[1], args.image_size[0]))
    errs, times, window, resized = RunningErrors(), [], [], 0
    volume, fuse_ms, targets = None, [], []
    volume_gt = None                                                         # --score-3d without a path: the ground-truth depth maps, fused
    geo, errs_filtered, geo_count = None, RunningErrors(), {"gt": 0, "kept": 0}
    if args.geo_filter:
        from estdepth_amd.consistency import ConsistencyWindow
        from estdepth_amd.metrics import compute_valid_depth_mask as valid_depth
        geo = ConsistencyWindow(radius=args.geo_filter, min_views=args.geo_min_views, px_max=args.geo_px, rel_max=args.geo_rel)

    tracked, track_ms, fused_at = [], [], []
    seen_by = {}                     # --score-visible / --render-gt-mesh: frame name -> (intrinsics, image size, prediction, ground truth)

    def refined_pose(name, dmap, pose, intr):
        """--track: the pose to fuse a target at -- its own until something is fused, then the one TSDFVolume.track finds against the volume"""
        pose = pose.detach().reshape(4, 4).to("cpu", torch.float64)
        if volume.frames == 0:
            return pose
        torch.cuda.synchronize()
        t0 = time.time()
        out = volume.track(dmap, pose, intr, dist_max=args.track_dist, max_iter=args.track_iters)
        after = volume.check_frame(dmap, out["pose"], intr, dist_max=args.track_dist)
        torch.cuda.synchronize()
        track_ms.append(1e3 * (time.time() - t0))
        tracked.append({"frame": os.path.basename(str(name)), "correction_m": out["correction"][0], "correction_rad": out["correction"][1],
                        "rmse_before": out["trace"][0]["rmse"], "rmse_after": after["rmse"], "matched_share": out["matched_share"],
                        "converged": out["converged"], "reason": out["reason"], "iterations": out["iterations"]})
        return out["pose"]

    def take_filtered(rec):
        """a target the consistency window hands back: fuse it (--fuse) and score its averaged depth on the kept pixels"""
        if volume is not None and args.track:                                # the filtered record is refined on the pixels that will be fused
            kept_dev = torch.where(rec["views"] >= float(args.geo_min_views), rec["depth"], torch.zeros_like(rec["depth"]))
            rec = dict(rec, pose=refined_pose(rec["extra"]["name"], kept_dev, rec["pose"], rec["K"]))
        if volume is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            volume.integrate_filtered(dict(rec, extra=rec["extra"]["rgb"]))
            fused_at.append((rec["extra"]["name"], rec["pose"].detach().reshape(4, 4).to("cpu", torch.float64).clone()))
            e1.record()
            torch.cuda.synchronize()
            fuse_ms.append(e0.elapsed_time(e1))
        kept = torch.where(rec["views"] >= float(args.geo_min_views), rec["depth"], torch.zeros_like(rec["depth"])).cpu().numpy().astype(np.float64)
        gt = rec["extra"]["gt"]
        if gt.shape != kept.shape:
            kept = to_gt_grid(kept, gt.shape)
        errs_filtered.add(kept, gt)
        gt_ok = valid_depth(gt)
        geo_count["gt"] += int(gt_ok.sum())
        geo_count["kept"] += int((gt_ok & (kept > 0)).sum())

    for idx in range(len(reader)):
        s = reader[idx]
        window.append(s)
        window = window[-args.lwindow:]
        torch.cuda.synchronize()
        t0 = time.time()
        res = stream.push(s["img"].to(dev), s["cam_pose"].to(dev), s["cam_intr"].to(dev),
                          s["dmap"].to(dev), s["dmask"].to(dev))
        torch.cuda.synchronize()
        if res is None:
            continue
        times.append(time.time() - t0)
        outputs = res[0]
        target = window[args.lwindow // 2]                                   # eval_hybrid_seq.py:197
        if args.fuse:
            from estdepth_amd.fusion3d import TSDFVolume, frustum_volume
            if volume is None:      # centred on the first camera's frustum between depth_min and depth_max
                h, w = s["img"].shape[-2:]
                origin = frustum_volume(window[0]["cam_pose"], s["cam_intr"], (h, w), args.depth_min, args.depth_max,
                                        args.volume_dims, args.voxel_size)
                volume = TSDFVolume(args.volume_dims, args.voxel_size, origin, device=dev, color=args.color)
                if args.score_3d is True:
                    volume_gt = TSDFVolume(args.volume_dims, args.voxel_size, origin, device=dev)
            if volume_gt is not None:                                        # the target's ground truth on its own grid, intrinsics scaled to it
                gt_map, image_hw = target["dmap"][0, 0].to(dev), tuple(s["img"].shape[-2:])
                intr_gt = s["cam_intr"].reshape(3, 3).clone()
                if tuple(gt_map.shape) != image_hw:
                    intr_gt[0] = intr_gt[0] * (gt_map.shape[1] / float(image_hw[1]))
                    intr_gt[1] = intr_gt[1] * (gt_map.shape[0] / float(image_hw[0]))
                volume_gt.integrate(gt_map[None], target["cam_pose"].reshape(1, 4, 4), intr_gt)
        if args.fuse and geo is None:
            frames_rgb = torch.stack([f["img"][0] for f in window])[None].to(dev) if args.color else None
            window_poses = torch.stack([f["cam_pose"].reshape(4, 4) for f in window])[None]
            if args.track:
                dmap, intr, image_hw = outputs[("depth", 0, 0)][0, 0], s["cam_intr"].reshape(3, 3).clone(), tuple(s["img"].shape[-2:])
                if tuple(dmap.shape) != image_hw:                            # as TSDFVolume.integrate_outputs: the intrinsics of the maps' size
                    intr[0:2] = intr[0:2] * (dmap.shape[0] / float(image_hw[0]))
                window_poses = window_poses.detach().to("cpu", torch.float64).clone()
                window_poses[0, args.lwindow // 2] = refined_pose(target["img_path"], dmap, target["cam_pose"], intr)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            volume.integrate_outputs(outputs, window_poses, s["cam_intr"].reshape(1, 3, 3),
                                     image_hw=tuple(s["img"].shape[-2:]), imgs=frames_rgb)
            e1.record()
            torch.cuda.synchronize()
            fuse_ms.append(e0.elapsed_time(e1))
            fused_at.append((target["img_path"], window_poses[0, args.lwindow // 2].detach().to("cpu", torch.float64).clone()))
        save_window_outputs(outputs, args.out, target["img_path"])
        pred = outputs[("depth", 0, 0)][0, 0].cpu().numpy().astype(np.float64)
        gt = target["dmap"][0, 0].numpy().astype(np.float64)
        if gt.shape != pred.shape:
            # the ground-truth depth stays at native resolution (general_eval_seq.py:191) while the network runs at
            # --image-size: bring the PREDICTION to the ground-truth grid (nearest neighbour on pixel centres, no new
            # depth values are invented) instead of silently skipping the frame
            pred = to_gt_grid(pred, gt.shape)
            resized += 1
        errs.add(pred, gt)
        if geo is not None:
            dmap = outputs[("depth", 0, 0)][0, 0]
            intr, image_hw = s["cam_intr"].reshape(3, 3).clone(), tuple(s["img"].shape[-2:])
            if tuple(dmap.shape) != image_hw:                                # as TSDFVolume.integrate_outputs: the intrinsics of the maps' size
                intr[0:2] = intr[0:2] * (dmap.shape[0] / float(image_hw[0]))
            rgb = target["img"][0].to(dev) if args.color else None           # the colour frame travels with its depth
            rec = geo.push(dmap, target["cam_pose"].reshape(4, 4), intr, extra={"rgb": rgb, "gt": gt, "name": target["img_path"]})
            if rec is not None:
                take_filtered(rec)
        if args.score_visible is not None or args.render_gt_mesh:
            seen_by[target["img_path"]] = (s["cam_intr"].reshape(3, 3).clone(), tuple(s["img"].shape[-2:]), pred, gt)
        if args.render_fused:
            targets.append((target["img_path"], target["cam_pose"].reshape(4, 4), s["cam_intr"].reshape(3, 3), tuple(s["img"].shape[-2:]), pred, gt))
    if geo is not None:
        for rec in geo.flush():
            take_filtered(rec)
    report = {"scene": scene_dir, "frames": len(reader), "windows": stream.windows,
              "mean_window_ms": 1e3 * float(np.mean(times[1:] or times or [0.0])), "errors": errs.mean(),
              "predictions_resized_to_gt_grid": resized}
    if geo is not None:
        report.update(consistency=geo.summary(), errors_filtered=errs_filtered.mean(), filtered_coverage=geo_count["kept"] / max(geo_count["gt"], 1))
    clusters = None
    if volume is not None and args.cloud_min_cluster is not None:                # the floaters leave before the cloud is written and scored
        clusters = dict(eps=args.cloud_cluster_eps if args.cloud_cluster_eps is not None else 2.0 * args.voxel_size,
                        min_points=args.cloud_cluster_min_points if args.cloud_cluster_min_points is not None else 6, min_size=args.cloud_min_cluster)
    if volume is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.fuse)), exist_ok=True)
        found = {}
        report.update(fused_voxels=volume.fused_voxels(), points=volume.save_ply(args.fuse, clusters=clusters, stats=found),
                      mean_fuse_ms=float(np.mean(fuse_ms[1:] or fuse_ms)))
        if clusters is not None:
            report["cloud_clusters"] = dict(found, eps=clusters["eps"], min_points=clusters["min_points"], min_size=clusters["min_size"])
    if volume is not None and args.mesh:
        from estdepth_amd.fusion3d import mesh_edge_stats
        os.makedirs(os.path.dirname(os.path.abspath(args.mesh)), exist_ok=True)
        n_vertices, n_faces = volume.save_mesh(args.mesh, min_component=args.mesh_min_component or 0, simplify=args.mesh_simplify)
        mesh = volume.extract_mesh(min_component=args.mesh_min_component or 0, simplify=args.mesh_simplify)
        stats = mesh_edge_stats(mesh["faces"])
        report["mesh"] = {"path": args.mesh, "vertices": n_vertices, "faces": n_faces, "boundary_edges": stats["boundary"],
                          "manifold_edges": stats["manifold"], "non_manifold_edges": stats["non_manifold"]}
        if args.mesh_min_component is not None:       # the file and the edge statistics above are the filtered mesh's
            report["mesh"].update(components=mesh["components"] + mesh["dropped"]["components"], components_kept=mesh["components"],
                                  vertices_dropped=mesh["dropped"]["vertices"], faces_dropped=mesh["dropped"]["faces"])
        if args.mesh_simplify is not None:            # the file, the edge statistics and the 3D scores are the simplified mesh's
            report["mesh"].update(simplify=dict(mesh["stats"], cell=args.mesh_simplify, euler=stats["euler"]))
    if args.track and volume is not None:
        report["tracking"] = {"frames": tracked, "dist_max": args.track_dist if args.track_dist is not None else volume.trunc,
                              "max_iter": args.track_iters, "mean_track_ms": float(np.mean(track_ms[1:] or track_ms or [0.0]))}
    if volume is not None and args.score_3d is not None:
        from estdepth_amd.fusion3d import read_ply
        if volume_gt is not None:
            other, gt_name = volume_gt, "ground-truth depth maps fused into a volume of the same geometry"
        else:
            ply = read_ply(args.score_3d)
            other, gt_name = {"xyz": ply["xyz"], "normal": ply["normal"]}, args.score_3d
            if args.color and ply["rgb"] is not None:                        # the volume keeps the reader's 0..255 RGB
                other["color"] = ply["rgb"].astype(np.float32)
        max_dist = args.score_max_dist if args.score_max_dist is not None else 20.0 * args.score_threshold
        align = {}
        if args.score_align is not None:
            align = dict(align=dict(metric=args.score_align, max_iter=args.score_align_iters,
                                    dist_max=tuple(args.score_align_dist) if args.score_align_dist is not None else None))
            if args.score_align_global is not None:
                align["align"].update(init="global", voxel=1.5 * args.score_threshold if args.score_align_global == -1.0 else args.score_align_global)
        if args.score_normals is not None:
            align["normals"] = dict(k=args.score_normals, radius=args.score_normals_radius)
        if clusters is not None:
            align["clusters"] = dict(clusters, sides=("pred",))
        torch.cuda.synchronize()
        t0 = time.time()
        if args.score_sample is None:
            scores = volume.compare(other, threshold=args.score_threshold, max_dist=max_dist, downsample=args.score_downsample, **align)
        else:
            # surfaces, not vertices: both sides as triangle meshes sampled by area at the same density (csrc/mesh/mesh_sample.hip); a
            # ground-truth file without faces stays the cloud it is
            from estdepth_amd.cloud_metrics import compare_meshes
            if volume_gt is not None:
                other = volume_gt.extract_mesh()
            else:
                faces = read_ply(args.score_3d, faces=True)["faces"]
                if faces.shape[0]:
                    other["faces"] = faces
            visible = None
            if args.score_visible is not None:                               # only the ground truth some fused target saw
                visible = dict(cam_poses=torch.stack([p for _, p in fused_at]), cam_intr=torch.stack([seen_by[n][0] for n, _ in fused_at]),
                               image_hw=seen_by[fused_at[0][0]][1], min_views=args.score_visible, depth_max=args.depth_max)
            scores = compare_meshes(volume.extract_mesh(min_component=args.mesh_min_component or 0, simplify=args.mesh_simplify), other, args.score_sample,
                                    threshold=args.score_threshold, max_dist=max_dist, downsample=args.score_downsample, visible=visible,
                                    **(dict(exact=True) if args.score_exact else {}), **align)
        torch.cuda.synchronize()
        report["recon_3d"] = dict(scores, threshold=args.score_threshold, max_dist=max_dist, downsample=args.score_downsample, ground_truth=gt_name,
                                  compare_ms=1e3 * (time.time() - t0))
    if volume is not None and args.render_gt_mesh:
        # the ground-truth mesh in every fused target's camera: depth maps for a scene that ships a mesh and no depth
        from estdepth_amd.fusion3d import read_ply
        from estdepth_amd.mesh_render import render_mesh
        from estdepth_amd.metrics import compute_valid_depth_mask
        gt_mesh = read_ply(args.score_3d, faces=True)
        gt_mesh = {"xyz": gt_mesh["xyz"], "faces": gt_mesh["faces"]}
        errs_mesh, errs_depth, n_px, n_hit = RunningErrors(), RunningErrors(), 0, 0
        out_dir = os.path.join(args.out, "gt_mesh_depth")
        os.makedirs(out_dir, exist_ok=True)
        for name, pose in fused_at:
            intr, hw, pred, gt = seen_by[name]
            depth = render_mesh(gt_mesh, pose, intr, hw, normals=None, color=False)["depth"].cpu().numpy()
            np.save(os.path.join(out_dir, os.path.splitext(os.path.basename(str(name)))[0] + ".npy"), depth[None])
            depth = to_gt_grid(depth.astype(np.float64), gt.shape)
            hit = compute_valid_depth_mask(depth)
            both = hit & compute_valid_depth_mask(gt) & compute_valid_depth_mask(pred)             # ONE pixel set for both scores
            n_px += depth.size
            n_hit += int((depth > 0).sum())
            errs_mesh.add(np.where(both, pred, 0.0), np.where(both, depth, 0.0))
            errs_depth.add(np.where(both, pred, 0.0), gt)
        report.update(errors_vs_gt_mesh=errs_mesh.mean(), gt_mesh_coverage=n_hit / max(n_px, 1), errors_on_gt_mesh_covered=errs_depth.mean())
    if volume is not None and args.render_fused:
        # the fused model in every target's camera, on the pixel grid and in the units of the per-frame predictions
        from estdepth_amd.metrics import compute_valid_depth_mask
        errs_fused, errs_covered, n_gt, n_covered, render_ms = RunningErrors(), RunningErrors(), 0, 0, []
        out_dir, rgb_dir = os.path.join(args.out, "fused_depth"), os.path.join(args.out, "fused_rgb")
        os.makedirs(out_dir, exist_ok=True)
        if args.color:
            from PIL import Image
            os.makedirs(rgb_dir, exist_ok=True)
        for img_path, pose, intr, hw, pred, gt in targets:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            maps = volume.render(pose, intr, hw, depth_min=args.depth_min, depth_max=args.depth_max)
            e1.record()
            torch.cuda.synchronize()
            render_ms.append(e0.elapsed_time(e1))
            fused = maps["depth"].cpu().numpy()
            if args.color:          # what the fused scene looks like from this pose, to hold beside the photograph; black where no surface is hit
                rgb = maps["color"].round().clamp(0, 255).byte().cpu().numpy()
                Image.fromarray(rgb).save(os.path.join(rgb_dir, os.path.splitext(os.path.basename(img_path))[0] + ".png"))
            np.save(os.path.join(out_dir, os.path.splitext(os.path.basename(img_path))[0] + ".npy"), np.float16(fused[None]))
            fused = to_gt_grid(fused.astype(np.float64), gt.shape)
            gt_ok = compute_valid_depth_mask(gt)
            both = gt_ok & compute_valid_depth_mask(fused) & compute_valid_depth_mask(pred)        # ONE pixel set for both scores
            n_gt += int(gt_ok.sum())
            n_covered += int((gt_ok & (fused > 0)).sum())
            errs_fused.add(np.where(both, fused, 0.0), gt)
            errs_covered.add(np.where(both, pred, 0.0), gt)
        report.update(errors_fused=errs_fused.mean(), fused_coverage=n_covered / max(n_gt, 1), errors_on_covered=errs_covered.mean(),
                      mean_render_ms=float(np.mean(render_ms[1:] or render_ms or [0.0])))
    return report, argparse.Namespace(volume=volume, volume_gt=volume_gt, geo=geo, fused=fused_at, targets=targets)


def main():
    args = parse()
    report, _ = run(args)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "metrics.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
