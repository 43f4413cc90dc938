"""Rigid registration of a point cloud to a point cloud or a triangle mesh on the device: ICP with a point-to-plane or a point-to-point
metric, the step evaluation protocols take before they score a reconstruction against a ground truth from another frame of reference.

    sys = rigid_system(src, T, target, metric="plane", dist_max=0.1)                  # A, b, count, rmse, residual, match, overlap
    out = register(src, target, dist_max=(0.4, 0.2, 0.1))                             # out["T"] moves src onto the target
    scores = compare_meshes(pred, gt, density, align=dict(metric="plane"))            # cloud_metrics: register first, score afterwards

One iteration is one apply (csrc/track/rigid_align.hip: moved = T p, normals rotated), one search with the existing structures
(``PointGrid.query``: the nearest target point; ``TriangleGrid.query(closest=True)``: the closest surface point and its face), one system
(the same source: 29 float64 sums in a fixed order, no atomics -- the contract is include/estd_hip.h, estd_rigid_system) and one read-back
of 29 doubles.  The 6 x 6 solve, the exponential map and the stopping rule are ``tracking.gauss_newton``'s, on the host in float64: the
update is on the LEFT, T <- Exp(xi) T with xi = (t, omega) in the target's axes.  There is no CPU path.

The kernel's Jacobian rows pivot on the world origin; ``register`` has every system solved about the PIVOT of its target, the centre of
the target's bounding box (``target_pivot``), so that its verdict does not depend on where the target lies in the world.  ``rigid_system``
keeps returning the sums, A and b about the world origin.

``src`` is [N,3] float32 on a ROCm device (``src_normal`` likewise); ``target`` is a ``PointGrid`` (with ``target_normal`` [Nt,3] for the
plane metric or a cosine gate), a ``TriangleGrid`` (its face normals are estd_mesh_face_area's, float64 rounded to fp32 once), or a dict:
with ``faces`` a mesh, else a cloud with ``xyz`` and optionally ``normal``; numpy arrays are moved to the device.  T is [4,4] float64.

From an arbitrary start, ``register_global`` goes first (csrc/register/global_register.hip): FPFH descriptors of both sides (``fpfh``),
mutual nearest matches in descriptor space (``match_features``), three-point hypotheses scored over the correspondences
(``ransac_pairs``), and ``register(init=)`` from the winner.

    out = register_global(src, target, voxel=0.05, refine=dict(metric="plane"))       # out["T"], out["T_global"], out["fitness"]

Out of scope: a scale (Sim(3)), robust kernels beyond the two gates, colour terms (in the metric or the descriptors), graph-based or
branch-and-bound global methods, hypotheses scored against the whole target instead of the correspondences, orientation propagation
for estimated normals.
"""
import math

import numpy as np
import torch

from . import ops, tracking
from .cloud_metrics import PointGrid, TriangleGrid, _check_cloud, _check_max_dist

_need = tracking._need
REFUSALS = ("count", "cholesky", "condition")


class _Target:
    """a target with its search structure, normals and the way ``estd_rigid_system`` reads it, prepared once per registration"""

    def __init__(self, target, max_dist, target_normal, op):
        from . import fusion3d
        if isinstance(target, dict):
            _need(target.get("xyz") is not None, "%s: a target dict needs 'xyz'" % op)
            if target.get("faces") is not None:
                target = TriangleGrid(target, max_dist)
            else:
                devs = [v.device for v in target.values() if isinstance(v, torch.Tensor) and v.is_cuda]
                dev = devs[0] if devs else torch.device("cuda")
                if target_normal is None and target.get("normal") is not None:
                    target_normal = fusion3d._on_device(target["normal"], dev)
                target = PointGrid(fusion3d._on_device(target["xyz"], dev), max_dist)
        _need(isinstance(target, (PointGrid, TriangleGrid)), "%s: target must be a PointGrid, a TriangleGrid or a dict (a cloud or a mesh), got %s"
              % (op, type(target).__name__))
        _need(target.max_dist >= max_dist, "%s: the target's grid finds partners within %g but dist_max is %g" % (op, target.max_dist, max_dist))
        self.grid, self.device, self.mesh = target, target.device, isinstance(target, TriangleGrid)
        self.pivot = 0.5 * (target.lo.double().numpy() + target.hi.double().numpy())          # host values of the grid: no read-back
        if self.mesh:
            _need(target_normal is None, "%s: a mesh target takes its normals from its faces; target_normal is for clouds" % op)
            self.normal = ops.mesh_face_area(target.xyz, target.faces)[1] if target.faces.shape[0] else torch.empty((0, 3), device=self.device)
        else:
            self.normal = None
            if target_normal is not None:
                self.normal = _check_cloud(target_normal, "target_normal", op, self.device)
                _need(self.normal.shape[0] == target.n, "%s: target_normal has %d rows but the target %d points" % (op, self.normal.shape[0], target.n))

    def search(self, moved):
        """-> (index int64 [N], target [.,3], by_index)"""
        if self.mesh:
            _, face, closest = self.grid.query(moved, closest=True)
            return face.long(), closest, False
        _, index = self.grid.query(moved)
        return index, self.grid.target, True


def _src(src, src_normal, op, dev):
    src = _check_cloud(src, "src", op, dev)
    if src_normal is not None:
        src_normal = _check_cloud(src_normal, "src_normal", op, dev)
        _need(src_normal.shape[0] == src.shape[0], "%s: src_normal has %d rows but src %d" % (op, src_normal.shape[0], src.shape[0]))
    return src, src_normal


def _matrix(T, op):
    T = tracking._host(T, (4, 4), "T", op)
    _need(bool((T[3] == np.array([0.0, 0.0, 0.0, 1.0])).all()), "%s: T must be a rigid transform [R t; 0 0 0 1], its last row is %r" % (op, T[3].tolist()))
    return T


def _t12(T):
    return torch.from_numpy(np.ascontiguousarray(T[:3, :4].astype(np.float32)))


def transform(points, T, normals=None):
    """``points`` [N,3] (and ``normals`` [N,3]) moved by the [4,4] ``T`` on the device (estd_rigid_apply) -> moved, or (moved, normals)"""
    T = _matrix(T, "transform")
    points, normals = _src(points, normals, "transform", None)
    moved, mn = ops.rigid_apply(points, normals, _t12(T))
    return moved if normals is None else (moved, mn)


def _system(src, src_normal, T, tgt, metric, dist_max, cos_min, two_sided):
    moved, mn = ops.rigid_apply(src, src_normal, _t12(T))
    index, target, by_index = tgt.search(moved)
    gate = src_normal is not None and cos_min is not None
    residual, match, sums = ops.rigid_system(moved, mn if gate else None, index, target, tgt.normal, by_index, metric, dist_max,
                                             cos_min if gate else None, two_sided)
    host = sums.cpu().numpy()
    A, b, rr, count = tracking.unpack_sums(host)
    n = int(src.shape[0])
    return dict(A=A, b=b, count=count, rmse=math.sqrt(rr / count) if count else 0.0, residual=residual, match=match, sums=host,
                overlap=count / n if n else 0.0)


def _args(metric, cos_min, tgt, src_normal, op):
    _need(metric in ops.RIGID_METRICS, "%s: metric must be 'plane' or 'point', got %r" % (op, metric))
    _need(cos_min is None or (isinstance(cos_min, (int, float)) and -1.0 <= cos_min <= 1.0), "%s: cos_min must be a cosine in -1 .. 1 or None, got %r" % (op, cos_min))
    _need(cos_min is None or src_normal is not None, "%s: cos_min compares normals: src_normal is missing" % op)
    _need(tgt.normal is not None or (metric == "point" and cos_min is None),
          "%s: the plane metric and the cosine gate need the target's normals (target_normal, or 'normal' in the dict)" % op)


def target_pivot(target, max_dist=0.1, target_normal=None):
    """The pivot ``register`` solves about -> float64 [3]: the centre of the bounding box of the target's points (a cloud) or of the
    vertices of its faces that can be valid (a mesh), (lo + hi) / 2 in float64 from the fp32 corners the search structure holds"""
    tgt = target if isinstance(target, _Target) else _Target(target, _check_max_dist(max_dist, "target_pivot"), target_normal, "target_pivot")
    return tgt.pivot.copy()


def rigid_system(src, T, target, metric="plane", dist_max=0.1, src_normal=None, cos_min=None, two_sided=False, target_normal=None):
    """The Gauss-Newton system of ``src`` [N,3] moved by ``T`` [4,4] against ``target`` -> dict(A float64 [6,6] symmetric, b float64 [6]
    (numpy, host), count, rmse = sqrt(sum r^2 / count), residual [N] and match int64 [N] on the device (0 / -1 where a point has no
    partner: none within ``dist_max``, or with ``src_normal`` and ``cos_min`` one whose normal's cosine is below it -- ``two_sided``: whose
    absolute cosine is), sums float64 [29] host, overlap = count / N).  ``metric``: "plane" (r = n . (q - T p)) or "point" (the vector
    q - T p).  One apply, one search, one system, one 29-double read-back."""
    op = "rigid_system"
    dist_max = _check_max_dist(dist_max, op)
    tgt = target if isinstance(target, _Target) else _Target(target, dist_max, target_normal, op)
    src, src_normal = _src(src, src_normal, op, tgt.device)
    _args(metric, cos_min, tgt, src_normal, op)
    return _system(src, src_normal, _matrix(T, op), tgt, metric, dist_max, cos_min, bool(two_sided))


def register(src, target, init=None, metric="plane", dist_max=0.1, max_iter=30, min_count=100, src_normal=None, cos_min=None, two_sided=False,
             target_normal=None):
    """ICP from ``init`` (default: the identity): Gauss-Newton on ``rigid_system`` (``tracking.gauss_newton``: a step below 1e-5 m and 1e-5 rad
    ends it) -> dict(T float64 [4,4] numpy: src moved by it lies on the target; converged; reason; iterations; trace = [dict(rmse, count)
    per evaluation]; correction = (metres, radians) of T relative to ``init``; rmse, count, overlap of the last evaluation).
    ``dist_max`` may be a decreasing sequence, e.g. (8 tau, 4 tau, 2 tau): each stage runs up to ``max_iter`` steps from the previous
    stage's result; the search structure is built once with the largest value and the system kernel's gate removes what lies beyond a
    stage's own.  A refused step -- fewer than ``min_count`` partners ("count"), A not positive definite ("cholesky") or its extreme
    eigenvalues more than 1e6 apart ("condition") -- returns the transform of the last accepted stage, or ``init``, with converged False
    and the reason: nothing half-done is handed back.  Every system is solved about ONE pivot, chosen once per call from the target
    alone: the centre of its bounding box (``target_pivot``; the box is the search structure's, host values, so the choice costs no
    read-back and is the same for every run).  The three tests above are those of the system about the pivot, and the step norms of the
    stopping rule are those of the twist about it: the 1e-5 m is a motion at the target, not at the world origin."""
    op = "register"
    stages = [dist_max] if isinstance(dist_max, (int, float)) else list(dist_max)
    _need(len(stages) >= 1, "%s: dist_max must be a distance or a sequence of them" % op)
    stages = [_check_max_dist(d, op) for d in stages]
    _need(all(a > b for a, b in zip(stages, stages[1:])), "%s: the stages of dist_max must decrease, got %r" % (op, stages))
    _need(int(max_iter) >= 0 and int(min_count) >= 1, "%s: max_iter must not be negative and min_count at least 1, got %r and %r" % (op, max_iter, min_count))
    tgt = _Target(target, stages[0], target_normal, op)
    src, src_normal = _src(src, src_normal, op, tgt.device)
    _args(metric, cos_min, tgt, src_normal, op)
    T0 = _matrix(np.eye(4) if init is None else init, op)
    T, trace, iterations, last = T0.copy(), [], 0, None
    converged, reason, accepted = False, "max_iter", False

    def system_at(d):
        def f(P):
            nonlocal last
            last = _system(src, src_normal, P, tgt, metric, d, cos_min, bool(two_sided))
            return last
        return f
    for d in stages:
        out = tracking.gauss_newton(system_at(d), T, max_iter, min_count, pivot=tgt.pivot)
        trace += out["trace"]
        iterations += out["iterations"]
        converged, reason = out["converged"], out["reason"]
        if reason in REFUSALS:
            break
        T, accepted = out["pose"], accepted or out["iterations"] > 0
    D = T @ np.linalg.inv(T0) if accepted else np.eye(4)                                     # nothing accepted: no correction, to the bit
    angle = math.acos(min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0)))
    return dict(T=T, converged=converged, reason=reason, iterations=iterations, trace=trace, correction=(float(np.linalg.norm(D[:3, 3])), angle),
                rmse=trace[-1]["rmse"] if trace else 0.0, count=trace[-1]["count"] if trace else 0,
                overlap=last["overlap"] if last is not None else 0.0)


# ---------------------------------------------------------------------------------- global registration (csrc/register/global_register.hip)
STATUS = ("scored", "repeated", "edges", "degenerate")       # estd_ransac_pairs' status 0 .. 3
MIN_INLIERS = 20


def fpfh(points, normal, k=32, radius=None, oriented=True, grid=None):
    """FPFH descriptors of the cloud ``points`` [N,3] with ``normal`` [N,3] (a zero row: no normal) over each point's ``k`` nearest
    neighbours within ``radius`` (``PointGrid.knn``, the point itself among them) -> dict(desc [N,33] float32: three groups of 11 bins,
    each summing to 1; valid uint8 [N]: the point has a normal and at least 3 counted pairs; pairs int32 [N]; invalid: the rows that are
    not valid, an int; hist int32 [N,33]: the SPFH counts).  ``oriented=False`` folds the angles so that the descriptor does not depend
    on the sign of any normal -- what ``estimate_normals(toward=None)`` needs.  ``grid``: a ``PointGrid`` of these very points (its
    ``max_dist`` is then the radius).  The bins use a pseudo-angle instead of atan2 and there is no source/target swap: not PCL's bits.
    The contract: include/estd_hip.h (estd_cloud_spfh, estd_cloud_fpfh)."""
    op = "fpfh"
    _need(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= ops.CLOUD_KNN_MAX, "%s: k must be an integer in 1 .. %d, got %r" % (op, ops.CLOUD_KNN_MAX, k))
    _need(grid is not None or radius is not None, "%s: radius (or a grid) must be given" % op)
    if grid is None:
        grid = PointGrid(points, _check_max_dist(radius, op))
    _need(isinstance(grid, PointGrid), "%s: grid must be a PointGrid" % op)
    points = _check_cloud(points, "points", op, grid.device)
    normal = _check_cloud(normal, "normal", op, grid.device)
    _need(grid.n == points.shape[0] == normal.shape[0], "%s: the grid holds %d points, the cloud %d and normal %d rows"
          % (op, grid.n, points.shape[0], normal.shape[0]))
    _, index, count = grid.knn(points, k)
    hist, pairs = ops.cloud_spfh(points, normal, index, count, bool(oriented))
    desc, valid, invalid = ops.cloud_fpfh(points, normal, index, count, hist, pairs)
    return dict(desc=desc, valid=valid, pairs=pairs, invalid=int(invalid.item()), hist=hist)


def match_features(a, b, a_valid=None, b_valid=None, mutual=True, ratio=None):
    """Correspondences between the descriptors ``a`` [M,33] and ``b`` [N,33] (estd_feature_match: brute force, nearest and second
    nearest) -> (pairs int64 [C,2]: rows of a and b, ascending in a; d2 float32 [C]).  ``mutual``: row i of a and row j of b are kept
    only when each is the other's nearest (the kernel runs both ways, the intersection is taken with torch).  ``ratio``: Lowe's test,
    kept iff d2 < ratio^2 d2_second (in float64), i.e. the distance ratio is below ``ratio``."""
    op = "match_features"
    _need(ratio is None or (isinstance(ratio, (int, float)) and 0 < ratio <= 1), "%s: ratio must lie in (0, 1] or be None, got %r" % (op, ratio))
    index, d2, second = ops.feature_match(a, b, a_valid, b_valid)
    keep = index >= 0
    if mutual:
        back = ops.feature_match(b, a, b_valid, a_valid)[0]
        if back.shape[0]:
            keep &= back[index.clamp_min(0).long()].long() == torch.arange(index.shape[0], device=index.device)
    if ratio is not None:
        keep &= d2.double() < float(ratio) * float(ratio) * second.double()
    rows = torch.nonzero(keep)[:, 0]
    return torch.stack([rows, index[rows].long()], 1), d2[rows]


def ransac_pairs(src_xyz, tgt_xyz, pairs, dist_max, hypotheses=65536, seed=0, edge_ratio=0.9):
    """The rigid transform most of the correspondences ``pairs`` int64 [C,2] (rows of ``src_xyz`` and ``tgt_xyz``) agree on: every one of
    ``hypotheses`` three-point samples (a counter-based draw from ``seed``) is tested and scored over all C pairs (estd_ransac_pairs)
    -> dict(T float64 [4,4] numpy: the winner's transform, the identity when nothing was scored; hypothesis: its number or -1; count:
    its inliers within ``dist_max``; fitness = count / C; ssq: the sum of their squared residuals; status: dict of tallies -- scored,
    repeated (an index drawn twice), edges (Open3D's edge-length test with ``edge_ratio``), degenerate).  The winner is the largest
    count and among equals the smallest hypothesis number: the same from every call."""
    op = "ransac_pairs"
    src_xyz = _check_cloud(src_xyz, "src_xyz", op)
    tgt_xyz = _check_cloud(tgt_xyz, "tgt_xyz", op, src_xyz.device)
    _need(isinstance(pairs, torch.Tensor) and pairs.dtype == torch.int64 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.device == src_xyz.device,
          "%s: pairs must be int64 [C,2] on the clouds' device" % op)
    C = int(pairs.shape[0])
    if C:
        lo, hi = pairs.amin(0).tolist(), pairs.amax(0).tolist()
        _need(min(lo) >= 0 and hi[0] < src_xyz.shape[0] and hi[1] < tgt_xyz.shape[0], "%s: pairs names a row outside the clouds" % op)
    P, Q = src_xyz[pairs[:, 0]].contiguous(), tgt_xyz[pairs[:, 1]].contiguous()
    count, status, ssq, Tm, best = ops.ransac_pairs(P, Q, hypotheses, seed, dist_max, edge_ratio)
    key = int(best.item())
    tally = torch.bincount(status.long(), minlength=4).tolist() if status.shape[0] else [0, 0, 0, 0]
    out = dict(T=np.eye(4), hypothesis=-1, count=0, fitness=0.0, ssq=0.0, status=dict(zip(STATUS, tally)))
    if key:
        h = 0xffffffff - (key & 0xffffffff)
        out["T"][:3, :4] = Tm[h].cpu().numpy().reshape(3, 4)
        out.update(hypothesis=h, count=key >> 32, fitness=(key >> 32) / C, ssq=float(ssq[h].item()))
    return out


def _unit_rows(n):
    """rows scaled to unit length in float64 and rounded once; a zero row stays zero"""
    d = n.double()
    length = d.norm(dim=1, keepdim=True)
    return torch.where(length > 0, d / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(d)).float().contiguous()


def _thinned(xyz, normal, voxel, k, normal_radius):
    """one side of ``register_global``: voxel-thinned points with unit normals -> (points, normals, estimated)"""
    from .cloud_metrics import estimate_normals, voxel_downsample
    points, attrs, _ = voxel_downsample(xyz, voxel, normal)
    if normal is not None:
        return points, _unit_rows(attrs), False
    return points, estimate_normals(points, min(k, ops.CLOUD_KNN_MAX), normal_radius)["normal"], True


def register_global(src, target, voxel, src_normal=None, target_normal=None, k=32, feature_radius=None, normal_radius=None, dist_max=None,
                    hypotheses=65536, seed=0, min_count=MIN_INLIERS, refine=None, edge_ratio=0.9, oriented=None):
    """Registration from an ARBITRARY start: FPFH descriptors on both sides, mutual nearest matches, three-point hypotheses over them,
    and -- with ``refine`` -- ``register`` from the winner.  ``src`` [N,3]; ``target``: a cloud [M,3], a dict(xyz[, normal]) or a mesh
    dict(xyz, faces), which is sampled by area first (4 / voxel^2 points per square metre, with its face normals).  Both sides are
    thinned with ``voxel_downsample(voxel)`` (normals averaged and scaled to unit length); a side without normals gets them from
    ``estimate_normals(k, normal_radius = 2 voxel)``, and then BOTH sides use the folded descriptor (``oriented=False``), since estimated
    normals have no side (``oriented=False`` asks for the folded descriptor also where both sides bring normals, for sources whose
    normals follow different conventions).  ``feature_radius`` = 5 voxel, ``dist_max`` = 1.5 voxel by default.  The stage needs
    distinctive geometry and overlap: on a plane with two spheres, or against a target most of which the source never saw, no
    hypothesis gathers ``min_count`` inliers and the winner is refused.
    ``refine``: None, or a dict of ``register``'s arguments (metric, dist_max -- default (4, 2, 1) voxel --, max_iter, min_count, cos_min,
    two_sided); the refinement runs on the thinned source against the mesh, or against the thinned target cloud with its normals.
    -> dict(T float64 [4,4]: src moved by it lies on the target; T_global: the winner of the hypotheses; fitness, count, pairs (the
    number of correspondences), hypothesis, status; converged, reason; refine: ``register``'s dict or None; clouds: the thinned points
    and normals of both sides and ``oriented``).  A winner with fewer than ``min_count`` inliers is never applied: T and T_global are the
    identity, converged False, reason "inliers" -- the rule of ``register``'s refusals.  Without ``refine`` a winner that passes has
    reason "global"; with it converged and reason are the refinement's."""
    from . import fusion3d
    op = "register_global"
    _need(isinstance(voxel, (int, float)) and math.isfinite(voxel) and voxel > 0, "%s: voxel must be positive and finite, got %r" % (op, voxel))
    _need(isinstance(min_count, int) and min_count >= 3, "%s: min_count must be an integer of at least 3, got %r" % (op, min_count))
    _need(refine is None or isinstance(refine, dict), "%s: refine must be None or a dict of register's arguments" % op)
    voxel = float(voxel)
    feature_radius = 5.0 * voxel if feature_radius is None else feature_radius
    normal_radius = 2.0 * voxel if normal_radius is None else normal_radius
    dist_max = 1.5 * voxel if dist_max is None else dist_max
    src, src_normal = _src(src, src_normal, op, None)
    dev, mesh = src.device, None
    if isinstance(target, dict):
        _need(target.get("xyz") is not None, "%s: a target dict needs 'xyz'" % op)
        if target.get("faces") is not None:
            _need(target_normal is None, "%s: a mesh target takes its normals from its faces; target_normal is for clouds" % op)
            mesh = dict(zip(("xyz", "faces"), fusion3d._mesh_arg(dict(xyz=fusion3d._on_device(target["xyz"], dev), faces=target["faces"]), op)))
            sampled = fusion3d.sample_mesh(mesh, density=4.0 / (voxel * voxel), seed=seed)
            target, target_normal = sampled["xyz"], sampled["normal"]
        else:
            if target_normal is None and target.get("normal") is not None:
                target_normal = fusion3d._on_device(target["normal"], dev)
            target = fusion3d._on_device(target["xyz"], dev)
    target, target_normal = _src(target, target_normal, op, dev)
    sp, sn, s_est = _thinned(src, src_normal, voxel, k, normal_radius)
    tp, tn, t_est = _thinned(target, target_normal, voxel, k, normal_radius)
    _need(oriented is None or (isinstance(oriented, bool) and not (oriented and (s_est or t_est))),
          "%s: oriented must be None or a bool, and True only when both sides bring their normals" % op)
    oriented = not (s_est or t_est) if oriented is None else oriented
    fs = fpfh(sp, sn, k, feature_radius, oriented)
    ft = fpfh(tp, tn, k, feature_radius, oriented)
    pairs, _ = match_features(fs["desc"], ft["desc"], fs["valid"], ft["valid"], mutual=True)
    win = ransac_pairs(sp, tp, pairs, dist_max, hypotheses, seed, edge_ratio)
    out = dict(T=np.eye(4), T_global=np.eye(4), fitness=win["fitness"], count=win["count"], pairs=int(pairs.shape[0]), hypothesis=win["hypothesis"],
               status=win["status"], converged=False, reason="inliers", refine=None,
               clouds=dict(src=sp, src_normal=sn, target=tp, target_normal=tn, oriented=oriented))
    if win["count"] < min_count:
        return out
    out.update(T=win["T"].copy(), T_global=win["T"], converged=True, reason="global")
    if refine is not None:
        kw = dict(refine)
        kw.setdefault("dist_max", (4.0 * voxel, 2.0 * voxel, voxel))
        fine = register(sp, mesh if mesh is not None else dict(xyz=tp, normal=tn), init=win["T"], src_normal=sn, **kw)
        out.update(T=fine["T"], converged=fine["converged"], reason=fine["reason"], refine=fine)
    return out
