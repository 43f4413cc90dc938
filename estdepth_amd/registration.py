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

Out of scope: a scale (Sim(3)), robust kernels beyond the two gates, global registration from an arbitrary start, colour terms.
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
