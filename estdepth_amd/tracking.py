"""Frame-to-model tracking on the device: projective point-to-plane alignment of a depth map against depth / normal maps rendered from the
fused volume (KinectFusion's tracking step).  It answers "does this frame sit on the model" and moves the frame's pose so that it does.

    model = dict(volume.render(pose_guess, K, (H, W)), pose=pose_guess, K=K)        # the model as the guess sees it, rendered ONCE
    sys = align_step(depth, K, pose_guess, model, dist_max=volume.trunc)             # A, b, count, rmse, residual, match
    out = refine_pose(depth, K, pose_guess, model, dist_max=volume.trunc)            # Gauss-Newton: out["pose"], out["converged"], ...
    out = volume.track(depth, pose_guess, K)                                         # the two lines above in one (fusion3d.TSDFVolume)

All per-pixel arithmetic and the 29 sums are csrc/track/frame_align.hip's (the contract: include/estd_hip.h, estd_frame_align); there is
no CPU path.  The 6 x 6 solve, the exponential map and the stopping rule run on the host in float64; every iteration reads 29 doubles
back.  Depth maps are [H,W] (leading 1s allowed) float32 device tensors, z-depth with pixel centres on integers; poses are
camera-to-world [4,4]; K is [3,3] in pixels of the maps.  The update is on the LEFT, P <- Exp(xi) P with xi = (t, omega) in world axes.

The kernel's Jacobian rows (n, p x n) pivot on the world origin; the host re-expresses the 6 x 6 system about a PIVOT near the scene
before it tests and solves it (``solve_step``, ``gauss_newton``): ``refine_pose`` takes the model camera's centre, ``TSDFVolume.track``
the centre of its volume.  The sums, A and b that ``align_step`` returns stay those about the world origin.
"""
import math

import numpy as np
import torch

from . import camera, ops

COND_MAX = 1e6               # refine_pose refuses a system whose extreme eigenvalues are further apart than this
STEP_T, STEP_R = 1e-5, 1e-5  # a step below 1e-5 m and 1e-5 rad ends the iteration
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]      # the layout of sums[0..20] (include/estd_hip.h)


def _need(ok, msg):
    if not ok:
        raise RuntimeError(msg)


def _map(x, name, op, device=None, last=None):
    _need(isinstance(x, torch.Tensor), "%s: %s must be a tensor" % (op, name))
    _need(x.is_cuda, "%s: %s must live on a ROCm device (estdepth_amd has no CPU path); got %s" % (op, name, x.device))
    _need(x.dtype == torch.float32, "%s: %s must be float32, got %s" % (op, name, x.dtype))
    _need(device is None or x.device == device, "%s: %s is on %s but the depth on %s" % (op, name, x.device, device))
    if last is None:
        _need(x.dim() >= 2 and x.numel() == x.shape[-2] * x.shape[-1] and x.numel() > 0,
              "%s: %s must be [H,W] (leading 1s allowed), got %s" % (op, name, tuple(x.shape)))
        return x.reshape(x.shape[-2], x.shape[-1]).contiguous()
    _need(x.dim() >= 3 and x.shape[-1] == last and x.numel() == x.shape[-3] * x.shape[-2] * last and x.numel() > 0,
          "%s: %s must be [H,W,%d], got %s" % (op, name, last, tuple(x.shape)))
    return x.reshape(x.shape[-3], x.shape[-2], last).contiguous()


def _host(x, shape, name, op):
    _need(isinstance(x, (torch.Tensor, np.ndarray)) and int(np.prod(tuple(x.shape))) == int(np.prod(shape)),
          "%s: %s must be %s, got %s" % (op, name, list(shape), tuple(getattr(x, "shape", ()))))
    a = (x.detach().to("cpu", torch.float64).numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)).reshape(shape)
    _need(bool(np.isfinite(a).all()), "%s: %s holds a value that is not finite" % (op, name))
    return a


def _dist(dist_max, op):
    f32 = lambda v: np.float32(v)                                                       # noqa: E731
    _need(isinstance(dist_max, (int, float)) and math.isfinite(dist_max) and float(f32(dist_max)) > 0
          and math.isfinite(float(f32(dist_max) * f32(dist_max))) and float(f32(dist_max) * f32(dist_max)) > 0,
          "%s: dist_max must be positive and finite (and its square in fp32 too), got %r" % (op, dist_max))
    return float(dist_max)


def exp_se3(xi):
    """Exp of the twist xi = (t, omega) -> float64 [4,4]: the rotation by Rodrigues' formula, the translation V t with
    V = I + (1 - cos th) / th^2 [omega]x + (th - sin th) / th^3 [omega]x^2 (their series below 1e-6 rad)"""
    xi = np.asarray(xi, np.float64).reshape(6)
    t, w = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-6:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th), (th - math.sin(th)) / th ** 3
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + a * Wx + b * (Wx @ Wx)
    out[:3, 3] = (np.eye(3) + b * Wx + c * (Wx @ Wx)) @ t
    return out


def unpack_sums(sums):
    """the 29 sums of estd_frame_align (host values) -> (A float64 [6,6] symmetric, b [6], sum r^2, count)"""
    s = np.asarray(sums, np.float64).reshape(ops.FRAME_ALIGN_SUMS)
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(TRIU):
        A[i, j] = A[j, i] = s[k]
    return A, s[21:27].copy(), float(s[27]), int(round(float(s[28])))


def align_step(depth, cam_intr, pose_guess, model, conf=None, conf_min=0.0, dist_max=0.1, z_near=1e-3):
    """The Gauss-Newton system of the live ``depth`` [H,W] at the camera-to-world ``pose_guess`` [4,4] with ``cam_intr`` [3,3] against
    ``model``: a ``TSDFVolume.render`` result (``depth`` [Hm,Wm], ``normal`` [Hm,Wm,3]) plus the ``pose`` [4,4] and ``K`` [3,3] it was
    rendered with.  Pixels whose ``conf`` [H,W] is below ``conf_min`` and matches farther than ``dist_max`` metres from their model point
    are left out.  -> dict(A float64 [6,6] symmetric, b float64 [6] (numpy, host), count, rmse = sqrt(sum r^2 / count), residual [H,W]
    and match int32 [H,W] on the device (0 / -1 where a pixel has no match), sums float64 [29] host).  One launch, one 29-double
    read-back."""
    op = "align_step"
    depth = _map(depth, "depth", op)
    dev = depth.device
    if conf is not None:
        conf = _map(conf, "conf", op, dev)
        _need(tuple(conf.shape) == tuple(depth.shape), "%s: conf is %s but the depth %s" % (op, tuple(conf.shape), tuple(depth.shape)))
    _need(isinstance(model, dict) and all(model.get(k) is not None for k in ("depth", "normal", "pose", "K")),
          "%s: model must be a dict with depth, normal, pose and K (a render() result plus its pose and intrinsics)" % op)
    m_depth = _map(model["depth"], "model depth", op, dev)
    m_normal = _map(model["normal"], "model normal", op, dev, last=3)
    _need(tuple(m_normal.shape[:2]) == tuple(m_depth.shape), "%s: the model's normal map is %s but its depth %s" % (op, tuple(m_normal.shape), tuple(m_depth.shape)))
    Pg, Pm = _host(pose_guess, (4, 4), "pose_guess", op), _host(model["pose"], (4, 4), "the model's pose", op)
    Kg, Km = _host(cam_intr, (3, 3), "cam_intr", op), _host(model["K"], (3, 3), "the model's K", op)
    dist_max = _dist(dist_max, op)
    z_near, conf_min = float(z_near), float(conf_min)
    _need(0 <= z_near < float("inf"), "%s: z_near must be finite and not negative, got %r" % (op, z_near))
    _need(conf_min == conf_min, "%s: conf_min must not be NaN" % op)
    mats = camera.frame_align_matrices(torch.from_numpy(Pg), torch.from_numpy(Kg), torch.from_numpy(Pm), torch.from_numpy(Km))
    _need(bool(torch.isfinite(mats).all()), "%s: the poses / intrinsics give a matrix that is not finite" % op)
    residual, match, sums = ops.frame_align(depth, conf, m_depth, m_normal, mats.contiguous(), dist_max, z_near, conf_min)
    host = sums.cpu().numpy()
    A, b, rr, count = unpack_sums(host)
    return dict(A=A, b=b, count=count, rmse=math.sqrt(rr / count) if count else 0.0, residual=residual, match=match, sums=host)


def pivot_matrix(pivot):
    """G = [[I, 0], [-[c]x, I]] float64 [6,6] for the pivot c: a Jacobian row (n, q x n) about the world origin is G^-1 times the row
    (n, (q - c) x n) about c, so the system about c is A_c = G A G^T, b_c = G b"""
    c = np.asarray(pivot, np.float64).reshape(3)
    G = np.eye(6)
    G[3:, :3] = -np.array([[0.0, -c[2], c[1]], [c[2], 0.0, -c[0]], [-c[1], c[0], 0.0]])
    return G


def pivoted(A, b, pivot):
    """the system (A, b) of twists about the world origin re-expressed about ``pivot`` in float64 -> (A_c symmetric, b_c); unchanged for None"""
    if pivot is None:
        return A, b
    G = pivot_matrix(pivot)
    Ac = G @ np.asarray(A, np.float64) @ G.T
    return 0.5 * (Ac + Ac.T), G @ np.asarray(b, np.float64)


def pivot_step(xi, pivot):
    """the rigid motion float64 [4,4] of the twist ``xi`` about ``pivot``: C Exp(xi) C^-1 with C the translation by the pivot (Exp(xi) for None)"""
    E = exp_se3(xi)
    if pivot is not None:
        c = np.asarray(pivot, np.float64).reshape(3)
        E[:3, 3] += c - E[:3, :3] @ c
    return E


def solve_step(A, b, count, min_count, cond_max=COND_MAX, pivot=None):
    """The Gauss-Newton step of one system -> (xi float64 [6] or None, reason): refused with ``reason`` "count" when fewer than
    ``min_count`` pixels matched, "cholesky" when A is not positive definite (or not finite), "condition" when the extreme eigenvalues
    of A are more than ``cond_max`` apart; else A xi = b by Cholesky and ``reason`` None.  With ``pivot`` (a float64 3-vector c) the
    system is first re-expressed about c (``pivoted``): the three tests and the solve are those of A_c, b_c, and xi is the twist ABOUT c
    (``pivot_step`` applies it).  The kernels' Jacobians pivot on the world origin, where |q| couples rotation and translation: the
    condition of A grows with the square of the scene's distance from the origin, that of A_c does not."""
    if count < min_count:
        return None, "count"
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None, "cholesky"
    A, b = pivoted(A, b, pivot)
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None, "cholesky"
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None, "cholesky"
    ev = np.linalg.eigvalsh(A)
    if not ev[0] > 0 or ev[-1] > cond_max * ev[0]:
        return None, "condition"
    return np.linalg.solve(Lc.T, np.linalg.solve(Lc, b)), None


def gauss_newton(system, pose_guess, max_iter=10, min_count=100, cond_max=COND_MAX, pivot=None):
    """The host side of ``refine_pose`` for any ``system(pose float64 [4,4]) -> dict(A, b, count, rmse)``: up to ``max_iter`` steps
    P <- Exp(xi) P.  -> dict(pose float64 [4,4], converged, reason, iterations, trace = [dict(rmse, count) per evaluation], correction =
    (translation in metres, angle in radians) of pose relative to the guess).  A refused step (``solve_step``) returns the guess
    unchanged with converged False and the reason; ``reason`` is "converged" once a step is below 1e-5 m and 1e-5 rad, "max_iter" when
    the iterations run out first (the pose is the refined one, converged False).  ``max_iter=0`` evaluates the system once.
    ``pivot`` (float64 [3], fixed for the whole iteration; None: the world origin): every system is solved about it and the step is
    the twist about it, P <- C Exp(xi) C^-1 P; the step norms of the stopping rule are those of that twist, so the 1e-5 m is the motion
    of the pivot, not of the world origin."""
    guess = np.asarray(pose_guess, np.float64).reshape(4, 4).copy()
    if pivot is not None:
        pivot = np.asarray(pivot, np.float64).reshape(3).copy()
        _need(bool(np.isfinite(pivot).all()), "gauss_newton: the pivot holds a value that is not finite")
    P, trace, reason, done = guess.copy(), [], "max_iter", 0
    for it in range(max(int(max_iter), 1)):
        s = system(P)
        trace.append(dict(rmse=float(s["rmse"]), count=int(s["count"])))
        if int(max_iter) < 1:
            break
        xi, why = solve_step(s["A"], s["b"], s["count"], min_count, cond_max, pivot)
        if xi is None:
            return dict(pose=guess, converged=False, reason=why, iterations=it, trace=trace, correction=(0.0, 0.0))
        P = pivot_step(xi, pivot) @ P
        done = it + 1
        if np.linalg.norm(xi[:3]) < STEP_T and np.linalg.norm(xi[3:]) < STEP_R:
            reason = "converged"
            break
    D = P @ np.linalg.inv(guess) if done else np.eye(4)
    angle = math.acos(min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0)))
    return dict(pose=P, converged=reason == "converged", reason=reason, iterations=done, trace=trace,
                correction=(float(np.linalg.norm(D[:3, 3])), angle))


def refine_pose(depth, cam_intr, pose_guess, model, conf=None, conf_min=0.0, dist_max=0.1, max_iter=10, min_count=100, z_near=1e-3, pivot=None):
    """Gauss-Newton refinement of ``pose_guess`` against the FIXED ``model`` maps (arguments as ``align_step``): up to ``max_iter`` steps,
    each one launch and one 29-double read-back, solved on the host in float64 (``gauss_newton``).  The update is refused -- converged
    False, the reason, the guess unchanged -- when fewer than ``min_count`` pixels match, when the Cholesky factorisation of A fails, or
    when A's extreme eigenvalues are more than COND_MAX = 1e6 apart.  The system is solved about ``pivot`` (float64 [3], world
    coordinates; default: the centre of the MODEL's camera, ``model["pose"][:3, 3]``, a host value that is there before the first launch
    and lies within the depth range of the surface it sees), so the verdict does not depend on where the scene lies in the world.
    ``pose`` comes back as a float64 CPU tensor [4,4]."""
    guess = _host(pose_guess, (4, 4), "pose_guess", "refine_pose")
    _need(int(max_iter) >= 0 and int(min_count) >= 1, "refine_pose: max_iter must not be negative and min_count at least 1, got %r and %r" % (max_iter, min_count))
    _need(isinstance(model, dict) and model.get("pose") is not None, "refine_pose: model must be a dict with depth, normal, pose and K")
    pivot = _host(model["pose"], (4, 4), "the model's pose", "refine_pose")[:3, 3] if pivot is None else _host(pivot, (3,), "pivot", "refine_pose")
    out = gauss_newton(lambda P: align_step(depth, cam_intr, P, model, conf, conf_min, dist_max, z_near), guess, max_iter, min_count, pivot=pivot)
    out["pose"] = torch.from_numpy(out["pose"])
    return out
