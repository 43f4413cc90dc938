"""Cross-view consistency of depth maps on the device: the geometric filter multi-view stereo pipelines (MVSNet, COLMAP) put between "a depth
map per frame" and fusion.  A target's depth is reprojected into its neighbouring views, their depths are read there and carried back into
the target; a pixel is kept where enough views agree, with the agreeing depths averaged.  The same pass measures how consistent the depths
of neighbouring frames are in 3D.

    out = check_views(depth, pose, K, src_depths, src_poses)           # one target against 1..8 sources -> views / visible / depth / rel_err
    out = filter_window(depths, poses, K, radius=2, min_views=2)        # every frame of a stack against its neighbours; out["mask"]

    win = ConsistencyWindow(radius=2, min_views=2)                      # streams: a frame comes back ``radius`` pushes later
    for depth, pose in stream:
        rec = win.push(depth, pose, K, conf=fused_prob)
        if rec is not None:
            volume.integrate_filtered(rec)
    for rec in win.flush():
        volume.integrate_filtered(rec)
    print(win.summary())

All arithmetic is csrc/depth_consistency.hip's (the contract: include/estd_hip.h, estd_depth_consistency); there is no CPU path.  Depth maps
are [H,W] (leading 1s allowed) float32 device tensors, z-depth with pixel centres on integers; poses are camera-to-world [4,4]; K is [3,3] in
pixels of the maps.
"""
import torch

from . import camera, ops

MAX_SOURCES = ops.CONSISTENCY_MAX_SOURCES
NAMES = ("views", "visible", "depth", "rel_err")


def _map(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() < 2 or x.numel() != x.shape[-2] * x.shape[-1]:
        raise RuntimeError("%s must be a tensor [H,W] (leading 1s allowed), got %s" % (name, tuple(getattr(x, "shape", ()))))
    return x.reshape(x.shape[-2], x.shape[-1])


def _thresholds(px_max, rel_max, z_near):
    px_max, rel_max, z_near = float(px_max), float(rel_max), float(z_near)
    if not (0 < px_max < float("inf")) or not (0 < rel_max < float("inf")):
        raise RuntimeError("px_max and rel_max must be positive and finite, got %r and %r" % (px_max, rel_max))
    if not (0 <= z_near < float("inf")):
        raise RuntimeError("z_near must be finite and not negative, got %r" % z_near)
    return px_max, rel_max, z_near


def check_views(depth, pose, K, src_depths, src_poses, src_K=None, px_max=1.0, rel_max=0.01, z_near=1e-3):
    """One target ``depth`` [H,W] with ``pose`` [4,4] and ``K`` [3,3] against the 1..8 sources ``src_depths`` ([S,H,W] or a list of [H,W]) with
    ``src_poses`` [S,4,4] and ``src_K`` ([3,3] or [S,3,3]; default: the target's) -> dict(views, visible, depth, rel_err), each [H,W]: the
    number of sources that land within ``px_max`` pixels and ``rel_max`` relative depth of the pixel after the round trip, the number that
    see it at all, the average of the target's and the agreeing depths (the target's own where none agrees) and the mean relative
    difference of the agreeing ones."""
    px_max, rel_max, z_near = _thresholds(px_max, rel_max, z_near)
    target = _map(depth, "depth")
    sources = [_map(s, "source depth %d" % i) for i, s in enumerate(src_depths)]
    if not 1 <= len(sources) <= MAX_SOURCES:
        raise RuntimeError("check_views: 1..%d sources per call, got %d" % (MAX_SOURCES, len(sources)))
    for i, s in enumerate(sources):
        if tuple(s.shape) != tuple(target.shape):
            raise RuntimeError("check_views: source %d is %s, the target %s" % (i, tuple(s.shape), tuple(target.shape)))
    if not isinstance(src_poses, torch.Tensor) or src_poses.numel() != 16 * len(sources):
        raise RuntimeError("check_views: %d sources need src_poses [%d,4,4], got %s" % (len(sources), len(sources), tuple(getattr(src_poses, "shape", ()))))
    if not isinstance(pose, torch.Tensor) or pose.numel() != 16 or not isinstance(K, torch.Tensor) or K.numel() != 9:
        raise RuntimeError("check_views: pose must be [4,4] and K [3,3]")
    src_K = K if src_K is None else src_K
    if not isinstance(src_K, torch.Tensor) or src_K.numel() not in (9, 9 * len(sources)):
        raise RuntimeError("check_views: src_K must be [3,3] or [%d,3,3], got %s" % (len(sources), tuple(getattr(src_K, "shape", ()))))
    mats = camera.consistency_matrices(pose, K, src_poses, src_K)
    if not bool(torch.isfinite(mats).all()):
        raise RuntimeError("check_views: the poses / intrinsics give a matrix that is not finite")
    out = ops.depth_consistency(target.contiguous(), [s.contiguous() for s in sources], mats, px_max, rel_max, z_near)
    return dict(zip(NAMES, out))


def neighbours(t, n, radius):
    """the frames frame ``t`` of ``n`` is checked against: up to ``radius`` on either side, the nearest first, at most MAX_SOURCES; sorted"""
    out = []
    for k in range(1, radius + 1):
        out += [i for i in (t - k, t + k) if 0 <= i < n]
    return sorted(out[:MAX_SOURCES])


def filter_window(depths, poses, K, radius=2, min_views=2, px_max=1.0, rel_max=0.01, z_near=1e-3):
    """Every frame of the stack ``depths`` [T,H,W] (``poses`` [T,4,4], ``K`` [3,3] or [T,3,3]) against its up-to-``2 radius`` neighbours in the
    stack (at most 8, the nearest first) -> dict(depth [T,H,W], views, visible, rel_err, mask = views >= min_views).  A stack of one frame
    has nothing to check against and is an error."""
    if not isinstance(depths, torch.Tensor) or depths.dim() != 3:
        raise RuntimeError("filter_window: depths must be [T,H,W], got %s" % (tuple(getattr(depths, "shape", ())),))
    T = depths.shape[0]
    if T < 2:
        raise RuntimeError("filter_window: at least two frames (a frame is checked against its neighbours), got %d" % T)
    if not isinstance(poses, torch.Tensor) or poses.numel() != 16 * T:
        raise RuntimeError("filter_window: %d frames need poses [%d,4,4], got %s" % (T, T, tuple(getattr(poses, "shape", ()))))
    if not isinstance(K, torch.Tensor) or K.numel() not in (9, 9 * T):
        raise RuntimeError("filter_window: K must be [3,3] or [%d,3,3], got %s" % (T, tuple(getattr(K, "shape", ()))))
    if int(radius) < 1 or int(min_views) < 1:
        raise RuntimeError("filter_window: radius and min_views must be at least 1, got %r and %r" % (radius, min_views))
    _thresholds(px_max, rel_max, z_near)
    poses, Ks = poses.reshape(T, 4, 4), K.reshape(-1, 3, 3)
    per = []
    for t in range(T):
        nb = neighbours(t, T, int(radius))
        per.append(check_views(depths[t], poses[t], Ks[t if Ks.shape[0] > 1 else 0], [depths[i] for i in nb], poses[nb],
                               Ks[nb] if Ks.shape[0] > 1 else Ks[0], px_max, rel_max, z_near))
    out = {k: torch.stack([p[k] for p in per]) for k in NAMES}
    out["mask"] = out["views"] >= float(min_views)
    return out


class ConsistencyWindow:
    """The filter for streams: frames are pushed one at a time and come back, checked against up to ``radius`` frames on either side,
    ``radius`` pushes later; ``flush()`` yields the frames still waiting at the end of the stream, each checked against the neighbours it
    has.  Running totals over everything returned so far: ``summary()``."""

    def __init__(self, radius=2, min_views=2, px_max=1.0, rel_max=0.01, z_near=1e-3):
        if int(radius) < 1 or 2 * int(radius) > MAX_SOURCES:
            raise RuntimeError("ConsistencyWindow: radius must be in 1..%d, got %r" % (MAX_SOURCES // 2, radius))
        if int(min_views) < 1:
            raise RuntimeError("ConsistencyWindow: min_views must be at least 1, got %r" % (min_views,))
        self.radius, self.min_views = int(radius), int(min_views)
        self.px_max, self.rel_max, self.z_near = _thresholds(px_max, rel_max, z_near)
        self.frames = []                    # the last 2 radius + 1 frames at most
        self.pushed = 0                     # frames pushed so far
        self.returned = 0                   # frames returned so far = the frame_index of the next one
        self.checked = 0                    # frames in the totals
        self._acc = None                    # float64 [6]: valid pixels, sum views, sum visible, pixels with views > 0, sum rel_err, kept pixels

    def push(self, depth, pose, K, conf=None, extra=None):
        """Store a frame (the depth is CLONED: the static outputs of a captured graph are overwritten by the next forward) and return the
        record of the frame ``radius`` pushes back once it has all its successors, else None.  A record is a dict: depth (the averaged
        map), views, visible, rel_err, pose, K, conf (the caller's, as given), extra (as given), frame_index, min_views (the window's: what
        ``TSDFVolume.integrate_filtered`` gates with by default)."""
        self.frames.append(dict(depth=_map(depth, "depth").clone(), pose=pose, K=K, conf=conf, extra=extra, index=self.pushed))
        self.pushed += 1
        if self.pushed - self.returned <= self.radius:
            return None
        rec = self._check(self.returned)
        self.frames = [f for f in self.frames if f["index"] >= self.returned - self.radius]
        return rec

    def flush(self):
        """the records of the frames still waiting, in order; the window is empty afterwards (the totals stay)"""
        while self.returned < self.pushed:
            yield self._check(self.returned)
        self.frames = []

    def _check(self, index):
        by_index = {f["index"]: f for f in self.frames}
        frame = by_index[index]
        nb = [i for i in range(index - self.radius, index + self.radius + 1) if i != index and i in by_index]
        if nb:
            out = check_views(frame["depth"], frame["pose"], frame["K"], [by_index[i]["depth"] for i in nb],
                              torch.stack([by_index[i]["pose"].reshape(4, 4).detach().to("cpu", torch.float64) for i in nb]),
                              torch.stack([by_index[i]["K"].reshape(3, 3).detach().to("cpu", torch.float64) for i in nb]),
                              self.px_max, self.rel_max, self.z_near)
        else:                               # a stream of one frame: nothing to check against
            d = frame["depth"]
            ok = torch.isfinite(d) & (d > self.z_near)
            zero = torch.zeros_like(d)
            out = dict(views=zero, visible=zero.clone(), depth=torch.where(ok, d, zero), rel_err=zero.clone())
        self.returned = index + 1
        # the totals stay on the device until summary() asks for them: no synchronisation per frame
        valid, agree, kept = out["depth"] > 0, out["views"] > 0, out["views"] >= float(self.min_views)
        vec = torch.stack([t.double().sum() for t in (valid, out["views"], out["visible"], agree, out["rel_err"], kept)])
        self._acc = vec if self._acc is None else self._acc + vec.to(self._acc.device)
        self.checked += 1
        out.update(pose=frame["pose"], K=frame["K"], conf=frame["conf"], extra=frame["extra"], frame_index=index, min_views=self.min_views)
        return out

    def summary(self):
        """the totals over every frame returned so far: consistent_share = sum views / sum visible over the valid pixels, rel_err = the
        mean over the pixels with views > 0, kept_share = pixels with views >= min_views / valid pixels"""
        valid, views, visible, agreeing, rel_err, kept = self._acc.tolist() if self._acc is not None else [0.0] * 6
        return {"frames": self.checked, "valid_pixels": int(valid), "consistent_share": views / visible if visible else 0.0,
                "rel_err": rel_err / agreeing if agreeing else 0.0, "kept_share": kept / valid if valid else 0.0,
                "radius": self.radius, "min_views": self.min_views, "px_max": self.px_max, "rel_max": self.rel_max}
