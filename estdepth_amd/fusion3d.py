"""Volumetric fusion of the model's depth maps on the device: a truncated signed distance (TSDF) volume as in KinectFusion, fed with the
``("depth", t, s)`` / ``("fused_prob", t)`` maps ``DepthNetHybrid.forward`` returns, and read back as an oriented point cloud or as depth / normal / weight maps ray-cast from any camera.

    vol = TSDFVolume(dims=(256, 256, 256), voxel_size=0.03, origin=(-3.8, -3.8, 0.0), device="cuda:0")
    stream = JointStream(model, seq_len=5, graph=True)
    for clip in clips:                                              # consecutive clips share two frames
        outputs, _, _ = stream.push_clip(clip.imgs, clip.poses, K)
        vol.integrate_outputs(outputs, clip.poses[None], K[None], conf_min=0.3)
    vol.save_ply("scene.ply")
    maps = vol.render(pose, K, (H, W))                              # depth / normal / weight of the fused surface in any camera
    out = vol.track(depth, pose_guess, K)                           # the guess refined against the fused surface before the frame is fused
    mesh = vol.extract_mesh()                                       # the fused surface as triangles (surface nets); vol.save_mesh("scene_mesh.ply")

Colour: ``TSDFVolume(..., color=True)`` keeps the frames' colour beside the distances -- pass ``imgs=clip.imgs`` to ``integrate_outputs`` (or
``images=`` to ``integrate``); ``extract_points`` and ``render`` then return a ``"color"`` entry and ``save_ply`` writes red / green / blue.

Which frames are fused: target ``t`` of a call is frame ``t + 1`` of its ``cam_poses``.  ``JointStream`` clips advance by ``seq_len - 2`` frames
and their targets are the INNER frames 1 .. seq_len - 2, so consecutive clips hand over disjoint targets and no frame is fused twice;
``ESTMStream.push`` returns one target (the window's middle frame) per push, each frame once.  Both keep their signatures and results: pass
what they return to ``integrate_outputs`` together with the poses of the same window / clip.

The volume is one float32 tensor ``[2, Z, Y, X]`` (plane 0 = D in [-1, 1], plane 1 = weight; x fastest; zeros = empty); voxel ``(ix, iy, iz)`` has
its centre at ``origin + (idx + 0.5) * voxel_size``.  All arithmetic is csrc/tsdf.hip's and csrc/tsdf_raycast.hip's (the contract: include/estd_hip.h); there is no CPU
path.  A colour volume adds ``self.color``, float32 ``[3, Z, Y, X]`` (12 more bytes per voxel: 201 MB at 256^3 beside the volume's 134 MB), the
weighted average of the image values at the pixels the depths were read at, with the SAME weight plane; values are kept as they are given
(0..255, 0..1 or normalised), so ``save_ply(color_scale=, color_offset=)`` maps them to 0..255 at export.  ``integrate`` only READS the maps, on the current stream -- the static output buffers of ``GraphedForward(clone_outputs=False)`` can
be passed as they are, before the next forward overwrites them.
"""
import math

import numpy as np
import torch

from . import camera, ops

MAX_FRAMES = ops.TSDF_MAX_FRAMES


def frame_groups(n, size=MAX_FRAMES):
    """[(start, stop), ...]: ``n`` frames in call order, at most ``size`` per integrate call"""
    return [(i, min(n, i + size)) for i in range(0, n, size)]


def _as_maps(x, name):
    """[T,H,W] / [T,1,H,W] tensor or a list of [H,W] / [1,H,W] / [1,1,H,W] maps -> list of T tensors"""
    if isinstance(x, torch.Tensor):
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3:
            raise RuntimeError("%s must be [T,H,W] or [T,1,H,W], got %s" % (name, tuple(x.shape)))
        return [x[t] for t in range(x.shape[0])]
    return list(x)


def _as_images(x):
    """[T,3,H,W] tensor or a list of [3,H,W] / [1,3,H,W] images -> list of T tensors"""
    if isinstance(x, torch.Tensor):
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError("images must be [T,3,H,W], got %s" % (tuple(x.shape),))
        return [x[t] for t in range(x.shape[0])]
    return list(x)


def _three(v, name):
    """a scalar or three values -> float64 array [3]"""
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size not in (1, 3):
        raise RuntimeError("%s must be a scalar or three values, got %r" % (name, v))
    return np.broadcast_to(a, (3,)) if a.size == 1 else a


class TSDFVolume:
    def __init__(self, dims, voxel_size, origin, trunc=None, w_max=64.0, z_near=1e-3, device="cuda:0", color=False):
        """dims (Z, Y, X) voxels, X a multiple of 4; ``origin`` (x0, y0, z0) = world position of the corner of voxel (0, 0, 0);
        ``trunc`` in metres (default: 4 voxels).  ``color=True`` allocates the colour planes ``self.color`` [3,Z,Y,X] (12 bytes per voxel,
        201 MB at 256^3); every ``integrate`` call then needs the frames' images."""
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) <= 0:
            raise RuntimeError("TSDFVolume: dims must be three positive sizes (Z, Y, X), got %r" % (dims,))
        if dims[2] % 4:
            raise RuntimeError("TSDFVolume: X must be a multiple of 4 (a lane moves four voxels per access), got %d" % dims[2])
        if not voxel_size > 0:
            raise RuntimeError("TSDFVolume: voxel_size must be positive")
        if len(tuple(origin)) != 3:
            raise RuntimeError("TSDFVolume: origin must be (x0, y0, z0)")
        self.dims, self.voxel_size = dims, float(voxel_size)
        self.origin = torch.tensor([float(v) for v in origin], dtype=torch.float32)
        self.trunc = float(trunc) if trunc is not None else 4.0 * self.voxel_size
        if not self.trunc > 0 or not w_max > 0 or z_near < 0:
            raise RuntimeError("TSDFVolume: trunc and w_max must be positive and z_near must not be negative")
        self.w_max, self.z_near = float(w_max), float(z_near)
        self.device = torch.device(device)
        self.volume = None
        self.frames = 0
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume lives on a ROCm device (estdepth_amd has no CPU path); got %s" % self.device)
        self.volume = torch.zeros((2,) + dims, device=self.device, dtype=torch.float32)
        self.color = torch.zeros((3,) + dims, device=self.device, dtype=torch.float32) if color else None

    # ------------------------------------------------------------------------------------------------ fusion
    @staticmethod
    def check_frames(depths, cam_poses, cam_intr, conf=None, weighted=False, images=None):
        """argument checks of integrate() that need no device -> (depth list, conf list, poses [T,4,4], T); with ``images`` the list of
        [3,H,W] images is appended"""
        depths = _as_maps(depths, "depths")
        confs = _as_maps(conf, "conf") if conf is not None else []
        n = len(depths)
        if n < 1:
            raise RuntimeError("integrate: at least one depth map")
        poses = cam_poses.reshape(-1, 4, 4)
        if poses.shape[0] != n:
            raise RuntimeError("integrate: %d depth maps but %d poses" % (n, poses.shape[0]))
        if cam_intr.numel() not in (9, 9 * n):
            raise RuntimeError("integrate: cam_intr must be [3,3] or [T,3,3], got %s" % (tuple(cam_intr.shape),))
        if confs and len(confs) != n:
            raise RuntimeError("integrate: %d depth maps but %d confidence maps" % (n, len(confs)))
        if weighted and not confs:
            raise RuntimeError("integrate: weighted fusion needs confidence maps")
        hw = tuple(depths[0].shape[-2:])
        for i, m in enumerate(depths + confs):
            if tuple(m.shape[-2:]) != hw or m.numel() != hw[0] * hw[1]:
                raise RuntimeError("integrate: %s map %d is %s, expected %s" % ("depth" if i < n else "confidence", i % n, tuple(m.shape), hw))
        if images is None:
            return depths, confs, poses, n
        images = _as_images(images)
        if len(images) != n:
            raise RuntimeError("integrate: %d depth maps but %d images" % (n, len(images)))
        for i, m in enumerate(images):
            if not isinstance(m, torch.Tensor) or m.dim() < 3 or tuple(m.shape[-3:]) != (3,) + hw or m.numel() != 3 * hw[0] * hw[1]:
                raise RuntimeError("integrate: image %d is %s, expected %s (the depth maps' size)" % (i, tuple(getattr(m, "shape", ())), (3,) + hw))
            if m.device != depths[i].device:
                raise RuntimeError("integrate: image %d is on %s but its depth map on %s" % (i, m.device, depths[i].device))
            if m.dtype != torch.float32:
                raise RuntimeError("integrate: image %d must be float32, got %s" % (i, m.dtype))
        return depths, confs, poses, n, images

    def integrate(self, depths, cam_poses, cam_intr, conf=None, conf_min=0.0, weighted=False, images=None):
        """depths [T,H,W] / [T,1,H,W] (or a list of maps), cam_poses [T,4,4] camera-to-world, cam_intr [3,3] / [T,3,3] in pixels of the maps;
        ``conf``: confidence maps of the same shape -- samples below ``conf_min`` are skipped, ``weighted`` uses them as weights.
        More than 8 frames are fused in groups of 8, in order.  ``images`` [T,3,H,W] (or a list of [3,H,W]): the frames the maps belong
        to, at the maps' size -- required by a colour volume (weight and colour would drift apart without), an error for any other."""
        if (images is None) != (self.color is None):
            raise RuntimeError("integrate: a colour volume needs images= with every call" if images is None else
                               "integrate: images= given but the volume has no colour (TSDFVolume(..., color=True))")
        if images is None:
            depths, confs, poses, n = self.check_frames(depths, cam_poses, cam_intr, conf, weighted)
        else:
            depths, confs, poses, n, images = self.check_frames(depths, cam_poses, cam_intr, conf, weighted, images)
        mats = camera.tsdf_matrices(poses, cam_intr, self.origin, self.voxel_size)
        for a, b in frame_groups(n):
            dd, cc = [d.contiguous() for d in depths[a:b]], [c.contiguous() for c in confs[a:b]]
            if images is None:
                ops.tsdf_integrate_(self.volume, dd, cc, mats[a:b].contiguous(), self.trunc, self.z_near, conf_min, weighted, self.w_max)
            else:
                ops.tsdf_integrate_color_(self.volume, self.color, dd, cc, [m.contiguous() for m in images[a:b]], mats[a:b].contiguous(),
                                          self.trunc, self.z_near, conf_min, weighted, self.w_max)
        self.frames += n
        return self

    def integrate_outputs(self, outputs, cam_poses, cam_intr, scale=0, conf_min=0.0, weighted=False, image_hw=None, imgs=None):
        """The output dict of ``DepthNetHybrid.forward`` (or of the streams) as it is: ("depth", t, scale) and ("fused_prob", t) of every
        target t = frame t + 1 of ``cam_poses`` [1,V,4,4]; ONE integrate call (for up to 8 targets).  ``cam_intr`` [1,3,3] belongs to the
        input images; the decoder returns every scale's depth map at the images' resolution, so it applies as it is -- for maps of another
        size pass the images' ``image_hw`` and rows 0, 1 are scaled to the maps' the way ``scale_cam_intr`` does.  ``imgs``: the forward's
        own [1,V,3,H,W] images for a colour volume -- target t takes ``imgs[0, t + 1]`` as it lies (no copy); they must have the depth
        maps' size."""
        n = 0
        while ("depth", n, scale) in outputs:
            n += 1
        if n == 0:
            raise RuntimeError("integrate_outputs: no (\"depth\", t, %d) in the outputs" % scale)
        poses = cam_poses.reshape(-1, 4, 4)
        if poses.shape[0] != n + 2:
            raise RuntimeError("integrate_outputs: %d targets need %d poses (target t is frame t + 1), got %d" % (n, n + 2, poses.shape[0]))
        depths = [outputs[("depth", t, scale)] for t in range(n)]
        h, w = depths[0].shape[-2:]
        k = cam_intr.reshape(3, 3).clone()
        if image_hw is not None and tuple(image_hw) != (h, w):
            if h * image_hw[1] != w * image_hw[0]:
                raise RuntimeError("integrate_outputs: depth maps %s and images %s differ in aspect" % ((h, w), tuple(image_hw)))
            k[0:2] = k[0:2] * (h / float(image_hw[0]))             # model_hybrid.py:104-108 scale_cam_intr
        confs = []
        for t in range(n):
            c = outputs[("fused_prob", t)]
            ch, cw = c.shape[-2:]
            if (ch, cw) != (h, w):                                 # nearest-neighbour replication to the depth maps' resolution
                if h % ch or w % cw:
                    raise RuntimeError("integrate_outputs: fused_prob %s does not divide the depth map %s" % ((ch, cw), (h, w)))
                c = c.reshape(ch, cw).repeat_interleave(h // ch, 0).repeat_interleave(w // cw, 1)
            confs.append(c)
        images = None
        if imgs is not None:
            if not isinstance(imgs, torch.Tensor) or imgs.dim() != 5 or imgs.shape[0] != 1 or imgs.shape[1] != n + 2 or imgs.shape[2] != 3:
                raise RuntimeError("integrate_outputs: imgs must be [1,%d,3,H,W], got %s" % (n + 2, tuple(getattr(imgs, "shape", ()))))
            if tuple(imgs.shape[-2:]) != (h, w):
                raise RuntimeError("integrate_outputs: images %s and depth maps %s differ in size" % (tuple(imgs.shape[-2:]), (h, w)))
            images = [imgs[0, t + 1] for t in range(n)]
        return self.integrate(depths, poses[1:n + 1], k, conf=confs, conf_min=conf_min, weighted=weighted, images=images)

    def integrate_filtered(self, record, min_views=None, conf_min=0.0):
        """Fuse one frame that went through the cross-view filter: ``record`` as ``consistency.ConsistencyWindow`` returns it (or any dict
        with depth, views, pose, K and optionally conf, min_views, extra).  Only pixels on which ``views >= min_views`` sources agree enter
        the volume (default: the record's own ``min_views``, else 2).  Without a network confidence this is
        ``integrate(depth, pose, K, conf=views, conf_min=min_views)``; with ``record["conf"]`` the depth is set to 0 -- "no sample" for the
        integrate kernel -- where too few views agree, and the confidence gates (``conf_min``) as in ``integrate``.  A colour volume takes the frame's image from ``record["extra"]`` ([3,H,W])."""
        if min_views is None:
            min_views = record.get("min_views", 2)
        if not float(min_views) >= 1:
            raise RuntimeError("integrate_filtered: min_views must be at least 1, got %r" % (min_views,))
        for key in ("depth", "views", "pose", "K"):
            if record.get(key) is None:
                raise RuntimeError("integrate_filtered: the record has no %r" % key)
        depth, views = record["depth"], record["views"]
        if tuple(views.shape[-2:]) != tuple(depth.shape[-2:]):
            raise RuntimeError("integrate_filtered: views is %s but the depth %s" % (tuple(views.shape), tuple(depth.shape)))
        hw = tuple(depth.shape[-2:])
        images = None if self.color is None else record.get("extra")
        if images is not None:
            images = images.reshape((1, 3) + hw)
        pose, K = record["pose"].reshape(1, 4, 4), record["K"].reshape(3, 3)
        conf = record.get("conf")
        if conf is None:
            return self.integrate(depth.reshape((1,) + hw), pose, K, conf=views.reshape((1,) + hw), conf_min=float(min_views), images=images)
        if tuple(conf.shape[-2:]) != hw or conf.numel() != hw[0] * hw[1]:
            raise RuntimeError("integrate_filtered: conf is %s but the depth %s" % (tuple(conf.shape), hw))
        kept = torch.where(views.reshape(hw) >= float(min_views), depth.reshape(hw), torch.zeros_like(depth.reshape(hw)))
        return self.integrate(kept[None], pose, K, conf=conf.reshape((1,) + hw), conf_min=conf_min, images=images)

    # ------------------------------------------------------------------------------------------------ read-back
    def extract_points(self, w_min=1.0, capacity=None):
        """Zero crossings between voxels of weight >= ``w_min`` -> dict(xyz [N,3], normal [N,3], weight [N], edge [N] int64, count) on
        the device; ``edge`` = 3 * linear voxel index + axis makes the unordered records sortable.  ``capacity=None`` counts first and
        allocates exactly; a smaller ``capacity`` keeps that many records (``count`` is the total either way).  A colour volume adds
        ``color`` [N,3]: the colour planes blended along each edge with the crossing's own s."""
        if capacity is None:
            capacity = int(ops.tsdf_extract_points(self.volume, self.voxel_size, self.origin, w_min, 0)[0].item())
        count, xyz, normal, weight, edge = ops.tsdf_extract_points(self.volume, self.voxel_size, self.origin, w_min, int(capacity))
        total = int(count.item())
        n = min(total, int(capacity))
        out = {"xyz": xyz[:n], "normal": normal[:n], "weight": weight[:n], "edge": edge[:n], "count": total}
        if self.color is not None:
            out["color"] = ops.tsdf_edge_colors(self.volume, self.color, out["edge"].contiguous())
        return out

    def render(self, cam_pose, cam_intr, image_hw, depth_min=None, depth_max=None, step=None, w_min=1.0):
        """The fused surface as the camera ``cam_pose`` [4,4] (camera-to-world) with ``cam_intr`` [3,3] (pixels of an ``image_hw`` = (H, W)
        image) sees it -> dict(depth [H,W], normal [H,W,3], weight [H,W]) on the device: z-depth along the optical axis with pixel centres
        on integers (the convention of the model's depth maps, so a render can be scored or fused again as it is), the unit normal in
        world axes towards the cameras that saw the surface, and the interpolated fusion weight; all zeros where a ray finds no surface
        between voxels of weight >= ``w_min``.  A pose stack [V,4,4] (``cam_intr`` [3,3] or [V,3,3]) renders V views: leading dimension V.
        Rays are sampled every ``step`` metres of z-depth (default: one voxel) from ``depth_min`` (default: the volume's ``z_near``) to
        ``depth_max`` (default: past the farthest corner of the volume, per view).  A colour volume adds ``color`` [H,W,3] ([V,H,W,3]): the
        fused colour at the hit, zeros without one.  The contract: include/estd_hip.h, estd_tsdf_raycast / estd_tsdf_raycast_color."""
        mats, (H, W), t_min, dt, n_steps, stacked = render_plan(self.dims, self.voxel_size, self.origin, self.z_near, cam_pose, cam_intr, image_hw,
                                                                depth_min, depth_max, step, w_min)
        if self.color is None:
            names = ("depth", "normal", "weight")
            views = [ops.tsdf_raycast(self.volume, mats[i].contiguous(), H, W, t_min, dt, n_steps[i], w_min) for i in range(mats.shape[0])]
        else:
            names = ("depth", "normal", "weight", "color")
            views = [ops.tsdf_raycast_color(self.volume, self.color, mats[i].contiguous(), H, W, t_min, dt, n_steps[i], w_min)
                     for i in range(mats.shape[0])]
        if not stacked:
            return dict(zip(names, views[0]))
        return {name: torch.stack([v[j] for v in views]) for j, name in enumerate(names)}

    # ------------------------------------------------------------------------------------------------ frame-to-model tracking
    def _model_at(self, cam_pose, cam_intr, image_hw, w_min):
        """the model maps of align_step: the surface as the camera ``cam_pose`` sees it (a colour volume's colour is not used)"""
        if not isinstance(cam_pose, torch.Tensor) or tuple(cam_pose.shape) != (4, 4):
            raise RuntimeError("track: cam_pose must be a tensor [4,4], got %s" % (tuple(getattr(cam_pose, "shape", ())),))
        maps = self.render(cam_pose, cam_intr, image_hw, w_min=w_min)
        return dict(depth=maps["depth"], normal=maps["normal"], pose=cam_pose, K=cam_intr)

    @property
    def centre(self):
        """the centre of the volume in world coordinates, float64 [3] (numpy): origin + voxel_size * (W, H, D) / 2"""
        D, H, W = self.dims
        return self.origin.double().numpy() + 0.5 * self.voxel_size * np.array([W, H, D], np.float64)

    def track(self, depth, cam_pose, cam_intr, conf=None, conf_min=0.0, dist_max=None, max_iter=10, min_count=100, w_min=1.0):
        """Refine the camera-to-world guess ``cam_pose`` [4,4] of the depth map ``depth`` [H,W] (``cam_intr`` [3,3], optional ``conf`` gated
        at ``conf_min``) against the fused surface: the model is rendered ONCE at the guess (``render``), then ``tracking.refine_pose``
        runs up to ``max_iter`` Gauss-Newton steps of projective point-to-plane alignment, keeping matches within ``dist_max`` metres
        (default: the truncation distance).  -> its dict: pose (float64 CPU [4,4]; the guess itself where the update was refused),
        converged, reason, iterations, trace, correction (metres, radians), plus ``matched_share`` = first count / valid depth pixels.
        The Gauss-Newton systems are solved about the volume's ``centre`` (the pivot of ``tracking.gauss_newton``): the surface lies
        inside the volume, so the refusal thresholds judge the scene and not its distance from the world origin."""
        from . import tracking
        if not isinstance(depth, torch.Tensor) or depth.dim() < 2:
            raise RuntimeError("track: depth must be a tensor [H,W] (leading 1s allowed), got %s" % (tuple(getattr(depth, "shape", ())),))
        dist_max = self.trunc if dist_max is None else dist_max
        model = self._model_at(cam_pose, cam_intr, tuple(depth.shape[-2:]), w_min)
        out = tracking.refine_pose(depth, cam_intr, cam_pose, model, conf, conf_min, dist_max, max_iter, min_count, self.z_near, pivot=self.centre)
        out["matched_share"] = out["trace"][0]["count"] / max(int((torch.isfinite(depth) & (depth > self.z_near)).sum().item()), 1)
        return out

    def check_frame(self, depth, cam_pose, cam_intr, conf=None, conf_min=0.0, dist_max=None, w_min=1.0):
        """Does the frame sit on the model?  The zero-iteration form of ``track``: the model rendered at ``cam_pose`` and one evaluation of
        the alignment -> dict(residual [H,W] (the point-to-plane distance in metres, 0 without a match), match int32 [H,W], rmse, count,
        matched_share = count / valid depth pixels)."""
        from . import tracking
        if not isinstance(depth, torch.Tensor) or depth.dim() < 2:
            raise RuntimeError("check_frame: depth must be a tensor [H,W] (leading 1s allowed), got %s" % (tuple(getattr(depth, "shape", ())),))
        dist_max = self.trunc if dist_max is None else dist_max
        model = self._model_at(cam_pose, cam_intr, tuple(depth.shape[-2:]), w_min)
        s = tracking.align_step(depth, cam_intr, cam_pose, model, conf, conf_min, dist_max, self.z_near)
        valid = int((torch.isfinite(depth) & (depth > self.z_near)).sum().item())
        return dict(residual=s["residual"], match=s["match"], rmse=s["rmse"], count=s["count"], matched_share=s["count"] / max(valid, 1))

    def fused_voxels(self):
        """voxels some frame has updated"""
        return int((self.volume[1] > 0).sum().item())

    def save_ply(self, path, w_min=1.0, color_scale=1.0, color_offset=0.0, clusters=None, stats=None):
        """binary little-endian PLY with normals (host side); returns the number of points.  A colour volume appends uchar red / green /
        blue = clamp(round(c * color_scale + color_offset), 0, 255); ``color_scale`` / ``color_offset``: a scalar or three values (one per
        channel), e.g. 255 for 0..1 images or (255 std, 255 mean) to undo a normalisation.
        ``clusters=dict(eps, min_points=10, min_size=None, keep_largest=None)``: the points (in the order they are written in) go through
        ``cloud_metrics.filter_clusters`` first and only the rows it keeps are written; ``stats`` (a dict) then receives n_clusters,
        clusters_kept, kept, dropped and noise.  With the default None nothing more is launched and the file is the same bytes."""
        pts = self.extract_points(w_min=w_min)
        order = torch.argsort(pts["edge"])
        if clusters is not None:
            from . import cloud_metrics
            f = cloud_metrics.filter_clusters(pts["xyz"][order].contiguous(), **clusters)
            order = order[f["keep"]]
            if stats is not None:
                stats.update({k: f[k] for k in ("n_clusters", "clusters_kept", "kept", "dropped", "noise")})
        rec = torch.cat([pts["xyz"][order], pts["normal"][order]], 1).cpu().contiguous()
        rgb = None
        if self.color is not None:
            c = pts["color"][order].cpu().numpy().astype(np.float64) * _three(color_scale, "color_scale") + _three(color_offset, "color_offset")
            rgb = np.clip(np.rint(np.nan_to_num(c)), 0, 255).astype(np.uint8)
        write_ply(path, rec.numpy(), rgb)
        return rec.shape[0]

    def extract_mesh(self, w_min=1.0, min_component=0, simplify=None):
        """The fused surface as a triangle mesh by naive surface nets (csrc/mesh/tsdf_mesh.hip; the contract: include/estd_hip.h,
        estd_tsdf_mesh_vertices / estd_tsdf_mesh_faces): one vertex per cell whose eight corner voxels have weight >= ``w_min`` and differ
        in sign, one quad = two triangles per sign-changing voxel edge whose four cells are observed -> dict(xyz [V,3], normal [V,3] (towards
        the free space; the triangles are counter-clockwise seen from there), weight [V], cell [V] int64, faces [F,3] int32, edge [F/2]
        int64, count = V) on the device, and ``color`` [V,3] for a colour volume.  Vertices come in ascending cell id, quads in ascending
        edge id (= 3 * voxel + axis, the ids of ``extract_points``) with their two triangles consecutive: the result is the same from
        call to call, bit for bit.  A vertex no face references is kept.  Both kernels count first, the outputs are allocated exactly.
        Known limit: a cell that two separate sheets cross gets one vertex, so the sheets pinch together there.
        ``min_component=N`` > 0 passes the mesh through ``filter_mesh(min_triangles=N)``: connected components of fewer than N triangles and
        the unreferenced vertices are dropped, and the dict gains ``components`` and ``dropped``; with the default nothing more is launched.
        ``simplify=cell`` (metres) passes the result through ``simplify_mesh(cell, origin=the volume's origin)`` -- after ``min_component``,
        because clustering would weld floaters to the surface -- and returns its dict (no ``cell`` / ``edge``; ``components`` and
        ``dropped`` are carried over); with the default None nothing more is launched and the mesh is the same bits."""
        mesh = sorted_mesh(ops.tsdf_mesh_vertices, ops.tsdf_mesh_faces, self.volume, self.color, self.voxel_size, self.origin, w_min)
        mesh = filter_mesh(mesh, min_triangles=min_component) if min_component else mesh
        if simplify is None:
            return mesh
        out = simplify_mesh(mesh, simplify, origin=[float(v) for v in self.origin])
        out.update({k: mesh[k] for k in ("components", "dropped") if k in mesh})
        return out

    def save_mesh(self, path, w_min=1.0, color_scale=1.0, color_offset=0.0, min_component=0, simplify=None):
        """``extract_mesh`` as a binary little-endian PLY with normals and a face element (host side); colour as in ``save_ply``;
        ``min_component`` and ``simplify`` as in ``extract_mesh``.  -> (vertices, triangles)"""
        m = self.extract_mesh(w_min=w_min, min_component=min_component, simplify=simplify)
        rec = torch.cat([m["xyz"], m["normal"]], 1).cpu().contiguous()
        rgb = None
        if self.color is not None:
            c = m["color"].cpu().numpy().astype(np.float64) * _three(color_scale, "color_scale") + _three(color_offset, "color_offset")
            rgb = np.clip(np.rint(np.nan_to_num(c)), 0, 255).astype(np.uint8)
        faces = m["faces"].cpu().numpy()
        write_ply(path, rec.numpy(), rgb, faces=faces)
        return rec.shape[0], faces.shape[0]

    def compare(self, other, threshold=0.05, w_min=1.0, max_dist=None, downsample=None, cell=None, sample=None, seed=0, visible=None, exact=False,
                align=None, normals=None, clusters=None):
        """The 3D scores (``cloud_metrics.compare_clouds``: accuracy, completeness, chamfer, precision / recall / F-score at ``threshold``
        metres, ...) of this volume's surface as the prediction against ``other`` as the ground truth: another ``TSDFVolume`` -- both sides
        go through ``extract_points(w_min)`` -- or a dict with ``xyz`` [N,3] and optionally ``normal`` / ``color`` (device tensors or numpy
        arrays, e.g. what ``read_ply`` returns).  Normals are compared when both sides have them, colours when both have a ``color``.
        ``sample=density`` (points per square metre) scores surfaces instead of vertices: a ``TSDFVolume`` side goes through
        ``extract_mesh(w_min)`` and ``sample_mesh(density=sample, seed=seed)``, a dict side with ``faces`` through ``sample_mesh``, a
        dict without faces stays the cloud it is; with the default None nothing of this runs.
        ``visible=dict(cam_poses, cam_intr, image_hw, min_views=1, tol=None, depth_max=None)`` (needs ``sample``) drops the ground-truth
        samples the cameras did not see, as ``cloud_metrics.compare_meshes`` documents it; the result gains ``n_gt`` / ``n_gt_visible``.
        ``exact=True`` (needs ``sample``) hands both sides as meshes to ``cloud_metrics.compare_meshes(exact=True)``: distances to the
        surfaces themselves (csrc/mesh/mesh_distance.hip), and its result (with ``sampled`` and ``exact``) comes back as it is.
        ``align=dict(metric=, dist_max=, max_iter=, init=)`` registers this volume's surface to ``other`` first and scores the moved
        surface (``cloud_metrics.compare_clouds`` / ``compare_meshes`` document it; the result gains ``alignment``): with ``sample`` both
        sides go to ``compare_meshes`` as meshes, so that the registration runs against the ground truth's surface; without, the two
        clouds are registered.  With the default None nothing of this runs.
        ``normals=dict(k=16, radius=None)`` is handed on: a side that comes without normals (a dict without ``normal`` and without faces) gets
        them estimated from its own points (``cloud_metrics.estimate_normals``); the result gains ``normals``.  With the default None nothing
        of this runs.
        ``clusters=dict(eps, min_points=10, min_size=None, keep_largest=None, sides=("pred",))`` is handed on too: the named sides lose
        their floaters first (``cloud_metrics.filter_clusters``; not with ``exact=True``); the result gains ``clusters``.  With the default
        None nothing of this runs."""
        from . import cloud_metrics
        more = {} if normals is None else dict(normals=normals)
        if clusters is not None:
            more["clusters"] = clusters
        if visible is not None and sample is None:
            raise RuntimeError("compare: visible= needs sample=density (the ground-truth surface is sampled, then restricted)")
        if exact and sample is None:
            raise RuntimeError("compare: exact=True needs sample=density (the query points are samples of the two surfaces)")
        if exact or (align is not None and sample is not None):    # the surfaces themselves: cloud_metrics.compare_meshes owns that path
            mesh = lambda x: x.extract_mesh(w_min=w_min) if isinstance(x, TSDFVolume) else x
            return cloud_metrics.compare_meshes(mesh(self), mesh(other), sample, threshold=threshold, max_dist=max_dist, downsample=downsample,
                                                seed=seed, cell=cell, visible=visible, exact=bool(exact), **({} if align is None else dict(align=align)), **more)

        def side(x):
            if sample is not None:
                if isinstance(x, TSDFVolume):
                    x = x.extract_mesh(w_min=w_min)
                if isinstance(x, dict) and x.get("faces") is not None:
                    x = sample_mesh(x, density=sample, seed=seed)
            pts = x.extract_points(w_min=w_min) if isinstance(x, TSDFVolume) else x
            if isinstance(x, TSDFVolume):                      # records come back in no fixed order: sorted by edge, so that which of two equally
                order = torch.argsort(pts["edge"])             # near neighbours is the nearest (its normal, its colour) does not change from run to run
                pts = {k: v[order] for k, v in pts.items() if isinstance(v, torch.Tensor)}
            if not isinstance(pts, dict) or pts.get("xyz") is None:
                raise RuntimeError("compare: the other side must be a TSDFVolume or a dict with 'xyz'")
            out = {}
            for k in ("xyz", "normal", "color"):
                v = pts.get(k)
                if v is not None:
                    out[k] = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) if isinstance(v, np.ndarray) else v).to(self.device).contiguous()
            return out
        a, b = side(self), side(other)
        seen = None
        if visible is not None:
            gt_mesh = other.extract_mesh(w_min=w_min) if isinstance(other, TSDFVolume) else other
            b, n_gt, n_seen = cloud_metrics.restrict_to_visible(gt_mesh, b, visible, threshold, "compare")
            seen = dict(n_gt=n_gt, n_gt_visible=n_seen)
        out = cloud_metrics.compare_clouds(a["xyz"], b["xyz"], threshold=threshold, max_dist=max_dist, downsample=downsample,
                                           pred_normal=a.get("normal") if "normal" in b or normals is not None else None,
                                           gt_normal=b.get("normal") if "normal" in a or normals is not None else None,
                                           pred_color=a.get("color") if "color" in b else None, gt_color=b.get("color") if "color" in a else None,
                                           cell=cell, **({} if align is None else dict(align=align)), **more)
        return out if seen is None else dict(out, **seen)

    def reset(self):
        self.volume.zero_()
        if self.color is not None:
            self.color.zero_()
        self.frames = 0
        return self


def render_plan(dims, voxel_size, origin, z_near, cam_pose, cam_intr, image_hw, depth_min=None, depth_max=None, step=None, w_min=1.0):
    """The argument checks and the host arithmetic of ``TSDFVolume.render`` (no device needed) -> (mats CPU float32 [V,12], (H, W), t_min,
    dt, [n_steps per view], stacked): ``depth_max=None`` marches each view to the z-depth of the volume's farthest corner in that camera,
    beyond which no ray is inside the volume."""
    if not isinstance(cam_pose, torch.Tensor) or cam_pose.dim() not in (2, 3) or tuple(cam_pose.shape[-2:]) != (4, 4):
        raise RuntimeError("render: cam_pose must be [4,4] or [V,4,4], got %s" % (tuple(getattr(cam_pose, "shape", ())),))
    stacked = cam_pose.dim() == 3
    n = cam_pose.shape[0] if stacked else 1
    if n < 1:
        raise RuntimeError("render: at least one pose")
    if not isinstance(cam_intr, torch.Tensor) or cam_intr.numel() not in (9, 9 * n) or tuple(cam_intr.shape[-2:]) != (3, 3):
        raise RuntimeError("render: cam_intr must be [3,3] or [V,3,3], got %s" % (tuple(getattr(cam_intr, "shape", ())),))
    if len(tuple(image_hw)) != 2 or int(image_hw[0]) <= 0 or int(image_hw[1]) <= 0:
        raise RuntimeError("render: image_hw must be two positive sizes (H, W), got %r" % (image_hw,))
    H, W = int(image_hw[0]), int(image_hw[1])
    t_min = float(z_near if depth_min is None else depth_min)
    dt = float(voxel_size if step is None else step)
    if not (t_min >= 0 and t_min < float("inf")):
        raise RuntimeError("render: depth_min must be finite and not negative, got %r" % (depth_min,))
    if not (dt > 0 and dt < float("inf")):
        raise RuntimeError("render: step must be positive and finite, got %r" % (step,))
    if depth_max is not None and not (float(depth_max) > t_min and float(depth_max) < float("inf")):
        raise RuntimeError("render: depth_max must be finite and beyond depth_min = %g, got %r" % (t_min, depth_max))
    if not float(w_min) == float(w_min):
        raise RuntimeError("render: w_min must not be NaN")
    mats = camera.tsdf_ray_matrix(cam_pose, cam_intr, origin, voxel_size)
    if not bool(torch.isfinite(mats).all()):
        raise RuntimeError("render: the poses / intrinsics give a matrix that is not finite")
    P = cam_pose.detach().to("cpu", torch.float64).reshape(-1, 4, 4)
    org = torch.as_tensor(origin, dtype=torch.float64).reshape(3)
    ext = float(voxel_size) * torch.tensor([dims[2], dims[1], dims[0]], dtype=torch.float64)
    corners = torch.stack([org + ext * torch.tensor([i, j, k], dtype=torch.float64) for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    n_steps = []
    for t in range(n):
        far = float(depth_max) if depth_max is not None else float(((corners - P[t, :3, 3]) @ P[t, :3, 2]).max())
        k = int(math.ceil(max(far - t_min, 0.0) / dt)) + 1
        if k > 1 << 24:
            raise RuntimeError("render: %d samples per ray (at most 2^24): step %g is too small for the range %g .. %g" % (k, dt, t_min, far))
        n_steps.append(k)
    return mats, (H, W), t_min, dt, n_steps, stacked


def sorted_mesh(vertices_op, faces_op, volume, color, voxel_size, origin, w_min):
    """The host ordering of ``TSDFVolume.extract_mesh`` over the two operators (ops.tsdf_mesh_vertices / ops.tsdf_mesh_faces): count,
    allocate exactly, sort the vertex records by cell id and the quads by edge id, turn the quads' cell ids into vertex indices by a
    binary search in the sorted cell ids, and split every quad into its triangles (0, 1, 2), (0, 2, 3)."""
    n_v = int(vertices_op(volume, color, voxel_size, origin, w_min, 0)[0].item())
    n_q = int(faces_op(volume, w_min, 0)[0].item())
    _, cell, xyz, normal, weight, rgb = vertices_op(volume, color, voxel_size, origin, w_min, n_v)
    _, edge, quad = faces_op(volume, w_min, n_q)
    cell, order = torch.sort(cell)
    edge, q_order = torch.sort(edge)
    index = torch.searchsorted(cell, quad[q_order].to(torch.int64))
    faces = index[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3).to(torch.int32)
    out = {"xyz": xyz[order], "normal": normal[order], "weight": weight[order], "cell": cell, "faces": faces, "edge": edge, "count": n_v}
    if rgb is not None:
        out["color"] = rgb[order]
    return out


def mesh_edge_stats(faces):
    """``faces`` [F,3] integer tensor (any device) -> dict(boundary, manifold, non_manifold: the mesh edges shared by one, by two and by
    more than two triangles; euler: referenced vertices - edges + faces), by a ``unique`` over int64 keys lo * (max + 1) + hi."""
    f = faces.to(torch.int64)
    if f.shape[0] == 0:
        return dict(boundary=0, manifold=0, non_manifold=0, euler=0)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = e.min(1).values * (int(f.max().item()) + 1) + e.max(1).values
    counts = torch.unique(key, return_counts=True)[1]
    used = int(torch.unique(f).shape[0])
    return dict(boundary=int((counts == 1).sum().item()), manifold=int((counts == 2).sum().item()), non_manifold=int((counts > 2).sum().item()),
                euler=used - int(counts.shape[0]) + int(f.shape[0]))


def _faces_arg(faces, what, device=None):
    """the triangle list of ``mesh_components`` / ``filter_mesh``: a device tensor (int32 [F,3]) as it is, or a numpy integer array [F,3]
    (e.g. from ``read_ply(faces=True)``), which is moved to ``device`` (default: the current ROCm device).  The rules a host array can be
    held to are checked before anything touches a device."""
    if isinstance(faces, np.ndarray):
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
            raise RuntimeError("%s: faces must be an integer array [F,3], got %s %s" % (what, faces.dtype, faces.shape))
        if faces.size and (int(faces.min()) < -0x80000000 or int(faces.max()) > 0x7fffffff):
            raise RuntimeError("%s: a face index does not fit int32" % what)
        return torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(device if device is not None else "cuda")
    if not isinstance(faces, torch.Tensor):
        raise RuntimeError("%s: faces must be a device tensor or a numpy array [F,3], got %s" % (what, type(faces).__name__))
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("%s: faces must be [F,3], got %s" % (what, tuple(faces.shape)))
    if not faces.is_cuda:
        raise RuntimeError("%s: a faces tensor must live on a ROCm device (a host array is passed as numpy); got %s" % (what, faces.device))
    return faces.contiguous()


def mesh_components(faces, n_vertices=None, device=None):
    """The connected components of a triangle mesh (csrc/mesh/mesh_components.hip; the contract: include/estd_hip.h,
    estd_mesh_components).  ``faces``: int32 [F,3] on the device, or a numpy integer array, which is moved to ``device``; ``n_vertices``:
    default the largest index + 1.  -> dict(label [V] int32: the smallest vertex index of each vertex's component, roots [C] int64
    ascending, triangles [C] int32 and vertices [C] int64: the size of the component of each root, count = C) on the device.  Components
    are ordered by root; a vertex no face uses is a component of its own with 0 triangles.  A face that names a vertex outside
    0..n_vertices-1 raises RuntimeError with the number of such faces."""
    if n_vertices is not None and int(n_vertices) < 0:
        raise RuntimeError("mesh_components: n_vertices must not be negative, got %r" % (n_vertices,))
    faces = _faces_arg(faces, "mesh_components", device)
    if n_vertices is None:
        n_vertices = int(faces.max().item()) + 1 if faces.shape[0] else 0
    label, triangles, invalid = ops.mesh_components(faces, int(n_vertices))
    bad = int(invalid.item())
    if bad:
        raise RuntimeError("mesh_components: %d of %d faces name a vertex outside 0..%d" % (bad, faces.shape[0], int(n_vertices) - 1))
    wide = label.to(torch.int64)
    roots = torch.nonzero(wide == torch.arange(wide.shape[0], device=wide.device)).reshape(-1)
    return dict(label=label, roots=roots, triangles=triangles[roots], vertices=torch.bincount(wide, minlength=wide.shape[0])[roots],
                count=int(roots.shape[0]))


PER_VERTEX = ("xyz", "normal", "weight", "cell", "color", "rgb")      # the entries of a mesh dict with one row per vertex


def filter_mesh(mesh, min_triangles=1, keep_largest=None):
    """``mesh`` (any dict with ``xyz`` [V,3] and ``faces`` [F,3]: what ``extract_mesh`` returns, or ``read_ply(faces=True)``) without its
    small connected components: those with at least ``min_triangles`` triangles are kept, and with ``keep_largest=k`` only the k of them
    with the most triangles (ties go to the smaller root).  -> a dict with the input's keys on the device: the per-vertex entries (xyz,
    normal, weight, cell, color / rgb where present) filtered with their order kept, ``faces`` re-indexed (int32, order kept), ``edge``
    (one id per quad = two consecutive triangles, which always share a component) filtered by quad, ``count`` = the new V,
    ``components`` = the components kept and ``dropped`` = dict(vertices, faces, components: those with at least one triangle; a vertex
    no face uses counts under vertices only).  The default ``min_triangles=1`` drops exactly the unreferenced vertices.  The labelling
    is the kernels' (``mesh_components``); the compaction (a mask, a running sum, indexing) is torch glue as in ``sorted_mesh``."""
    if not isinstance(mesh, dict) or mesh.get("xyz") is None or mesh.get("faces") is None:
        raise RuntimeError("filter_mesh: the mesh must be a dict with 'xyz' and 'faces'")
    if int(min_triangles) != min_triangles or min_triangles < 0:
        raise RuntimeError("filter_mesh: min_triangles must be an integer that is not negative, got %r" % (min_triangles,))
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 0):
        raise RuntimeError("filter_mesh: keep_largest must be None or an integer that is not negative, got %r" % (keep_largest,))
    n_v = int(mesh["xyz"].shape[0])
    edge = mesh.get("edge")
    if edge is not None and 2 * int(edge.shape[0]) != int(mesh["faces"].shape[0]):
        raise RuntimeError("filter_mesh: %d edge ids for %d faces (one per two triangles expected)" % (edge.shape[0], mesh["faces"].shape[0]))
    for k in PER_VERTEX:
        if mesh.get(k) is not None and int(mesh[k].shape[0]) != n_v:
            raise RuntimeError("filter_mesh: %s has %d rows for %d vertices" % (k, mesh[k].shape[0], n_v))
    devs = [v.device for v in mesh.values() if isinstance(v, torch.Tensor) and v.is_cuda]
    faces = _faces_arg(mesh["faces"], "filter_mesh", devs[0] if devs else None)
    dev = faces.device
    comp = mesh_components(faces, n_v)
    with_faces = comp["triangles"] > 0
    keep = with_faces & (comp["triangles"] >= int(min_triangles)) if min_triangles > 0 else torch.ones_like(with_faces)
    if keep_largest is not None:
        at = torch.nonzero(keep).reshape(-1)                                     # by ascending root: the stable sort settles ties that way
        order = torch.sort(comp["triangles"][at].to(torch.int64), descending=True, stable=True)[1]
        keep = torch.zeros_like(keep)
        keep[at[order[:int(keep_largest)]]] = True
    root_kept = torch.zeros(n_v, dtype=torch.bool, device=dev)
    root_kept[comp["roots"][keep]] = True
    v_mask = root_kept[comp["label"].to(torch.int64)]
    new_index = torch.cumsum(v_mask, 0) - 1
    f_mask = v_mask[faces[:, 0].to(torch.int64)]
    out = {}
    for k, v in mesh.items():
        if k in PER_VERTEX and v is not None:
            out[k] = (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v).to(dev)[v_mask]
        else:
            out[k] = v
    out["faces"] = new_index[faces[f_mask].to(torch.int64)].to(torch.int32)
    if edge is not None:
        out["edge"] = (torch.from_numpy(np.ascontiguousarray(edge)) if isinstance(edge, np.ndarray) else edge).to(dev)[f_mask[0::2]]
    out["count"] = int(v_mask.sum().item())
    out["components"] = int(keep.sum().item())
    out["dropped"] = dict(vertices=n_v - out["count"], faces=int(faces.shape[0] - out["faces"].shape[0]),
                          components=int((with_faces & ~keep).sum().item()))
    return out


def _on_device(v, dev, dtype=torch.float32):
    """a per-vertex entry of a mesh dict (numpy array or tensor) as a contiguous ``dtype`` tensor on ``dev``"""
    t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
    return t.to(device=dev, dtype=dtype).contiguous()


def _mesh_arg(mesh, what):
    """the ``xyz`` and ``faces`` of a mesh dict on one device -> (xyz float32 [V,3], finite; faces int32 [F,3])"""
    from .cloud_metrics import _check_cloud
    if not isinstance(mesh, dict) or mesh.get("xyz") is None or mesh.get("faces") is None:
        raise RuntimeError("%s: the mesh must be a dict with 'xyz' and 'faces'" % what)
    devs = [v.device for v in mesh.values() if isinstance(v, torch.Tensor) and v.is_cuda]
    faces = _faces_arg(mesh["faces"], what, devs[0] if devs else None)
    return _check_cloud(_on_device(mesh["xyz"], faces.device), "xyz", what, faces.device), faces


def mesh_area(mesh):
    """The area of a triangle mesh (csrc/mesh/mesh_sample.hip; the contract: include/estd_hip.h, estd_mesh_face_area).  ``mesh``: a dict
    with ``xyz`` [V,3] and ``faces`` [F,3] (what ``extract_mesh``, ``filter_mesh`` or ``read_ply(faces=True)`` return; numpy arrays are
    moved to the device) -> dict(total: float, the sum in float64; area [F] float64 on the device; invalid: the faces that name a vertex
    outside the mesh, which have area 0)."""
    xyz, faces = _mesh_arg(mesh, "mesh_area")
    area, _, invalid = ops.mesh_face_area(xyz, faces)
    return dict(total=float(area.sum().item()), area=area, invalid=int(invalid.item()))


def unique_faces(triple):
    """The host glue behind ops.mesh_cluster_faces: ``triple`` [F,3] int32 (-1 -1 -1 = no face) -> (faces [F',3] int32, kept [F'] int64: the
    input face of each).  The surviving triples; among equal triples the one with the smallest input face index; in ascending input face
    index.  The same three clusters in the opposite winding are another triple and stay.  Three stable sorts, column by column: no packed
    key that could leave int64."""
    at = torch.nonzero(triple[:, 0] >= 0).reshape(-1)
    t = triple[at]
    order = torch.arange(t.shape[0], device=t.device)
    for col in (2, 1, 0):
        order = order[torch.sort(t[order, col], stable=True)[1]]
    ts = t[order]
    first = torch.ones(ts.shape[0], dtype=torch.bool, device=t.device)
    first[1:] = (ts[1:] != ts[:-1]).any(1)
    kept = torch.sort(order[first])[0]                         # equal triples stand in ascending input order: the first is the smallest
    return t[kept].contiguous(), at[kept]


def simplify_mesh(mesh, cell, origin=None, placement="quadric", reg=2.0 ** -12):
    """``mesh`` simplified by vertex clustering (csrc/mesh/mesh_simplify.hip; the contract: include/estd_hip.h, estd_mesh_cluster_faces /
    estd_mesh_cluster_quadrics): every vertex that falls in one cell of a uniform grid of edge ``cell`` becomes one vertex, triangles
    that lose a corner disappear and duplicates are merged.  ``mesh`` as in ``mesh_area`` (numpy arrays are moved to the device).  The
    grid is ``cloud_cell_keys``' and starts at ``origin`` (three values, none above the bounding box's minimum; default: that minimum,
    as in ``voxel_downsample``).  ``placement="quadric"`` puts the new vertex where the summed plane quadrics of the cell's triangles
    are smallest, regularised towards the cell's mean by ``reg`` times the trace, and falls back to the mean where that point is not
    well defined or leaves the cell: edges and corners survive, which the mean rounds off.  ``placement="mean"`` is the mean throughout
    (``voxel_downsample``'s bits) and launches the faces kernel only.
    -> dict on the device: xyz [K,3]; normal [K,3] (quadric: the area-weighted normal of the cluster's faces; mean: the normalised mean
    of the input's normals, where it has them); faces [F',3] int32, in ascending input face index; weight / color / rgb: the clusters'
    means, where the input has them; cluster [V] int32: input vertex -> output vertex; cell_key [K] int64, ascending; placed [K] bool;
    count = K; stats = dict(vertices_in, faces_in, vertices, faces, collapsed, duplicates, invalid, placed, fallback: the clusters the
    quadric placement left at their mean).  The per-vertex ``cell`` and per-quad ``edge`` of a surface-net mesh no longer apply and are
    dropped.  A face that names a vertex outside the mesh raises RuntimeError, as in ``mesh_components``.
    Known limit: vertex clustering does not preserve topology.  Two sheets closer than a cell weld, and edges shared by more than two
    triangles can appear; ``mesh_edge_stats`` reports them, nothing repairs them."""
    from .cloud_metrics import _dims
    what = "simplify_mesh"
    if not (isinstance(cell, (int, float)) and math.isfinite(cell) and float(np.float32(cell)) > 0):
        raise RuntimeError("%s: cell must be positive and finite, got %r" % (what, cell))
    if placement not in ("quadric", "mean"):
        raise RuntimeError("%s: placement must be 'quadric' or 'mean', got %r" % (what, placement))
    if not (isinstance(reg, (int, float)) and math.isfinite(reg) and reg >= 0):
        raise RuntimeError("%s: reg must be finite and not negative, got %r" % (what, reg))
    xyz, faces = _mesh_arg(mesh, what)
    dev, n_v, n_f = faces.device, int(xyz.shape[0]), int(faces.shape[0])
    cell = float(np.float32(cell))
    cols, names = [], []
    for k in ("weight", "color", "rgb") + (("normal",) if placement == "mean" else ()):
        if mesh.get(k) is not None:
            width = 1 if k == "weight" else 3
            if int(mesh[k].shape[0]) != n_v or int(np.prod(mesh[k].shape)) != n_v * width:
                raise RuntimeError("%s: %s must be [%d%s], got %s" % (what, k, n_v, "" if width == 1 else ",3", tuple(mesh[k].shape)))
            cols.append(_on_device(mesh[k], dev).reshape(n_v, width))
            names.append(k)
    if n_v:
        lo, hi = xyz.amin(0).cpu(), xyz.amax(0).cpu()
        if origin is not None:
            org = torch.as_tensor(np.asarray(origin, dtype=np.float32).reshape(-1))
            if org.numel() != 3 or not bool(torch.isfinite(org).all()) or bool((org > lo).any()):
                raise RuntimeError("%s: origin must be three finite values, none above the bounding box's minimum %s, got %r" % (what, lo.tolist(), origin))
            lo = org
        dims = _dims((hi.double() - lo.double()).tolist(), cell)
        if max(dims) > ops.CLOUD_KEY_MAX_DIM:
            raise RuntimeError("%s: %r cells per axis (at most %d): the cell %g is too small for this mesh" % (what, dims, ops.CLOUD_KEY_MAX_DIM, cell))
        keys = ops.cloud_cell_keys(xyz, lo.contiguous(), cell, dims)
        sorted_keys, order = torch.sort(keys, stable=True)
        cell_key, rank, counts = torch.unique_consecutive(sorted_keys, return_inverse=True, return_counts=True)
        cluster = torch.empty(n_v, device=dev, dtype=torch.int32)
        cluster[order] = rank.to(torch.int32)
        segments = torch.zeros(counts.shape[0] + 1, device=dev, dtype=torch.int64)
        segments[1:] = torch.cumsum(counts, 0)
        order = order.contiguous()
        attrs = torch.cat(cols, 1) if cols else None
        mean, mean_attrs = ops.cloud_cell_centroids(xyz, attrs[:, :ops.CLOUD_MAX_ATTRS].contiguous() if cols else None, order, segments)
        if cols and attrs.shape[1] > ops.CLOUD_MAX_ATTRS:      # more columns than one call takes
            mean_attrs = torch.cat([mean_attrs, ops.cloud_cell_centroids(xyz, attrs[:, ops.CLOUD_MAX_ATTRS:].contiguous(), order, segments)[1]], 1)
    else:
        lo, dims = torch.zeros(3), (1, 1, 1)
        cell_key = torch.empty(0, device=dev, dtype=torch.int64)
        cluster = torch.empty(0, device=dev, dtype=torch.int32)
        mean, mean_attrs = xyz, (torch.cat(cols, 1) if cols else None)
    n_k = int(cell_key.shape[0])
    corner, triple, counts = ops.mesh_cluster_faces(faces, cluster, n_k)
    invalid, collapsed = (int(v) for v in counts.tolist())
    if invalid:
        raise RuntimeError("%s: %d of %d faces name a vertex outside 0..%d" % (what, invalid, n_f, n_v - 1))
    new_faces, _ = unique_faces(triple)
    out = {"faces": new_faces, "cluster": cluster, "cell_key": cell_key, "count": n_k}
    if placement == "quadric":
        rec_cluster, rec_order = torch.sort(corner, stable=True)
        rec_segments = torch.searchsorted(rec_cluster, torch.arange(n_k + 1, device=dev, dtype=torch.int32))
        out["xyz"], out["normal"], out["placed"] = ops.mesh_cluster_quadrics(xyz, faces, rec_order.contiguous(), rec_segments.contiguous(), cell_key,
                                                                             mean, lo.contiguous(), cell, dims, float(reg))
    else:
        out["xyz"], out["placed"] = mean, torch.zeros(n_k, device=dev, dtype=torch.bool)
    at = 0
    for k, c in zip(names, cols):
        v = mean_attrs[:, at:at + c.shape[1]]
        at += c.shape[1]
        out[k] = torch.nn.functional.normalize(v, dim=1) if k == "normal" else (v.reshape(-1) if k == "weight" else v.contiguous())
    placed = int(out["placed"].sum().item())
    n_out = int(new_faces.shape[0])
    out["stats"] = dict(vertices_in=n_v, faces_in=n_f, vertices=n_k, faces=n_out, collapsed=collapsed, duplicates=n_f - invalid - collapsed - n_out,
                        invalid=invalid, placed=placed, fallback=n_k - placed if placement == "quadric" else 0)
    return out


def sample_mesh(mesh, n=None, density=None, seed=0, normals="face"):
    """An evenly spread point cloud on a triangle mesh: ``n`` points, or ``density`` points per square metre (n = ceil(density x area)),
    stratified along the cumulative area (csrc/mesh/mesh_sample.hip; the contract: include/estd_hip.h, estd_mesh_sample) -- every
    triangle holds its share of the points within +-2, whatever its size, and a triangle without area none.  ``mesh`` as in ``mesh_area``;
    uint8 ``rgb`` counts as float32 ``color``.  -> dict(xyz [n,3], normal [n,3], color [n,3] (if the mesh has one), face [n] int32: the
    triangle of each point, bary [n,2]: its barycentric pair, area [F] float64, total: their sum, n, invalid) on the device.
    ``normals="face"`` (the default: ground-truth files usually carry no normals) gives the triangle's unit normal, ``"vertex"`` the
    mesh's vertex normals interpolated and normalised.  The result is a function of (mesh, n, seed): the same bits from every call."""
    what = "sample_mesh"
    if not isinstance(mesh, dict) or mesh.get("xyz") is None or mesh.get("faces") is None:
        raise RuntimeError("%s: the mesh must be a dict with 'xyz' and 'faces'" % what)
    if (n is None) == (density is None):
        raise RuntimeError("%s: exactly one of n and density must be given, got n = %r and density = %r" % (what, n, density))
    if n is not None and (not isinstance(n, (int, np.integer)) or not 0 <= n < 2 ** 31):
        raise RuntimeError("%s: n must be an integer in 0 .. 2^31 - 1, got %r" % (what, n))
    if density is not None and not (isinstance(density, (int, float)) and math.isfinite(density) and density > 0):
        raise RuntimeError("%s: density must be positive and finite (points per square metre), got %r" % (what, density))
    if normals not in ("face", "vertex"):
        raise RuntimeError("%s: normals must be 'face' or 'vertex', got %r" % (what, normals))
    if normals == "vertex" and mesh.get("normal") is None:
        raise RuntimeError("%s: normals='vertex' needs a mesh with vertex normals ('normal')" % what)
    xyz, faces = _mesh_arg(mesh, what)
    dev, n_v = faces.device, int(xyz.shape[0])
    color = mesh.get("color") if mesh.get("color") is not None else mesh.get("rgb")
    cols = [_on_device(v, dev) for v in ((mesh["normal"] if normals == "vertex" else None), color) if v is not None]
    for c in cols:
        if c.dim() != 2 or c.shape[0] != n_v or c.shape[1] != 3:
            raise RuntimeError("%s: normal and color must be [%d,3], got %s" % (what, n_v, tuple(c.shape)))
    if n is None:
        total = float(ops.mesh_face_area(xyz, faces)[0].sum().item())
        n = int(math.ceil(float(density) * total))
        if n >= 2 ** 31:
            raise RuntimeError("%s: density %r over %.6g square metres asks for %d points (at most 2^31 - 1)" % (what, density, total, n))
    p, face, bary, normal, attrs, area, invalid = ops.mesh_sample(xyz, faces, torch.cat(cols, 1) if cols else None, int(n), seed)
    out = dict(xyz=p, normal=normal, face=face, bary=bary, area=area, total=float(area.sum().item()), n=int(p.shape[0]),
               invalid=int(invalid.item()))
    if normals == "vertex":
        out["normal"] = torch.nn.functional.normalize(attrs[:, :3], dim=1)
    if color is not None:
        out["color"] = attrs[:, -3:].contiguous()
    return out


def write_ply(path, xyz_normal, rgb=None, faces=None):
    """xyz_normal: float32 array [N,6] -> binary little-endian PLY (x y z nx ny nz); ``rgb``: uint8 array [N,3] appends uchar red green
    blue to every vertex (27 bytes per record); ``faces``: integer array [F,3] appends a face element (``property list uchar int
    vertex_indices``, 13 bytes per triangle).  Without ``faces`` the file is what it was before the argument existed, byte for byte."""
    n = int(xyz_normal.shape[0])
    tail, face_body = "", b""
    if faces is not None:
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
            raise RuntimeError("write_ply: faces must be an integer array [F,3], got %s %s" % (faces.dtype, faces.shape))
        if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= n):
            raise RuntimeError("write_ply: a face names a vertex outside 0..%d" % (n - 1))
        tail = "element face %d\nproperty list uchar int vertex_indices\n" % faces.shape[0]
        frec = np.empty(faces.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
        frec["n"], frec["v"] = 3, faces
        face_body = frec.tobytes()
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\n" % n)
    if rgb is None:
        body = xyz_normal.astype("<f4").tobytes()
    else:
        rgb = np.asarray(rgb)
        if rgb.shape != (n, 3) or rgb.dtype != np.uint8:
            raise RuntimeError("write_ply: rgb must be uint8 [%d,3], got %s %s" % (n, rgb.dtype, rgb.shape))
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        rec = np.empty(n, dtype=[("v", "<f4", (6,)), ("c", "u1", (3,))])
        rec["v"], rec["c"] = xyz_normal, rgb
        body = rec.tobytes()
    with open(path, "wb") as f:
        f.write((head + tail + "end_header\n").encode("ascii"))
        f.write(body)
        f.write(face_body)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path, faces=False):
    """The counterpart of ``write_ply`` -> dict(xyz float32 [N,3], normal float32 [N,3] or None, rgb uint8 [N,3] or None) as numpy arrays.
    Reads what ``write_ply`` writes and any ``binary_little_endian`` or ``ascii`` file whose vertex element has float x y z, optionally
    float nx ny nz and uchar red green blue; other vertex properties are skipped by their declared size, other elements (faces) are
    ignored -- the vertex element must come first in a binary file unless the elements before it have no list property.  A big-endian or
    malformed file raises RuntimeError.  ``faces=True`` adds ``faces`` int32 [F,3] from the face element's one list property
    (``vertex_indices`` / ``vertex_index``; [0,3] without a face element): triangles only, a list of any other length raises RuntimeError,
    and so does an index outside the vertices."""
    def bad(why):
        raise RuntimeError("read_ply: %s: %s" % (path, why))
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    stop = data.find(b"\n", end)                               # the header may end its lines with CR LF
    if not data.startswith(b"ply") or end < 0 or stop < 0:
        bad("not a PLY file (no 'ply' magic or no end_header)")
    try:
        lines = [l.split() for l in data[:end].decode("ascii").splitlines()]
    except UnicodeDecodeError:
        bad("the header is not ASCII")
    body = data[stop + 1:]
    fmt, elements, lists = None, [], {}                        # elements: [name, count, [(property, dtype or None for a list)]]
    for w in lines[1:]:
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format" and len(w) == 3:
            fmt = w[1]
        elif w[0] == "element" and len(w) == 3 and w[2].isdigit():
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property" and elements and len(w) == 3 and w[1] in _PLY_TYPES:
            elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
        elif w[0] == "property" and elements and len(w) == 5 and w[1] == "list" and w[2] in _PLY_TYPES and w[3] in _PLY_TYPES:
            elements[-1][2].append((w[4], None))
            lists[(len(elements) - 1, w[4])] = (_PLY_TYPES[w[2]], _PLY_TYPES[w[3]])     # (type of the length, type of the items)
        else:
            bad("header line %r not understood" % " ".join(w))
    if fmt not in ("binary_little_endian", "ascii"):
        bad("format %r is not supported (binary_little_endian and ascii are)" % (fmt,))
    at = [i for i, e in enumerate(elements) if e[0] == "vertex"]
    if len(at) != 1:
        bad("expected one vertex element, found %d" % len(at))
    _, n, props = elements[at[0]]
    names = [p[0] for p in props]
    if len(set(names)) != len(names) or any(t is None for _, t in props):
        bad("the vertex element has a repeated or a list property")
    types = dict(props)
    if not all(types.get(k) == "f4" for k in ("x", "y", "z")):
        bad("the vertex element needs float x, y, z")
    has_normal = all(types.get(k) == "f4" for k in ("nx", "ny", "nz"))
    has_rgb = all(types.get(k) == "u1" for k in ("red", "green", "blue"))
    if fmt == "ascii":
        rows = body.decode("ascii", errors="replace").split("\n")
        skip = 0
        for e in elements[:at[0]]:
            skip += e[1]
        if len(rows) < skip + n:
            bad("%d vertex lines declared, the file ends early" % n)
        try:
            table = np.array([[float(v) for v in r.split()] for r in rows[skip:skip + n]], dtype=np.float64).reshape(n, -1)
        except ValueError:
            bad("a vertex line is not numeric or the lines differ in length")
        if n and table.shape[1] != len(props):
            bad("a vertex line has %d values, the header declares %d properties" % (table.shape[1], len(props)))
        col = lambda keys, dt: np.ascontiguousarray(np.stack([table[:, names.index(k)] for k in keys], 1).astype(dt)) if n else np.zeros((0, 3), dt)
    else:
        offset = 0
        for e in elements[:at[0]]:
            if any(t is None for _, t in e[2]):
                bad("a list property in front of the vertex element")
            offset += e[1] * sum(np.dtype(t).itemsize for _, t in e[2])
        dt = np.dtype([(k, "<" + t) for k, t in props])
        if len(body) < offset + n * dt.itemsize:
            bad("%d vertices of %d bytes declared, the file holds %d bytes" % (n, dt.itemsize, len(body) - offset))
        rec = np.frombuffer(body, dtype=dt, count=n, offset=offset)
        col = lambda keys, dt_: np.ascontiguousarray(np.stack([rec[k] for k in keys], 1).astype(dt_)) if n else np.zeros((0, 3), dt_)
    out = dict(xyz=col(("x", "y", "z"), np.float32), normal=col(("nx", "ny", "nz"), np.float32) if has_normal else None,
               rgb=col(("red", "green", "blue"), np.uint8) if has_rgb else None)
    if not faces:
        return out
    fat = [i for i, e in enumerate(elements) if e[0] == "face"]
    if len(fat) > 1:
        bad("more than one face element")
    tri = np.zeros((0, 3), np.int32)
    if fat:
        _, nf, fprops = elements[fat[0]]
        if len(fprops) != 1 or fprops[0][1] is not None or fprops[0][0] not in ("vertex_indices", "vertex_index"):
            bad("the face element needs exactly one property, the list vertex_indices")
        if any(t is None for e in elements[:fat[0]] for _, t in e[2]):
            bad("a list property in front of the face element")
        ct, it = lists[(fat[0], fprops[0][0])]
        if fmt == "ascii":
            skip = sum(e[1] for e in elements[:fat[0]])
            if len(rows) < skip + nf:
                bad("%d face lines declared, the file ends early" % nf)
            try:
                table = [[int(v) for v in r.split()] for r in rows[skip:skip + nf]]
            except ValueError:
                bad("a face line is not a list of integers")
            if any(len(r) != 4 or r[0] != 3 for r in table):
                bad("a face is not a triangle (only lists of three indices are read)")
            tri = np.array([r[1:] for r in table], dtype=np.int64).reshape(nf, 3)
        else:
            offset = sum(e[1] * sum(np.dtype(t).itemsize for _, t in e[2]) for e in elements[:fat[0]])
            fdt = np.dtype([("n", "<" + ct), ("v", "<" + it, (3,))])
            have = min(nf, max(len(body) - offset, 0) // fdt.itemsize)
            frec = np.frombuffer(body, dtype=fdt, count=have, offset=offset)
            if np.any(frec["n"] != 3):
                bad("a face is not a triangle (only lists of three indices are read)")
            if have < nf:
                bad("%d faces of %d bytes declared, the file holds %d bytes" % (nf, fdt.itemsize, len(body) - offset))
            tri = frec["v"].astype(np.int64)
        if tri.size and (tri.min() < 0 or tri.max() >= n):
            bad("a face names a vertex outside 0..%d" % (n - 1))
    out["faces"] = np.ascontiguousarray(tri.astype(np.int32))
    return out


def frustum_volume(cam_pose, cam_intr, image_hw, depth_min, depth_max, dims, voxel_size):
    """origin (x0, y0, z0) of a ``dims`` (Z, Y, X) volume centred on the frustum of the camera ``cam_pose`` [4,4] (camera-to-world) between
    ``depth_min`` and ``depth_max``: the centre of the bounding box of the frustum's eight corners (tools/run_stream.py --fuse)."""
    P = cam_pose.detach().to("cpu", torch.float64).reshape(4, 4)
    K = cam_intr.detach().to("cpu", torch.float64).reshape(3, 3)
    h, w = image_hw
    corners = []
    for d in (depth_min, depth_max):
        for u, v in ((-0.5, -0.5), (w - 0.5, -0.5), (-0.5, h - 0.5), (w - 0.5, h - 0.5)):
            pc = torch.linalg.solve(K, torch.tensor([u, v, 1.0], dtype=torch.float64)) * d
            corners.append(P[:3, :3] @ pc + P[:3, 3])
    c = torch.stack(corners)
    centre = 0.5 * (c.min(0).values + c.max(0).values)
    half = 0.5 * float(voxel_size) * torch.tensor([dims[2], dims[1], dims[0]], dtype=torch.float64)
    return tuple(float(v) for v in (centre - half))
