"""Triangle meshes seen by a camera (csrc/mesh/mesh_raster.hip; the contract: include/estd_hip.h, estd_mesh_raster): depth, normal and
colour views of any mesh the project writes or reads, ground-truth depth maps for scenes that ship a mesh and no depth, and the
restriction of a ground-truth surface to what the cameras could see -- the step of the usual 3D protocol (Atlas, NeuralRecon,
TransformerFusion) without which completeness and recall measure the camera path and not the reconstruction.

Conventions of ``TSDFVolume.render`` and ``integrate``: pixel centres on integers, depth = the z-depth along the optical axis, poses
camera-to-world.  The rasteriser is the hot path; everything after it (attribute interpolation, counting, the visibility test) is torch
glue on the device."""
import math

import numpy as np
import torch

from . import ops
from .camera import mesh_raster_matrix
from .fusion3d import _mesh_arg, _on_device


def _hw(image_hw, what):
    if not (isinstance(image_hw, (tuple, list)) and len(image_hw) == 2 and all(isinstance(v, (int, np.integer)) and v > 0 for v in image_hw)):
        raise RuntimeError("%s: image_hw must be two positive integers (H, W), got %r" % (what, image_hw))
    return int(image_hw[0]), int(image_hw[1])


def _interpolate(attr, faces, face, bary, hit):
    """vertex attributes [V,C] at the hits: a + b1 (b - a) + b2 (c - a) per pixel, zeros elsewhere -> [H,W,C]"""
    tri = faces[face.clamp(min=0).long()].long()                                 # [H,W,3]
    a, b, c = attr[tri[..., 0]], attr[tri[..., 1]], attr[tri[..., 2]]
    out = a + bary[..., :1] * (b - a) + bary[..., 1:] * (c - a)
    return torch.where(hit[..., None], out, torch.zeros_like(out))


def render_mesh(mesh, cam_pose, cam_intr, image_hw, z_near=1e-3, normals="face", color=True):
    """One view of a triangle mesh.  ``mesh``: a dict with ``xyz`` [V,3] and ``faces`` [F,3] (what ``extract_mesh``, ``filter_mesh`` or
    ``read_ply(faces=True)`` return; numpy arrays are moved to the device), ``cam_pose`` [4,4] camera-to-world, ``cam_intr`` [3,3] in pixels
    of the ``image_hw`` = (H, W) image -> dict on the device:
      depth [H,W]    the z-depth of the nearest triangle along every pixel's ray, 0 where nothing was hit (hits at or below ``z_near`` do
                     not count; a triangle that crosses the camera plane is drawn where it lies in front)
      face [H,W]     int32, the triangle's index, -1 = nothing;  bary [H,W,2]: the perspective-correct weights of its second and third
                     vertex (the point is a + b1 (b - a) + b2 (c - a));  facing [H,W] int32: +1 where the triangle runs counter-clockwise
                     seen from the camera (``extract_mesh``'s triangles seen from the free side), -1 clockwise, 0 = nothing
      invalid        the triangles that name a vertex outside the mesh: they cover nothing
      normal [H,W,3] ``normals="face"``: the triangle's unit normal (``mesh_area``'s kernel); ``"vertex"``: the mesh's vertex normals
                     (``normal``) interpolated and normalised; None: left out
      color [H,W,3]  the vertex colours (``color``, or uint8 ``rgb`` as float32) interpolated, when ``color`` is true and the mesh has them
    Zeros where nothing was hit.  Defined to the bit (depth, face, bary, facing): the same from every call and binding."""
    what = "render_mesh"
    if normals not in ("face", "vertex", None):
        raise RuntimeError("%s: normals must be 'face', 'vertex' or None, got %r" % (what, normals))
    if normals == "vertex" and (not isinstance(mesh, dict) or mesh.get("normal") is None):
        raise RuntimeError("%s: normals='vertex' needs a mesh with vertex normals ('normal')" % what)
    H, W = _hw(image_hw, what)
    xyz, faces = _mesh_arg(mesh, what)
    mat = mesh_raster_matrix(torch.as_tensor(cam_pose).reshape(4, 4), torch.as_tensor(cam_intr).reshape(3, 3))
    depth, face, bary, facing, invalid = ops.mesh_raster(xyz, faces, mat, H, W, z_near)
    out = dict(depth=depth, face=face, bary=bary, facing=facing, invalid=int(invalid.item()))
    hit = face >= 0
    n_v = xyz.shape[0]

    def attr(v, name):
        t = _on_device(v, faces.device)
        if t.dim() != 2 or t.shape[0] != n_v or t.shape[1] != 3:
            raise RuntimeError("%s: %s must be [%d,3], got %s" % (what, name, n_v, tuple(t.shape)))
        return t
    if normals == "face":
        fn = ops.mesh_face_area(xyz, faces)[1]
        out["normal"] = torch.where(hit[..., None], fn[face.clamp(min=0).long()], torch.zeros((), device=faces.device)) if faces.shape[0] \
            else torch.zeros((H, W, 3), device=faces.device)
    elif normals == "vertex":
        out["normal"] = torch.nn.functional.normalize(_interpolate(attr(mesh["normal"], "normal"), faces, face, bary, hit), dim=-1) if faces.shape[0] \
            else torch.zeros((H, W, 3), device=faces.device)
    col = mesh.get("color") if mesh.get("color") is not None else mesh.get("rgb")
    if color and col is not None:
        out["color"] = _interpolate(attr(col, "color"), faces, face, bary, hit) if faces.shape[0] else torch.zeros((H, W, 3), device=faces.device)
    return out


def _poses(cam_poses, cam_intr, what):
    P = torch.as_tensor(cam_poses).detach().to("cpu", torch.float64).reshape(-1, 4, 4)
    K = torch.as_tensor(cam_intr).detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    if K.shape[0] not in (1, P.shape[0]):
        raise RuntimeError("%s: cam_intr must be [3,3] or one [3,3] per pose, got %d for %d poses" % (what, K.shape[0], P.shape[0]))
    return P, K


def mesh_visibility(mesh, cam_poses, cam_intr, image_hw, z_near=1e-3):
    """How much of a mesh the cameras see: one render per view (``cam_poses`` [T,4,4], ``cam_intr`` [3,3] or [T,3,3]) -> dict(pixels [F]
    int64: how many pixels each triangle owns, summed over the views; depth: the per-view depth maps [T,H,W] (what ``visible_points``
    takes); covered: the pixels that saw the mesh, per view [T] int64; invalid)."""
    what = "mesh_visibility"
    H, W = _hw(image_hw, what)
    xyz, faces = _mesh_arg(mesh, what)
    P, K = _poses(cam_poses, cam_intr, what)
    mats = mesh_raster_matrix(P, K)
    n_f = int(faces.shape[0])
    pixels = torch.zeros(n_f, device=faces.device, dtype=torch.int64)
    depths, covered, invalid = [], [], 0
    for t in range(P.shape[0]):
        depth, face, _, _, bad = ops.mesh_raster(xyz, faces, mats[t].contiguous(), H, W, z_near)
        seen = face[face >= 0].long()
        if n_f:
            pixels += torch.bincount(seen, minlength=n_f)
        depths.append(depth)
        covered.append(seen.numel())
        invalid = int(bad.item())
    depth = torch.stack(depths) if depths else torch.zeros((0, H, W), device=faces.device)
    return dict(pixels=pixels, depth=depth, covered=torch.tensor(covered, dtype=torch.int64), invalid=invalid)


def visible_points(points, depth_maps, cam_poses, cam_intr, tol, z_near=1e-3, depth_max=None):
    """In how many views a point is seen -> int32 [N] on the device.  ``points`` [N,3]; ``depth_maps`` [T,H,W]: the mesh rendered at
    ``cam_poses`` [T,4,4] / ``cam_intr`` (``mesh_visibility``'s ``depth``).  Per view, in float64 on the device: the point is projected with
    the float64-formed matrix of the rasteriser (q = M (p, 1) in the contract's order, c = q_z), its nearest pixel is (rint(q_x / c),
    rint(q_y / c)), and it is SEEN iff that pixel lies inside the image, c > z_near, c <= depth_max (when given), the rendered depth
    there is positive and c <= depth + tol: a point less than ``tol`` behind the nearest surface counts as seen."""
    what = "visible_points"
    if not (isinstance(tol, (int, float)) and math.isfinite(tol) and tol >= 0):
        raise RuntimeError("%s: tol must be finite and not negative, got %r" % (what, tol))
    if not isinstance(depth_maps, torch.Tensor) or depth_maps.dim() != 3 or not depth_maps.is_cuda:
        raise RuntimeError("%s: depth_maps must be a device tensor [T,H,W]" % what)
    dev = depth_maps.device
    pts = _on_device(points, dev)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError("%s: points must be [N,3], got %s" % (what, tuple(pts.shape)))
    P, K = _poses(cam_poses, cam_intr, what)
    if P.shape[0] != depth_maps.shape[0]:
        raise RuntimeError("%s: %d depth maps for %d poses" % (what, depth_maps.shape[0], P.shape[0]))
    T, H, W = depth_maps.shape
    mats = mesh_raster_matrix(P, K)
    x, y, z = (pts[:, i].double() for i in range(3))
    views = torch.zeros(pts.shape[0], device=dev, dtype=torch.int32)
    for t in range(T):
        M = mats[t].tolist()
        q = [((M[4 * j] * x + M[4 * j + 1] * y) + M[4 * j + 2] * z) + M[4 * j + 3] for j in range(3)]
        c = q[2]
        u, v = torch.round(q[0] / c), torch.round(q[1] / c)                      # round half to even, as rint
        ok = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (c > float(z_near))
        if depth_max is not None:
            ok &= c <= float(depth_max)
        ui, vi = torch.where(ok, u, torch.zeros_like(u)).long(), torch.where(ok, v, torch.zeros_like(v)).long()
        d = depth_maps[t].reshape(-1)[vi * W + ui].double()
        views += (ok & (d > 0) & (c <= d + float(tol))).to(torch.int32)
    return views


def visible_mask(mesh, points, cam_poses, cam_intr, image_hw, min_views=1, tol=0.05, depth_max=None, z_near=1e-3):
    """``points`` (samples of ``mesh``) seen by at least ``min_views`` of the views -> (bool mask [N], views int32 [N]); the mesh is rendered
    once per view (``mesh_visibility``) and the points are tested against those depth maps (``visible_points``)."""
    if not (isinstance(min_views, (int, np.integer)) and min_views >= 1):
        raise RuntimeError("visible_mask: min_views must be an integer >= 1, got %r" % (min_views,))
    vis = mesh_visibility(mesh, cam_poses, cam_intr, image_hw, z_near=z_near)
    views = visible_points(points, vis["depth"], cam_poses, cam_intr, tol, z_near=z_near, depth_max=depth_max)
    return views >= int(min_views), views
