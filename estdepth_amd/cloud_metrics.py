"""3D scores of a fused reconstruction on the device: nearest-neighbour distances between two point clouds (csrc/cloud_nn.hip) and the figures
reconstruction papers on ScanNet / 7-Scenes report from them (Atlas, NeuralRecon, SimpleRecon): accuracy, completeness, chamfer distance,
precision / recall / F-score at a threshold.  The clouds are what ``TSDFVolume.extract_points`` produces or ``fusion3d.read_ply`` reads.

    pred = vol.extract_points()                                        # dict(xyz, normal, ...)
    gt = fusion3d.read_ply("scene_gt.ply")
    scores = compare_clouds(pred["xyz"], torch.from_numpy(gt["xyz"]).to(dev), threshold=0.05, downsample=0.02)
    scores = vol.compare(other_volume)                                 # the same between two volumes

    grid = PointGrid(target, max_dist=1.0)                             # sort and cell table once ...
    dist, index = grid.query(points)                                   # ... any number of queries

    tri = TriangleGrid(dict(xyz=xyz, faces=faces), max_dist=1.0)       # the same for a triangle mesh (csrc/mesh/mesh_distance.hip):
    dist, face, bary = tri.query(points, bary=True)                    # the distance to the SURFACE, the face and where on it
    scores = compare_meshes(pred_mesh, gt_mesh, 1111.0, exact=True)    # surfaces scored against surfaces, not against samples

    dist, index, count = grid.knn(points, 16)                          # the 16 nearest targets (csrc/cloud/cloud_knn.hip)
    fit = estimate_normals(scan, 16, 0.05, toward=(0.0, 0.0, 1.5))     # normals of a cloud that came without: a PCA plane fit
    keep = remove_outliers(scan, k=16, std_ratio=2.0)["keep"]          # statistical outlier removal over the same search
    scores = compare_clouds(pred, scan, pred_normal=n, normals=dict(k=16))      # the side without normals gets them estimated
    near = grid.count_within(points, 0.05)                             # how many targets within 5 cm, no cap (csrc/cloud/cloud_cluster.hip)
    c = cluster_dbscan(cloud, eps=0.04, min_points=6)                  # DBSCAN: label, cluster, sizes, noise
    keep = filter_clusters(cloud, 0.04, 6, min_size=200)["keep"]       # the cloud without its floaters
    scores = compare_clouds(pred, gt, clusters=dict(eps=0.04, min_points=6, min_size=200))      # ... dropped before the scoring

The nearest-neighbour result is defined to the bit (include/estd_hip.h, estd_cloud_nearest): per query the smallest fp32
``d2 = fma(dx, dx, fma(dy, dy, dz * dz))`` over ALL targets, the smallest original index attaining it, found iff ``d2 <= max_dist^2``;
``dist = sqrt(d2)`` or ``max_dist``, ``index`` or -1.  The uniform grid behind it only decides which targets are looked at first; the cell
edge is a tuning parameter and never changes a bit of the output.  There is no CPU path.

The cell edge (``grid_plan``, ``cell=None``): two points per occupied cell of a SURFACE -- ``sqrt(2 A / n)`` with A the product of the two
largest extents of the target's bounding box -- but not below ``max_dist / 32`` (a query with no target within ``max_dist`` walks at most 32
rings).  The dense cell table is capped at 2^24 cells and 1024 cells per axis; a cell edge (the default or a given one) that would exceed
either is enlarged in steps of 1/8 until it fits.
"""
import ctypes
import math

import numpy as np
import torch

from . import ops

MAX_CELLS = ops.CLOUD_MAX_CELLS          # the dense table: cells in all
MAX_DIM = ops.CLOUD_MAX_DIM              # ... and per axis (the kernel's conservative ring bound is derived for this many)
RINGS_MAX = 32                           # the default cell is at least max_dist / RINGS_MAX
POINTS_PER_CELL = 2.0                    # the default cell aims at this many points per occupied cell of a surface


def _need(ok, msg):
    if not ok:
        raise RuntimeError(msg)


def _dims(ext, cell):
    return tuple(int(math.floor(e / cell)) + 1 for e in ext)


def grid_plan(lo, hi, n, max_dist, cell=None):
    """The grid of a target cloud with bounding box ``lo`` .. ``hi`` (three values each) and ``n`` points -> (cell, (nx, ny, nz)): the cell
    edge as the fp32 value the kernels receive and the number of cells along x, y, z, ``floor((hi - lo) / cell) + 1`` each.  ``cell=None``:
    the default rule of the module docstring.  Needs no device."""
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    _need(lo.size == 3 and hi.size == 3 and np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all(),
          "grid_plan: lo and hi must be three finite values each with lo <= hi, got %r, %r" % (lo.tolist(), hi.tolist()))
    _need(int(n) >= 1, "grid_plan: n must be at least 1, got %r" % (n,))
    max_dist = float(max_dist)
    _need(math.isfinite(max_dist) and max_dist > 0, "grid_plan: max_dist must be positive and finite, got %r" % (max_dist,))
    ext = (hi - lo).tolist()
    if cell is None:
        e = sorted(ext, reverse=True)
        cell = max(math.sqrt(POINTS_PER_CELL * e[0] * e[1] / int(n)), max_dist / RINGS_MAX)
    else:
        cell = float(cell)
        _need(math.isfinite(cell) and cell > 0, "grid_plan: cell must be positive and finite, got %r" % (cell,))
    cell = float(np.float32(cell))
    _need(cell > 0 and math.isfinite(cell), "grid_plan: the cell edge %r leaves fp32" % (cell,))
    dims = _dims(ext, cell)
    while max(dims) > MAX_DIM or dims[0] * dims[1] * dims[2] > MAX_CELLS:
        cell = float(np.float32(cell * 1.125))
        _need(math.isfinite(cell), "grid_plan: the bounding box %r .. %r is too large for fp32" % (lo.tolist(), hi.tolist()))
        dims = _dims(ext, cell)
    return cell, dims


def _check_cloud(t, name, op, device=None):
    _need(isinstance(t, torch.Tensor), "%s: %s must be a tensor" % (op, name))
    _need(t.is_cuda, "%s: %s must live on a ROCm device (estdepth_amd has no CPU path); got %s" % (op, name, t.device))
    _need(t.dtype == torch.float32, "%s: %s must be float32, got %s" % (op, name, t.dtype))
    _need(t.dim() == 2 and t.shape[1] == 3 and t.shape[0] < 2 ** 31, "%s: %s must be [n,3] with n < 2^31, got %s" % (op, name, tuple(t.shape)))
    _need(device is None or t.device == device, "%s: %s is on %s but the other cloud on %s" % (op, name, t.device, device))
    t = t.contiguous()
    _need(bool(torch.isfinite(t).all()), "%s: %s holds a coordinate that is not finite" % (op, name))
    return t


def _check_max_dist(max_dist, op):
    f32 = lambda v: ctypes.c_float(v).value
    _need(isinstance(max_dist, (int, float)) and math.isfinite(max_dist) and f32(max_dist) > 0 and math.isfinite(f32(f32(max_dist) ** 2)),
          "%s: max_dist must be positive and finite (and its square in fp32 too), got %r" % (op, max_dist))
    return float(max_dist)


def _cell_starts(sorted_keys, dims):
    """the dense cell table of a grid: cell_start[key] = how many of the (ascending) ``sorted_keys`` are smaller than ``key``, int32"""
    cells = dims[0] * dims[1] * dims[2]
    return torch.searchsorted(sorted_keys, torch.arange(cells + 1, device=sorted_keys.device, dtype=torch.int64), out_int32=True).contiguous()


def _query_order(grid, points, gridded):
    """the order a search takes its queries in: by their own cell key in ``grid`` (stable), or as they come when nothing is ``gridded``"""
    if gridded:
        return torch.sort(ops.cloud_cell_keys(points, grid.lo, grid.cell, grid.dims), stable=True)[1]
    return torch.arange(points.shape[0], device=grid.device, dtype=torch.int64)


class PointGrid:
    """The search structure of one target cloud: the stable sort by cell key, the dense cell table and the 16-byte records, built once.
    ``target`` [N,3] float32 on a ROCm device with finite coordinates (N = 0: nothing is ever found); ``cell``: the cell edge, None for the
    default rule of ``grid_plan``."""

    def __init__(self, target, max_dist, cell=None):
        self.max_dist = _check_max_dist(max_dist, "PointGrid")
        _need(cell is None or (isinstance(cell, (int, float)) and math.isfinite(cell) and cell > 0), "PointGrid: cell must be positive and finite, got %r" % (cell,))
        target = _check_cloud(target, "target", "PointGrid")
        self.device, self.n, self.target = target.device, int(target.shape[0]), target      # the cloud in its original order: ``index`` names its rows
        if self.n == 0:
            self.cell, self.dims, self.lo, self.hi = float(np.float32(self.max_dist)), (1, 1, 1), torch.zeros(3), torch.zeros(3)
            self.records = torch.empty((0, 4), device=self.device)
            self.cell_start = torch.zeros(2, device=self.device, dtype=torch.int32)
            return
        lo, hi = target.amin(0).cpu(), target.amax(0).cpu()
        self.lo, self.hi = lo.contiguous(), hi.contiguous()                                   # the cloud's box, host values
        self.cell, self.dims = grid_plan(lo.tolist(), hi.tolist(), self.n, self.max_dist, cell)
        keys = ops.cloud_cell_keys(target, self.lo, self.cell, self.dims)
        sorted_keys, order = torch.sort(keys, stable=True)
        self.cell_start = _cell_starts(sorted_keys, self.dims)
        rec = torch.empty((self.n, 4), device=self.device, dtype=torch.int32)    # filled as integers: the bits of the coordinates and the original index
        rec[:, :3] = target[order].view(torch.int32)
        rec[:, 3] = order.to(torch.int32)
        self.records = rec.view(torch.float32)

    def query(self, points, stats=False):
        """``points`` [M,3] -> (dist [M] float32, index [M] int64): the distance to and the original index of the nearest target within
        ``max_dist``; ``max_dist`` and -1 where there is none.  ``stats=True`` (measurement only) appends the candidates examined per
        query, int32 [M]."""
        points = _check_cloud(points, "points", "PointGrid.query", self.device)
        if points.shape[0] == 0:
            out = (torch.empty(0, device=self.device), torch.empty(0, device=self.device, dtype=torch.int64))
            return out + (torch.empty(0, device=self.device, dtype=torch.int32),) if stats else out
        order = _query_order(self, points, self.n > 0)
        return ops.cloud_nearest(points, order, self.records, self.cell_start, self.lo, self.cell, self.dims, self.max_dist, stats=stats)

    def knn(self, points, k, stats=False):
        """``points`` [M,3], ``k`` in 1 .. 32 -> (dist [M,k] float32, index [M,k] int32, count [M] int32): the ``k`` nearest targets within
        ``max_dist``, ascending by (d2, original index); ``count`` of them were found, the slots behind hold ``max_dist`` and -1
        (csrc/cloud/cloud_knn.hip; include/estd_hip.h, estd_cloud_knn).  Column 0 is ``query``'s result.  ``stats=True`` (measurement
        only) appends the candidates examined per query, int32 [M]."""
        _need(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= ops.CLOUD_KNN_MAX, "PointGrid.knn: k must be an integer in 1 .. %d, got %r" % (ops.CLOUD_KNN_MAX, k))
        points = _check_cloud(points, "points", "PointGrid.knn", self.device)
        if points.shape[0] == 0:
            out = (torch.empty((0, k), device=self.device), torch.empty((0, k), device=self.device, dtype=torch.int32),
                   torch.empty(0, device=self.device, dtype=torch.int32))
            return out + (torch.empty(0, device=self.device, dtype=torch.int32),) if stats else out
        order = _query_order(self, points, self.n > 0)
        return ops.cloud_knn(points, order, self.records, self.cell_start, self.lo, self.cell, self.dims, self.max_dist, k, stats=stats)

    def count_within(self, points, radius=None):
        """``points`` [M,3] -> int32 [M]: the number of targets within ``radius`` of each point (d2 <= radius^2 in fp32, inclusive; a
        point that is a target counts itself), without a cap (csrc/cloud/cloud_cluster.hip; include/estd_hip.h, estd_cloud_count_within).
        ``radius`` must not exceed the grid's ``max_dist`` (the default cell is chosen for it); None: ``max_dist``."""
        radius = self.max_dist if radius is None else _check_max_dist(radius, "PointGrid.count_within")
        _need(radius <= self.max_dist, "PointGrid.count_within: radius %g exceeds the grid's max_dist %g" % (radius, self.max_dist))
        points = _check_cloud(points, "points", "PointGrid.count_within", self.device)
        if points.shape[0] == 0:
            return torch.empty(0, device=self.device, dtype=torch.int32)
        order = _query_order(self, points, self.n > 0)
        return ops.cloud_count_within(points, order, self.records, self.cell_start, self.lo, self.cell, self.dims, radius)


def nearest(query, target, max_dist, cell=None):
    """One-shot form of ``PointGrid(target, max_dist, cell).query(query)`` -> (dist [M], index [M])."""
    _check_max_dist(max_dist, "nearest")
    _need(isinstance(query, torch.Tensor) and isinstance(target, torch.Tensor), "nearest: query and target must be tensors")
    _need(query.device == target.device, "nearest: query is on %s but the target on %s" % (query.device, target.device))
    return PointGrid(target, max_dist, cell).query(query)


def knn(query, target, k, max_dist, cell=None):
    """One-shot form of ``PointGrid(target, max_dist, cell).knn(query, k)`` -> (dist [M,k], index [M,k], count [M])."""
    _check_max_dist(max_dist, "knn")
    _need(isinstance(query, torch.Tensor) and isinstance(target, torch.Tensor), "knn: query and target must be tensors")
    _need(query.device == target.device, "knn: query is on %s but the target on %s" % (query.device, target.device))
    return PointGrid(target, max_dist, cell).knn(query, k)


def estimate_normals(points, k, max_dist, toward=None, cov=False, grid=None):
    """Normals of the cloud ``points`` [N,3] by a plane fit (PCA) over each point's ``k`` nearest neighbours within ``max_dist`` -- the
    point itself among them, as in PCL and Open3D (csrc/cloud/cloud_knn.hip; include/estd_hip.h, estd_cloud_normals) -> dict:
    normal [N,3] float32 (unit; zero where not valid), eig [N,3] float32 (the covariance's eigenvalues, ascending), curvature [N]
    float64 = l0 / (l0 + l1 + l2), the surface variation (0 where the sum is 0), valid [N] uint8 (at least 3 neighbours, l2 > 0 and
    l1 - l0 > 2^-16 l2: a plane, not a line or a ball), count [N] int32 (the neighbours found), invalid (the rows that are not valid,
    an int); with ``cov=True`` also cov [N,6] float64 (xx, xy, xz, yy, yz, zz; for tests).  ``toward``: a viewpoint (three numbers) or one
    per point [N,3] the normals are turned to; None: the component of largest magnitude is positive -- an UNORIENTED normal, which is
    what normal_consistency (an absolute cosine) and the point-to-plane metric need.  ``grid``: a ``PointGrid`` of these very points to
    search in (its ``max_dist`` then holds), None to build one."""
    op = "estimate_normals"
    _need(isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= ops.CLOUD_KNN_MAX, "%s: k must be an integer in 1 .. %d, got %r" % (op, ops.CLOUD_KNN_MAX, k))
    if grid is None:
        grid = PointGrid(points, _check_max_dist(max_dist, op))
    _need(isinstance(grid, PointGrid), "%s: grid must be a PointGrid" % op)
    points = _check_cloud(points, "points", op, grid.device)
    _need(grid.n == points.shape[0], "%s: the grid holds %d points but the cloud %d" % (op, grid.n, points.shape[0]))
    if toward is not None:
        if not isinstance(toward, torch.Tensor):
            toward = torch.from_numpy(np.ascontiguousarray(toward, dtype=np.float32))
        toward = toward.to(device=grid.device, dtype=torch.float32).contiguous()
        _need(tuple(toward.shape) in ((3,), tuple(points.shape)) and bool(torch.isfinite(toward).all()),
              "%s: toward must be three finite numbers or [%d,3], got %s" % (op, points.shape[0], tuple(toward.shape)))
    _, index, count = grid.knn(points, k)
    normal, eig, valid, invalid, c = ops.cloud_normals(grid.target, points, index, count, toward, cov=cov)
    e = eig.double()
    total = e.sum(1)
    out = dict(normal=normal, eig=eig, curvature=torch.where(total > 0, e[:, 0] / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(total)),
               valid=valid, count=count, invalid=int(invalid.item()))
    if cov:
        out["cov"] = c
    return out


def remove_outliers(points, k=16, std_ratio=2.0, max_dist=None, min_neighbours=None):
    """Statistical (and radius) outlier removal of the cloud ``points`` [N,3] over ``PointGrid.knn`` -> dict(keep [N] bool, mean_dist [N]
    float64, mu, sigma, dropped).  Per point the mean distance to the found neighbours OTHER than the point's own row (``k`` are searched,
    the point itself among them); mu and sigma (the population's: divided by the number of values) are taken over the points with at
    least one such neighbour; a point is kept where mean <= mu + ``std_ratio`` sigma, and dropped where it has no other neighbour within
    ``max_dist`` (mean_dist is ``max_dist`` there).  ``min_neighbours=n`` additionally asks for n neighbours other than itself within
    ``max_dist`` (the radius rule; needs k > n).  ``max_dist`` None: the diagonal of the cloud's box, so that every point is in reach.
    Float64 torch arithmetic over the kernel's output."""
    op = "remove_outliers"
    _need(isinstance(k, int) and not isinstance(k, bool) and 2 <= k <= ops.CLOUD_KNN_MAX, "%s: k must be an integer in 2 .. %d, got %r" % (op, ops.CLOUD_KNN_MAX, k))
    _need(isinstance(std_ratio, (int, float)) and math.isfinite(std_ratio) and std_ratio >= 0, "%s: std_ratio must be finite and not negative, got %r" % (op, std_ratio))
    _need(min_neighbours is None or (isinstance(min_neighbours, int) and 1 <= min_neighbours < k), "%s: min_neighbours must be in 1 .. k - 1, got %r" % (op, min_neighbours))
    points = _check_cloud(points, "points", op)
    n, dev = int(points.shape[0]), points.device
    if n == 0:
        return dict(keep=torch.zeros(0, device=dev, dtype=torch.bool), mean_dist=torch.zeros(0, device=dev, dtype=torch.float64), mu=0.0, sigma=0.0, dropped=0)
    if max_dist is None:
        max_dist = float((points.amax(0).double() - points.amin(0).double()).norm().item()) * (1.0 + 2.0 ** -20) or 1.0
    max_dist = _check_max_dist(max_dist, op)
    dist, index, _ = PointGrid(points, max_dist).knn(points, k)
    other = (index >= 0) & (index != torch.arange(n, device=dev, dtype=torch.int32)[:, None])
    n_other = other.sum(1)
    has = n_other > 0
    total = torch.where(other, dist.double(), torch.zeros((), device=dev, dtype=torch.float64)).sum(1)
    mean = torch.where(has, total / n_other.clamp(min=1).double(), torch.full((), float(np.float32(max_dist)), device=dev, dtype=torch.float64))
    sel = mean[has]
    mu = float(sel.mean().item()) if sel.shape[0] else 0.0
    sigma = float(sel.std(unbiased=False).item()) if sel.shape[0] else 0.0
    keep = has & (mean <= mu + float(std_ratio) * sigma)
    if min_neighbours is not None:
        keep = keep & (n_other >= min_neighbours)
    return dict(keep=keep, mean_dist=mean, mu=mu, sigma=sigma, dropped=n - int(keep.sum().item()))


def _check_min_points(min_points, op):
    _need(isinstance(min_points, int) and not isinstance(min_points, bool) and 1 <= min_points < 2 ** 31, "%s: min_points must be an integer >= 1, got %r" % (op, min_points))
    return min_points


def cluster_dbscan(points, eps, min_points=10, cell=None):
    """Density-based clustering (DBSCAN) of the cloud ``points`` [N,3] (csrc/cloud/cloud_cluster.hip; the contract, defined to the
    integer: include/estd_hip.h, estd_cloud_dbscan).  Two points are neighbours when their fp32 ``d2 <= eps^2`` (inclusive; a point is
    its own neighbour), a point with at least ``min_points`` neighbours is a CORE point, clusters are the connected components of the
    core points under that relation, a point that is not core joins the cluster of its nearest core neighbour (the smaller index among
    equals) or is noise -> dict:
    label [N] int32 (the smallest core index of the point's cluster, -1 for noise), cluster [N] int32 (-1, or a dense id 0 .. C-1, the
    clusters ordered by ascending label), count [N] int32 (the neighbours, the point among them), core [N] bool, roots [C] int64 (the
    labels, ascending), sizes [C] int32 (the points per cluster, borders included), n_clusters, noise (ints).
    The search grid is built with cell edge ``eps`` -- not ``grid_plan``'s surface default: a walk to a fixed radius visits about
    ``eps / cell + 2`` rings whatever it finds -- unless ``cell`` gives another; it never changes an output, and neither does the order
    of the rows beyond permuting the partition with them."""
    op = "cluster_dbscan"
    eps = _check_max_dist(eps, op)
    min_points = _check_min_points(min_points, op)
    _need(cell is None or (isinstance(cell, (int, float)) and math.isfinite(cell) and cell > 0), "%s: cell must be positive and finite, got %r" % (op, cell))
    points = _check_cloud(points, "points", op)
    n, dev = int(points.shape[0]), points.device
    if n == 0:
        e = lambda dtype: torch.empty(0, device=dev, dtype=dtype)
        return dict(label=e(torch.int32), cluster=e(torch.int32), count=e(torch.int32), core=e(torch.bool), roots=e(torch.int64), sizes=e(torch.int32),
                    n_clusters=0, noise=0)
    grid = PointGrid(points, eps, eps if cell is None else cell)
    label, count, size, noise = ops.cloud_dbscan(grid.records, grid.cell_start, grid.lo, grid.cell, grid.dims, eps, min_points)
    roots = torch.nonzero(size > 0).reshape(-1)
    dense = torch.full((n,), -1, device=dev, dtype=torch.int32)
    dense[roots] = torch.arange(roots.shape[0], device=dev, dtype=torch.int32)
    cluster = torch.where(label >= 0, dense[label.clamp(min=0).long()], torch.full((), -1, device=dev, dtype=torch.int32))
    return dict(label=label, cluster=cluster, count=count, core=count >= min_points, roots=roots, sizes=size[roots], n_clusters=int(roots.shape[0]),
                noise=int(noise.item()))


def _check_cluster_filter(min_size, keep_largest, op):
    for name, v in (("min_size", min_size), ("keep_largest", keep_largest)):
        _need(v is None or (isinstance(v, int) and not isinstance(v, bool) and v >= 0), "%s: %s must be None or an integer that is not negative, got %r" % (op, name, v))


def filter_clusters(points, eps, min_points=10, min_size=None, keep_largest=None, cell=None):
    """The rows of the cloud ``points`` [N,3] that belong to its large clusters (``cluster_dbscan(points, eps, min_points)``): the
    clusters with at least ``min_size`` points are kept (None: every cluster), and with ``keep_largest=k`` only the k of them with the
    most points (ties go to the smaller label).  Noise is always dropped.  -> dict(keep [N] bool, cluster [N] int32 and sizes [C] as
    ``cluster_dbscan`` returns them, n_clusters, clusters_kept, kept / dropped: the points kept / dropped, noise: the noise points among
    the dropped).  What ``fusion3d.filter_mesh`` does for a mesh by its connectivity; the mask is torch glue over the kernels' labels."""
    op = "filter_clusters"
    _check_cluster_filter(min_size, keep_largest, op)
    c = cluster_dbscan(points, eps, min_points, cell)
    sizes, dev = c["sizes"], c["cluster"].device
    keep_c = sizes >= (0 if min_size is None else min_size)
    if keep_largest is not None:
        at = torch.nonzero(keep_c).reshape(-1)                                  # by ascending label: the stable sort settles ties that way
        order = torch.sort(sizes[at].to(torch.int64), descending=True, stable=True)[1]
        keep_c = torch.zeros_like(keep_c)
        keep_c[at[order[:keep_largest]]] = True
    keep = (c["cluster"] >= 0) & torch.cat([keep_c, torch.zeros(1, device=dev, dtype=torch.bool)])[c["cluster"].long()]
    kept = int(keep.sum().item())
    return dict(keep=keep, cluster=c["cluster"], sizes=sizes, n_clusters=c["n_clusters"], clusters_kept=int(keep_c.sum().item()), kept=kept,
                dropped=int(keep.shape[0]) - kept, noise=c["noise"])


CLUSTERS_KEYS = ("eps", "min_points", "min_size", "keep_largest", "sides")


def _clusters_arg(clusters, op):
    """``clusters=dict(eps, min_points=10, min_size=None, keep_largest=None, sides=("pred",))`` -> (filter_clusters' arguments, sides)"""
    _need(isinstance(clusters, dict) and "eps" in clusters and all(k in CLUSTERS_KEYS for k in clusters),
          "%s: clusters must be a dict with eps and optionally %s" % (op, ", ".join(CLUSTERS_KEYS[1:])))
    sides = clusters.get("sides", ("pred",))
    sides = (sides,) if isinstance(sides, str) else tuple(sides)
    _need(len(sides) > 0 and all(s in ("pred", "gt") for s in sides), "%s: clusters['sides'] must name 'pred', 'gt' or both, got %r" % (op, sides))
    kw = dict(eps=_check_max_dist(clusters["eps"], op + " (clusters['eps'])"),
              min_points=_check_min_points(10 if clusters.get("min_points") is None else clusters["min_points"], op + " (clusters)"),
              min_size=clusters.get("min_size"), keep_largest=clusters.get("keep_largest"))
    _check_cluster_filter(kw["min_size"], kw["keep_largest"], op + " (clusters)")
    return kw, sides


def _drop_floaters(xyz, cols, kw):
    """one side of a comparison through ``filter_clusters`` -> (the rows kept, the per-point tensors ``cols`` (a dict; None entries
    pass) alike, the side's entry of the ``clusters`` block)"""
    f = filter_clusters(xyz, **kw)
    keep = f["keep"]
    return (xyz[keep].contiguous(), {k: (v if v is None else v[keep].contiguous()) for k, v in cols.items()},
            dict(n_clusters=f["n_clusters"], kept=f["kept"], dropped=f["dropped"], noise=f["noise"]))


NORMALS_KEYS = ("k", "radius")


def _normals_arg(normals, threshold, op):
    """``normals=dict(k=16, radius=None)`` -> (k, radius): ``radius`` None is ``threshold``"""
    _need(isinstance(normals, dict) and all(key in NORMALS_KEYS for key in normals), "%s: normals must be a dict with keys among %s" % (op, ", ".join(NORMALS_KEYS)))
    k = 16 if normals.get("k") is None else normals["k"]
    _need(isinstance(k, int) and not isinstance(k, bool) and 3 <= k <= ops.CLOUD_KNN_MAX, "%s: normals['k'] must be an integer in 3 .. %d, got %r" % (op, ops.CLOUD_KNN_MAX, k))
    radius = threshold if normals.get("radius") is None else normals["radius"]
    return k, _check_max_dist(radius, op + " (normals['radius'])")


MAX_PAIRS =ops.MESH_DISTANCE_MAX_PAIRS      # the (cell, face) pairs of a TriangleGrid
BIG_CELLS = ops.MESH_DISTANCE_BIG_CELLS      # a triangle whose box covers more cells goes on the big list


class TriangleGrid:
    """The search structure of one triangle mesh for point-to-SURFACE distances (csrc/mesh/mesh_distance.hip; the contract:
    include/estd_hip.h, estd_mesh_nearest): every valid triangle registered in the cells its bounding box covers, the 48-byte records in
    cell order, and the big list of the triangles whose box covers more than ``big_cells`` cells, which every query tests in full.
    ``mesh``: a dict with ``xyz`` [V,3] and ``faces`` [F,3] (device tensors or numpy arrays).  A face with an index outside [0, V), with a
    vertex that is not finite or without area in fp32 is ignored and counted: ``.invalid``; ``.faces_valid`` are the others.
    ``cell``: the cell edge; None: ``sqrt(2 x the median area)`` of the triangles with an area -- about their edge, and the median so
    that two wall-sized triangles among thousands of small ones do not set it: they go on the big list -- and not below
    ``max_dist / 32``; ``math.inf``: no grid, every valid triangle on the big list.  ``big_cells``: None for the default (64), 0 forces
    the big list as well, "grid" forces every triangle into the grid.  The caps of ``grid_plan`` hold, and at most 2^23 pairs: a cell
    edge that exceeds one grows in steps of 1/8.  None of this changes a bit of a result: the structure only decides what is looked at
    first."""

    def __init__(self, mesh, max_dist, cell=None, big_cells=None):
        from . import fusion3d
        op = "TriangleGrid"
        self.max_dist = _check_max_dist(max_dist, op)
        _need(cell is None or (isinstance(cell, (int, float)) and not math.isnan(cell) and cell > 0), "%s: cell must be positive (math.inf: the big list only), got %r" % (op, cell))
        _need(big_cells is None or big_cells == "grid" or (isinstance(big_cells, int) and 0 <= big_cells < 2 ** 31),
              "%s: big_cells must be None, 'grid' or a count in 0 .. 2^31 - 1, got %r" % (op, big_cells))
        _need(isinstance(mesh, dict) and mesh.get("xyz") is not None and mesh.get("faces") is not None, "%s: the mesh must be a dict with 'xyz' and 'faces'" % op)
        devs = [v.device for v in mesh.values() if isinstance(v, torch.Tensor) and v.is_cuda]
        faces = fusion3d._faces_arg(mesh["faces"], op, devs[0] if devs else None)
        _need(faces.dtype == torch.int32, "%s: faces must be int32, got %s" % (op, faces.dtype))
        xyz = fusion3d._on_device(mesh["xyz"], faces.device)
        _need(xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.shape[0] < 2 ** 31, "%s: xyz must be [V,3] with V < 2^31, got %s" % (op, tuple(xyz.shape)))
        _need(faces.shape[0] <= (2 ** 31 - 1) // 3, "%s: at most %d faces, got %d" % (op, (2 ** 31 - 1) // 3, faces.shape[0]))
        self.device, self.xyz, self.faces = faces.device, xyz, faces
        dev, V, F = self.device, int(xyz.shape[0]), int(faces.shape[0])
        self.cell, self.dims, self.lo, self.hi = float(np.float32(self.max_dist)), (1, 1, 1), torch.zeros(3), torch.zeros(3)
        self.big_cells = 0 if (cell is not None and math.isinf(cell)) else BIG_CELLS if big_cells is None else big_cells
        self.records = self.big_records = torch.empty((0, 12), device=dev)
        self.cell_start = torch.zeros(2, device=dev, dtype=torch.int32)
        self.invalid, self.faces_valid, self.n_pairs, self.n_big = F, 0, 0, 0
        # the box and the mean area of the faces that can be valid (indices in range, finite vertices): tuning only, by torch
        ok = ((faces >= 0) & (faces < V)).all(1) if F else torch.zeros(0, device=dev, dtype=torch.bool)
        tri = xyz[faces[ok].long()] if F else xyz.new_empty((0, 3, 3))                              # [K,3,3]
        tri = tri[torch.isfinite(tri).all(2).all(1)]
        if tri.shape[0] == 0:
            if F:
                self.invalid = int(ops.mesh_tri_bins(xyz, faces, self.lo, self.cell, self.dims, 0)[2].item())
                self.faces_valid = F - self.invalid
            return
        lo, hi = tri.amin((0, 1)).cpu(), tri.amax((0, 1)).cpu()
        self.lo, self.hi = lo.contiguous(), hi.contiguous()                                   # the box of the faces that can be valid, host values
        if cell is not None and math.isinf(cell):
            cell = None
        if cell is None:
            area = 0.5 * torch.linalg.cross(tri[:, 1].double() - tri[:, 0].double(), tri[:, 2].double() - tri[:, 0].double()).norm(dim=1)
            area = area[torch.isfinite(area) & (area > 0)]
            typical = float(area.median().item()) if area.shape[0] else 0.0
            cell = max(math.sqrt(2.0 * typical), self.max_dist / RINGS_MAX, float(np.finfo(np.float32).tiny))
            cell = min(cell, float(np.finfo(np.float32).max) / 4)
        big = MAX_CELLS if self.big_cells == "grid" else int(self.big_cells)
        self.cell, self.dims = grid_plan(lo.tolist(), hi.tolist(), 1, self.max_dist, cell)
        while True:
            count, flag, invalid = ops.mesh_tri_bins(xyz, faces, self.lo, self.cell, self.dims, big)
            cum = torch.cumsum(count.to(torch.int64), 0)
            pairs = int(cum[-1].item())
            if pairs <= MAX_PAIRS:
                break
            _need(self.dims != (1, 1, 1), "%s: %d triangles for the grid, at most %d pairs" % (op, pairs, MAX_PAIRS))
            self.cell, self.dims = grid_plan(lo.tolist(), hi.tolist(), 1, self.max_dist, self.cell * 1.125)
        self.invalid = int(invalid.item())
        self.faces_valid = F - self.invalid
        self.n_pairs = pairs
        big_faces = torch.nonzero(flag == 2).reshape(-1)
        self.n_big = int(big_faces.shape[0])
        self.big_records = self._records(big_faces)
        if pairs:
            keys, pair_face = ops.mesh_tri_fill(xyz, faces, self.lo, self.cell, self.dims, big, (cum - count).contiguous(), pairs)
            sorted_keys, order = torch.sort(keys, stable=True)
            self.cell_start = _cell_starts(sorted_keys, self.dims)
            self.records = self._records(pair_face[order].long())
        else:
            self.cell, self.dims = float(np.float32(self.max_dist)), (1, 1, 1)                    # no grid: phase B does not run

    def _records(self, face):
        """the 48-byte records of the faces ``face`` (int64, all valid), gathered here once: the search loads a candidate with three
        16-byte loads and follows no index"""
        rec = torch.zeros((face.shape[0], 12), device=self.device, dtype=torch.int32)
        if face.shape[0]:
            rec[:, :9] = self.xyz[self.faces[face].long()].reshape(-1, 9).view(torch.int32)
            rec[:, 9] = face.to(torch.int32)
        return rec.view(torch.float32)

    def query(self, points, bary=False, closest=False):
        """``points`` [M,3] (finite) -> (dist [M] float32, face [M] int32[, bary [M,2]][, closest [M,3]]): the distance to the nearest
        point of the mesh within ``max_dist`` and the face it lies on, the barycentric pair (v, w) of that point (it is
        a + v (b - a) + w (c - a)) and the point; ``max_dist``, -1 and zeros where there is none."""
        points = _check_cloud(points, "points", "TriangleGrid.query", self.device)
        M = int(points.shape[0])
        if M == 0 or self.faces_valid == 0:                       # nothing to search: no launch
            out = (torch.full((M,), float(np.float32(self.max_dist)), device=self.device), torch.full((M,), -1, device=self.device, dtype=torch.int32))
            return out + ((torch.zeros((M, 2), device=self.device),) if bary else ()) + ((torch.zeros((M, 3), device=self.device),) if closest else ())
        order = _query_order(self, points, self.n_pairs > 0)
        dist, face, b, c = ops.mesh_nearest(points, order, self.big_records, self.records, self.cell_start, self.lo, self.cell, self.dims,
                                            self.max_dist, bary=bary, closest=closest)
        return (dist, face) + ((b,) if bary else ()) + ((c,) if closest else ())


def point_mesh_distance(points, mesh, max_dist, cell=None):
    """One-shot form of ``TriangleGrid(mesh, max_dist, cell).query(points)`` -> (dist [M], face [M])."""
    return TriangleGrid(mesh, max_dist, cell).query(points)


def voxel_downsample(points, cell, attrs=None):
    """Voxel-grid down-sampling: one point per occupied cell of edge ``cell`` (the grid starts at the cloud's bounding-box minimum), the mean
    of the cell's points -> (points [K,3], attrs [K,C] or None, counts [K] int64), cells in ascending key order (z, then y, then x).
    ``attrs`` [N,C], C <= 6 (normals, colour) are averaged the same way.  Sums run in float64 in the original order of the points and are
    rounded to fp32 once: the result is the same for every call."""
    _need(isinstance(cell, (int, float)) and math.isfinite(cell) and float(np.float32(cell)) > 0, "voxel_downsample: cell must be positive and finite, got %r" % (cell,))
    points = _check_cloud(points, "points", "voxel_downsample")
    n = points.shape[0]
    if attrs is not None:
        _need(isinstance(attrs, torch.Tensor) and attrs.dtype == torch.float32 and attrs.dim() == 2 and attrs.shape[0] == n
              and 1 <= attrs.shape[1] <= ops.CLOUD_MAX_ATTRS and attrs.device == points.device,
              "voxel_downsample: attrs must be float32 [%d,C] with 1 <= C <= %d on the points' device" % (n, ops.CLOUD_MAX_ATTRS))
        attrs = attrs.contiguous()
    if n == 0:
        return points, attrs, torch.empty(0, device=points.device, dtype=torch.int64)
    lo, hi = points.amin(0).cpu(), points.amax(0).cpu()
    cell = float(np.float32(cell))
    dims = _dims((hi.double() - lo.double()).tolist(), cell)
    _need(max(dims) <= ops.CLOUD_KEY_MAX_DIM, "voxel_downsample: %r cells per axis (at most %d): the cell %g is too small for this cloud" % (dims, ops.CLOUD_KEY_MAX_DIM, cell))
    keys = ops.cloud_cell_keys(points, lo.contiguous(), cell, dims)
    sorted_keys, order = torch.sort(keys, stable=True)
    _, counts = torch.unique_consecutive(sorted_keys, return_counts=True)
    segments = torch.zeros(counts.shape[0] + 1, device=points.device, dtype=torch.int64)
    segments[1:] = torch.cumsum(counts, 0)
    out, out_attrs = ops.cloud_cell_centroids(points, attrs, order.contiguous(), segments)
    return out, out_attrs, counts


def _side(dist, index, max_dist, threshold):
    """the figures of one direction from the clamped distances"""
    n = int(dist.shape[0])
    d64 = dist.double()
    return dict(mean=float(d64.mean().item()) if n else 0.0, median=float(d64.median().item()) if n else 0.0,
                share=float((dist < threshold).double().mean().item()) if n else 0.0, clamped=int((index < 0).sum().item()))


ALIGN_KEYS = ("metric", "dist_max", "max_iter", "init", "voxel", "hypotheses", "seed")


def _align(src, src_normal, target, target_normal, align, threshold, op):
    """``align=dict(metric="plane", dist_max=(8, 4, 2) x threshold, max_iter=30, init=None)``: register the predicted points ``src`` to the
    ground truth (registration.register) -> (T float64 [4,4] or None when the registration did not converge, the ``alignment`` block).
    ``init="global"`` with ``voxel=V`` (and optionally ``hypotheses``, ``seed``) starts from ``registration.register_global``: the block
    gains ``global`` = dict(fitness, count, pairs, hypothesis, T_global); a winner refused for its inliers ends the alignment there."""
    from . import registration
    _need(isinstance(align, dict) and all(k in ALIGN_KEYS for k in align), "%s: align must be a dict with keys among %s" % (op, ", ".join(ALIGN_KEYS)))
    _need(isinstance(threshold, (int, float)) and math.isfinite(threshold) and threshold > 0, "%s: threshold must be positive and finite, got %r" % (op, threshold))
    dist = align.get("dist_max")
    init, first = align.get("init"), None
    is_global = isinstance(init, str)
    _need(is_global or not any(k in align for k in ("voxel", "hypotheses", "seed")), "%s: align's voxel, hypotheses and seed go with init='global'" % op)
    if is_global:
        _need(init == "global" and align.get("voxel") is not None, "%s: align's init must be a [4,4] transform or 'global' with voxel=V, got %r" % (op, init))
        whole = dict(xyz=target.xyz, faces=target.faces) if isinstance(target, TriangleGrid) else target.target
        g = registration.register_global(src, whole, align["voxel"], src_normal=src_normal, target_normal=target_normal,
                                         hypotheses=align.get("hypotheses", 65536), seed=align.get("seed", 0), refine=None)
        first = dict(fitness=float(g["fitness"]), count=int(g["count"]), pairs=int(g["pairs"]), hypothesis=int(g["hypothesis"]),
                     T_global=[float(v) for v in g["T_global"].reshape(-1)])
        init = g["T_global"]
        if g["reason"] == "inliers":
            eye = [float(v) for v in np.eye(4).reshape(-1)]
            return None, {"T": eye, "correction": [0.0, 0.0], "rmse": 0.0, "overlap": 0.0, "iterations": 0, "converged": False, "reason": "inliers",
                          "global": first}
    out = registration.register(src, target, init=init, metric=align.get("metric", "plane"),
                                dist_max=tuple(k * threshold for k in (8.0, 4.0, 2.0)) if dist is None else dist,
                                max_iter=30 if align.get("max_iter") is None else align["max_iter"], target_normal=target_normal)
    block = dict(T=[float(v) for v in out["T"].reshape(-1)], correction=[float(v) for v in out["correction"]], rmse=float(out["rmse"]),
                 overlap=float(out["overlap"]), iterations=int(out["iterations"]), converged=bool(out["converged"]), reason=out["reason"])
    if first is not None:
        block["global"] = first
    return (out["T"] if out["converged"] else None), block


def compare_clouds(pred, gt, threshold=0.05, max_dist=None, downsample=None, pred_normal=None, gt_normal=None, pred_color=None, gt_color=None,
                   cell=None, align=None, normals=None, clusters=None):
    """The 3D scores of the cloud ``pred`` [P,3] against ``gt`` [G,3] (float32, one ROCm device, finite) -> dict of floats / ints:

    accuracy / completeness: the mean distance pred -> gt / gt -> pred, each distance clamped to ``max_dist`` (default 20 ``threshold``);
    chamfer: their mean;  precision / recall: the share of pred / gt with dist < ``threshold``;  fscore = 2 P R / (P + R), 0 when both are 0;
    accuracy_median, completeness_median (torch.median: the lower of two middle values);  n_pred, n_gt;  clamped_pred, clamped_gt: the points with no neighbour within ``max_dist``, which
    enter the means as ``max_dist`` -- with any, the means are lower bounds.  With both normals: normal_consistency = the mean
    |n_pred . n_gt[index]| over found pairs, both directions averaged.  With both colours: color_l1 = the mean absolute colour difference at
    the nearest neighbour over pairs with dist < ``threshold``, both directions averaged.  ``downsample``: a voxel edge -- both clouds (and
    their normals / colours) go through ``voxel_downsample`` first, as evaluation protocols do (2 cm in Atlas's).  An empty cloud gives
    zeros for its own means and shares.  Means are float64 sums by torch; ``cell`` is the search grid's edge (None: the default).
    ``align=dict(metric="plane", dist_max=None, max_iter=30, init=None)`` registers ``pred`` to ``gt`` first (registration.register; the
    plane metric needs ``gt_normal``; ``dist_max`` defaults to 8, 4 and 2 thresholds) and scores the moved prediction, its normals
    rotated; the result gains ``alignment`` = dict(T: 16 numbers row by row, correction, rmse, overlap, iterations, converged, reason).  A
    registration that did not converge is reported there and the UNMOVED prediction is scored.  With the default None nothing of this runs.
    ``normals=dict(k=16, radius=None)``: whichever side comes without normals gets them from its own points (``estimate_normals`` over
    the ``k`` nearest neighbours within ``radius``, None: ``threshold``; after ``downsample``; unoriented).  Rows the estimate finds not
    valid leave the normal_consistency pairs, and with ``align`` and the plane metric a ground truth without normals is registered to
    through its valid rows only (estimated before the down-sampling, on the cloud the registration sees).  The result gains ``normals`` =
    dict(k, radius, estimated: the sides among "pred", "gt", invalid_pred, invalid_gt).  With the default None nothing of this runs.
    ``clusters=dict(eps, min_points=10, min_size=None, keep_largest=None, sides=("pred",))``: the named sides lose their floaters FIRST
    (``filter_clusters`` on the cloud as it came, its normals and colours carried along); alignment, normal estimation and
    down-sampling see the filtered cloud.  The result gains ``clusters`` = dict(side: dict(n_clusters, kept, dropped, noise)).  With the
    default None nothing of this runs and every result is the same bits as before."""
    _need(isinstance(threshold, (int, float)) and math.isfinite(threshold) and threshold > 0, "compare_clouds: threshold must be positive and finite, got %r" % (threshold,))
    if max_dist is None:
        max_dist = 20.0 * threshold
    max_dist = _check_max_dist(max_dist, "compare_clouds")
    _need(threshold <= max_dist, "compare_clouds: threshold %g must not exceed max_dist %g" % (threshold, max_dist))
    _need(downsample is None or (isinstance(downsample, (int, float)) and math.isfinite(downsample) and downsample > 0),
          "compare_clouds: downsample must be a positive voxel edge, got %r" % (downsample,))
    _need(isinstance(pred, torch.Tensor) and isinstance(gt, torch.Tensor), "compare_clouds: pred and gt must be tensors")
    _need(pred.device == gt.device, "compare_clouds: pred is on %s but gt on %s" % (pred.device, gt.device))
    pred, gt = _check_cloud(pred, "pred", "compare_clouds"), _check_cloud(gt, "gt", "compare_clouds", pred.device)
    attrs = {}
    for name, cloud, a in (("pred_normal", pred, pred_normal), ("gt_normal", gt, gt_normal), ("pred_color", pred, pred_color), ("gt_color", gt, gt_color)):
        if a is not None:
            _need(isinstance(a, torch.Tensor) and a.dtype == torch.float32 and tuple(a.shape) == tuple(cloud.shape) and a.device == cloud.device,
                  "compare_clouds: %s must be float32 %s on the cloud's device" % (name, tuple(cloud.shape)))
            attrs[name] = a.contiguous()
    dropped = None
    if clusters is not None:
        kw, sides = _clusters_arg(clusters, "compare_clouds")
        dropped = {}
        for side in ("pred", "gt"):
            if side in sides:
                names = [k for k in (side + "_normal", side + "_color") if k in attrs]
                cloud, cols, dropped[side] = _drop_floaters(pred if side == "pred" else gt, {k: attrs[k] for k in names}, kw)
                attrs.update(cols)
                if side == "pred":
                    pred = cloud
                else:
                    gt = cloud
    alignment = None
    est, rows_ok, early = None, {}, None
    if normals is not None:
        nk, nr = _normals_arg(normals, threshold, "compare_clouds")
        est = dict(k=nk, radius=nr, estimated=[], invalid_pred=0, invalid_gt=0)
    if align is not None:
        from . import registration
        tgt, tgt_normal = gt, attrs.get("gt_normal")
        if est is not None and tgt_normal is None and isinstance(align, dict) and align.get("metric", "plane") == "plane":
            early = estimate_normals(gt, nk, nr)                              # the registration's target: the valid rows of the cloud as it came
            ok = early["valid"].bool()
            tgt, tgt_normal = gt[ok].contiguous(), early["normal"][ok].contiguous()
        T, alignment = _align(pred, attrs.get("pred_normal"), PointGrid(tgt, _align_reach(align, threshold)), tgt_normal, align, threshold,
                              "compare_clouds")
        if T is not None:
            moved = registration.transform(pred, T, attrs.get("pred_normal"))
            if "pred_normal" in attrs:
                pred, attrs["pred_normal"] = moved
            else:
                pred = moved
    if downsample is not None:
        for side, cloud in (("pred", pred), ("gt", gt)):
            cols = [attrs[k] for k in (side + "_normal", side + "_color") if k in attrs]
            pts, att, _ = voxel_downsample(cloud, downsample, torch.cat(cols, 1) if cols else None)
            for j, k in enumerate(k for k in (side + "_normal", side + "_color") if k in attrs):
                attrs[k] = att[:, 3 * j:3 * j + 3].contiguous()
            if side == "pred":
                pred = pts
            else:
                gt = pts
    if est is not None:
        for side, cloud in (("pred", pred), ("gt", gt)):
            if side + "_normal" not in attrs:
                e = early if (side == "gt" and early is not None and downsample is None) else estimate_normals(cloud, nk, nr)
                attrs[side + "_normal"], rows_ok[side] = e["normal"], e["valid"].bool()
                est["estimated"].append(side)
                est["invalid_" + side] = e["invalid"]
    thr32 = float(np.float32(threshold))
    d_pg, i_pg = PointGrid(gt, max_dist, cell).query(pred)
    d_gp, i_gp = PointGrid(pred, max_dist, cell).query(gt)
    a, c = _side(d_pg, i_pg, max_dist, thr32), _side(d_gp, i_gp, max_dist, thr32)
    P, R = a["share"], c["share"]
    out = dict(accuracy=a["mean"], completeness=c["mean"], chamfer=0.5 * (a["mean"] + c["mean"]), precision=P, recall=R,
               fscore=2.0 * P * R / (P + R) if P + R > 0 else 0.0, accuracy_median=a["median"], completeness_median=c["median"],
               n_pred=int(pred.shape[0]), n_gt=int(gt.shape[0]), clamped_pred=a["clamped"], clamped_gt=c["clamped"])

    def pairs(src, dst, dist, index, fn, keep):
        m = keep(dist, index)
        if not bool(m.any()):
            return None
        return float(fn(src[m].double(), dst[index[m]].double()).mean().item())

    if "pred_normal" in attrs and "gt_normal" in attrs:
        dot = lambda x, y: (x * y).sum(1).abs()
        found = lambda dist, index: index >= 0

        def found_valid(src, dst):
            """found pairs whose estimated normals are valid on both ends (a side with given normals has no mask)"""
            def keep(dist, index):
                m = index >= 0
                if src in rows_ok:
                    m = m & rows_ok[src]
                if dst in rows_ok:
                    m = m & rows_ok[dst][index.clamp(min=0)]
                return m
            return keep if rows_ok else found
        v = [x for x in (pairs(attrs["pred_normal"], attrs["gt_normal"], d_pg, i_pg, dot, found_valid("pred", "gt")),
                         pairs(attrs["gt_normal"], attrs["pred_normal"], d_gp, i_gp, dot, found_valid("gt", "pred"))) if x is not None]
        out["normal_consistency"] = sum(v) / len(v) if v else 0.0
    if "pred_color" in attrs and "gt_color" in attrs:
        l1 = lambda x, y: (x - y).abs().mean(1)
        near = lambda dist, index: (index >= 0) & (dist < thr32)
        v = [x for x in (pairs(attrs["pred_color"], attrs["gt_color"], d_pg, i_pg, l1, near),
                         pairs(attrs["gt_color"], attrs["pred_color"], d_gp, i_gp, l1, near)) if x is not None]
        out["color_l1"] = sum(v) / len(v) if v else 0.0
    if alignment is not None:
        out["alignment"] = alignment
    if est is not None:
        out["normals"] = est
    if dropped is not None:
        out["clusters"] = dropped
    return out


def _align_reach(align, threshold):
    """the largest distance the registration of ``align`` looks for partners at: what its search structure is built for"""
    d = align.get("dist_max") if isinstance(align, dict) else None
    if d is None:
        return 8.0 * threshold
    return float(d) if isinstance(d, (int, float)) else max(float(v) for v in d)


VISIBLE_KEYS = ("cam_poses", "cam_intr", "image_hw", "min_views", "tol", "depth_max", "z_near")


def restrict_to_visible(mesh, cloud, visible, threshold, op):
    """The samples ``cloud`` (a dict of per-point tensors with ``xyz``) of the ground-truth ``mesh`` that at least ``min_views`` of the
    cameras in ``visible`` saw (mesh_render.visible_mask) -> (the restricted dict, n before, n after).  ``tol`` defaults to ``threshold``:
    a point hidden less than the matching distance behind another surface is one the metric would match anyway."""
    from . import mesh_render
    _need(isinstance(visible, dict) and all(k in visible for k in VISIBLE_KEYS[:3]) and all(k in VISIBLE_KEYS for k in visible),
          "%s: visible must be a dict with cam_poses, cam_intr, image_hw and optionally min_views, tol, depth_max, z_near" % op)
    _need(isinstance(mesh, dict) and mesh.get("faces") is not None,
          "%s: visible= needs a ground truth with faces (a triangle mesh): a point cloud cannot be rendered" % op)
    tol = visible.get("tol")
    keep, _ = mesh_render.visible_mask(mesh, cloud["xyz"], visible["cam_poses"], visible["cam_intr"], visible["image_hw"],
                                       min_views=visible.get("min_views", 1), tol=float(threshold if tol is None else tol),
                                       depth_max=visible.get("depth_max"), z_near=visible.get("z_near", 1e-3))
    n = int(cloud["xyz"].shape[0])
    out = {k: (v[keep].contiguous() if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == n else v) for k, v in cloud.items()}
    return out, n, int(out["xyz"].shape[0])


def _exact_scores(a, b, pred, gt, dev, threshold, max_dist, downsample, cell):
    """compare_meshes(exact=True) behind the sampling: the clouds ``a`` (of pred) and ``b`` (of gt, already restricted) are the QUERIES,
    the meshes the targets -> the dict of compare_clouds plus ``exact``"""
    from . import fusion3d
    _need(isinstance(threshold, (int, float)) and math.isfinite(threshold) and threshold > 0, "compare_meshes: threshold must be positive and finite, got %r" % (threshold,))
    max_dist = _check_max_dist(20.0 * threshold if max_dist is None else max_dist, "compare_meshes")
    _need(threshold <= max_dist, "compare_meshes: threshold %g must not exceed max_dist %g" % (threshold, max_dist))
    _need(downsample is None or (isinstance(downsample, (int, float)) and math.isfinite(downsample) and downsample > 0),
          "compare_meshes: downsample must be a positive voxel edge, got %r" % (downsample,))
    both = lambda k: k in a and k in b
    dev = a["xyz"].device
    clouds = []
    for s in (a, b):
        q = {k: s[k] for k in ("xyz", "normal", "color") if k in s and (k == "xyz" or both(k))}
        q["xyz"] = _check_cloud(q["xyz"], "xyz", "compare_meshes", dev)
        if downsample is not None:
            names = [k for k in ("normal", "color") if k in q]
            pts, att, _ = voxel_downsample(q["xyz"], downsample, torch.cat([q[k] for k in names], 1) if names else None)
            q = dict(xyz=pts, **{k: att[:, 3 * j:3 * j + 3].contiguous() for j, k in enumerate(names)})
        clouds.append(q)
    qa, qb = clouds

    def towards(query, cloud, mesh):
        """the distances of ``query`` to the target (its mesh where it has faces, else its cloud) -> (dist, index, the target's normal and
        colour at the nearest point or None, the grid)"""
        if mesh.get("faces") is None:
            dist, index = PointGrid(cloud["xyz"], max_dist, cell).query(query["xyz"])
            at = lambda k: cloud[k][index.clamp(min=0)] if k in cloud else None
            return dist, index, at("normal"), at("color"), None
        grid = TriangleGrid(mesh, max_dist, cell)
        dist, face, bary = grid.query(query["xyz"], bary=True)
        f = face.clamp(min=0).long()
        normal = ops.mesh_face_area(grid.xyz, grid.faces)[1][f] if "normal" in query else None      # sample_mesh(normals="face")'s normal
        color = None
        if "color" in query:
            c = mesh.get("color") if mesh.get("color") is not None else mesh.get("rgb")
            c = fusion3d._on_device(c, dev)[grid.faces[f].clamp(0, max(grid.xyz.shape[0] - 1, 0)).long()]      # [M,3,3]: the three vertices' colours
            color = c[:, 0] + bary[:, :1] * (c[:, 1] - c[:, 0]) + bary[:, 1:] * (c[:, 2] - c[:, 0])
        return dist, face, normal, color, grid
    d_pg, i_pg, n_pg, c_pg, grid_gt = towards(qa, b, gt)
    d_gp, i_gp, n_gp, c_gp, grid_pred = towards(qb, a, pred)
    thr32 = float(np.float32(threshold))
    sa, sc = _side(d_pg, i_pg, max_dist, thr32), _side(d_gp, i_gp, max_dist, thr32)
    P, R = sa["share"], sc["share"]
    out = dict(accuracy=sa["mean"], completeness=sc["mean"], chamfer=0.5 * (sa["mean"] + sc["mean"]), precision=P, recall=R,
               fscore=2.0 * P * R / (P + R) if P + R > 0 else 0.0, accuracy_median=sa["median"], completeness_median=sc["median"],
               n_pred=int(qa["xyz"].shape[0]), n_gt=int(qb["xyz"].shape[0]), clamped_pred=sa["clamped"], clamped_gt=sc["clamped"])

    def pairs(src, dst, keep, fn):
        return float(fn(src[keep].double(), dst[keep].double()).mean().item()) if bool(keep.any()) else None
    if both("normal"):
        dot = lambda x, y: (x * y).sum(1).abs()
        v = [x for x in (pairs(qa["normal"], n_pg, i_pg >= 0, dot), pairs(qb["normal"], n_gp, i_gp >= 0, dot)) if x is not None]
        out["normal_consistency"] = sum(v) / len(v) if v else 0.0
    if both("color"):
        l1 = lambda x, y: (x - y).abs().mean(1)
        v = [x for x in (pairs(qa["color"], c_pg, (i_pg >= 0) & (d_pg < thr32), l1), pairs(qb["color"], c_gp, (i_gp >= 0) & (d_gp < thr32), l1)) if x is not None]
        out["color_l1"] = sum(v) / len(v) if v else 0.0
    out["exact"] = dict(faces_pred=None if grid_pred is None else grid_pred.faces_valid, faces_gt=None if grid_gt is None else grid_gt.faces_valid,
                        invalid_pred=0 if grid_pred is None else grid_pred.invalid, invalid_gt=0 if grid_gt is None else grid_gt.invalid)
    return out


def compare_meshes(pred, gt, density, threshold=0.05, max_dist=None, downsample=None, seed=0, cell=None, visible=None, exact=False, align=None,
                   normals=None, clusters=None):
    """The 3D scores of the SURFACE ``pred`` against the surface ``gt``: both triangle meshes (dicts with ``xyz`` and ``faces``: what
    ``extract_mesh``, ``filter_mesh`` or ``read_ply(faces=True)`` return) are sampled by area at ``density`` points per square metre
    (``fusion3d.sample_mesh``, face normals), and the two clouds go to ``compare_clouds`` unchanged -> its dict plus ``sampled`` =
    dict(density, n_pred, n_gt, area_pred, area_gt, invalid_pred, invalid_gt).  A side without ``faces`` is a plain cloud (``xyz``,
    optionally ``normal`` / ``color``) and is used as it is: its area is None.  A decimated mesh -- a wall as two triangles -- then counts
    by its area, not by its vertices.  By default every distance is the distance to the nearest SAMPLE of the other surface, not to the
    surface: for a point on it about ``1 / (2 sqrt(density))`` instead of 0, a floor that moves with ``density``.
    ``exact=True`` scores against the surfaces themselves (``TriangleGrid``; csrc/mesh/mesh_distance.hip): accuracy and precision from the
    distances of the predicted samples to the ground-truth MESH, completeness and recall from the ground-truth samples' distances to the
    predicted MESH; a side without ``faces`` keeps the nearest-sample search for the direction that targets it; ``downsample`` applies
    to the query clouds; ``visible`` restricts the ground-truth samples as below while accuracy still looks at the whole ground-truth
    mesh; normal_consistency takes the face normal of the nearest face (``sample_mesh(normals="face")``'s), color_l1 the vertex colours
    interpolated at the nearest point; the result gains ``exact`` = dict(faces_pred, faces_gt: the valid faces searched, None for a
    side without faces; invalid_pred, invalid_gt: the faces ignored).  With the default False nothing of this runs.
    ``visible=dict(cam_poses [T,4,4], cam_intr, image_hw, min_views=1, tol=None, depth_max=None)`` scores only the ground truth the
    cameras saw: the ground-truth mesh is rendered in every view (csrc/mesh/mesh_raster.hip) and its samples seen by fewer than
    ``min_views`` views are dropped before the comparison (``tol`` defaults to ``threshold``); ``sampled`` gains n_gt_visible and
    visible_share.  The predicted side is untouched.  A ground truth without faces cannot be rendered and is refused.  With the default
    None nothing of this runs.
    ``align=dict(metric="plane", dist_max=None, max_iter=30, init=None)`` registers the prediction to the ground truth first, as
    evaluation protocols with a ground truth from another frame of reference do: the prediction's samples against the ground-truth
    SURFACE (a ``TriangleGrid``; against its points where it has no faces), ``registration.register``; then the moved prediction is
    scored -- its samples, their normals and, for ``exact``, its vertices moved by T.  The result gains ``alignment`` (see
    ``compare_clouds``); a registration that did not converge is reported there and the unmoved prediction is scored.  With the
    default None nothing of this runs.
    ``normals=dict(k=16, radius=None)``: a side WITHOUT faces that comes without normals gets them estimated from its points, as
    ``compare_clouds`` documents it (a side with faces has its face normals); with ``align`` and the plane metric such a ground truth is
    registered to through its valid rows.  Not with ``exact=True``.  The result gains ``normals``.  With the default None nothing of
    this runs.
    ``clusters=dict(eps, min_points=10, min_size=None, keep_largest=None, sides=("pred",))``: the SAMPLES of the named sides lose their
    floaters first, as ``compare_clouds`` documents it -- before the alignment and the visibility restriction; the result gains
    ``clusters``.  Not with ``exact=True`` (the surfaces themselves are the targets there: ``fusion3d.filter_mesh`` cleans a mesh).  With
    the default None nothing of this runs."""
    _need(isinstance(density, (int, float)) and math.isfinite(density) and density > 0, "compare_meshes: density must be positive and finite, got %r" % (density,))
    from . import fusion3d
    _need(all(isinstance(x, dict) and x.get("xyz") is not None for x in (pred, gt)), "compare_meshes: pred and gt must be dicts with 'xyz'")
    devs = [v.device for x in (pred, gt) for v in x.values() if isinstance(v, torch.Tensor) and v.is_cuda]
    dev = devs[0] if devs else torch.device("cuda")

    def side(x):
        if x.get("faces") is not None:
            s = fusion3d.sample_mesh(x, density=density, seed=seed)
            return s, s["total"], s["invalid"]
        color = x.get("color") if x.get("color") is not None else x.get("rgb")
        out = {k: fusion3d._on_device(v, dev) for k, v in (("xyz", x["xyz"]), ("normal", x.get("normal")), ("color", color)) if v is not None}
        return out, None, 0
    (a, area_a, bad_a), (b, area_b, bad_b) = side(pred), side(gt)
    dropped = None
    if clusters is not None:
        _need(not exact, "compare_meshes: clusters= is not available with exact=True")
        kw, sides = _clusters_arg(clusters, "compare_meshes")
        dropped = {}

        def cleaned(s, name):
            xyz, cols, dropped[name] = _drop_floaters(_check_cloud(s["xyz"], name, "compare_meshes"), {k: s[k] for k in ("normal", "color") if k in s}, kw)
            return dict(s, xyz=xyz, **cols)
        a = cleaned(a, "pred") if "pred" in sides else a
        b = cleaned(b, "gt") if "gt" in sides else b
    n_gt = int(b["xyz"].shape[0])
    alignment = None
    if normals is not None:
        nk, nr = _normals_arg(normals, threshold, "compare_meshes")
        _need(not exact, "compare_meshes: normals= is not available with exact=True")
    if align is not None:
        from . import registration
        reach = _align_reach(align, threshold)
        tgt, tgt_normal = b["xyz"], b.get("normal")
        if gt.get("faces") is None and normals is not None and tgt_normal is None and isinstance(align, dict) and align.get("metric", "plane") == "plane":
            early = estimate_normals(_check_cloud(tgt, "gt", "compare_meshes"), nk, nr)      # the registration's target: the valid rows
            ok = early["valid"].bool()
            tgt, tgt_normal = tgt[ok].contiguous(), early["normal"][ok].contiguous()
        target = TriangleGrid(gt, reach) if gt.get("faces") is not None else PointGrid(_check_cloud(tgt, "gt", "compare_meshes"), reach)
        T, alignment = _align(a["xyz"], a.get("normal"), target, None if gt.get("faces") is not None else tgt_normal, align, threshold,
                              "compare_meshes")
        if T is not None:
            a = dict(a)
            if a.get("normal") is not None:
                a["xyz"], a["normal"] = registration.transform(a["xyz"], T, a["normal"])
            else:
                a["xyz"] = registration.transform(a["xyz"], T)
            if exact and pred.get("faces") is not None:
                pred = dict(pred, xyz=registration.transform(fusion3d._on_device(pred["xyz"], a["xyz"].device), T))
    if visible is not None:
        b, n_gt, _ = restrict_to_visible(gt, b, visible, threshold, "compare_meshes")
    both = lambda k: k in a and k in b
    if exact:
        out = _exact_scores(a, b, pred, gt, dev, threshold, max_dist, downsample, cell)
    else:
        one = (lambda k: k in a or k in b) if normals is not None else both      # with normals=: the side that lacks them gets them estimated
        out = compare_clouds(a["xyz"], b["xyz"], threshold=threshold, max_dist=max_dist, downsample=downsample,
                             pred_normal=a.get("normal") if one("normal") else None, gt_normal=b.get("normal") if one("normal") else None,
                             pred_color=a["color"] if both("color") else None, gt_color=b["color"] if both("color") else None, cell=cell,
                             **({} if normals is None else dict(normals=normals)))
    out["sampled"] = dict(density=float(density), n_pred=int(a["xyz"].shape[0]), n_gt=n_gt, area_pred=area_a, area_gt=area_b,
                          invalid_pred=bad_a, invalid_gt=bad_b)
    if visible is not None:
        out["sampled"].update(n_gt_visible=int(b["xyz"].shape[0]), visible_share=int(b["xyz"].shape[0]) / n_gt if n_gt else 0.0)
    if alignment is not None:
        out["alignment"] = alignment
    if dropped is not None:
        out["clusters"] = dropped
    return out
