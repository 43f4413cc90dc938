"""float64 reference of the point-cloud contracts of the library (csrc/cloud_nn.hip, include/estd_hip.h: estd_cloud_nearest and
estd_cloud_cell_centroids) and of estdepth_amd/cloud_metrics.py, in the style of tests/tsdf_ref.py.  A plain helper module of the test suite
(not a conftest); numpy and torch only.

``nearest64`` is a brute-force nearest neighbour in float64, chunked over the queries: every query against EVERY target, the differences
formed directly (no |q|^2 - 2 q.p + |p|^2 expansion, which cancels).  It takes the fp32 coordinates as exact.  It runs with torch on any device,
so the 200 000 x 200 000 case of the GPU suite can be evaluated where the clouds already are.

Rounding bound of the contract's ``dist`` against float64, relative to the distance D (first order, u = 2^-24):
    dx = fl(qx - px): one rounding, RELATIVE TO THE DIFFERENCE (the inputs are exact fp32 values): dx = (qx - px)(1 + e1), |e1| <= u; dy, dz alike.
        Each squared difference is off by 2 u of itself, so the sum of the three -- all terms positive, nothing cancels -- by at most 2 u D^2.
    dz * dz rounds once; fma(dy, dy, .) rounds the partial sum once; fma(dx, dx, .) rounds the sum once.  A term sees at most the three of
        them: <= 3 u D^2.
    d2 is therefore within 5 u of D^2, its square root within 2.5 u of D, and the IEEE square root adds one rounding:
        |dist - D| <= 3.5 u D            FIRST = 3.5
    (the three differences contribute 2 u / 2 = 1 u, the three products with their sums 3 u / 2 = 1.5 u, the square root 1 u).
    The bound is relative to the DISTANCE, not to the coordinates: a cloud translated by 100 m keeps it.  Not covered: d2 in the denormal
    range (distances below 1e-18) -- no case goes there; a distance of exactly 0 is exact.
Route constant C_CLOUD = 2: the index rule compares TWO rounded distances (the winner's and the true nearest's), which is 2 x the first-order
bound exactly; the higher orders are 1e-7 of it.   BOUND = C_CLOUD * FIRST * u = 7 u = 4.2e-7.

THE comparison of the suite (``compare``; device results and the fp32 stand-in alike), per query, with Dmin the float64 minimum:
    index >= 0:  the float64 distance of the reported index <= Dmin (1 + BOUND);  |dist - Dmin| <= BOUND Dmin;  Dmin <= max_dist (1 + BOUND)
    index = -1:  dist == max_dist exactly;  Dmin >= max_dist (1 - BOUND)
Threshold counts (``count_bracket``): between the float64 counts at threshold (1 -/+ BOUND).

``nearest32`` is the stand-in that follows the contract in fp32 with numpy.  numpy has no fused multiply-add: fma(a, a, c) is emulated as
fl32(float64(a) * float64(a) + float64(c)) -- the product of two fp32 values is exact in float64, the sum rounds to float64 and then to fp32.
Double-rounding caveat: where the float64 sum lands within 2^-53 of a tie between two fp32 values the second rounding can go the other way
than a true fma's single one, so the stand-in may differ from the device in the last bit of d2 (and then in a tied index); it is held to
the same BOUND, not to bit equality.

``metrics64`` evaluates the dict of ``cloud_metrics.compare_clouds`` from float64 distances.
"""
import numpy as np
import torch

import tsdf_ref as R

U = 2.0 ** -24
FIRST = 3.5                  # first-order bound of dist, in u, relative to the distance (derivation above)
C_CLOUD = 2.0                # route constant
BOUND = C_CLOUD * FIRST * U
# test-only knob: plausible kernel mistakes of the nearest-neighbour search, evaluated by ``nearest32`` (tests/test_cloud_metrics_cpu.py
# asserts that compare / check_ties / the closed form of the lattice pair reject each on some case)
MISTAKES = ("largest_index_on_ties", "strict_radius", "ring_early")


# ------------------------------------------------------------------------------------------------------------ float64 brute force
def nearest64(query, target, chunk=None, device="cpu"):
    """-> (Dmin float64 [M] (inf for an empty target), argmin int64 [M] (an index attaining it; -1 for an empty target)) as numpy arrays"""
    q = torch.as_tensor(np.ascontiguousarray(query) if isinstance(query, np.ndarray) else query).to(device=device, dtype=torch.float64)
    p = torch.as_tensor(np.ascontiguousarray(target) if isinstance(target, np.ndarray) else target).to(device=device, dtype=torch.float64)
    M, N = q.shape[0], p.shape[0]
    if N == 0:
        return np.full(M, np.inf), np.full(M, -1, dtype=np.int64)
    if chunk is None:
        chunk = max(1, (1 << 25) // N)
    dmin, arg = torch.empty(M, dtype=torch.float64, device=device), torch.empty(M, dtype=torch.int64, device=device)
    for a in range(0, M, chunk):
        d2 = (q[a:a + chunk, None, 0] - p[None, :, 0]) ** 2
        d2 += (q[a:a + chunk, None, 1] - p[None, :, 1]) ** 2
        d2 += (q[a:a + chunk, None, 2] - p[None, :, 2]) ** 2
        v, i = d2.min(1)
        dmin[a:a + chunk], arg[a:a + chunk] = v.sqrt(), i
    return dmin.cpu().numpy(), arg.cpu().numpy()


def distance64(query, target, index):
    """float64 distance of query i to target index[i] (inf where index < 0)"""
    q, p = np.asarray(query, dtype=np.float64), np.asarray(target, dtype=np.float64)
    out = np.full(q.shape[0], np.inf)
    ok = index >= 0
    out[ok] = np.sqrt(((q[ok] - p[index[ok]]) ** 2).sum(1))
    return out


# ------------------------------------------------------------------------------------------------------------ the contract in fp32
def nearest32(query, target, max_dist, chunk=256, mistake=None, cell=None):
    """the contract of estd_cloud_nearest with numpy in fp32 (fma through float64, see above) -> (dist float32 [M], index int64 [M]).
    ``mistake``: one of MISTAKES, a deliberately wrong variant ("ring_early" searches a grid of edge ``cell`` anchored at the targets'
    minimum and leaves out the last ring of cells a candidate within max_dist can lie in)."""
    assert mistake is None or mistake in MISTAKES, mistake
    q, p = np.asarray(query, dtype=np.float32), np.asarray(target, dtype=np.float32)
    M, N = q.shape[0], p.shape[0]
    md = np.float32(max_dist)
    r2 = np.float32(md * md)
    dist, index = np.full(M, md, dtype=np.float32), np.full(M, -1, dtype=np.int64)
    if N == 0:
        return dist, index
    for a in range(0, M, chunk):
        dx = (q[a:a + chunk, None, 0] - p[None, :, 0]).astype(np.float32)
        dy = (q[a:a + chunk, None, 1] - p[None, :, 1]).astype(np.float32)
        dz = (q[a:a + chunk, None, 2] - p[None, :, 2]).astype(np.float32)
        inner = (dz * dz).astype(np.float32)
        inner = (dy.astype(np.float64) * dy.astype(np.float64) + inner.astype(np.float64)).astype(np.float32)
        d2 = (dx.astype(np.float64) * dx.astype(np.float64) + inner.astype(np.float64)).astype(np.float32)
        if mistake == "ring_early":                              # candidates in the rings 0 .. ceil(max_dist / cell) - 1 only
            lo = p.min(0).astype(np.float64)
            cq = np.floor((q[a:a + chunk].astype(np.float64) - lo) / cell)
            cp = np.floor((p.astype(np.float64) - lo) / cell)
            ring = np.abs(cq[:, None] - cp[None]).max(2)
            d2 = np.where(ring <= np.ceil(float(md) / cell - 1e-6) - 1, d2, np.float32(np.inf))
        i = d2.argmin(1)                                         # the first = smallest index attaining the minimum
        if mistake == "largest_index_on_ties":
            i = d2.shape[1] - 1 - d2[:, ::-1].argmin(1)
        v = d2[np.arange(d2.shape[0]), i]
        found = (v < r2) if mistake == "strict_radius" else (v <= r2)
        dist[a:a + chunk] = np.where(found, np.sqrt(v), md)
        index[a:a + chunk] = np.where(found, i, -1)
    return dist, index


# ------------------------------------------------------------------------------------------------------------ the comparison
def compare(dist, index, query, target, max_dist, dmin, label=""):
    """assert the rule of the module docstring; -> figures (largest errors in units of BOUND)"""
    dist, index = np.asarray(dist), np.asarray(index)
    M = np.asarray(query).shape[0]
    assert dist.shape == (M,) and index.shape == (M,) and dist.dtype == np.float32 and index.dtype == np.int64, (dist.shape, index.shape, dist.dtype, index.dtype)
    md = float(np.float32(max_dist))
    N = np.asarray(target).shape[0]
    found = index >= 0
    assert ((index >= -1) & (index < max(N, 1))).all() and (N > 0 or not found.any()), label
    fig = dict(n=M, found=int(found.sum()), e_dist=0.0, e_index=0.0)
    if found.any():
        dm = dmin[found]
        own = distance64(np.asarray(query)[found], target, index[found])
        scale = np.where(dm > 0, dm, 1.0)
        e_index = (own - dm) / scale
        e_dist = np.abs(dist[found].astype(np.float64) - dm) / scale
        fig["e_index"], fig["e_dist"] = float(e_index.max() / BOUND), float(e_dist.max() / BOUND)
        print("cloud_nearest %s: %d queries, %d found; |dist - Dmin| / Dmin <= %.3f BOUND, (D(index) - Dmin) / Dmin <= %.3f BOUND"
              % (label, M, fig["found"], fig["e_dist"], fig["e_index"]))
        assert (own <= dm * (1 + BOUND)).all(), (label, fig)
        assert (np.abs(dist[found].astype(np.float64) - dm) <= BOUND * dm).all(), (label, fig)
        assert (dm <= md * (1 + BOUND)).all(), label
    else:
        print("cloud_nearest %s: %d queries, none found" % (label, M))
    if (~found).any():
        assert (dist[~found] == np.float32(max_dist)).all(), label
        assert (dmin[~found] >= md * (1 - BOUND)).all(), label
    return fig


def check_ties(index, target, label=""):
    """the tie rule where it is exact: among targets with identical coordinates (identical d2 whatever the rounding) the reported index
    is the smallest"""
    index, t = np.asarray(index), np.ascontiguousarray(np.asarray(target, dtype=np.float32))
    if t.shape[0] == 0:
        return 0
    _, first, inv = np.unique(t.view(np.uint32).reshape(t.shape[0], 3), axis=0, return_index=True, return_inverse=True)
    first_of = first[inv.reshape(-1)]                  # per target: the smallest index with its coordinates
    found = index >= 0
    bad = found & (first_of[np.where(found, index, 0)] != index)
    assert not bad.any(), "%s: %d queries report a duplicate target that is not the smallest index, first query %d" % (label, int(bad.sum()), int(np.argmax(bad)))
    return int((first_of != np.arange(t.shape[0])).sum())


def count_bracket(dmin, threshold):
    """(lowest, highest) admissible count of distances below ``threshold``: the float64 counts at threshold (1 -/+ BOUND)"""
    return int((dmin < threshold * (1 - BOUND)).sum()), int((dmin < threshold * (1 + BOUND)).sum())


def metrics64(pred, gt, threshold, max_dist, device="cpu", d_pg=None, d_gp=None):
    """the entries of cloud_metrics.compare_clouds from float64 distances (clamped to max_dist) -> dict; besides the values the admissible
    count brackets ``precision_counts`` / ``recall_counts`` and the float64 distances ``d_pred`` / ``d_gt``"""
    d_pg = nearest64(pred, gt, device=device)[0] if d_pg is None else d_pg
    d_gp = nearest64(gt, pred, device=device)[0] if d_gp is None else d_gp
    md = float(np.float32(max_dist))
    ca, cc = np.minimum(d_pg, md), np.minimum(d_gp, md)
    mean = lambda x: float(x.mean()) if x.size else 0.0
    P, Rc = mean(d_pg < threshold), mean(d_gp < threshold)
    return dict(accuracy=mean(ca), completeness=mean(cc), chamfer=0.5 * (mean(ca) + mean(cc)), precision=P, recall=Rc,
                fscore=2 * P * Rc / (P + Rc) if P + Rc > 0 else 0.0, n_pred=int(d_pg.size), n_gt=int(d_gp.size),
                precision_counts=count_bracket(d_pg, threshold), recall_counts=count_bracket(d_gp, threshold), d_pred=d_pg, d_gt=d_gp)


def check_metrics(got, ref, threshold, label=""):
    """compare_clouds' dict against metrics64's: counts bracketed, means within BOUND plus the float64 summation (n u64 relative, far below)"""
    for k in ("n_pred", "n_gt"):
        assert got[k] == ref[k], (label, k, got[k], ref[k])
    for k, n, br in (("precision", ref["n_pred"], ref["precision_counts"]), ("recall", ref["n_gt"], ref["recall_counts"])):
        cnt = got[k] * n
        assert br[0] - 1e-6 <= cnt <= br[1] + 1e-6, (label, k, cnt, br)
    tol = BOUND + 2.0 ** -40
    for k in ("accuracy", "completeness", "chamfer"):
        print("compare_clouds %s: %s %.9g (float64 %.9g, rel %.3g, bar %.3g)" % (label, k, got[k], ref[k], abs(got[k] - ref[k]) / max(ref[k], 1e-300), tol))
        assert abs(got[k] - ref[k]) <= tol * ref[k], (label, k, got[k], ref[k])
    if ref["precision_counts"][0] == ref["precision_counts"][1] and ref["recall_counts"][0] == ref["recall_counts"][1]:
        assert abs(got["fscore"] - ref["fscore"]) <= 1e-12, (label, got["fscore"], ref["fscore"])


# ------------------------------------------------------------------------------------------------------------ voxel down-sampling
def downsample64(points, keys, attrs=None):
    """float64 group-by of ``points`` (and attrs) by ``keys`` -> (means [K,3], attr means [K,C] or None, counts [K]) in ascending key order"""
    uniq, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    def means(x):
        out = np.zeros((uniq.size, x.shape[1]))
        np.add.at(out, inv, x.astype(np.float64))
        return out / counts[:, None]
    return means(np.asarray(points)), (means(np.asarray(attrs)) if attrs is not None else None), counts


# ------------------------------------------------------------------------------------------------------------ closed forms and cases
DELTA = float(np.float32(0.03))          # the lattice offset: |z difference| is exactly this fp32 value


def lattice_pair(n=24, spacing=0.05, delta=DELTA):
    """two copies of an n x n planar lattice, the second offset by ``delta`` along the normal: every nearest distance is ``delta`` exactly
    (the in-plane neighbours are at sqrt(spacing^2 + delta^2))"""
    g = np.arange(n, dtype=np.float32) * np.float32(spacing)
    x, y = np.meshgrid(g, g, indexing="ij")
    a = np.stack([x.ravel(), y.ravel(), np.zeros(n * n, dtype=np.float32)], 1).astype(np.float32)
    b = a.copy()
    b[:, 2] = np.float32(delta)
    return a, b


def check_lattice(dist, index, delta=DELTA):
    """the closed form of ``lattice_pair`` queried with max_dist = delta itself: dx = dy = 0 and dz = delta exactly, so d2 = fl(delta^2) = r2
    and the contract's d2 <= r2 finds every query's own partner at exactly delta"""
    dist, index = np.asarray(dist), np.asarray(index)
    assert (index == np.arange(index.shape[0])).all(), "%d of %d partners at exactly max_dist were not found" % (int((index < 0).sum()), index.shape[0])
    assert (dist == np.float32(delta)).all()


def surface_points(pose, K, H, W):
    """points of the analytic plane + sphere of tsdf_ref.raycast_scene, one per pixel the camera sees -> float32 [n,3]"""
    depth = R.raycast_scene(pose, K, H, W)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([u, v, np.ones_like(u)], -1) @ np.linalg.inv(K).T
    pts = (rays * depth[..., None]) @ pose[:3, :3].T + pose[:3, 3]
    return pts[depth > 0].astype(np.float32)


SIZES = ((1, 63), (63, 1), (64, 65), (65, 64), (257, 4096), (4096, 257), (4096, 4096))      # (targets, queries)
CASES = ["rand_%dx%d" % s for s in SIZES] + ["outside", "one_cell", "cell_faces", "negative", "translated", "sparse", "clusters"]
CELL_FACES = 0.25            # the explicit cell edge of "cell_faces" (and the lattice its targets sit on)


# the route suite's clouds: every pair of these target / query counts (none, one, one short of / exactly / one past a block of 256)
ROUTE_SIZES = (0, 1, 255, 256, 257)


def route_case(n_target, n_query):
    """dict(target, query, max_dist): uniform clouds of the route suite; with more than one point each the last target duplicates the
    first (the smaller index wins) and the first query sits on it (distance exactly 0)"""
    rng = np.random.RandomState(1000 * n_target + n_query)
    target = rng.uniform(0.0, 1.0, (n_target, 3)).astype(np.float32)
    query = rng.uniform(-0.1, 1.1, (n_query, 3)).astype(np.float32)
    if n_target > 1 and n_query > 1:
        target[-1] = target[0]
        query[0] = target[0]
    return dict(target=target, query=query, max_dist=0.2)


PLACED_CASE = "rand_64x65"    # the case that is also built at placement.FAMILY_PLACES: the smallest with more than one wave of either cloud


def build_case(name, place=None):
    """dict(target [N,3] f32, query [M,3] f32, max_dist, cell (None or the case's explicit edge)).  ``place`` (placement.py; the rand_
    cases): the same draws kept in float64, moved to the placement and rounded to fp32 once -- unlike "translated", which adds 100 to
    fp32 data and so keeps the unplaced cloud's low bits"""
    import placement as PL
    rng = np.random.RandomState(sum(name.encode()))
    if PL.key(place) is not None:
        n, m = (int(v) for v in name[5:].split("x"))
        t, q = rng.uniform(0.0, 2.0, size=(n, 3)), rng.uniform(0.0, 2.0, size=(m, 3))
        return dict(name="%s@%s" % (name, PL.label(place)), max_dist=0.15, cell=None, target=PL.points(t, place).astype(np.float32),
                    query=PL.points(q, place).astype(np.float32))
    box = lambda n, lo=0.0, hi=2.0: rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    c = dict(name=name, max_dist=0.15, cell=None)
    if name.startswith("rand_"):
        n, m = (int(v) for v in name[5:].split("x"))
        c.update(target=box(n), query=box(m))
    elif name == "outside":                   # queries beyond every face of the target's box, near (some found) and far
        t, q = box(4096), []
        for axis in range(3):
            for sign in (-1, 1):
                p = box(40)
                p[:, axis] = (2.0 + rng.uniform(0, 0.3, 40)) if sign > 0 else -rng.uniform(0, 0.3, 40)
                far = box(2)
                far[:, axis] = sign * 50.0
                q += [p, far]
        q.append(np.array([[-30.0, -40.0, -50.0], [60.0, 70.0, 80.0], [1.0, 1.0, 1.0e6]], dtype=np.float32))
        c.update(target=t, query=np.concatenate(q).astype(np.float32))
    elif name == "one_cell":                  # all targets within a millimetre, the second half exact duplicates of the first
        half = (1.0 + 1e-3 * rng.uniform(0, 1, size=(32, 3))).astype(np.float32)
        t = np.concatenate([half, half])
        q = np.concatenate([half[::-1], (1.0 + 1e-3 * rng.uniform(-1, 2, size=(33, 3))).astype(np.float32)])
        c.update(target=t, query=q, max_dist=0.01)
    elif name == "cell_faces":                # targets exactly on the faces of cells of edge 0.25 anchored at the box minimum 0
        g = np.arange(9, dtype=np.float32) * np.float32(CELL_FACES)
        t = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        c.update(target=t, query=box(257, -0.1, 2.1), cell=CELL_FACES)
    elif name == "negative":
        c.update(target=box(257, -3.0, -1.0), query=box(4096, -3.0, -1.0))
    elif name == "translated":                # the same kind of cloud 100 m away: the bound stays relative to the distance
        c.update(target=(box(4096) + np.float32(100.0)).astype(np.float32), query=(box(257) + np.float32(100.0)).astype(np.float32))
    elif name == "sparse":                    # max_dist below the point spacing: mostly not found
        c.update(target=box(257), query=box(4096), max_dist=0.02)
    elif name == "clusters":                  # two clusters a kilometre apart; the explicit cell would need 10^5 cells per axis
        t = np.concatenate([box(128, 0.0, 1.0), box(129, 0.0, 1.0) + np.float32([1000.0, 0.0, 0.0])]).astype(np.float32)
        q = np.concatenate([box(100, 0.0, 1.0), box(100, 0.0, 1.0) + np.float32([1000.0, 0.0, 0.0]), box(57, 0.0, 1.0) + np.float32([500.0, 0.0, 0.0])])
        c.update(target=t, query=q.astype(np.float32), max_dist=0.05, cell=0.01)
    else:
        raise KeyError(name)
    return c
