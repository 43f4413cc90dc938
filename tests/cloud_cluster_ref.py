"""Reference of the density-based clustering of the library (csrc/cloud/cloud_cluster.hip, include/estd_hip.h: estd_cloud_dbscan and
estd_cloud_count_within) and of estdepth_amd/cloud_metrics.py's count_within / cluster_dbscan / filter_clusters, in the style of
tests/cloud_knn_ref.py.  A plain helper module of the test suite (not a conftest); numpy only, no device.

``dbscan32`` follows the contract with numpy, a brute force over ALL pairs: d2 from ``cloud_knn_ref.d2_32`` (an exact emulation of the
kernels' fma, see there), the neighbour relation d2 <= r2 = fl(eps * eps), the counts, the components of the core points by a union-find
over the core-core edges, the border rule by the key (d2, index).  Every output is an integer, so the device is held to it by EQUALITY:
there is no tolerance anywhere in this suite.
``dbscan64`` is the same in float64 (the fp32 coordinates taken as exact); it reports where a distance is too close to eps, or two
border keys too close to each other, for fp32 and float64 to be expected to agree.
"""
import numpy as np

import cloud_knn_ref as KR
import cloud_metrics_ref as CM
import placement as PL

BOUND = CM.BOUND                 # |fl32 dist - float64 dist| <= BOUND dist (derived in cloud_metrics_ref for this very d2)
MISTAKES = ("strict_radius", "count_without_self", "border_links_clusters", "border_smallest_label", "border_tie_largest_index",
            "label_largest_index", "ring_early")


# ------------------------------------------------------------------------------------------------------------ the contract in fp32
def _d2_all(q, p, chunk=512):
    out = np.empty((q.shape[0], p.shape[0]), np.float32)
    for a in range(0, q.shape[0], chunk):
        out[a:a + chunk] = KR.d2_32(q[a:a + chunk], p)
    return out


def _within(q, p, radius, mistake, cell):
    """-> (d2 float32 [M,N], the neighbour relation bool [M,N])"""
    d2 = _d2_all(q, p)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    nb = (d2 < r2) if mistake == "strict_radius" else (d2 <= r2)
    if mistake == "ring_early" and p.shape[0]:               # candidates in the rings 0 .. ceil(radius / cell) - 1 only (cloud_metrics_ref.nearest32's)
        lo = p.min(0).astype(np.float64)
        cq = np.floor((q.astype(np.float64) - lo) / cell)
        cp = np.floor((p.astype(np.float64) - lo) / cell)
        ring = np.abs(cq[:, None] - cp[None]).max(2)
        nb &= ring <= np.ceil(float(r) / cell - 1e-6) - 1
    return d2, nb


def count_within32(query, target, radius, mistake=None, cell=None):
    """the contract of estd_cloud_count_within -> int32 [M]"""
    assert mistake is None or mistake in MISTAKES, mistake
    q, p = np.asarray(query, np.float32).reshape(-1, 3), np.asarray(target, np.float32).reshape(-1, 3)
    if p.shape[0] == 0:
        return np.zeros(q.shape[0], np.int32)
    return _within(q, p, radius, mistake, cell)[1].sum(1).astype(np.int32)


def _find(parent, v):
    while parent[v] != v:
        parent[v] = parent[parent[v]]
        v = parent[v]
    return v


def _finish(label, n):
    """label -> the dict every variant returns: size by label, noise, the dense ids ordered by ascending label and their sizes"""
    size = np.bincount(label[label >= 0], minlength=n).astype(np.int32)
    roots = np.nonzero(size > 0)[0]
    dense = np.full(n + 1, -1, np.int32)
    dense[roots] = np.arange(roots.shape[0], dtype=np.int32)
    return dict(label=label.astype(np.int32), size=size, noise=int((label < 0).sum()), roots=roots.astype(np.int64),
                cluster=dense[label].astype(np.int32), sizes=size[roots], n_clusters=int(roots.shape[0]))


def dbscan32(points, eps, min_points, mistake=None, cell=None):
    """the contract of estd_cloud_dbscan -> dict(label, count, size [N] int32, noise, and cloud_metrics.cluster_dbscan's core, roots,
    cluster, sizes, n_clusters).  ``mistake``: one of MISTAKES, a deliberately wrong variant (``cell``: the grid edge "ring_early" walks)"""
    assert mistake is None or mistake in MISTAKES, mistake
    p = np.asarray(points, np.float32).reshape(-1, 3)
    n = p.shape[0]
    if n == 0:
        return dict(_finish(np.zeros(0, np.int64), 0), count=np.zeros(0, np.int32), core=np.zeros(0, bool))
    d2, nb = _within(p, p, eps, mistake, cell)
    count = nb.sum(1).astype(np.int32) - (1 if mistake == "count_without_self" else 0)
    core = count >= min_points
    parent = np.arange(n)
    links = nb & core[:, None] & (np.ones(n, bool) if mistake == "border_links_clusters" else core)[None, :]
    for a, b in zip(*np.nonzero(links)):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    comp = np.array([_find(parent, v) for v in range(n)])
    of = {}                                                   # component -> its label: the smallest (largest) CORE index in it
    for v in np.nonzero(core)[0]:
        of[comp[v]] = max(of.get(comp[v], v), v) if mistake == "label_largest_index" else min(of.get(comp[v], v), v)
    label = np.full(n, -1, np.int64)
    for v in np.nonzero(core)[0]:
        label[v] = of[comp[v]]
    for v in np.nonzero(~core)[0]:
        cand = np.nonzero(nb[v] & core)[0]
        if cand.shape[0] == 0:
            continue
        if mistake == "border_links_clusters":
            label[v] = of[comp[v]]
        elif mistake == "border_smallest_label":
            label[v] = label[cand].min()
        else:
            tie = -cand if mistake == "border_tie_largest_index" else cand
            label[v] = label[cand[np.lexsort((tie, d2[v, cand]))[0]]]
    return dict(_finish(label, n), count=count, core=core)


def filter32(ref, min_size=None, keep_largest=None):
    """cloud_metrics.filter_clusters' mask from a dbscan32 result -> bool [N]"""
    sizes = ref["sizes"].astype(np.int64)
    keep_c = sizes >= (0 if min_size is None else min_size)
    if keep_largest is not None:
        at = np.nonzero(keep_c)[0]
        order = np.argsort(-sizes[at], kind="stable")[:keep_largest]
        keep_c = np.zeros_like(keep_c)
        keep_c[at[order]] = True
    return (ref["cluster"] >= 0) & np.concatenate([keep_c, [False]])[ref["cluster"]]


# ------------------------------------------------------------------------------------------------------------ float64 brute force
def dbscan64(points, eps, min_points):
    """-> (count int64 [N], label int64 [N], clear_radius: no pair's distance within BOUND of eps, clear_border: every border point's two
    smallest core keys further apart than BOUND can bridge)"""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    n = p.shape[0]
    e = float(np.float32(eps))
    D = np.sqrt(((p[:, None] - p[None]) ** 2).sum(2))
    clear_radius = not (np.abs(D - e) <= 2 * BOUND * e).any()
    nb = D <= e
    count = nb.sum(1)
    core = count >= min_points
    parent = np.arange(n)
    for a, b in zip(*np.nonzero(nb & core[:, None] & core[None, :])):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.full(n, -1, np.int64)
    for v in np.nonzero(core)[0]:
        label[v] = _find(parent, v)
    clear_border = True
    for v in np.nonzero(~core)[0]:
        cand = np.nonzero(nb[v] & core)[0]
        if cand.shape[0]:
            d = np.sort(D[v, cand])
            if d.shape[0] > 1 and d[1] - d[0] <= 2 * BOUND * d[1] and d[1] != d[0]:
                clear_border = False
            label[v] = label[cand[np.lexsort((cand, D[v, cand]))[0]]]
    return count, label, clear_radius, clear_border


# ------------------------------------------------------------------------------------------------------------ the comparison
KEYS = ("label", "count", "size", "noise", "cluster", "sizes")


def compare(got, want, label=""):
    """``got``: dict with KEYS (numpy arrays, ints) -> equality with dbscan32's, every key"""
    for k in KEYS:
        g, w = got[k], want[k]
        if isinstance(w, int):
            assert int(g) == w, "%s: %s is %d, expected %d" % (label, k, int(g), w)
        else:
            g = np.asarray(g)
            assert g.shape == w.shape and g.dtype == w.dtype, (label, k, g.shape, g.dtype, w.shape, w.dtype)
            assert (g == w).all(), "%s: %s differs in %d of %d entries, first %d" % (label, k, int((g != w).sum()), w.shape[0], int(np.argmax(g != w)))
    return dict(points=int(want["label"].shape[0]), core=int(want["core"].sum()), clusters=want["n_clusters"], noise=want["noise"],
                border=int(((want["label"] >= 0) & ~want["core"]).sum()))


def same_partition(label_a, label_b, perm):
    """``label_b`` belongs to the cloud whose row j is row perm[j] of the cloud of ``label_a``: the two partitions are the same sets of
    points (the labels themselves, smallest indices, move with the rows)"""
    a, b = np.asarray(label_a)[perm], np.asarray(label_b)
    if ((a < 0) != (b < 0)).any():
        return False
    pairs = set(zip(a[a >= 0].tolist(), b[b >= 0].tolist()))
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})


# ------------------------------------------------------------------------------------------------------------ cases
SURFACES = (1, 63, 64, 65, 257)                                       # wave and workgroup edges
CASES = (["surface_%d" % n for n in SURFACES] + ["clusters_4096", "chain", "radius_edge", "duplicates", "bridge_tie", "bridge_near_larger",
                                                  "all_core", "all_noise", "sparse"])
PLACED_CASES = ("surface_64", "surface_65")
PLACED = ["%s@%s" % (c, at) for c in PLACED_CASES for at in PL.FAMILY_PLACES]
S = 2.0 ** -4                                                         # the lattice spacing of the dyadic cases


def _surface(rng, n):
    """n points of a gently curved surface over the unit square, float64"""
    x, y = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    return np.stack([x, y, 0.5 + 0.05 * np.sin(3.0 * x) * np.cos(2.0 * y)], 1)


def _blob(at):
    """a 3 x 3 x 3 lattice of spacing S with its low corner at ``at`` (in units of S): with eps = 1.25 S a corner has 4 neighbours (itself
    among them), an edge point 5, a face centre 6, the centre 7"""
    g = np.arange(3, dtype=np.float64)
    return (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.asarray(at, np.float64)) * S


def build_case(name):
    """dict(name, points [N,3] f32, eps, min_points, cell (None: the default, eps itself; else the explicit edge))"""
    place = None
    if "@" in name:
        name, at = name.split("@")
        place = PL.FAMILY_PLACES[at]
    rng = np.random.RandomState(sum(name.encode()))
    c = dict(name=name, cell=None)
    if name.startswith("surface_"):                   # about six neighbours besides the point: core, border and noise points all occur
        n = int(name[8:])
        pts = _surface(rng, n)
        if place is not None:
            c["name"] = "%s@%s" % (name, PL.label(place))
            pts = PL.points(pts, place)
        c.update(points=pts.astype(np.float32), eps=float(np.sqrt(6.0 / (np.pi * n))), min_points=5)
    elif name == "clusters_4096":                     # six blobs of different density and a uniform background, the rows shuffled over the workgroups
        centres = rng.uniform(0.2, 1.8, (6, 3))
        parts = [centres[j] + (0.02 + 0.01 * j) * rng.standard_normal((600, 3)) for j in range(6)]
        parts.append(rng.uniform(0.0, 2.0, (4096 - 3600, 3)))
        pts = np.concatenate(parts)[rng.permutation(4096)]
        c.update(points=pts.astype(np.float32), eps=0.03, min_points=8)
    elif name == "chain":                             # 2049 points on a line at 0.75 eps: one cluster, both ends are borders, long union-find paths
        pts = np.zeros((2049, 3))
        pts[:, 0] = np.arange(2049) * (0.75 * S)
        c.update(points=pts[rng.permutation(2049)].astype(np.float32), eps=S, min_points=3)
    elif name == "radius_edge":                       # a 9 x 9 lattice whose spacing IS eps: d2 == r2 for the four neighbours, and they must count
        g = np.arange(9, dtype=np.float64) * S
        x, y = np.meshgrid(g, g, indexing="ij")
        c.update(points=np.stack([x.ravel(), y.ravel(), np.full(81, 0.25)], 1).astype(np.float32), eps=S, min_points=5)
    elif name == "duplicates":                        # 70 copies of one point (one cluster), 3 of another (noise at min_points = 8)
        pts = np.concatenate([np.tile([0.3, 0.7, 1.1], (70, 1)), np.tile([0.9, 0.1, 0.4], (3, 1))])
        c.update(points=pts[rng.permutation(73)].astype(np.float32), eps=0.1, min_points=8)
    elif name in ("bridge_tie", "bridge_near_larger"):
        # row 0: the bridge, with 3 neighbours not core; rows 1..27: blob A (label 1); rows 28..54: blob B (label 28), 2 S apart: no link.
        # The bridge sits between A's (2, 1, 1) S and B's (4, 1, 1) S: at S from both (the tie is exact, the coordinates are dyadic), or
        # S / 8 nearer to B, the larger label -- 1.125 S and 0.875 S, both inside eps = 1.25 S.
        x = 3.0 if name == "bridge_tie" else 3.125
        pts = np.concatenate([np.array([[x, 1.0, 1.0]]) * S, _blob((0, 0, 0)), _blob((4, 0, 0))])
        c.update(points=pts.astype(np.float32), eps=1.25 * S, min_points=4)
    elif name == "all_core":                          # min_points = 1: every point is core, an isolated one its own cluster
        c.update(points=_surface(rng, 65).astype(np.float32), eps=0.12, min_points=1)
    elif name == "all_noise":                         # min_points = N + 1: nothing is core
        c.update(points=_surface(rng, 65).astype(np.float32), eps=0.3, min_points=66)
    elif name == "sparse":                            # cells of eps / 6: the neighbours lie up to six rings out, across empty cells
        c.update(points=rng.uniform(0.0, 2.0, (257, 3)).astype(np.float32), eps=0.3, min_points=3, cell=0.05)
    else:
        raise KeyError(name)
    return c


_EXPECTED = {}


def expected(name):
    """the case and dbscan32's result, computed once and left unchanged -> (case, dict)"""
    if name not in _EXPECTED:
        c = build_case(name)
        _EXPECTED[name] = (c, dbscan32(c["points"], c["eps"], c["min_points"]))
    return _EXPECTED[name]


# query != target counting: every pair of cloud_metrics_ref.ROUTE_SIZES (none, one, one short of / exactly / one past a block of 256)
COUNT_CASES = [(t, q) for t in CM.ROUTE_SIZES for q in CM.ROUTE_SIZES]


def count_case(n_target, n_query):
    """cloud_metrics_ref.route_case's clouds and radius -> (case, count_within32's counts)"""
    key = ("count", n_target, n_query)
    if key not in _EXPECTED:
        c = CM.route_case(n_target, n_query)
        _EXPECTED[key] = (c, count_within32(c["query"], c["target"], c["max_dist"]))
    return _EXPECTED[key]
