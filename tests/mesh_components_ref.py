"""Reference of the mesh-components contract of the library (csrc/mesh/mesh_components.hip, include/estd_hip.h: estd_mesh_components) and
of ``fusion3d.filter_mesh``.  A plain helper module of the test suite (not a conftest); numpy only.

``components`` labels by min-label propagation with pointer jumping until nothing changes -- no union-find, no atomics, nothing the
kernels could share a mistake with -- and returns the contract's three outputs:

    label [V] int32       the smallest vertex index of the vertex's component (a vertex in no valid triangle: its own index)
    triangles [V] int32   at a root the number of valid triangles of the component, 0 elsewhere
    invalid               the number of triangles with an index outside [0, V): ignored entirely

``compare`` is THE comparison of the suite: integer equality of all three, dtypes and shapes included.  There is no tolerance.
``filter_mesh`` is the numpy twin of ``fusion3d.filter_mesh``."""
import functools

import numpy as np

import tsdf_mesh_ref as M

# test-only knob: plausible kernel mistakes (tests/test_mesh_components_ref_cpu.py asserts that compare rejects each on some case)
MISTAKES = ("largest_index", "link_v0_v1_only", "count_vertices", "loose_minus_one", "counts_at_non_roots")


def components(faces, n_vertices, mistake=None):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = int(n_vertices)
    ok = ((faces >= 0) & (faces < V)).all(1)
    f = faces[ok]
    links = f[:, :2] if mistake == "link_v0_v1_only" else f
    pick, fold = (np.max, np.maximum) if mistake == "largest_index" else (np.min, np.minimum)
    label = np.arange(V, dtype=np.int64)
    while links.shape[0]:
        new = label.copy()
        best = pick(label[links], axis=1)                     # the best label among a triangle's vertices goes to each of them
        for k in range(links.shape[1]):
            fold.at(new, links[:, k], best)
        while True:                                           # pointer jumping: a label is a vertex of the same component
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            break
        label = new
    tri = np.bincount(label[f[:, 0]], minlength=V) if f.shape[0] else np.zeros(V, np.int64)
    if mistake == "count_vertices":
        tri = np.where(tri > 0, np.bincount(label, minlength=V), 0)
    if mistake == "counts_at_non_roots":
        tri = tri[label]
    if mistake == "loose_minus_one":
        used = np.zeros(V, bool)
        used[f.reshape(-1)] = True
        label = np.where(used, label, -1)
    return dict(label=label.astype(np.int32), triangles=tri.astype(np.int32), invalid=int((~ok).sum()))


def summary(ref):
    """-> (roots ascending, triangles per root, vertices per root) of a ``components`` result"""
    label = ref["label"].astype(np.int64)
    roots = np.nonzero(label == np.arange(label.shape[0]))[0]
    return roots, ref["triangles"][roots].astype(np.int64), np.bincount(label, minlength=label.shape[0])[roots]


def compare(got, ref, what=""):
    """``got``: dict(label, triangles, invalid) of numpy arrays / an integer, against ``ref`` = components(...): equal to the integer"""
    V = ref["label"].shape[0]
    for k in ("label", "triangles"):
        a = np.asarray(got[k])
        assert a.dtype == np.int32 and a.shape == (V,), "%s: %s is %s %s, expected int32 [%d]" % (what, k, a.dtype, a.shape, V)
        bad = np.nonzero(a != ref[k])[0]
        assert bad.size == 0, "%s: %s differs at %d of %d vertices, first at %d: %d for %d" % (
            what, k, bad.size, V, bad[0], a[bad[0]], ref[k][bad[0]])
    assert int(got["invalid"]) == ref["invalid"], "%s: invalid = %d, the reference has %d" % (what, int(got["invalid"]), ref["invalid"])
    roots, tri, _ = summary(ref)
    return dict(vertices=V, components=int(roots.shape[0]), with_faces=int((tri > 0).sum()), invalid=ref["invalid"])


PER_VERTEX = ("xyz", "normal", "weight", "cell", "color", "rgb")


def filter_mesh(mesh, min_triangles=1, keep_largest=None):
    """the numpy twin of fusion3d.filter_mesh: the same keys, the same order, the same counts"""
    faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    V = int(np.asarray(mesh["xyz"]).shape[0])
    ref = components(faces, V)
    assert ref["invalid"] == 0
    roots, tri, _ = summary(ref)
    with_faces = tri > 0
    keep = with_faces & (tri >= min_triangles) if min_triangles > 0 else np.ones_like(with_faces)
    if keep_largest is not None:
        at = np.nonzero(keep)[0]
        order = np.argsort(-tri[at], kind="stable")           # ties: the smaller root first
        keep = np.zeros_like(keep)
        keep[at[order[:keep_largest]]] = True
    root_kept = np.zeros(V, bool)
    root_kept[roots[keep]] = True
    v_mask = root_kept[ref["label"]]
    new_index = np.cumsum(v_mask) - 1
    f_mask = v_mask[faces[:, 0]] if faces.shape[0] else np.zeros(0, bool)
    out = {k: (np.asarray(v)[v_mask] if k in PER_VERTEX and v is not None else v) for k, v in mesh.items()}
    out["faces"] = new_index[faces[f_mask]].astype(np.int32).reshape(-1, 3)
    if mesh.get("edge") is not None:
        out["edge"] = np.asarray(mesh["edge"])[f_mask[0::2]]
    out["count"] = int(v_mask.sum())
    out["components"] = int(keep.sum())
    out["dropped"] = dict(vertices=V - out["count"], faces=int(faces.shape[0] - out["faces"].shape[0]), components=int((with_faces & ~keep).sum()))
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def _strip(n, ids):
    """n triangles (i, i + 1, i + 2) over n + 2 vertices renamed by ``ids``: one long chain"""
    i = np.arange(n)
    return ids[np.stack([i, i + 1, i + 2], 1)], n + 2


def _star(n, hub_last):
    """n triangles that share one vertex -- the last one (every hook contends for a root that keeps moving) or vertex 0"""
    V = 2 * n + 1
    i = np.arange(n)
    if hub_last:
        return np.stack([np.full(n, V - 1), 2 * i, 2 * i + 1], 1), V
    return np.stack([np.zeros(n, np.int64), 2 * i + 1, 2 * i + 2], 1), V


def _disjoint(n):
    """n triangles without a common vertex, ids interleaved: (i, i + n, i + 2n)"""
    i = np.arange(n)
    return np.stack([i, i + n, i + 2 * n], 1), 3 * n


def _islands(rows, cols, n, seed):
    """``n`` separate quad grids of rows x cols quads, two triangles each, then the vertex ids permuted and the faces shuffled"""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    v00 = (r * (cols + 1) + c).reshape(-1)
    quad = np.stack([v00, v00 + 1, v00 + cols + 2, v00 + cols + 1], 1)
    one = quad[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)
    per = (rows + 1) * (cols + 1)
    faces = np.concatenate([one + k * per for k in range(n)])
    rng = np.random.default_rng(seed)
    faces = rng.permutation(n * per)[faces]
    return faces[rng.permutation(faces.shape[0])], n * per


def _tsdf(name):
    ref = M.reference(M.build_case(name))
    return ref["faces"], ref["count"]


def _out_of_range():
    V = 12
    f = [(0, 1, 2), (-1, 2, 3), (2, 3, 4), (0, V, 1), (5, 6, 7), (2 ** 30, 1, 2), (7, 8, -2 ** 31), (9, 10, 11), (4, 5, 2 ** 31 - 1), (V, V, V)]
    return np.array(f, np.int64), V


CASES = {
    "empty": lambda: (np.zeros((0, 3), np.int64), 0),
    "no-faces": lambda: (np.zeros((0, 3), np.int64), 5),
    "one-v3": lambda: (np.array([[2, 0, 1]]), 3),
    "one-v7": lambda: (np.array([[5, 2, 6]]), 7),
    "degenerate": lambda: (np.array([[1, 1, 4], [6, 6, 6], [0, 2, 3], [0, 2, 3], [3, 2, 0], [7, 8, 7]]), 10),
    "strip-ascending": lambda: _strip(300, np.arange(302)),
    "strip-descending": lambda: _strip(300, np.arange(302)[::-1].copy()),
    "strip-permuted": lambda: _strip(300, np.random.default_rng(7).permutation(302)),
    "star-hub-last": lambda: _star(500, True),
    "star-hub-first": lambda: _star(500, False),
    "grid-48": lambda: _islands(16, 16, 9, 48),
    "grid-320": lambda: _islands(64, 320, 5, 320),
    "tsdf-3x5x7": lambda: _tsdf("3x5x7"), "tsdf-holes": lambda: _tsdf("holes"), "tsdf-9x17x66": lambda: _tsdf("9x17x66"),
    "tsdf-colour": lambda: _tsdf("colour"),
    "out-of-range": _out_of_range,
}
for _n in (63, 64, 65, 255, 256, 257):
    CASES["disjoint-%d" % _n] = functools.partial(_disjoint, _n)
# (components with faces, vertices no face uses) of the surface-net cases
TSDF_EXPECTED = {"tsdf-3x5x7": (2, 6), "tsdf-holes": (13, 34), "tsdf-9x17x66": (87, 596), "tsdf-colour": (12, 143)}


@functools.lru_cache(maxsize=None)
def build_case(name):
    """-> (faces int32 [F,3] contiguous, V); computed once and shared: not to be written to (left writable, torch refuses to wrap
    a read-only array without a warning)"""
    faces, V = CASES[name]()
    return np.ascontiguousarray(np.asarray(faces, np.int64).reshape(-1, 3).astype(np.int32)), int(V)


@functools.lru_cache(maxsize=None)
def reference(name):
    faces, V = build_case(name)
    ref = components(faces, V)
    for a in (ref["label"], ref["triangles"]):
        a.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------------------------ the two-sphere volume
SMALL_R, SMALL_AT = 0.075, (5.3, 6.1, 4.7)


@functools.lru_cache(maxsize=None)
def two_sphere_volume():
    """tsdf_mesh_ref.sphere_volume(radius=0.30) with a second, small sphere in a corner of the volume: D = min of the two truncated
    distances (same truncation and clip) -> (D, W, origin, centre of the large sphere): two closed surfaces, 3760 and 228 triangles"""
    D, W, origin, centre = M.sphere_volume(radius=0.30)
    Z, Y, X = D.shape
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    P = np.stack([x, y, z], -1) * M.VOXEL + (np.asarray(origin) + 0.5 * M.VOXEL)
    c2 = np.asarray(origin) + M.VOXEL * np.asarray(SMALL_AT)
    D2 = np.clip((np.linalg.norm(P - c2, axis=-1) - SMALL_R) / (4 * M.VOXEL), -1.0, 1.0).astype(np.float32)
    return np.minimum(D, D2), W, origin, centre


@functools.lru_cache(maxsize=None)
def two_sphere_mesh():
    D, W, origin, _ = two_sphere_volume()
    return M.mesh(D, W, M.W_MIN, M.VOXEL, origin)
