"""float64 reference of the surface-net contract of the library (csrc/mesh/tsdf_mesh.hip, include/estd_hip.h: estd_tsdf_mesh_vertices and
estd_tsdf_mesh_faces), in the style of tests/tsdf_ref.py.  A plain helper module of the test suite (not a conftest); numpy only.

``mesh`` evaluates the contract in float64 FROM THE fp32 PLANES AND CONSTANTS THE KERNEL RECEIVES and returns the mesh in the public
order (vertices by ascending cell id, quads by ascending edge id, the two triangles of a quad consecutive) with, per vertex attribute, a
first-order rounding bound.  ``compare`` is THE comparison of the suite (GPU results and the numpy-fp32 stand-in alike):

    EXACT, no case left out:   the number of vertices, the cell ids, the edge ids, the faces (int32 vertex indices)
    |xyz - ref| <= C_MESH E_xyz     |weight - ref| <= C_MESH E_w     |colour - ref| <= C_MESH E_c     |normal - ref| <= C_MESH E_n

Every topological decision (D < 0, Wt >= w_min) compares stored fp32 values, so nothing about the topology is ambiguous.

Rounding bounds (first order, u = 2^-24; the contract's operations one by one)
    s = D0 / (D0 - D1): the difference and the division round, both relatively: e_s = 2 u s, 0 <= s <= 1.
    sum_k: n <= 12 non-negative terms added from 0 in edge order -- s of the crossing k-edges, the exact offsets 0 / 1 of the others.
        The first addition is exact, each further one rounds a partial sum <= S_k = the whole sum:  e_sum = (n - 1) u S_k + sum_i e_s,i.
    p_k = sum_k / n: e_p = e_sum / n + u p_k.
    cell = (float)c_k + 0.5 + p_k: c_k + 0.5 is exact, the addition rounds: e_cell = e_p + u cell.
    xyz_k = fma(cell, voxel, origin_k): one rounding of the result; an evaluation without a fused multiply-add (the numpy stand-in)
        rounds the product as well:  E_xyz = voxel e_cell + u |cell voxel| + u |xyz_k|.
    weight = (sum of the eight corner weights) * 0.125: seven roundings of partial sums <= S_w = sum |Wt|, the scale is exact:
        E_w = 7 u S_w / 8.
    colour term v = fma(s, C1 - C0, C0): e_v = 2 u s |C1 - C0| (from s) + u s |C1 - C0| (the difference) + u s |C1 - C0| (the product,
        unfused) + u |v|;  mean: E_c = ((n - 1) u sum |v_i| + sum e_v,i) / n + u |mean|.
    g_k = the sum of four differences D1 - D0: each difference rounds, three additions round partial sums <= G_k = sum |D1 - D0|:
        e_g,k = 4 u G_k.  normal_k = g_k / |g|: the length (two fused multiply-adds, a product, a square root: <= 3 u |g|, and
        sum_j e_g,j from its operands) and the division (u |n_k|):  E_n,k = (e_g,k + |n_k| sum_j e_g,j) / |g| + 4 u |n_k|.
        A normal whose |g| is within NORMAL_GUARD sum_j e_g,j of zero is not compared (cancellation: the fp32 sum may or may not vanish);
        such vertices may be at most AMB_CAP of the vertices of a case.
    C_MESH = 2: the bounds above are worst cases of every single operation, so a correct evaluation stays below 1 x the bound up to
    second-order terms; the factor 2 is for those and for nothing else (the ray caster's route constant is 4).
"""
import numpy as np

U = 2.0 ** -24
C_MESH = 2.0                 # route constant of the attribute bounds, from the derivation above
NORMAL_GUARD = 16.0          # |g| <= NORMAL_GUARD * sum e_g: the normal is not compared (as tsdf_ref.compare_points)
AMB_CAP = 0.03               # vertices whose normal is left out: at most this share of a case's vertices
# test-only knob: plausible kernel mistakes (tests/test_tsdf_mesh_ref_cpu.py asserts that compare rejects each on some case)
MISTAKES = ("winding_reversed", "sign_le", "observed_from_edge_ends", "half_voxel_shift", "quad_cyclic_order")

# the twelve edges of a cell in the contract's order: (axis, (ox, oy, oz) of the lower end); axis 0 = x, 1 = y, 2 = z
EDGES = []
for _a in range(3):
    for _e in range(4):
        _lo, _hi = _e & 1, _e >> 1
        EDGES.append((_a, (0, _lo, _hi) if _a == 0 else (_lo, 0, _hi) if _a == 1 else (_lo, _hi, 0)))


def _corner(A, o, step=(0, 0, 0)):
    """the corner (ox, oy, oz) + step of every cell of the plane A [Z][Y][X] -> [Z-1][Y-1][X-1]"""
    Z, Y, X = A.shape
    ox, oy, oz = o[0] + step[0], o[1] + step[1], o[2] + step[2]
    return A[oz:Z - 1 + oz, oy:Y - 1 + oy, ox:X - 1 + ox]


def _shifted(obs_full, sx, sy, sz):
    """per voxel v: is the cell v - (sx, sy, sz) observed (False where it does not exist)"""
    Z, Y, X = obs_full.shape
    out = np.zeros_like(obs_full)
    out[sz:, sy:, sx:] = obs_full[:Z - sz, :Y - sy, :X - sx]
    return out


def mesh(D32, W32, w_min, voxel_size, origin, C32=None, dtype=np.float64, mistake=None):
    """The contract on the fp32 planes D32, W32 [Z][Y][X] (C32 [3][Z][Y][X] or None), arithmetic in ``dtype`` (np.float32: the stand-in
    for the kernel, without fused operations) -> dict(cell int64 [V], xyz [V,3], normal [V,3], weight [V], color [V,3] or None,
    faces int32 [F,3], edge int64 [F/2], count = V, and the bounds E_xyz, E_normal, E_weight, E_color, normal_ok)."""
    f = dtype
    D32, W32 = np.ascontiguousarray(D32, np.float32), np.ascontiguousarray(W32, np.float32)
    Z, Y, X = D32.shape
    wm = np.float32(w_min)
    voxel, org = np.float32(voxel_size), np.asarray(origin, np.float32)
    neg_of = (lambda a: a <= 0) if mistake == "sign_le" else (lambda a: a < 0)
    empty = dict(cell=np.zeros(0, np.int64), xyz=np.zeros((0, 3), f), normal=np.zeros((0, 3), f), weight=np.zeros(0, f),
                 color=None if C32 is None else np.zeros((0, 3), f), faces=np.zeros((0, 3), np.int32), edge=np.zeros(0, np.int64), count=0,
                 E_xyz=np.zeros((0, 3)), E_normal=np.zeros((0, 3)), E_weight=np.zeros(0), E_color=np.zeros((0, 3)), normal_ok=np.zeros(0, bool))
    if min(Z, Y, X) < 2:
        return empty
    corners = [(i, j, k) for k in (0, 1) for j in (0, 1) for i in (0, 1)]                # corner order: x fastest
    obs = np.ones((Z - 1, Y - 1, X - 1), bool)
    any_neg, any_pos = np.zeros_like(obs), np.zeros_like(obs)
    for o in corners:
        obs &= _corner(W32, o) >= wm
        n_ = neg_of(_corner(D32, o))
        any_neg |= n_
        any_pos |= ~n_
    active = obs & any_neg & any_pos
    cz, cy, cx = np.nonzero(active)                                                       # ascending cell id: C order of [Z][Y][X]
    cell = (cz.astype(np.int64) * Y + cy) * X + cx
    V = cell.shape[0]
    at = (cz, cy, cx)
    Df, Wf = D32.astype(f), W32.astype(f)
    Cf = None if C32 is None else np.ascontiguousarray(C32, np.float32).astype(f)

    # ---- vertices
    sums, S64, e_sum = [np.zeros(V, f) for _ in range(3)], [np.zeros(V) for _ in range(3)], [np.zeros(V) for _ in range(3)]
    g, G64 = [np.zeros(V, f) for _ in range(3)], [np.zeros(V) for _ in range(3)]
    csum, cabs, e_c = [np.zeros(V, f) for _ in range(3)], [np.zeros(V) for _ in range(3)], [np.zeros(V) for _ in range(3)]
    n = np.zeros(V, np.int64)
    for a, o in EDGES:
        step = tuple(int(a == k) for k in range(3))
        d0, d1 = _corner(Df, o)[at], _corner(Df, o, step)[at]
        diff = d1 - d0
        g[a] = g[a] + diff
        G64[a] += np.abs(diff.astype(np.float64))
        cross = neg_of(_corner(D32, o)[at]) != neg_of(_corner(D32, o, step)[at])
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(cross, d0 / (d0 - d1), f(0))
        s64 = s.astype(np.float64)
        for k in range(3):
            term = s if k == a else np.full(V, f(o[k]))
            sums[k] = sums[k] + np.where(cross, term, f(0))
            S64[k] += np.where(cross, term.astype(np.float64), 0.0)
            if k == a:
                e_sum[k] += np.where(cross, 2 * U * s64, 0.0)
        n += cross
        if Cf is not None:
            for k in range(3):
                c0, c1 = _corner(Cf[k], o)[at], _corner(Cf[k], o, step)[at]
                v = s * (c1 - c0) + c0
                csum[k] = csum[k] + np.where(cross, v, f(0))
                dc = np.abs((c1 - c0).astype(np.float64))
                cabs[k] += np.where(cross, np.abs(v.astype(np.float64)), 0.0)
                e_c[k] += np.where(cross, 4 * U * s64 * dc + U * np.abs(v.astype(np.float64)), 0.0)
    nf, n64 = n.astype(f), n.astype(np.float64)
    idx3 = (cx, cy, cz)
    xyz, E_xyz = np.zeros((V, 3), f), np.zeros((V, 3))
    shift = f(0.0) if mistake == "half_voxel_shift" else f(0.5)
    for k in range(3):
        p = sums[k] / nf
        e_p = ((n64 - 1) * U * S64[k] + e_sum[k]) / n64 + U * np.abs(p.astype(np.float64))
        cellpos = idx3[k].astype(f) + shift + p
        c64 = np.abs(cellpos.astype(np.float64))
        xyz[:, k] = cellpos * voxel.astype(f) + org[k].astype(f)
        E_xyz[:, k] = float(voxel) * (e_p + U * c64) + U * c64 * float(voxel) + U * np.abs(xyz[:, k].astype(np.float64))
    gv = np.stack(g, 1)
    length = np.sqrt(gv[:, 2] * gv[:, 2] + (gv[:, 1] * gv[:, 1] + gv[:, 0] * gv[:, 0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        normal = np.where(length[:, None] > 0, gv / length[:, None], f(0))
    e_g = np.stack([4 * U * G64[k] for k in range(3)], 1)
    len64 = length.astype(np.float64)
    normal_ok = len64 > NORMAL_GUARD * e_g.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        E_normal = np.where(normal_ok[:, None], (e_g + np.abs(normal.astype(np.float64)) * e_g.sum(1)[:, None]) / len64[:, None]
                            + 4 * U * np.abs(normal.astype(np.float64)), 0.0)
    ws, S_w = np.zeros(V, f), np.zeros(V)
    for o in corners:
        w = _corner(Wf, o)[at]
        ws = ws + w
        S_w += np.abs(w.astype(np.float64))
    weight = ws * f(0.125)
    color = E_color = None
    if Cf is not None:
        color = np.stack([csum[k] / nf for k in range(3)], 1)
        E_color = np.stack([((n64 - 1) * U * cabs[k] + e_c[k]) / n64 for k in range(3)], 1) + U * np.abs(color.astype(np.float64))

    # ---- faces
    obs_full = np.zeros((Z, Y, X), bool)
    obs_full[:Z - 1, :Y - 1, :X - 1] = obs
    Wobs = W32 >= wm
    neg = neg_of(D32)
    lin = np.arange(Z * Y * X, dtype=np.int64).reshape(Z, Y, X)
    stride = (1, X, X * Y)
    edges, quads = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ea, eb, ec = (tuple(int(k == j) for k in range(3)) for j in (a, b, c))
        far_neg, far_obs = np.zeros_like(neg), np.zeros_like(neg)
        sl_lo = tuple(slice(0, dim - e) for dim, e in zip((Z, Y, X), ea[::-1]))
        sl_hi = tuple(slice(e, dim) for dim, e in zip((Z, Y, X), ea[::-1]))
        far_neg[sl_lo], far_obs[sl_lo] = neg[sl_hi], Wobs[sl_hi]
        has_far = np.zeros_like(neg)
        has_far[sl_lo] = True
        cross = has_far & (neg != far_neg)
        if mistake == "observed_from_edge_ends":
            exist = _shifted(np.ones_like(obs_full), eb[0] + ec[0], eb[1] + ec[1], eb[2] + ec[2])
            exist[Z - 1], exist[:, Y - 1], exist[:, :, X - 1] = False, False, False
            ok = cross & exist & Wobs & far_obs
        else:
            ok = cross & _shifted(obs_full, eb[0] + ec[0], eb[1] + ec[1], eb[2] + ec[2]) & _shifted(obs_full, *ec) & obs_full & _shifted(obs_full, *eb)
        v = lin[ok]
        q = np.stack([v - stride[b] - stride[c], v - stride[c], v, v - stride[b]], 1)
        if mistake == "quad_cyclic_order":
            q = q[:, [0, 1, 3, 2]]
        free_plus = neg[ok]                                   # D0 < 0: free space on the +a side
        if mistake == "winding_reversed":
            free_plus = ~free_plus
        q = np.where(free_plus[:, None], q, q[:, ::-1])
        edges.append(3 * v + a)
        quads.append(q)
    edge = np.concatenate(edges)
    quad = np.concatenate(quads).reshape(-1, 4)
    order = np.argsort(edge, kind="stable")
    edge, quad = edge[order], quad[order]
    vi = np.clip(np.searchsorted(cell, quad), 0, max(V - 1, 0)).astype(np.int32)
    if mistake is None and quad.size:
        assert V > 0 and np.array_equal(cell[vi], quad), "a face names a cell that is not a vertex"
    faces = vi[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)
    return dict(cell=cell, xyz=xyz, normal=normal, weight=weight, color=color, faces=faces, edge=edge, count=V,
                E_xyz=E_xyz, E_normal=E_normal, E_weight=7 * U * S_w / 8, E_color=E_color, normal_ok=normal_ok)


def compare(got, ref, label=""):
    """``got``: dict(cell, xyz, normal, weight, faces, edge[, color]) of numpy arrays in the public order, against ``ref`` = mesh(...) in
    float64.  Asserts the exact parts and the attribute bounds; -> the figures (max |error| / bound per attribute, share left out)."""
    V = ref["count"]
    assert got["cell"].shape == (V,), "%s: %d vertices, the reference has %d" % (label, got["cell"].shape[0], V)
    assert np.array_equal(np.asarray(got["cell"], np.int64), ref["cell"]), "%s: the cell ids differ" % label
    assert got["edge"].shape == ref["edge"].shape, "%s: %d quads, the reference has %d" % (label, got["edge"].shape[0], ref["edge"].shape[0])
    assert np.array_equal(np.asarray(got["edge"], np.int64), ref["edge"]), "%s: the edge ids differ" % label
    assert got["faces"].dtype == np.int32 and got["faces"].shape == ref["faces"].shape, "%s: faces %s %s" % (label, got["faces"].dtype, got["faces"].shape)
    assert np.array_equal(got["faces"], ref["faces"]), "%s: the faces differ" % label
    fig = dict(vertices=V, faces=int(ref["faces"].shape[0]))

    def ratio(name, a, r, E, keep=None):
        a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
        assert a.shape == r.shape, "%s: %s has the shape %s, expected %s" % (label, name, a.shape, r.shape)
        err, tol = np.abs(a - r), C_MESH * E
        if keep is not None:
            err, tol = err[keep], tol[keep]
        assert np.all(np.isfinite(a)), "%s: %s is not finite somewhere" % (label, name)
        bad = err > tol
        worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
        assert not bad.any(), "%s: %s off by %.3f x the bound at %d of %d values" % (label, name, worst, int(bad.sum()), err.size)
        return worst

    fig["xyz_ratio"] = ratio("xyz", got["xyz"], ref["xyz"], ref["E_xyz"])
    fig["weight_ratio"] = ratio("weight", got["weight"], ref["weight"], ref["E_weight"])
    fig["normal_ratio"] = ratio("normal", got["normal"], ref["normal"], ref["E_normal"], ref["normal_ok"])
    fig["normal_left_out"] = float((~ref["normal_ok"]).mean()) if V else 0.0
    assert fig["normal_left_out"] <= AMB_CAP, "%s: %.4f of the normals left out" % (label, fig["normal_left_out"])
    if ref["color"] is not None:
        assert got.get("color") is not None, "%s: no colour" % label
        fig["color_ratio"] = ratio("color", got["color"], ref["color"], ref["E_color"])
    return fig


# ------------------------------------------------------------------------------------------------------------ mesh properties
def edge_stats(faces):
    """(boundary, manifold, non-manifold, euler): mesh edges shared by 1, 2, more than 2 triangles and V_used - E + F, in numpy"""
    faces = np.asarray(faces, np.int64)
    if faces.shape[0] == 0:
        return 0, 0, 0, 0
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    key = np.minimum(e[:, 0], e[:, 1]) * (faces.max() + 1) + np.maximum(e[:, 0], e[:, 1])
    _, counts = np.unique(key, return_counts=True)
    used = np.unique(faces).shape[0]
    return int((counts == 1).sum()), int((counts == 2).sum()), int((counts > 2).sum()), used - counts.shape[0] + faces.shape[0]


def triangle_normals(xyz, faces):
    """unnormalised geometric normals (v1 - v0) x (v2 - v0) [F,3] and centroids [F,3] in float64"""
    p = np.asarray(xyz, np.float64)[np.asarray(faces, np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p.mean(1)


def enclosed_volume(xyz, faces):
    p = np.asarray(xyz, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ------------------------------------------------------------------------------------------------------------ fixtures
VOXEL = 0.03
SPHERE_R, SPHERE_DIMS = 0.37, (40, 40, 40)


def sphere_volume(dims=SPHERE_DIMS, radius=SPHERE_R, voxel=VOXEL, trunc=4 * VOXEL, hole=None):
    """a solid sphere in the middle of a fully observed volume: D = clip((|p - centre| - radius) / trunc, -1, 1), free space outside;
    ``hole``: (z0, z1, y0, y1, x0, x1), a block of voxels left unobserved -> (D, W, origin, centre)"""
    Z, Y, X = dims
    origin = (-0.5 * X * voxel, -0.5 * Y * voxel, 0.4)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    P = np.stack([x, y, z], -1) * voxel + (np.asarray(origin) + 0.5 * voxel)
    centre = np.asarray(origin) + 0.5 * voxel * np.array([X, Y, Z]) + np.array([0.004, -0.007, 0.011])
    D = np.clip((np.linalg.norm(P - centre, axis=-1) - radius) / trunc, -1.0, 1.0).astype(np.float32)
    W = np.full(dims, 3.0, np.float32)
    if hole is not None:
        W[hole[0]:hole[1], hole[2]:hole[3], hole[4]:hole[5]] = 0.0
    return D, W, origin, centre


def wavy(dims, seed=0, holes=True):
    """an analytic volume whose zero set runs into every face of the box (tests/test_gpu_recon3d_routes.py: wavy_volume), any X"""
    Z, Y, X = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    D = (0.6 * np.sin(max(0.37, 2.5 / X) * x + 0.93 * y + 1.31 * z + 0.4 + seed)).astype(np.float32)
    W = np.full(dims, 2.0, np.float32)
    if holes:
        W[(x + 2 * y + 3 * z) % 29 == 0] = 0.0
    return D, W


def colours(dims, seed=3):
    Z, Y, X = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return np.stack([(120.0 + 100.0 * np.sin(0.31 * x + 0.2 * k + 0.17 * y * (k + 1) + 0.23 * z + seed)) for k in range(3)]).astype(np.float32)


# name: (dims (Z, Y, X), kind).  The shapes: one cell; two cells; X no multiple of 4; past a 63-cell wave, a 4-row workgroup and the
# 8-plane march in every direction; and the special volumes.
CASES = {
    "2x2x2": ((2, 2, 2), "wavy-full"), "2x2x3": ((2, 2, 3), "wavy-full"), "3x5x7": ((3, 5, 7), "wavy-full"),
    "9x17x66": ((9, 17, 66), "wavy"), "10x6x130": ((10, 6, 130), "wavy"),
    "unobserved": ((5, 6, 9), "unobserved"), "positive": ((5, 6, 9), "positive"), "holes": ((6, 9, 13), "holes"),
    "d1-zero": ((5, 6, 9), "zero"), "colour": ((6, 7, 70), "colour"),
}
W_MIN = 1.0


def build_case(name):
    """-> dict(D, W [Z][Y][X] fp32, C [3][Z][Y][X] or None, w_min, voxel, origin)"""
    dims, kind = CASES[name]
    D, W = wavy(dims, seed=len(name), holes=kind in ("wavy", "holes", "colour"))
    C = None
    if kind == "unobserved":
        W[:] = 0.0
    elif kind == "positive":
        D = np.abs(D) + np.float32(0.01)
    elif kind == "holes":
        W[2:4, 3:6, 4:8] = 0.5                    # a block below w_min, beside the scattered zeros
    elif kind == "zero":
        D[1::2, ::2, 1::3] = 0.0                  # exact zeros: D1 == 0 on edges from a negative voxel (s = 1), D0 == 0 towards one (s = 0)
        D[2, 3, 4] = -0.0                         # not negative
    elif kind == "colour":
        C = colours(dims)
    return dict(D=D, W=W, C=C, w_min=W_MIN, voxel=VOXEL, origin=(-0.31, 0.27, 1.13), dims=dims)


def reference(case, **kw):
    return mesh(case["D"], case["W"], case["w_min"], case["voxel"], case["origin"], case["C"], **kw)
