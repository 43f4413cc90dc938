"""Every kernel instance of the 3D reconstruction back end (csrc/tsdf.hip, csrc/tsdf_raycast.hip, csrc/depth_consistency.hip,
csrc/cloud_nn.hip) under the route protocol, against the five float64 references the feature suites already use (tests/tsdf_ref.py,
tsdf_color_ref.py, tsdf_raycast_ref.py, consistency_ref.py, cloud_metrics_ref.py) and their comparisons, unchanged.

A route is one kernel instance.  Each case
  * asserts WHICH instance ran, template arguments included (torch.profiler's demangled names);
  * runs the op under both bindings and once more through the C ABI (ctypes) with every device input and output carved out of buffers
    filled with a NaN sentinel -- the volume and colour planes the integration updates in place, the four extraction arrays and the
    counter, the edge colours, the ray-cast maps and the statistics, the consistency maps, the cloud keys / distances / indices /
    centroids: the three results are bit-identical (extraction records after sorting by edge id: their order is the atomic counter's) and
    every band keeps the sentinel;
  * compares with the float64 reference under that reference's own rule (ambiguous share <= 0.03 included);
  * sits on the edges of the launch shapes: volumes of one 16-byte group, one voxel short of / past / exactly one 64 x 16 x 8 brick of the
    integration; Z = 1, Y in 1 / 3 / 5 and X in 4 / 60 / 68 for the extraction with a surface that runs into every face; 0 / 1 / 256 / 257
    edge ids, the out-of-range ones included; images of 1, 2, 6, 7, 8, 9 and 17 ray-cast tiles (the XCD remap) with n_steps 1, 2 and the
    cases' own and rays parallel to an axis; M, N in 0 / 1 / 255 / 256 / 257 on a 1 x 1 x 1 grid; and one volume of more than 2^31 bytes per
    plane that is integrated, extracted and ray-cast.
The SKIP = false / STATS = true instances must give the bits of their plain twins."""
import ctypes
import re

import numpy as np
import pytest
import torch

import cloud_metrics_ref as CM
import consistency_ref as CO
import tsdf_color_ref as CR
import tsdf_raycast_ref as RR
import tsdf_ref as R
from test_gpu_conv2d_routes import BAND, SENT32, _Switches

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernel instances that reach it (tsdf_integrate_kernel<SKIP, COLOR>, tsdf_raycast_kernel<STATS, COLOR>, cloud_nearest_kernel<STATS>)
    "integrate": ["tsdf_integrate_kernel<%s, %s>" % (s, c) for s in ("true", "false") for c in ("false", "true")],
    "extract": ["tsdf_extract_kernel"],
    "edge_colors": ["tsdf_edge_colors_kernel"],
    "raycast": ["tsdf_raycast_kernel<%s, %s>" % (s, c) for s in ("false", "true") for c in ("false", "true")],
    "consistency": ["depth_consistency_kernel"],
    "cloud_keys": ["cloud_cell_keys_kernel"],
    "cloud_nearest": ["cloud_nearest_kernel<false>", "cloud_nearest_kernel<true>"],
    "cloud_centroids": ["cloud_cell_centroids_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(tsdf_\w+_kernel|depth_consistency_kernel|cloud_\w+_kernel)(<[^>()]*>)?")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


# ------------------------------------------------------------------------------------------------------------------- the protocol
class Guard:
    """a tensor of ``shape`` / ``dtype`` carved out of a buffer filled with the sentinel"""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        size = torch.empty(0, dtype=dtype).element_size()
        n = int(np.prod(shape)) * size // 4
        self.buf = torch.full((n + 2 * BAND,), SENT32, dtype=torch.int32, device=DEV)
        self.lo, self.hi = BAND, BAND + n
        self.t = self.buf[BAND:BAND + n].view(dtype).view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return int((self.buf[:self.lo] != SENT32).sum()) + int((self.buf[self.hi:] != SENT32).sum()) == 0

    def untouched(self):
        """nothing at all was written: the bands and the tensor itself still hold the sentinel"""
        return bool((self.buf != SENT32).sum() == 0)


def _intact(what, **guards):
    for k, g in guards.items():
        for i, one in enumerate(g if isinstance(g, (list, tuple)) else [g]):
            assert one.intact(), "%s: written outside %s[%d]" % (what, k, i)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def profiled(want, fn, binding="torch"):
    """run fn() under ``binding`` and the profiler; the suite's kernels that ran must be exactly ``want`` (a set; empty: no launch)"""
    with _Switches(None, binding):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            out = fn()
            torch.cuda.synchronize()
    ran = {m.group(1) + (m.group(2) or "") for e in prof.key_averages() for m in [KERNEL_RE.search(e.key)] if m}
    assert ran == set(want), "ran %s, expected %s" % (sorted(ran), sorted(want))
    return out


def under(binding, fn):
    with _Switches(None, binding):
        out = fn()
        torch.cuda.synchronize()
    return out


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from estdepth_amd import _native
    return _native.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cpu(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------- integrate
def _mats(case):
    from estdepth_amd import camera
    return camera.tsdf_matrices(torch.from_numpy(case["poses"]), torch.from_numpy(case["K"]), case["origin"], case["voxel"])


def _integrate(volume, color, depths, images, mats, p, no_skip):
    from estdepth_amd import ops
    if color is None:
        ops.tsdf_integrate_(volume, depths, [], mats, p["trunc"], p["z_near"], p["conf_min"], False, p["w_max"], no_skip=no_skip)
    else:
        ops.tsdf_integrate_color_(volume, color, depths, [], images, mats, p["trunc"], p["z_near"], p["conf_min"], False, p["w_max"], no_skip=no_skip)
    return volume, color


@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("name", sorted(R.ROUTE_CASES))
def test_integrate_route(name, colour):
    """all four instances on one case: the skipping one under both bindings and on guarded planes against the reference, the SKIP = false
    one the same way against the skipping one's bits"""
    case = R.build_case(name)
    p, dims = case["params"], tuple(case["dims"])
    mats = _mats(case)
    m3 = mats.numpy().reshape(-1, 3, 4)
    images = CR.case_images(case) if colour else None
    D0, W0 = CR.sentinel(dims, 11), np.zeros(dims, np.float32)
    C0 = CR.sentinel((3,) + dims, 12) if colour else None
    vol0 = _dev(np.stack([D0, W0]))
    col0 = _dev(C0) if colour else None
    depths = [_dev(d) for d in case["depths"]]
    imgs = [_dev(i) for i in images] if colour else None
    results = {}
    for no_skip in (False, True):
        want = "tsdf_integrate_kernel<%s, %s>" % ("false" if no_skip else "true", "true" if colour else "false")
        what = "%s %s" % (name, want)
        run = lambda v, c, d=depths, i=imgs: _integrate(v, c, d, i, mats, p, no_skip)           # noqa: E731
        vt, ct = profiled({want}, lambda: run(vol0.clone(), col0.clone() if colour else None))
        vc, cc = under("ctypes", lambda: run(vol0.clone(), col0.clone() if colour else None))
        assert _same(vt, vc) and (not colour or _same(ct, cc)), "%s: the bindings differ" % what
        # the C ABI on guarded planes and guarded maps
        gv = Guard(vol0.shape, fill=vol0)
        gc = Guard(col0.shape, fill=col0) if colour else None
        gd = [Guard(d.shape, fill=d) for d in depths]
        gi = [Guard(i.shape, fill=i) for i in imgs] if colour else []
        under("ctypes", lambda: run(gv.t, gc.t if colour else None, [g.t for g in gd], [g.t for g in gi]))
        _intact(what, volume=gv, depth=gd, image=gi, **({"colour": gc} if colour else {}))
        assert _same(gv.t, vt) and (not colour or _same(gc.t, ct)), "%s: the guarded launch differs from the op" % what
        results[no_skip] = (vt, ct)
    assert _same(results[True][0], results[False][0]), "%s: SKIP = false changes D or the weight" % name
    assert not colour or _same(results[True][1], results[False][1]), "%s: SKIP = false changes the colour" % name
    g = _cpu(results[False][0])
    if colour:
        ref = CR.integrate(D0, W0, C0, m3, case["depths"], images, None, **p)
        fig_c = CR.compare(_cpu(results[False][1]), ref, C_before=C0)
        ref = dict(ref, A=R.integrate(D0, W0, m3, case["depths"], None, **p)["A"], n_updates=None)
        print("RECON-RATIO integrate-colour %s %.3f amb %.4f" % (name, fig_c["max_ratio"], fig_c["amb_share"]))
    else:
        ref = R.integrate(D0, W0, m3, case["depths"], None, **p)
    fig = R.compare(g[0], g[1], ref, D_before=D0, W_before=W0)
    assert fig["updated"] >= 4
    print("RECON-RATIO integrate %s %.3f amb %.4f" % (name, fig["max_ratio"], fig["amb_share"]))


# ---------------------------------------------------------------------------------------------------------------------- extraction
def wavy_volume(dims, seed=0):
    """an analytic volume whose zero set runs into every face of the box: D = 0.6 sin(a x + b y + c z + phase), a few voxels unobserved
    (a = 0.37 rad per voxel, more where X is too short for a sign change)"""
    Z, Y, X = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    D = (0.6 * np.sin(max(0.37, 5.0 / X) * x + 0.93 * y + 1.31 * z + 0.4 + seed)).astype(np.float32)
    W = np.full(dims, 2.0, np.float32)
    W[(x + 2 * y + 3 * z) % 11 == 0] = 0.0
    return D, W


def _extract_raw(vol, dims, voxel, origin, w_min, cap, null=False):
    """estd_tsdf_extract_points on guarded outputs -> (status, count, guards dict)"""
    Z, Y, X = dims
    g = dict(count=Guard((1,), torch.int64, fill=torch.zeros(1, dtype=torch.int64)), xyz=Guard((cap, 3)), normal=Guard((cap, 3)), weight=Guard((cap,)),
             edge=Guard((cap,), torch.int64))
    org = (ctypes.c_float * 3)(*origin)
    pp = (lambda k: None) if null else (lambda k: _p(g[k].t))
    st = _lib().estd_tsdf_extract_points(_p(vol), ctypes.c_void_p(vol.data_ptr() + 4 * Z * Y * X), Z, Y, X, float(voxel), org, float(w_min),
                                         _p(g["count"].t), cap, pp("xyz"), pp("normal"), pp("weight"), pp("edge"), _stream())
    torch.cuda.synchronize()
    return st, int(g["count"].t.item()), g


def _sorted_records(xyz, normal, weight, edge):
    order = torch.argsort(edge)
    return dict(edge=edge[order], xyz=xyz[order], normal=normal[order], weight=weight[order])


EXTRACT_DIMS = [(1, 1, 4), (1, 3, 60), (1, 5, 68), (3, 1, 60), (5, 5, 68), (2, 3, 4), (9, 17, 68)]


@pytest.mark.parametrize("dims", EXTRACT_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_extract_route(dims):
    from estdepth_amd import ops
    voxel, origin, w_min = 0.05, (-0.3, 0.2, 1.0), 1.0
    D, W = wavy_volume(dims)
    ref = R.extract(D, W, w_min, voxel, origin)
    n = len(ref["edge"])
    Z, Y, X = dims
    idx = ref["edge"] // 3
    assert n >= 1 and (Z == 1) == (not (ref["edge"] % 3 == 2).any())              # Z = 1: no +z edge exists
    if min(dims) >= 3:                                                             # the surface reaches the first and last layer of every axis
        for coord, size in ((idx % X, X), ((idx // X) % Y, Y), (idx // (X * Y), Z)):
            assert coord.min() == 0 and coord.max() >= size - 2
    vol = _dev(np.stack([D, W]))
    org = torch.tensor(origin, dtype=torch.float32)
    what = "extract %s" % (dims,)
    run = lambda cap: ops.tsdf_extract_points(vol, voxel, org, w_min, cap)          # noqa: E731
    full = {}
    for binding in ("torch", "ctypes"):
        count, xyz, normal, weight, edge = profiled({"tsdf_extract_kernel"}, lambda: run(n), binding)
        assert int(count.item()) == n, what
        full[binding] = _sorted_records(xyz, normal, weight, edge)
    gvol = Guard(vol.shape, fill=vol)
    st, count, g = _extract_raw(gvol.t, dims, voxel, origin, w_min, n)
    assert st == 0 and count == n and gvol.intact() and _same(gvol.t, vol), what
    _intact(what, **g)
    full["raw"] = _sorted_records(g["xyz"].t, g["normal"].t, g["weight"].t, g["edge"].t)
    for k in ("edge", "xyz", "normal", "weight"):
        assert _same(full["torch"][k], full["ctypes"][k]) and _same(full["torch"][k], full["raw"][k]), "%s: %s differs between the three launches" % (what, k)
    got = {k: _cpu(v) for k, v in full["torch"].items()}
    assert np.array_equal(got["edge"], ref["edge"])
    fig = R.compare_points(got, ref)
    print("RECON-RATIO extract %s xyz %.3f normal %.3f weight %.3f" % ("x".join(map(str, dims)), fig["xyz"], fig["normal"], fig["weight"]))
    # capacity 0 with null output pointers: the count alone; capacity 1 and count - 1: that many records, each a crossing of the reference,
    # nothing written past them
    st, count, g = _extract_raw(vol, dims, voxel, origin, w_min, 0, null=True)
    assert st == 0 and count == n
    _intact(what, **g)
    for cap in sorted({1, n - 1} - {0, n}):
        for binding in ("torch", "ctypes"):
            count, xyz, normal, weight, edge = under(binding, lambda: run(cap))
            assert int(count.item()) == n and edge.shape[0] == cap
            R.compare_points({k: _cpu(v) for k, v in _sorted_records(xyz, normal, weight, edge).items()}, ref)
        st, count, g = _extract_raw(vol, dims, voxel, origin, w_min, cap)
        assert st == 0 and count == n
        _intact(what, **g)
        R.compare_points({k: _cpu(v) for k, v in _sorted_records(g["xyz"].t, g["normal"].t, g["weight"].t, g["edge"].t).items()}, ref)


# --------------------------------------------------------------------------------------------------------------------- edge colours
@pytest.mark.parametrize("n", [0, 1, 256, 257])
def test_edge_colors_route(n):
    """valid ids and, as the contract says, zeros for ids below 0, at 3 * plane or above and for ids whose far end is outside the volume
    (the kernel tests e >= 0 && e < 3 * plane and q[k] + 1 < dims[k] before any load: csrc/tsdf.hip tsdf_edge_colors_kernel)"""
    from estdepth_amd import ops
    dims = (5, 6, 8)
    Z, Y, X = dims
    plane = Z * Y * X
    rng = np.random.RandomState(n)
    D = rng.uniform(-1, 1, dims).astype(np.float32)
    C = rng.uniform(-50, 250, (3,) + dims).astype(np.float32)
    last = lambda x, y, z, k: 3 * ((z * Y + y) * X + x) + k                     # noqa: E731
    outside = [-1, -3 * plane, 3 * plane, 3 * plane + 1, 2 ** 62, -2 ** 62, last(X - 1, 2, 2, 0), last(3, Y - 1, 2, 1), last(3, 2, Z - 1, 2),
               last(X - 1, Y - 1, Z - 1, 0), last(X - 1, Y - 1, Z - 1, 1), last(X - 1, Y - 1, Z - 1, 2)]
    # the valid ids are crossings, as the extraction emits them (s = D0 / (D0 - D1) in [0, 1]: what the bound of the blend assumes)
    crossings = R.extract(D, np.ones(dims, np.float32), 1.0, 0.05, (0.0, 0.0, 0.0))["edge"]
    edge = crossings[rng.randint(0, len(crossings), size=n)].astype(np.int64)
    if n >= 256:
        edge[5:5 + len(outside)] = outside
        edge[-1] = 3 * plane
    vol, col, ed = _dev(np.stack([D, np.ones(dims, np.float32)])), _dev(C), _dev(edge)
    want = {"tsdf_edge_colors_kernel"} if n else set()
    out_t = profiled(want, lambda: ops.tsdf_edge_colors(vol, col, ed))
    out_c = under("ctypes", lambda: ops.tsdf_edge_colors(vol, col, ed))
    gv, gc, ge, go = Guard(vol.shape, fill=vol), Guard(col.shape, fill=col), Guard((n,), torch.int64, fill=ed), Guard((n, 3))
    st = _lib().estd_tsdf_edge_colors(_p(gv.t), _p(gc.t), Z, Y, X, _p(ge.t) if n else None, n, _p(go.t) if n else None, _stream())
    torch.cuda.synchronize()
    assert st == 0
    _intact("edge_colors %d" % n, volume=gv, colour=gc, edge=ge, out=go)
    assert tuple(out_t.shape) == (n, 3) and _same(out_t, out_c) and _same(out_t, go.t)
    got = _cpu(out_t)
    worst = CR.compare_edge_colors(got, edge, D, C)
    if n >= 256:
        assert (got[5:5 + len(outside)] == 0).all() and (got[-1] == 0).all() and (got[:5] != 0).any()
    print("RECON-RATIO edge_colors n%d %.3f" % (n, worst))


# ------------------------------------------------------------------------------------------------------------------------ ray cast
def _fused_slab():
    """the 9 x 17 x 68 slab of tsdf_ref.ROUTE_CASES after its eight frames (numpy-fp32 stand-in of the integration, colour included) and a
    hand-made colour volume; shared by the ray-cast cases (read-only)"""
    if not _SLAB:
        case = R.build_case("r9x17x68-t8-120x160")
        m3 = _mats(case).numpy().reshape(-1, 3, 4)
        Z0 = np.zeros(case["dims"], np.float32)
        o = CR.integrate(Z0, Z0, np.zeros((3,) + tuple(case["dims"]), np.float32), m3, case["depths"], CR.case_images(case), None, dtype=np.float32, **case["params"])
        _SLAB.update(case=case, D=o["D"], W=o["Wt"], C=o["C"])
    return _SLAB


_SLAB = {}
RAY_SIZES = RR.ROUTE_SIZES


def slab_view(H, W, n_steps=None, cam=(0.1, 0.05, 0.0), axis_aligned=False):
    """a render of the slab: the held-out pose (or an axis-aligned camera whose centre column / row has r_x = 0 / r_y = 0 exactly) through
    an H x W image that covers the slab"""
    case = _fused_slab()["case"]
    vox, origin = case["voxel"], case["origin"]
    f = 0.9 * max(H, W)
    if axis_aligned:
        cx, cy = float(W // 2), float(H // 2)
        a = np.float32(1.0 / (f * vox))
        o = (np.asarray(cam) - np.asarray(origin)) / vox - 0.5
        M = np.array([[a, 0, -np.float32(cx) * a, o[0]], [0, a, -np.float32(cy) * a, o[1]], [0, 0, 1.0 / vox, o[2]]], np.float32)
    else:
        K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
        M = RR.ray_matrix(R.look_at(cam, (0.1, 0.05, 1.45)), K, origin, vox)
    t_min, dt = 1.0, vox
    return dict(M=M, H=H, W=W, t_min=t_min, dt=dt, n_steps=n_steps or int(round(0.9 / vox)) + 1)


def _raycast_raw(vol, col, view, w_min, stats, dims):
    """estd_tsdf_raycast / estd_tsdf_raycast_color on guarded maps -> (status, guards dict)"""
    from estdepth_amd import _native
    Z, Y, X = dims
    H, W = view["H"], view["W"]
    g = dict(depth=Guard((H, W)), normal=Guard((H, W, 3)), weight=Guard((H, W)))
    if col is not None:
        g["color"] = Guard((H, W, 3))
    if stats:
        g["stats"] = Guard((H, W, 2), torch.int32)
    d = _native.TsdfRaycastColorDesc() if col is not None else _native.TsdfRaycastDesc()
    d.Z, d.Y, d.X, d.H, d.W, d.n_steps = Z, Y, X, H, W, view["n_steps"]
    d.t_min, d.dt, d.w_min = view["t_min"], view["dt"], w_min
    d.tsdf, d.weight = vol.data_ptr(), vol.data_ptr() + 4 * Z * Y * X
    d.depth, d.normal, d.out_weight = g["depth"].t.data_ptr(), g["normal"].t.data_ptr(), g["weight"].t.data_ptr()
    d.stats = g["stats"].t.data_ptr() if stats else None
    if col is not None:
        d.color, d.out_color = col.data_ptr(), g["color"].t.data_ptr()
    for i, v in enumerate(np.asarray(view["M"], np.float32).reshape(-1).tolist()):
        d.mat[i] = v
    fn = _lib().estd_tsdf_raycast_color if col is not None else _lib().estd_tsdf_raycast
    st = fn(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    return st, g


def _render_all_instances(view, w_min, what):
    """the four instances on one view -> (maps of the plain instance as numpy, colour map)"""
    from estdepth_amd import ops
    s = _fused_slab()
    dims = tuple(s["case"]["dims"])
    vol, col = _dev(np.stack([s["D"], s["W"]])), _dev(s["C"])
    mat = torch.from_numpy(np.asarray(view["M"], np.float32).reshape(12).copy())
    args = (mat, view["H"], view["W"], view["t_min"], view["dt"], view["n_steps"], w_min)
    names = ("depth", "normal", "weight")
    gv, gc = Guard(vol.shape, fill=vol), Guard(col.shape, fill=col)
    out = {}
    for colour in (False, True):
        for stats in (False, True):
            want = "tsdf_raycast_kernel<%s, %s>" % (str(stats).lower(), str(colour).lower())
            if colour and stats:             # the ops expose no statistics with colour: the C ABI alone reaches this instance
                st, g = profiled({want}, lambda: _raycast_raw(gv.t, gc.t, view, w_min, True, dims))
                assert st == 0
                _intact(what + want, volume=gv, colour=gc, **g)
                out[want] = tuple(g[k].t for k in names + ("color", "stats"))
                continue
            if colour:
                run = lambda: ops.tsdf_raycast_color(vol, col, *args)                    # noqa: E731
            else:
                run = lambda: ops.tsdf_raycast(vol, *args, stats=stats)                  # noqa: E731
            rt = profiled({want}, run)
            rc = under("ctypes", run)
            st, g = _raycast_raw(gv.t, gc.t if colour else None, view, w_min, stats, dims)
            assert st == 0
            _intact(what + want, volume=gv, colour=gc, **g)
            raw = tuple(g[k].t for k in names + (("color",) if colour else ()) + (("stats",) if stats else ()))
            assert len(rt) == len(rc) == len(raw)
            for a, b, c in zip(rt, rc, raw):
                assert _same(a, b) and _same(a, c), "%s %s: the three launches differ" % (what, want)
            out[want] = rt
    assert _same(gv.t, vol) and _same(gc.t, col)
    plain = out["tsdf_raycast_kernel<false, false>"]
    for want, maps in out.items():           # STATS and COLOR change no bit of depth / normal / weight; STATS none of the colour
        for a, b in zip(plain, maps[:3]):
            assert _same(a, b), "%s: %s changes a map" % (what, want)
    assert _same(out["tsdf_raycast_kernel<false, true>"][3], out["tsdf_raycast_kernel<true, true>"][3])
    assert _same(out["tsdf_raycast_kernel<true, false>"][3], out["tsdf_raycast_kernel<true, true>"][4])
    return {k: _cpu(v) for k, v in zip(names, plain)}, _cpu(out["tsdf_raycast_kernel<false, true>"][3])


def special_views():
    """(label, view) of the ray-cast cases beside RAY_SIZES: one and two samples, rays parallel to an axis inside and beside the slab"""
    out = []
    for n_steps in (1, 2):
        view = slab_view(17, 33, n_steps=n_steps)
        view["t_min"], view["dt"] = 1.40, 0.09
        out.append(("n_steps=%d" % n_steps, view))
    for cam_x in (0.1, 2.0):
        out.append(("axis-%s" % ("inside" if cam_x < 1 else "outside"), slab_view(17, 17, cam=(cam_x, 0.05, 0.0), axis_aligned=True)))
    return out


def _compare_render(got, colour, view, w_min, what):
    s = _fused_slab()
    ref = RR.raycast(s["D"], s["W"], view["M"], view["H"], view["W"], view["t_min"], view["dt"], view["n_steps"], w_min)
    fig = RR.compare(got, ref, what)
    cref = CR.render_colors(s["D"], s["W"], s["C"], view, w_min, ray=ref)
    cfig = CR.compare_render(colour, cref, what)
    print("RECON-RATIO raycast %s depth %.3f normal %.3f weight %.3f colour %.3f hit %d amb %.4f / %.4f"
          % (what, fig["depth_ratio"], fig["normal_ratio"], fig["weight_ratio"], cfig["color_ratio"], fig["hit"], fig["amb_share"], cfig["amb_share"]))
    return fig


@pytest.mark.parametrize("hw", RAY_SIZES, ids=lambda s: "%dx%d" % s)
def test_raycast_route(hw):
    view = slab_view(*hw)
    got, colour = _render_all_instances(view, 1.0, "raycast %dx%d " % hw)
    fig = _compare_render(got, colour, view, 1.0, "%dx%d" % hw)
    assert fig["hit"] >= max(1, hw[0] * hw[1] // 16)


@pytest.mark.parametrize("n_steps", [1, 2])
def test_raycast_one_and_two_samples(n_steps):
    """one sample can never hit (a hit needs a pair); two samples placed around the sphere's near side hit"""
    view = dict(special_views())["n_steps=%d" % n_steps]
    got, colour = _render_all_instances(view, 1.0, "raycast n_steps %d " % n_steps)
    fig = _compare_render(got, colour, view, 1.0, "n_steps=%d" % n_steps)
    assert (fig["hit"] == 0) if n_steps == 1 else (fig["hit"] > 20)


@pytest.mark.parametrize("cam_x,inside", [(0.1, True), (2.0, False)], ids=["inside", "outside"])
def test_raycast_rays_parallel_to_an_axis(cam_x, inside):
    """an axis-aligned camera: r_x = 0 exactly on the centre column and r_y = 0 on the centre row; with the camera beside the slab those
    rays never enter it (o_x outside [0, X - 1])"""
    view = dict(special_views())["axis-%s" % ("inside" if inside else "outside")]
    M = np.asarray(view["M"], np.float32)
    u = np.arange(17, dtype=np.float32)
    rx = (M[0, 0].astype(np.float64) * u + M[0, 2].astype(np.float64)).astype(np.float32)
    assert rx[8] == 0 and (rx[:8] < 0).all() and (rx[9:] > 0).all()
    assert (0 <= M[0, 3] <= 67) == inside
    got, colour = _render_all_instances(view, 1.0, "raycast axis %s " % inside)
    fig = _compare_render(got, colour, view, 1.0, "axis-%s" % ("inside" if inside else "outside"))
    assert (got["depth"][:, 8] > 0).any() == inside and (not inside or fig["hit"] >= 20)


# --------------------------------------------------------------------------------------------------------------------- consistency
CONS_SIZES = CO.ROUTE_SIZES


def _consistency_raw(target, sources, mats, hw):
    from estdepth_amd import _native
    H, W = hw
    g = {k: Guard((H, W)) for k in ("views", "visible", "depth", "rel_err")}
    d = _native.DepthConsistencyDesc()
    d.H, d.W, d.S = H, W, len(sources)
    d.px_max, d.rel_max, d.z_near = CO.PX_MAX, CO.REL_MAX, CO.Z_NEAR
    d.target = target.data_ptr()
    d.views, d.visible, d.depth, d.rel_err = (g[k].t.data_ptr() for k in ("views", "visible", "depth", "rel_err"))
    flat = mats.reshape(-1).tolist()
    for s, src in enumerate(sources):
        d.source[s] = src.data_ptr()
        for i in range(24):
            d.mats[s][i // 12][i % 12] = flat[s * 24 + i]
    st = _lib().estd_depth_consistency(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    return st, g


@pytest.mark.parametrize("S", CO.ROUTE_SOURCES)
@pytest.mark.parametrize("hw", CONS_SIZES, ids=lambda s: "%dx%d" % s)
def test_consistency_route(hw, S):
    from estdepth_amd import ops
    c = CO.make_case(hw, S, seed=S + hw[0], name="route")
    ref = CO.evaluate(c["target"], c["sources"], c["mats"])
    target, sources = _dev(c["target"]), [_dev(s) for s in c["sources"]]
    mats = torch.from_numpy(np.ascontiguousarray(c["mats"].reshape(S, 2, 12)))
    run = lambda: ops.depth_consistency(target, sources, mats, CO.PX_MAX, CO.REL_MAX, CO.Z_NEAR)             # noqa: E731
    rt = profiled({"depth_consistency_kernel"}, run)
    rc = under("ctypes", run)
    gt, gs = Guard(target.shape, fill=target), [Guard(s.shape, fill=s) for s in sources]
    st, g = _consistency_raw(gt.t, [x.t for x in gs], mats, hw)
    what = "consistency %dx%d S%d" % (hw + (S,))
    assert st == 0
    _intact(what, target=gt, source=gs, **g)
    for a, b, k in zip(rt, rc, ("views", "visible", "depth", "rel_err")):
        assert _same(a, b) and _same(a, g[k].t), "%s: %s differs between the three launches" % (what, k)
    fig = CO.compare({k: _cpu(v) for k, v in zip(("views", "visible", "depth", "rel_err"), rt)}, ref, what)
    assert fig["valid"] >= 4
    print("RECON-RATIO consistency %dx%d-S%d depth %.3f rel_err %.3f amb %.4f" % (hw + (S, fig["depth_ratio"], fig["rel_err_ratio"], fig["amb_share"])))


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_consistency_refuses_a_one_pixel_map(binding):
    """the bilinear read needs a 2 x 2 neighbourhood: a 1 x 1 map is refused before any launch by both bindings and by the C ABI"""
    from estdepth_amd import ops
    one = torch.ones(1, 1, device=DEV)
    mats = torch.zeros(1, 2, 12)
    with pytest.raises(RuntimeError):
        profiled(set(), lambda: ops.depth_consistency(one, [one], mats, 1.0, 0.01, 1e-3), binding)
    assert _consistency_raw(one, [one], mats, (1, 1))[0] == -1


# --------------------------------------------------------------------------------------------------------------------------- clouds
CLOUD_N = list(CM.ROUTE_SIZES)


def _grid(target, max_dist, cell):
    from estdepth_amd import cloud_metrics as M
    return M.PointGrid(target, max_dist, cell)


@pytest.mark.parametrize("M_", CLOUD_N)
@pytest.mark.parametrize("N_", CLOUD_N)
def test_cloud_nearest_route(N_, M_):
    """N targets x M queries on the default grid and on a grid of one cell; both instances; keys, distances and indices on guarded buffers"""
    from estdepth_amd import _native, ops
    case = CM.route_case(N_, M_)
    target, query, max_dist = case["target"], case["query"], case["max_dist"]
    dmin = CM.nearest64(query, target)[0]
    what = "cloud %d x %d" % (N_, M_)
    q, t = _dev(query).reshape(M_, 3), _dev(target).reshape(N_, 3)
    results = []
    for cell in (None, 1e7):
        grid = under("torch", lambda: _grid(t, max_dist, cell))
        assert cell is None or tuple(grid.dims) == (1, 1, 1)
        for stats in (False, True):
            want = {"cloud_nearest_kernel<%s>" % str(stats).lower()} | ({"cloud_cell_keys_kernel"} if N_ else set()) if M_ else set()
            rt = profiled(want, lambda: grid.query(q, stats=stats))
            rc = under("ctypes", lambda: grid.query(q, stats=stats))
            for a, b in zip(rt, rc):
                assert _same(a, b), "%s: the bindings differ" % what
            results.append(rt[:2])
            if not M_:
                continue
            # the C ABI: the query keys, then the search, everything on guarded buffers
            lo3, dims3 = (ctypes.c_float * 3)(*grid.lo.tolist()), (ctypes.c_int * 3)(*grid.dims)
            gq, gk = Guard(q.shape, fill=q), Guard((M_,), torch.int64)
            if N_:
                assert _lib().estd_cloud_cell_keys(_p(gq.t), M_, lo3, grid.cell, dims3, _p(gk.t), _stream()) == 0
                torch.cuda.synchronize()
                assert _same(gk.t, under("torch", lambda: ops.cloud_cell_keys(q, grid.lo, grid.cell, grid.dims)))
                order = torch.sort(gk.t, stable=True)[1]
            else:
                order = torch.arange(M_, device=DEV)
            go, gr = Guard((M_,), torch.int64, fill=order), Guard(grid.records.shape, fill=grid.records)
            gs, gd, gi = Guard(grid.cell_start.shape, torch.int32, fill=grid.cell_start), Guard((M_,)), Guard((M_,), torch.int64)
            gst = Guard((M_,), torch.int32)
            d = _native.CloudNearestDesc()
            d.M, d.N = M_, N_
            d.query, d.order, d.records, d.cell_start = gq.t.data_ptr(), go.t.data_ptr(), gr.t.data_ptr(), gs.t.data_ptr()
            d.dist, d.index, d.stats = gd.t.data_ptr(), gi.t.data_ptr(), gst.t.data_ptr() if stats else None
            d.cell, d.max_dist = grid.cell, max_dist
            for j in range(3):
                d.lo[j], d.dims[j] = float(grid.lo[j]), grid.dims[j]
            assert _lib().estd_cloud_nearest(ctypes.byref(d), _stream()) == 0
            torch.cuda.synchronize()
            _intact(what, query=gq, keys=gk, order=go, records=gr, cell_start=gs, dist=gd, index=gi, stats=gst)
            assert stats or gst.untouched()
            assert _same(gd.t, rt[0]) and _same(gi.t, rt[1]) and (not stats or _same(gst.t, rt[2])), "%s: the guarded launch differs" % what
    for dist, index in results[1:]:                  # neither the grid nor STATS changes a bit
        assert _same(dist, results[0][0]) and _same(index, results[0][1]), what
    dist, index = _cpu(results[0][0]), _cpu(results[0][1])
    fig = CM.compare(dist, index, query, target, max_dist, dmin, what)
    CM.check_ties(index, target, what)
    if N_ > 1 and M_ > 1:
        assert index[0] == 0 and dist[0] == 0
    print("RECON-RATIO cloud_nearest %dx%d dist %.3f index %.3f" % (N_, M_, fig["e_dist"], fig["e_index"]))


def test_cloud_nearest_finds_a_target_at_exactly_max_dist():
    """the closed form of the lattice pair with max_dist = the distance itself: d2 == r2 exactly, and d2 <= r2 finds it"""
    a, b = CM.lattice_pair()
    for binding in ("torch", "ctypes"):
        dist, index = under(binding, lambda: _grid(_dev(b), CM.DELTA, None).query(_dev(a)))
        CM.check_lattice(_cpu(dist), _cpu(index))


# K cells x (3 + C) values, one thread each in blocks of 256: 3 (the least), 255, 256 and 258 threads (3 + C divides neither 1 nor 257)
@pytest.mark.parametrize("K,C", [(1, 0), (85, 0), (51, 2), (32, 5), (43, 3)])
def test_cloud_centroids_route(K, C):
    from estdepth_amd import ops
    rng = np.random.RandomState(K * 10 + C)
    counts = rng.randint(1, 6, size=K)
    n = int(counts.sum())
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    att = rng.uniform(-1, 1, (n, C)).astype(np.float32) if C else None
    order = rng.permutation(n).astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    p, a, o, s = _dev(pts), (_dev(att) if C else None), _dev(order), _dev(seg)
    run = lambda: ops.cloud_cell_centroids(p, a, o, s)                                       # noqa: E731
    rt = profiled({"cloud_cell_centroids_kernel"}, run)
    rc = under("ctypes", run)
    gp, ga, go_, gs = Guard(p.shape, fill=p), (Guard(a.shape, fill=a) if C else None), Guard(o.shape, torch.int64, fill=o), Guard(s.shape, torch.int64, fill=s)
    out, oa = Guard((K, 3)), (Guard((K, C)) if C else None)
    st = _lib().estd_cloud_cell_centroids(_p(gp.t), _p(ga.t) if C else None, C, n, _p(go_.t), _p(gs.t), K, _p(out.t), _p(oa.t) if C else None, _stream())
    torch.cuda.synchronize()
    what = "centroids K%d C%d" % (K, C)
    assert st == 0 and K * (3 + C) in (3, 255, 256, 258)
    _intact(what, points=gp, order=go_, segments=gs, out=out, **({"attrs": ga, "out_attrs": oa} if C else {}))
    assert _same(rt[0], rc[0]) and _same(rt[0], out.t) and (not C or (_same(rt[1], rc[1]) and _same(rt[1], oa.t))), what
    # the mean of each segment, summed in float64 in the sorted order and rounded once
    for got, src in ((rt[0], pts),) + (((rt[1], att),) if C else ()):
        want = np.stack([src[order[seg[k]:seg[k + 1]]].astype(np.float64).sum(0) / counts[k] for k in range(K)])
        assert np.array_equal(_cpu(got), want.astype(np.float32)), what


# ---------------------------------------------------------------------------------------------- one volume above 2^31 bytes per plane
BIG_DIMS = (520, 1024, 1024)                # 2.18e9 bytes per plane: the layers z >= 512 lie past byte 2^31 of each
BIG_ORIGIN = (0.1 - 1000 * R.VOXEL, 0.05 - 1000 * R.VOXEL, 2.6 - 515 * R.VOXEL)      # the scene sits in the volume's far corner
BIG_BRICKS = [(504, 992, 960), (512, 992, 960), (504, 1008, 960), (512, 1008, 960), (472, 992, 960), (0, 0, 0)]      # (z0, y0, x0) of 8 x 16 x 64


def big_case():
    """one 120 x 160 frame of the scene into BIG_DIMS: the plane z = 2.6 runs through layer 515, the sphere sits around voxel (1000, 1000)"""
    poses = R.scene_poses(1, seed=3)
    K = R.intrinsics(120, 160)
    depths = np.stack([R.raycast_scene(poses[0], K, 120, 160)]).astype(np.float32)
    return dict(dims=BIG_DIMS, origin=BIG_ORIGIN, voxel=R.VOXEL, poses=poses, K=K, depths=depths,
                params=dict(trunc=4 * R.VOXEL, z_near=1e-3, conf_min=0.0, weighted=False, w_max=64.0))


def big_brick_range(b):
    return tuple((b[i], b[i] + s) for i, s in enumerate((8, 16, 64)))


BIG_EXTRACT_RANGE = ((500, 520), (980, 1024), (940, 1024))      # the far corner with a halo of two voxels on its inner faces
BIG_RAY_FIRST = (880, 880, 400)                                  # (x0, y0, z0): every observed voxel lies at or past it (asserted on the device)


def test_volume_above_2_31_bytes_per_plane():
    """integrate (both bindings, guarded planes), extract and ray-cast BIG_DIMS; the references on 8 x 16 x 64 bricks (the last one and
    the two pairs on either side of byte 2^31 included) evaluated at the volume's own voxel indices with the volume's own matrices, the
    extraction on the far corner, the ray cast on the region that holds every observed voxel.  No colour: 4.4 GB per volume as it is."""
    from estdepth_amd import ops
    case = big_case()
    Z, Y, X = BIG_DIMS
    assert Z * Y * X * 4 > 2 ** 31
    p, mats = case["params"], _mats(case)
    m3 = mats.numpy().reshape(-1, 3, 4)
    depths = [_dev(case["depths"][0])]
    want = "tsdf_integrate_kernel<true, false>"
    run = lambda v: _integrate(v, None, depths, None, mats, p, False)[0]                  # noqa: E731
    vt = profiled({want}, lambda: run(torch.zeros((2,) + BIG_DIMS, device=DEV)))
    vc = under("ctypes", lambda: run(torch.zeros((2,) + BIG_DIMS, device=DEV)))
    assert _same(vt, vc), "big: the bindings differ"
    del vc
    gv = Guard((2,) + BIG_DIMS)
    gv.t.zero_()
    under("ctypes", lambda: run(gv.t))
    assert gv.intact() and _same(gv.t, vt), "big: the guarded launch differs or wrote outside the planes"
    del gv
    torch.cuda.empty_cache()
    for b in BIG_BRICKS:
        rng = big_brick_range(b)
        sl = tuple(slice(a, c) for a, c in rng)
        Z0 = np.zeros((8, 16, 64), np.float32)
        ref = R.integrate(Z0, Z0, m3, case["depths"], None, voxel_range=rng, **p)
        got = _cpu(vt[(slice(None),) + sl])
        fig = R.compare(got[0], got[1], ref, D_before=Z0, W_before=Z0)
        assert (fig["updated"] == 0) == (b == (0, 0, 0)), (b, fig)
        print("RECON-RATIO integrate big-%s %.3f amb %.4f updated %d" % ("-".join(map(str, b)), fig["max_ratio"], fig["amb_share"], fig["updated"]))
    x0, y0, z0 = BIG_RAY_FIRST
    seen = int(torch.count_nonzero(vt[1]))
    assert seen == int(torch.count_nonzero(vt[1, z0:, y0:, x0:])) > 50000 and int(torch.count_nonzero(vt[1, 512:])) > 1000
    # ---- extraction: every crossing of the far corner, as the reference has them at the volume's own indices
    org = torch.tensor(BIG_ORIGIN, dtype=torch.float32)
    count = int(ops.tsdf_extract_points(vt, R.VOXEL, org, 1.0, 0)[0].item())
    assert count > 1000
    recs = {}
    for binding in ("torch", "ctypes"):
        c, xyz, normal, weight, edge = profiled({"tsdf_extract_kernel"}, lambda: ops.tsdf_extract_points(vt, R.VOXEL, org, 1.0, count), binding)
        assert int(c.item()) == count
        recs[binding] = _sorted_records(xyz, normal, weight, edge)
    st, c, g = _extract_raw(vt, BIG_DIMS, R.VOXEL, BIG_ORIGIN, 1.0, count)
    assert st == 0 and c == count
    _intact("big extract", **g)
    recs["raw"] = _sorted_records(g["xyz"].t, g["normal"].t, g["weight"].t, g["edge"].t)
    for k in ("edge", "xyz", "normal", "weight"):
        assert _same(recs["torch"][k], recs["ctypes"][k]) and _same(recs["torch"][k], recs["raw"][k]), "big extract: %s differs" % k
    (ez0, ez1), (ey0, ey1), (ex0, ex1) = BIG_EXTRACT_RANGE
    corner = _cpu(vt[:, ez0:ez1, ey0:ey1, ex0:ex1])
    ref = R.extract(corner[0], corner[1], 1.0, R.VOXEL, BIG_ORIGIN, voxel_range=BIG_EXTRACT_RANGE, dims=BIG_DIMS)

    def inner(edge):
        idx = edge // 3
        return (idx // (X * Y) >= ez0 + 2) & ((idx // X) % Y >= ey0 + 2) & (idx % X >= ex0 + 2)
    keep = inner(ref["edge"])
    ref = {k: v[keep] for k, v in ref.items()}
    got = {k: _cpu(v) for k, v in recs["torch"].items()}
    sel = inner(got["edge"])
    got = {k: v[sel] for k, v in got.items()}
    assert np.array_equal(got["edge"], ref["edge"]) and len(ref["edge"]) > 500 and int(ref["edge"].max()) // 3 * 4 > 2 ** 31
    fig = R.compare_points(got, ref)
    print("RECON-RATIO extract big xyz %.3f normal %.3f weight %.3f records %d of %d" % (fig["xyz"], fig["normal"], fig["weight"], len(ref["edge"]), count))
    # ---- ray cast from the fused camera
    M = RR.ray_matrix(case["poses"][0], case["K"], BIG_ORIGIN, R.VOXEL)
    view = dict(M=M, H=120, W=160, t_min=RR.T_MIN, dt=R.VOXEL, n_steps=RR.N_STEPS)
    mat = torch.from_numpy(M.reshape(12).copy())
    args = (mat, 120, 160, view["t_min"], view["dt"], view["n_steps"], 1.0)
    rt = profiled({"tsdf_raycast_kernel<false, false>"}, lambda: ops.tsdf_raycast(vt, *args))
    rc = under("ctypes", lambda: ops.tsdf_raycast(vt, *args))
    st, g = _raycast_raw(vt, None, view, 1.0, False, BIG_DIMS)
    assert st == 0
    _intact("big raycast", **g)
    for a, b, k in zip(rt, rc, ("depth", "normal", "weight")):
        assert _same(a, b) and _same(a, g[k].t), "big raycast: %s differs between the three launches" % k
    crop = _cpu(vt[:, z0:, y0:, x0:])
    ref = RR.raycast(crop[0], crop[1], M, 120, 160, view["t_min"], view["dt"], view["n_steps"], 1.0, index_offset=BIG_RAY_FIRST)
    fig = RR.compare({k: _cpu(v) for k, v in zip(("depth", "normal", "weight"), rt)}, ref, "big")
    assert fig["hit"] > 5000
    print("RECON-RATIO raycast big depth %.3f normal %.3f weight %.3f hit %d amb %.4f" % (fig["depth_ratio"], fig["normal_ratio"], fig["weight_ratio"], fig["hit"], fig["amb_share"]))
