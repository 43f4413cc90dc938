"""The kernels of the global registration (csrc/register/global_register.hip) under the route protocol of
tests/test_gpu_cloud_knn_routes.py, against the numpy reference of tests/global_reg_ref.py: EQUALITY TO THE BIT of hist, pairs, desc,
valid and invalid (descriptors), of index, d2 and d2_second (matching), of count, status, the winner and the winner's T (hypotheses);
ssq within the running error bound derived in the reference's docstring.

The source lives in a sub-directory the kernel ledger (tests/test_kernel_ledger_cpu.py) does not walk; this file carries the ledger's
guarantee for it: INSTANCES names every kernel the source emits (tests/test_global_reg_resources_cpu.py compiles the file and asserts that
the emitted set equals the claimed one, with nothing spilled), and every entry is exercised by a case here.

Every case asserts WHICH kernels ran (torch.profiler's demangled names; none for empty inputs) and runs under both bindings and twice:
the same bits.  The shapes are the smallest at which a kernel can go wrong: one point, two, a wave and one more, more than one workgroup;
k = 3, 8, 32; lists shorter than k, padded with -1, naming a row beyond the cloud; points and neighbours without a normal; duplicate
points (len = 0) and a neighbour straight along the normal (|v| = 0); the cloud 64 m and 512 m from the origin; query and target counts
around a wave, a workgroup and the LDS tile of the matcher (128 rows) with descriptors on a coarse lattice, so that equal distances are
the rule and the smallest index has to win; correspondences around a wave with every status produced on purpose."""
import ctypes
import re

import numpy as np
import pytest
import torch

from estdepth_amd.ops import cloud_fpfh, cloud_spfh, feature_match, ransac_pairs  # noqa: F401 -- the feature under test: without it this module does not import

import global_reg_ref as R
from cloud_knn_ref import knn32
from test_gpu_conv2d_routes import _Switches
from test_gpu_recon3d_routes import Guard, _cpu, _dev, _intact, _lib, _p, _same, _stream, under

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

INSTANCES = {
    # route: the kernels that reach it
    "cloud_spfh": ["greg_spfh_kernel<true>", "greg_spfh_kernel<false>"],
    "cloud_fpfh": ["greg_fpfh_kernel"],
    "feature_match": ["greg_match_kernel"],
    "ransac_pairs": ["greg_ransac_kernel"],
}
NOT_ROUTES = {}
KERNEL_RE = re.compile(r"\b(greg_\w+_kernel)(<[^>()]*>)?")
ALL = {k for ks in INSTANCES.values() for k in ks}
SPFH = {True: "greg_spfh_kernel<true>", False: "greg_spfh_kernel<false>"}
FPFH, MATCH, RANSAC = "greg_fpfh_kernel", "greg_match_kernel", "greg_ransac_kernel"
MATCH_TILE = 128
_RAN = set()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


def profiled(want, fn, binding="torch"):
    """run fn() under ``binding`` and the profiler; the suite's kernels that ran must be exactly ``want`` (a set; empty: no launch)"""
    with _Switches(None, binding):
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            out = fn()
            torch.cuda.synchronize()
    ran = {m.group(1) + (m.group(2) or "") for e in prof.key_averages() for m in [KERNEL_RE.search(e.key)] if m}
    assert ran == set(want), "ran %s, expected %s" % (sorted(ran), sorted(want))
    _RAN.update(ran)
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) if x.element_size() == 1 else _same(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ descriptors
def descriptor_case(n, k, offset=0.0, seed=0):
    """a cloud of ``n`` points in a 0.4 m box at ``offset`` with unit normals and its lists, with every special row the contract names"""
    rng = np.random.RandomState(seed + 31 * n + k)
    p = (rng.rand(n, 3) * 0.4).astype(np.float64)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    if n >= 65:
        p[5] = p[4]                                      # a duplicate point: len = 0
        p[9] = p[8] + (0.0625, 0.0, 0.0)                 # a neighbour straight along the normal: dn parallel to u, |v| = 0
        nrm[8] = (1.0, 0.0, 0.0)
        p[[8, 9]] = np.round(p[[8, 9]] * 1024) / 1024    # so that the difference is exact in fp32 at every placement
    p = (p + offset).astype(np.float32)
    nrm = nrm.astype(np.float32)
    if n >= 65:
        nrm[[0, 20, 63, 64, n - 1]] = 0.0                # no normal: on a point, on neighbours, either side of the wave boundary, the last row
    _, index, count = knn32(p, p, k, 0.15)
    if n >= 65:
        for s, t in SKIPPED_PAIRS:                       # whatever the draw: the special neighbour IS in the row's list
            if t not in index[s, :count[s]]:
                index[s, 1], count[s] = t, max(int(count[s]), 2)
        index[2, 0], index[3, min(1, k - 1)], index[64, 0], index[n - 1, 0] = n, -1, 2 ** 31 - 1, -2 ** 31      # never an address
        count[6] = min(int(count[6]), 1)                 # a list cut short: the entries behind it are not read
        count[7] = k + 5                                 # clamped to k
        count[10] = -3                                   # clamped to 0
    return p, nrm, index.astype(np.int32), count.astype(np.int32)


SKIPPED_PAIRS = ((8, 9), (4, 5))                         # (row, neighbour): |v| = 0 and len = 0


def counted_but_for(s, t, nrm, index, count):
    """the pairs row ``s`` counts when the ONLY entry skipped for its geometry is ``t``: the used entries that are not the row itself, lie in
    the cloud and have a normal, less that one"""
    n = nrm.shape[0]
    used = [int(j) for j in index[s, :min(max(int(count[s]), 0), index.shape[1])]]
    assert t in used, (s, t, used)
    return sum(1 for j in used if j != s and 0 <= j < n and nrm[j].any()) - 1


def run_descriptors(p, nrm, index, count, oriented):
    hist, pairs = cloud_spfh(p, nrm, index, count, oriented)
    return (hist, pairs) + tuple(cloud_fpfh(p, nrm, index, count, hist, pairs))


DESC_CASES = [(n, k, 0.0) for n in (1, 2, 65, 257) for k in (3, 8, 32)] + [(257, 8, 64.0), (257, 8, 512.0)]


@pytest.mark.parametrize("n,k,offset", DESC_CASES)
@pytest.mark.parametrize("oriented", [True, False])
def test_descriptor_route(n, k, offset, oriented):
    p, nrm, index, count = descriptor_case(n, k, offset)
    hist, pairs = R.spfh(p, nrm, index, count, oriented)
    desc, valid, invalid = R.fpfh(p, nrm, index, count, hist, pairs)
    args = tuple(_dev(x) for x in (p, nrm, index, count))
    ran = {SPFH[oriented], FPFH}
    first = profiled(ran, lambda: run_descriptors(*args, oriented))
    for binding in ("torch", "ctypes"):
        for again in range(2):
            assert same(first, profiled(ran, lambda: run_descriptors(*args, oriented), binding)), "the bits differ under %s, call %d" % (binding, again)
    got = [_cpu(x) for x in first]
    assert got[0].dtype == np.int32 and got[0].shape == (n, 33) and (got[0] == hist).all(), np.argwhere(got[0] != hist)[:5]
    assert (got[1] == pairs).all() and (got[1] == got[0][:, :11].sum(1)).all() and (got[1] == got[0][:, 22:].sum(1)).all()
    assert got[2].dtype == np.float32 and got[2].tobytes() == desc.tobytes(), np.argwhere(got[2] != desc)[:5]
    assert (got[3] == valid).all() and int(got[4][0]) == invalid == int((valid == 0).sum())
    if n >= 65:
        assert pairs[0] == 0 and pairs[10] == 0 and valid[0] == 0 and pairs.max() > 0 and (k < 8 or valid.sum() > n // 2)
        for s, t in SKIPPED_PAIRS:                       # the skip branches (|v| = 0, len = 0) were taken, by the reference and the device
            assert pairs[s] == got[1][s] == counted_but_for(s, t, nrm, index, count), (s, t, pairs[s])
    print("GLOBAL-REG-ROUTE descriptors n=%d k=%d at %g m oriented=%s: %d pairs counted, %d rows valid" % (n, k, offset, oriented, pairs.sum(), valid.sum()))


def test_fpfh_through_the_grid_equals_the_reference():
    from estdepth_amd import registration
    p, nrm, _, _ = descriptor_case(257, 16)
    for oriented in (True, False):
        want = R.descriptors(p, nrm, 16, 0.15, oriented)
        got = under("torch", lambda: registration.fpfh(_dev(p), _dev(nrm), 16, 0.15, oriented))
        assert _cpu(got["desc"]).tobytes() == want["desc"].tobytes() and (_cpu(got["valid"]) == want["valid"]).all()
        assert (_cpu(got["pairs"]) == want["pairs"]).all() and got["invalid"] == want["invalid"]


def test_the_descriptor_entry_points_on_guarded_buffers():
    n, k = 257, 8
    p, nrm, index, count = descriptor_case(n, k)
    g = dict(points=Guard((n, 3), fill=_dev(p)), normal=Guard((n, 3), fill=_dev(nrm)), index=Guard((n, k), torch.int32, fill=_dev(index)),
             count=Guard((n,), torch.int32, fill=_dev(count)), hist=Guard((n, 33), torch.int32), pairs=Guard((n,), torch.int32),
             desc=Guard((n, 33)), valid=Guard(((n + 3) // 4 * 4,), torch.uint8), invalid=Guard((1,), torch.int64))
    assert _lib().estd_cloud_spfh(_p(g["points"].t), _p(g["normal"].t), n, _p(g["index"].t), _p(g["count"].t), k, 1, _p(g["hist"].t),
                                  _p(g["pairs"].t), _stream()) == 0
    assert _lib().estd_cloud_fpfh(_p(g["points"].t), _p(g["normal"].t), n, _p(g["index"].t), _p(g["count"].t), k, _p(g["hist"].t),
                                  _p(g["pairs"].t), _p(g["desc"].t), _p(g["valid"].t), _p(g["invalid"].t), _stream()) == 0
    torch.cuda.synchronize()
    _intact("descriptors", **g)
    assert torch.equal(g["index"].t, _dev(index)) and torch.equal(g["points"].t, _dev(p)), "an input was written"
    want = under("ctypes", lambda: run_descriptors(_dev(p), _dev(nrm), _dev(index), _dev(count), True))
    assert same((g["hist"].t, g["pairs"].t, g["desc"].t, g["valid"].t[:n], g["invalid"].t), want)


# ------------------------------------------------------------------------------------------------------------ matching
def match_case(m, n, seed=0, masks=True):
    """descriptors on the lattice of eighths: equal distances are common, so the index decides"""
    rng = np.random.RandomState(seed + 1000 * m + n)
    a = (rng.randint(0, 3, size=(m, 33)) / 8.0).astype(np.float32)
    b = (rng.randint(0, 3, size=(n, 33)) / 8.0).astype(np.float32)
    if n >= 63:
        b[40] = b[11]                                    # duplicated target rows: the smallest index must win
        b[n - 1] = b[11]
        if m:
            a[0] = b[11]
    av = (rng.rand(m) < 0.8).astype(np.uint8) if masks else None
    bv = (rng.rand(n) < 0.8).astype(np.uint8) if masks else None
    if masks and n >= 63:
        bv[[11, 40, n - 1]] = 1
        if m:
            av[0] = 1
    return a, b, av, bv


SIZES = (0, 1, 63, 64, 65, 257, MATCH_TILE + 1)
MATCH_CASES = sorted({(m, MATCH_TILE + 1) for m in SIZES} | {(65, n) for n in SIZES} | {(0, 0), (1, 1), (257, 257), (64, 2 * MATCH_TILE)})


@pytest.mark.parametrize("m,n", MATCH_CASES)
@pytest.mark.parametrize("masks", [True, False])
def test_match_route(m, n, masks):
    a, b, av, bv = match_case(m, n, masks=masks)
    want = R.match(a, b, av, bv)
    args = tuple(None if x is None else _dev(x) for x in (a, b, av, bv))
    ran = {MATCH} if m else set()
    first = profiled(ran, lambda: feature_match(*args))
    for binding in ("torch", "ctypes"):
        for again in range(2):
            assert same(first, profiled(ran, lambda: feature_match(*args), binding)), "the bits differ under %s, call %d" % (binding, again)
    got = [_cpu(x) for x in first]
    assert got[0].dtype == np.int32 and (got[0] == want[0]).all(), np.argwhere(got[0] != want[0])[:5]
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    if m and n >= 63:
        assert got[0][0] == 11 and got[1][0] == 0 and got[2][0] == 0
    print("GLOBAL-REG-ROUTE match %d x %d masks=%s: %d rows matched, %d with a tie for the first place" % (m, n, masks, (got[0] >= 0).sum(), (got[1] == got[2]).sum()))


def test_all_invalid_sides_find_nothing():
    a, b, _, _ = match_case(65, MATCH_TILE + 1)
    for av, bv in ((np.zeros(65, np.uint8), None), (None, np.zeros(MATCH_TILE + 1, np.uint8)), (np.zeros(65, np.uint8), np.zeros(MATCH_TILE + 1, np.uint8))):
        for binding in ("torch", "ctypes"):
            index, d2, second = profiled({MATCH}, lambda: feature_match(_dev(a), _dev(b), None if av is None else _dev(av), None if bv is None else _dev(bv)), binding)
            assert bool((index == -1).all()) and bool(torch.isinf(d2).all()) and bool(torch.isinf(second).all())


def test_match_features_is_mutual():
    from estdepth_amd import registration
    a, b, av, bv = match_case(257, 257)
    want, wd2 = R.mutual_pairs(a, b, av, bv, fn=R.match)
    pairs, d2 = under("torch", lambda: registration.match_features(_dev(a), _dev(b), _dev(av), _dev(bv)))
    assert pairs.dtype == torch.int64 and (_cpu(pairs) == want).all() and _cpu(d2).tobytes() == wd2.tobytes() and want.shape[0] > 0
    one, _ = under("torch", lambda: registration.match_features(_dev(a), _dev(b), _dev(av), _dev(bv), mutual=False))
    assert one.shape[0] == int(av.sum()) >= pairs.shape[0]
    strict, _ = under("torch", lambda: registration.match_features(_dev(a), _dev(b), _dev(av), _dev(bv), mutual=False, ratio=0.9))
    idx, x, y = R.match(a, b, av, bv)
    assert strict.shape[0] == int(((idx >= 0) & (x.astype(np.float64) < 0.81 * y.astype(np.float64))).sum())


# ------------------------------------------------------------------------------------------------------------ hypotheses
def ransac_case(c, kind="mixed", seed=0):
    rng = np.random.RandomState(seed + c)
    P = rng.rand(c, 3).astype(np.float32)
    T = R.motion("skew175")
    Q = P.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    if kind == "mixed":                                  # a third of the rows are wrong partners: edges that do not agree, rows that are no inliers
        bad = (rng.rand(c) < 0.34) & (c > 4)             # three or four rows: all true, so that some hypothesis is scored
        Q[bad] = rng.rand(int(bad.sum()), 3) + T[:3, 3]
        Q += rng.normal(size=Q.shape) * 1e-3
    elif kind == "line":                                 # every triple is collinear: no frame
        P[:, 1:] = 0.0
        Q = P.astype(np.float64)
    elif kind == "twins":                                # rows in identical pairs: edges of length zero on both sides pass the edge test
        P[1::2] = P[0:-1:2][:P[1::2].shape[0]]
        Q = P.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    return P, Q.astype(np.float32)


def run_ransac(P, Q, H, seed, dist_max, edge_ratio):
    return tuple(ransac_pairs(P, Q, H, seed, dist_max, edge_ratio))


def check_ransac(first, want, H, label):
    count, status, ssq, T, best = [_cpu(x) for x in first]
    assert count.dtype == np.int32 and status.dtype == np.uint8 and ssq.dtype == np.float64 and T.shape == (H, 12)
    assert (status == want["status"]).all(), np.argwhere(status != want["status"])[:5]
    assert (count == want["count"]).all(), np.argwhere(count != want["count"])[:5]
    key = int(best[0])
    h = 0xffffffff - (key & 0xffffffff) if key else -1
    assert h == want["hypothesis"] and (key >> 32) == want["best_count"], (label, h, want["hypothesis"])
    if h >= 0:
        assert T[h].tobytes() == want["T"][h].tobytes(), (label, T[h], want["T"][h])
    assert (T[status != 0] == 0).all() and (count[status != 0] == 0).all() and (ssq[status != 0] == 0).all()
    gap = np.abs(ssq - want["ssq"])
    assert (gap <= want["ssq_bound"]).all(), (label, gap.max())
    return dict(tallies=np.bincount(status, minlength=4).tolist(), winner=h, count=key >> 32, ssq_gap=float(gap.max()),
                ssq_bound=float(want["ssq_bound"].max()), T_equal=bool((T == want["T"]).all()))


@pytest.mark.parametrize("c", [3, 4, 64, 65, 1000])
@pytest.mark.parametrize("H", [1, 64, 65, 4097])
def test_ransac_route(c, H):
    P, Q = ransac_case(c)
    seed, dist_max, edge_ratio = 5 + H, 0.01, 0.9
    want = R.ransac(P, Q, H, seed, dist_max, edge_ratio)
    args = (_dev(P), _dev(Q), H, seed, dist_max, edge_ratio)
    first = profiled({RANSAC}, lambda: run_ransac(*args))
    for binding in ("torch", "ctypes"):
        for again in range(2):
            assert same(first, profiled({RANSAC}, lambda: run_ransac(*args), binding)), "the bits differ under %s, call %d" % (binding, again)
    fig = check_ransac(first, want, H, "c=%d H=%d" % (c, H))
    if H >= 4097:
        assert fig["tallies"][0] > 0 and fig["tallies"][1] > 0 and (c <= 4 or fig["tallies"][2] > 0)
    print("GLOBAL-REG-ROUTE ransac c=%d H=%d: %s" % (c, H, fig))


@pytest.mark.parametrize("kind,status", [("line", 3), ("twins", 3), ("mixed", 2)])
def test_every_status_on_purpose(kind, status):
    P, Q = ransac_case(64, kind)
    want = R.ransac(P, Q, 512, 9, 0.01, 0.9)
    first = profiled({RANSAC}, lambda: run_ransac(_dev(P), _dev(Q), 512, 9, 0.01, 0.9))
    fig = check_ransac(first, want, 512, kind)
    assert fig["tallies"][status] > 0 and fig["tallies"][1] > 0, fig
    if kind == "line":
        assert fig["tallies"][0] == 0 and fig["winner"] == -1
    print("GLOBAL-REG-ROUTE ransac %s: %s" % (kind, fig))


def test_a_seed_above_2_63_and_the_python_front_end():
    from estdepth_amd import registration
    P, Q = ransac_case(65)
    seed = 2 ** 64 - 3
    want = R.ransac(P, Q, 257, seed, 0.01, 0.9)
    for binding in ("torch", "ctypes"):
        check_ransac(profiled({RANSAC}, lambda: run_ransac(_dev(P), _dev(Q), 257, seed, 0.01, 0.9), binding), want, 257, binding)
    pairs = torch.stack([torch.arange(65, device=DEV), torch.arange(65, device=DEV)], 1)
    out = under("torch", lambda: registration.ransac_pairs(_dev(P), _dev(Q), pairs, 0.01, hypotheses=257, seed=seed))
    assert out["hypothesis"] == want["hypothesis"] and out["count"] == want["best_count"] and out["fitness"] == want["best_count"] / 65
    assert out["T"][:3].tobytes() == want["T"][want["hypothesis"]].tobytes() and (out["T"][3] == (0, 0, 0, 1)).all()
    assert list(out["status"].values()) == np.bincount(want["status"], minlength=4).tolist()


def test_nothing_runs_for_empty_inputs():
    none3, nonei = torch.empty((0, 3), device=DEV), torch.empty((0, 8), device=DEV, dtype=torch.int32)
    cnt = torch.empty(0, device=DEV, dtype=torch.int32)
    for binding in ("torch", "ctypes"):
        out = profiled(set(), lambda: run_descriptors(none3, none3, nonei, cnt, True), binding)
        assert out[0].shape == (0, 33) and out[2].shape == (0, 33) and int(out[4].item()) == 0
        out = profiled(set(), lambda: run_ransac(none3, none3, 0, 0, 0.1, 0.9), binding)
        assert out[0].shape == (0,) and out[3].shape == (0, 12) and int(out[4].item()) == 0
        out = profiled({RANSAC}, lambda: run_ransac(none3, none3, 65, 0, 0.1, 0.9), binding)          # no correspondences: every draw is a repeat
        assert bool((out[1] == 1).all()) and int(out[4].item()) == 0


def _bad_calls():
    p, nrm, index, count = (_dev(x) for x in descriptor_case(65, 8))
    hist, pairs = under("torch", lambda: cloud_spfh(p, nrm, index, count, True))
    s = dict(points=p, normal=nrm, index=index, count=count)
    bad_s = [dict(points=p.double()), dict(points=p.cpu()), dict(normal=nrm[:-1].contiguous()), dict(normal=nrm.double()), dict(index=index.long()),
             dict(index=index[:-1].contiguous()), dict(index=torch.zeros((65, 33), dtype=torch.int32, device=DEV)), dict(count=count.long()),
             dict(count=count[:-1].contiguous())]
    f = dict(s, hist=hist, pairs=pairs)
    bad_f = bad_s + [dict(hist=hist[:, :32].contiguous()), dict(hist=hist.long()), dict(pairs=pairs[:-1].contiguous()), dict(pairs=pairs.float())]
    a, b, av, bv = (_dev(x) for x in match_case(65, 64))
    m = dict(a=a, b=b, a_valid=av, b_valid=bv)
    bad_m = [dict(a=a[:, :32].contiguous()), dict(a=a.cpu()), dict(b=b.double()), dict(b=b.t().contiguous().t()), dict(a_valid=av[:-1].contiguous()),
             dict(a_valid=av.bool()), dict(b_valid=bv.int())]
    P, Q = (_dev(x) for x in ransac_case(65))
    r = dict(P=P, Q=Q, hypotheses=64, seed=0, dist_max=0.1, edge_ratio=0.9)
    bad_r = [dict(P=P.double()), dict(Q=Q[:-1].contiguous()), dict(hypotheses=-1), dict(hypotheses=2 ** 31), dict(hypotheses=4.7), dict(hypotheses=True), dict(seed=0.5), dict(dist_max=-1.0), dict(dist_max=float("nan")),
             dict(dist_max=float("inf")), dict(edge_ratio=1.5), dict(edge_ratio=-0.1), dict(edge_ratio=float("nan"))]
    return (cloud_spfh, s, bad_s), (cloud_fpfh, f, bad_f), (feature_match, m, bad_m), (ransac_pairs, r, bad_r)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_a_refused_call_launches_nothing(binding):
    for op, base, bads in _bad_calls():
        for bad in bads:
            with pytest.raises(RuntimeError):
                profiled(set(), lambda: op(**dict(base, **bad)), binding)


def test_the_messages_are_the_same_under_both_bindings():
    calls = {op.__name__: (op, base) for op, base, _ in _bad_calls()}
    short = lambda t: t[:-1].contiguous()                                                     # noqa: E731 -- a row too few
    for name, kw, wrong in (("cloud_spfh", "normal", short), ("cloud_spfh", "index", short), ("cloud_fpfh", "hist", short), ("cloud_fpfh", "pairs", short),
                            ("feature_match", "b", lambda t: t[:, :32].contiguous()), ("feature_match", "a_valid", short), ("ransac_pairs", "Q", short),
                            ("ransac_pairs", "hypotheses", lambda v: -1), ("ransac_pairs", "hypotheses", lambda v: 4.7), ("ransac_pairs", "seed", lambda v: True),
                            ("ransac_pairs", "dist_max", lambda v: float("nan")), ("ransac_pairs", "edge_ratio", lambda v: 1.5)):
        op, base = calls[name]
        wrong = wrong(base[kw])
        texts = []
        for binding in ("torch", "ctypes"):
            with pytest.raises(RuntimeError) as e:
                under(binding, lambda: op(**dict(base, **{kw: wrong})))
            texts.append(str(e.value).split("\n")[0])
        assert texts[0] == texts[1] and texts[0].startswith(name + ": "), texts


def test_every_claimed_instance_ran():
    """the kernels the profiler saw under this suite's cases (one more call each here, should this test run alone) are exactly the claimed ones"""
    args = tuple(_dev(x) for x in descriptor_case(2, 3))
    for oriented in (True, False):
        profiled({SPFH[oriented], FPFH}, lambda: run_descriptors(*args, oriented))
    a, b, _, _ = match_case(1, 1)
    profiled({MATCH}, lambda: feature_match(_dev(a), _dev(b)))
    P, Q = ransac_case(4)
    profiled({RANSAC}, lambda: run_ransac(_dev(P), _dev(Q), 1, 0, 0.1, 0.9))
    assert _RAN == ALL, (sorted(_RAN), sorted(ALL))
