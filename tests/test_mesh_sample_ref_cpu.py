"""The reference of the mesh sampling (tests/mesh_sample_ref.py) on its own (CPU): what it computes has the properties the contract
promises, its comparison accepts itself and rejects every plausible kernel mistake, and the rules of the host layers that need no device
(the power of two, the stratum, the front end's refusals) hold at their edges."""
import math

import numpy as np
import pytest
import torch

import mesh_sample_ref as S


def _ref(name):
    return S.build_case(name), S.reference(name)


def test_total_area_of_a_unit_square_and_of_an_icosphere():
    xyz = np.asarray([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], np.float32)
    fa = S.face_area(xyz, [(0, 1, 2), (0, 2, 3)])
    assert fa["area"].sum() == 1.0 and np.array_equal(fa["normal"], [(0, 0, 1), (0, 0, 1)])
    # an icosphere inscribed in the unit sphere: its area approaches 4 pi from below, the deficit falling by 4 per level
    deficit = []
    for level in (2, 3, 4):
        x, f = S.icosphere(level)
        assert f.shape[0] == 20 * 4 ** level
        fa = S.face_area(x, f)
        deficit.append(1.0 - fa["area"].sum() / (4 * math.pi))
        assert (np.einsum("ij,ij->i", fa["normal"], x[f[:, 0]]) > 0.9).all()                 # counter-clockwise seen from outside
    assert 0 < deficit[2] < deficit[1] < deficit[0] < 0.02 and 3.5 < deficit[1] / deficit[2] < 4.5


def test_the_mixer_in_numpy_and_in_python_integers_agree():
    i = np.asarray([0, 1, 2, 63, 64, 255, 256, 2 ** 31 - 2], np.uint64)
    for seed in (0, 1, 12345, (1 << 63) + 12345, (1 << 64) - 1):
        for s in (0, 1, 2):
            assert [int(v) for v in S.h64(seed, i, s)] == [S.h64_int(seed, int(k), s) for k in i]
    assert len({S.h64_int(0, k, s) for k in range(100) for s in range(3)}) == 300
    # a seed is taken modulo 2^64
    assert np.array_equal(S.h64(-1, i, 0), S.h64((1 << 64) - 1, i, 0))


@pytest.mark.parametrize("name", [c for c in S.CASES if c not in ("no-faces", "no-samples")])
def test_counts_points_and_order(name):
    (xyz, faces, attrs, n, seed), ref = _ref(name)
    F = faces.shape[0]
    q = S.quantise(ref["area"])[0]
    assert q.sum() == ref["total"] < 1 << 62 and ref["w"] >= S.MIN_STRATUM
    counts = np.bincount(ref["face"], minlength=F)
    assert counts.sum() == n and (np.abs(counts - n * (q / ref["total"])) <= 2).all()
    assert (counts[q == 0] == 0).all()                                       # a zero-area or invalid triangle is never chosen
    assert (np.diff(ref["face"]) >= 0).all()
    u, v = ref["bary"][:, 0].astype(np.float64), ref["bary"][:, 1].astype(np.float64)
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1).all()
    tri = faces[ref["face"]].astype(np.int64)
    a = xyz[tri[:, 0]].astype(np.float64)
    nrm = ref["normal"].astype(np.float64)
    size = np.abs(xyz).max()
    assert (np.abs(np.einsum("ij,ij->i", ref["xyz"] - a, nrm)) <= 1e-6 * size).all()      # on the triangle's plane
    assert not ref["fa"]["left_out"].any()                                   # the reference alone leaves no normal out


def test_the_cases_are_what_their_names_say():
    assert S.build_case("spheres")[1].shape[0] == 5120 + 1280
    area = S.reference("areas-1e6")["area"]
    assert 0.9e6 < area.max() / area.min() < 1.1e6
    z = S.reference("zero-area")
    assert (z["area"] == 0).sum() == 8 and z["area"][0] == 0 and z["area"][1] == 0 and z["area"][-1] == 0 and z["area"][-2] == 0
    o = S.reference("out-of-range")
    assert o["invalid"] == 6 and (o["area"] == 0).sum() == 6
    assert np.abs(S.build_case("far")[0]).min() > 990
    for name, shape in (("no-faces", 0), ("no-samples", 0)):
        assert S.reference(name)["face"].shape[0] == shape
    assert {S.build_case(c)[2].shape[1] for c in ("attrs-1", "attrs-3", "attrs-6")} == {1, 3, 6}
    a, b = S.reference("f65-n1000"), S.reference("f65-n1000-seed")
    assert not np.array_equal(a["bary"], b["bary"]) and not np.array_equal(a["xyz"], b["xyz"])


def test_the_face_order_only_permutes_the_result():
    """per triangle the number of samples changes by the strata's edges only (within the +-2 of the contract on both sides), and the
    areas are the same bits"""
    xyz, faces, _, n, seed = S.build_case("f65-n1000")
    perm = np.random.default_rng(0).permutation(faces.shape[0])
    a, b = S.sample(xyz, faces, None, n, seed), S.sample(xyz, faces[perm], None, n, seed)
    assert np.array_equal(a["area"][perm], b["area"]) and a["total"] == b["total"] and a["w"] == b["w"]
    ca, cb = np.bincount(a["face"], minlength=65), np.bincount(b["face"], minlength=65)
    assert (np.abs(ca[perm] - cb) <= 4).all()


def test_a_sample_does_not_depend_on_how_the_launch_is_split():
    xyz, faces, attrs, n, seed = S.build_case("attrs-3")
    whole = S.sample(xyz, faces, attrs, n, seed)
    for first, count in ((0, 1), (1, 63), (64, 192), (256, n - 256)):
        part = S.sample(xyz, faces, attrs, n, seed, first=first, count=count)
        for k in ("xyz", "face", "bary", "normal", "attrs"):
            assert np.array_equal(part[k], whole[k][first:first + count]), (k, first)


@pytest.mark.parametrize("name", S.CASES)
def test_the_comparison_accepts_the_reference(name):
    xyz, faces, attrs, n, seed = S.build_case(name)
    fig = S.compare(S.as_got(S.reference(name)), xyz, faces, attrs, n, seed, name)
    assert fig["area"] == 0 and fig["left_out"] == 0 and fig["xyz"] <= 1.0 and fig.get("attrs", 0) <= 1.0


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_the_comparison_rejects_a_mistake(mistake):
    """each on a case that exposes it.  A lower bound differs from the upper bound only where a target hits a prefix sum exactly:
    ``tie_case`` has t_0 = 0 = cum[0] with a first triangle of no area.  `unhalved` doubles every area, hence the N of a density too."""
    w = None
    if mistake == "lower_bound":
        xyz, faces, n, seed, w = S.tie_case()
        attrs = None
        good = S.sample(xyz, faces, None, n, seed, w=w)
        assert good["w"] == S.MIN_STRATUM and S.h64_int(seed, 0, 0) % w == 0 and (good["face"] == 1).all()
        S.compare(S.as_got(good), xyz, faces, None, n, seed, w=w)
    else:
        xyz, faces, attrs, n, seed = S.build_case("f65-n64" if mistake == "no_jitter" else "attrs-3")
    bad = S.sample(xyz, faces, attrs, n, seed, mistake=mistake, w=w)
    with pytest.raises(AssertionError):
        S.compare(S.as_got(bad), xyz, faces, attrs, n, seed, mistake, w=w)
    if mistake == "lower_bound":
        assert bad["face"][0] == 0 and (bad["face"][1:] == 1).all()
    if mistake == "unhalved":
        total = S.sample(xyz, faces, attrs, n, seed)["area"].sum()
        assert S.n_for_density(100.0, bad["area"].sum()) in (2 * S.n_for_density(100.0, total), 2 * S.n_for_density(100.0, total) - 1)


def test_the_scale_and_stratum_rules_at_their_edges():
    from estdepth_amd import ops
    for F, amax in ((1, 1.0), (1, 0.999), (2, 1.0), (3, 1e-30), (2 ** 20, 7.5), (2 ** 20 + 1, 7.5), (2 ** 31 // 3, 1e30), (5, 5e-324), (1, 2.0 ** -1000)):
        e = ops.mesh_sample_scale(F, amax)
        assert e == S.scale_exponent(F, amax) <= 1000
        top = math.floor(math.ldexp(amax, e))
        assert F * top < 1 << 62                                             # the sum of F such values fits
        assert e == 1000 or 2 * F * (math.floor(math.ldexp(amax, e + 1)) + 1) > 1 << 61      # and the scale is within 2 bits of the largest
    assert ops.mesh_sample_scale(0, 0.0) == 0 and ops.mesh_sample_scale(10, 0.0) == 0
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(RuntimeError, match="mesh_sample: xyz holds a coordinate that is not finite"):
            ops.mesh_sample_scale(4, bad)
    # one triangle of area 1: 2^61 units
    q, e = S.quantise(np.asarray([1.0]))
    assert e == 61 and int(q[0]) == 1 << 61
    assert ops.mesh_sample_stratum(1 << 61, 2 ** 31 - 1) == (1 << 61) // (2 ** 31 - 1)
    assert ops.mesh_sample_stratum((1 << 20) * 10, 10) == 1 << 20
    with pytest.raises(RuntimeError, match="mesh_sample: n_samples = 10 leaves strata of 1048575 units"):
        ops.mesh_sample_stratum((1 << 20) * 10 - 1, 10)
    with pytest.raises(RuntimeError, match="mesh_sample: the mesh has no area"):
        ops.mesh_sample_stratum(0, 3)
    assert ops.MESH_SAMPLE_MIN_STRATUM == S.MIN_STRATUM


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_the_front_end_refuses_host_tensors_and_bad_shapes_without_a_device(binding):
    from estdepth_amd import ops
    from test_gpu_conv2d_routes import _Switches
    xyz, faces = torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32)
    with _Switches(None, binding):
        for fn in (lambda: ops.mesh_sample(xyz, faces, None, 4, 0), lambda: ops.mesh_face_area(xyz, faces),
                   lambda: ops.mesh_sample(xyz, faces.to(torch.int64), None, 4, 0), lambda: ops.mesh_sample(xyz, faces.reshape(-1), None, 4, 0)):
            with pytest.raises(RuntimeError):
                fn()


def test_the_host_layer_refusals_that_need_no_device():
    from estdepth_amd import cloud_metrics, fusion3d
    mesh = dict(xyz=np.zeros((3, 3), np.float32), faces=np.asarray([(0, 1, 2)], np.int32))
    for kw in (dict(), dict(n=4, density=2.0)):
        with pytest.raises(RuntimeError, match="sample_mesh: exactly one of n and density"):
            fusion3d.sample_mesh(mesh, **kw)
    for kw in (dict(n=-1), dict(n=2.5), dict(density=0.0), dict(density=float("nan")), dict(n=4, normals="smooth")):
        with pytest.raises(RuntimeError, match="sample_mesh: "):
            fusion3d.sample_mesh(mesh, **kw)
    with pytest.raises(RuntimeError, match="sample_mesh: normals='vertex' needs a mesh with vertex normals"):
        fusion3d.sample_mesh(mesh, n=4, normals="vertex")
    with pytest.raises(RuntimeError, match="sample_mesh: the mesh must be a dict with 'xyz' and 'faces'"):
        fusion3d.sample_mesh(dict(xyz=mesh["xyz"]), n=4)
    with pytest.raises(RuntimeError, match="mesh_area: the mesh must be a dict with 'xyz' and 'faces'"):
        fusion3d.mesh_area(None)
    for bad in (0.0, -1.0, float("inf"), None):
        with pytest.raises(RuntimeError, match="compare_meshes: density must be positive and finite"):
            cloud_metrics.compare_meshes(mesh, mesh, bad)
