"""CPU-only checks of the colour path of the TSDF volume: the float64 reference of tests/tsdf_color_ref.py against tests/tsdf_ref.py (the
restated decisions cannot drift), its bound against a numpy-fp32 evaluation of the contract, the semantic bar and its teeth, the edge and
render colour references, and the host side (check_frames with images, the PLY writer, the descriptors' layout, null descriptors).

Measured here (numpy fp32 stand-in): largest |C - C_ref| / (2^-24 A_c) 0.25 (unweighted cases) to 0.54 ("weighted"), bound C_COLOR = 2;
ambiguous share 0.0026; median colour error of the float64 reference at its own points 0.43 ("t3") of 255, 4.3 with the images shifted
by one pixel along u, 61 with two channels swapped."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_color_ref as CR
import tsdf_raycast_ref as RR
import tsdf_ref as R
from helpers import check_desc_layout


def _stand_in(fx, D0, W0, C0, images=None):
    case = fx["case"]
    return CR.integrate(D0, W0, C0, fx["mats"], case["depths"], fx["images"] if images is None else images, case["confs"], dtype=np.float32,
                        **case["params"])


@pytest.mark.parametrize("name", CR.CASES)
def test_reference_restates_tsdf_ref_and_bounds_fp32(name):
    """D, Wt, updated and amb equal tsdf_ref.integrate's exactly; the fp32 evaluation of step 7 meets the colour bound; untouched voxels
    keep their bits; the ambiguous share stays under the cap"""
    fx = CR.fixture(name)
    case = fx["case"]
    D0, W0, C0, ref = fx["D0"], fx["W0"], fx["C0"], fx["ref"]
    for call in range(case["calls"]):
        if call:
            ref = CR.integrate(D0, W0, C0, fx["mats"], case["depths"], fx["images"], case["confs"], **case["params"])
        base = R.integrate(D0, W0, fx["mats"], case["depths"], case["confs"], **case["params"])
        for k in ("D", "Wt", "updated", "amb"):
            assert np.array_equal(ref[k], base[k]), k
        got = _stand_in(fx, D0, W0, C0)
        R.compare(got["D"], got["Wt"], base, weighted=case["params"]["weighted"], D_before=D0, W_before=W0)
        fig = CR.compare(got["C"], ref, C_before=C0)
        assert fig["updated"] > 1000 and fig["amb_share"] <= R.AMB_CAP
        D0, W0, C0 = got["D"], got["Wt"], got["C"]


@pytest.mark.parametrize("mistake", CR.MISTAKES)
def test_compare_rejects_each_colour_mistake(mistake):
    """the colour blended with the weight the D update leaves behind, evaluated in fp32 as the kernel would: rejected (eight frames, so
    every voxel but the first update sees the difference)"""
    c = R.build_case("r8x16x64-t8-120x160")
    from estdepth_amd import camera
    mats = camera.tsdf_matrices(torch.from_numpy(c["poses"]), torch.from_numpy(c["K"]), c["origin"], c["voxel"]).numpy().reshape(-1, 3, 4)
    images = CR.case_images(c)
    Z0, C0 = np.zeros(c["dims"], np.float32), np.zeros((3,) + tuple(c["dims"]), np.float32)
    ref = CR.integrate(Z0, Z0, C0, mats, c["depths"], images, None, **c["params"])
    good = CR.integrate(Z0, Z0, C0, mats, c["depths"], images, None, dtype=np.float32, **c["params"])
    assert CR.compare(good["C"], ref, C_before=C0)["updated"] > 1000
    bad = CR.integrate(Z0, Z0, C0, mats, c["depths"], images, None, dtype=np.float32, mistake=mistake, **c["params"])
    assert np.array_equal(bad["D"], good["D"]) and np.array_equal(bad["Wt"], good["Wt"])       # D and the weight are not affected
    with pytest.raises(AssertionError):
        CR.compare(bad["C"], ref, C_before=C0)


@pytest.mark.parametrize("name", CR.NORMALISED)
def test_normalised_images_with_negative_values(name):
    fx = CR.fixture(name, True)
    assert fx["images"].min() < -0.5
    got = _stand_in(fx, fx["D0"], fx["W0"], fx["C0"])
    CR.compare(got["C"], fx["ref"], C_before=fx["C0"])


def test_semantic_bar_and_its_teeth():
    """the float64 reference's own median colour error against the analytic texture is small, and the bar of 1.25 x that median fails a
    reference fed images shifted by one pixel along u and one fed images with two channels swapped"""
    fx = CR.fixture("t3")
    case = fx["case"]
    med, p95 = CR.reference_median(fx["ref"], case)
    print("reference median %.3f, 95th percentile %.2f of 255" % (med, p95))
    assert 0 < med < 1.0
    bar = CR.MEDIAN_FACTOR * med
    for label, images in (("shifted", np.roll(fx["images"], 1, axis=3)), ("swapped", np.ascontiguousarray(fx["images"][:, [1, 0, 2]]))):
        bad = CR.integrate(fx["D0"], fx["W0"], fx["C0"], fx["mats"], case["depths"], images, case["confs"], **case["params"])
        m, _ = CR.reference_median(bad, case)
        print("%s images: median %.3f (bar %.3f)" % (label, m, bar))
        assert m > bar, label


def test_edge_and_render_colour_references():
    """edge colours: the end points at s = 0 / 1, zeros for ids outside the volume; render colours on the reference volume: close to the
    analytic texture at the rendered depth, ambiguous pixels under the cap, the fp32 volume's own render within the bound of itself"""
    fx = CR.fixture("t3")
    case, ref = fx["case"], fx["ref"]
    D32, W32, C32 = ref["D"].astype(np.float32), ref["Wt"].astype(np.float32), ref["C"].astype(np.float32)
    Z, Y, X = D32.shape
    n = Z * Y * X
    col, tol = CR.edge_colors(D32, C32, np.array([-1, 3 * n, 3 * n + 5, 3 * (X - 1), 3 * (n - 1) + 2, 3 * (n - 1) + 1], np.int64))
    assert (col == 0).all() and (tol == 0).all()
    pts = R.extract(D32, W32, 1.0, case["voxel"], case["origin"])
    col, tol = CR.edge_colors(D32, C32, pts["edge"])
    idx, k = pts["edge"] // 3, pts["edge"] % 3
    far = idx + np.array([1, X, X * Y])[k]
    lo = np.minimum(C32.reshape(3, -1)[:, idx], C32.reshape(3, -1)[:, far]).T
    hi = np.maximum(C32.reshape(3, -1)[:, idx], C32.reshape(3, -1)[:, far]).T
    assert (col >= lo - tol).all() and (col <= hi + tol).all()
    CR.compare_edge_colors(col.astype(np.float32), pts["edge"], D32, C32)
    view = RR.view(case)
    rc = CR.render_colors(D32, W32, C32, view, 1.0)
    hit = rc["ray"]["hit"] & ~rc["amb"]
    assert hit.sum() > 5000 and rc["amb"].sum() <= RR.AMB_CAP * rc["ray"]["hit"].sum()
    world = RR.backproject(rc["ray"]["depth"], view["pose"], case["K"])
    e = np.abs(rc["color"] - CR.texture(world)).max(-1)[hit]
    print("render colour vs texture: median %.3f, 95th percentile %.2f of 255" % (np.median(e), np.percentile(e, 95)))
    assert np.median(e) < 2.0
    CR.compare_render(rc["color"].astype(np.float32), rc, "t3 reference")


# ------------------------------------------------------------------------------------------------------------ host side
def test_check_frames_with_images():
    from estdepth_amd.fusion3d import TSDFVolume
    d = torch.ones(2, 6, 8)
    poses, K = torch.eye(4).expand(2, 4, 4), torch.eye(3)
    out = TSDFVolume.check_frames(d, poses, K, images=torch.zeros(2, 3, 6, 8))
    assert len(out) == 5 and len(out[4]) == 2 and tuple(out[4][0].shape) == (3, 6, 8)
    assert len(TSDFVolume.check_frames(d, poses, K, images=[torch.zeros(3, 6, 8), torch.zeros(1, 3, 6, 8)])[4]) == 2
    assert len(TSDFVolume.check_frames(d, poses, K)) == 4
    for bad in (torch.zeros(3, 3, 6, 8), torch.zeros(2, 3, 6, 9), torch.zeros(2, 1, 6, 8), torch.zeros(2, 3, 12, 16), [torch.zeros(3, 6, 8)],
                torch.zeros(2, 3, 6, 8, device="meta"), torch.zeros(2, 3, 6, 8, dtype=torch.float64), [torch.zeros(3, 6, 8), None]):
        with pytest.raises(RuntimeError):
            TSDFVolume.check_frames(d, poses, K, images=bad)


def test_write_ply_with_and_without_rgb(tmp_path):
    from estdepth_amd.fusion3d import write_ply
    rec = np.arange(18, dtype=np.float32).reshape(3, 6) * 0.5
    plain, colour = tmp_path / "a.ply", tmp_path / "b.ply"
    write_ply(str(plain), rec)
    today = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
             "property float nx\nproperty float ny\nproperty float nz\nend_header\n").encode("ascii") + rec.astype("<f4").tobytes()
    assert plain.read_bytes() == today
    rgb = np.array([[1, 2, 3], [0, 128, 255], [9, 8, 7]], np.uint8)
    write_ply(str(colour), rec, rgb)
    head, body = colour.read_bytes().split(b"end_header\n", 1)
    assert head.decode("ascii").splitlines()[-3:] == ["property uchar red", "property uchar green", "property uchar blue"]
    assert head.startswith(today.split(b"end_header\n")[0]) and len(body) == 27 * 3
    for i in range(3):
        assert body[27 * i:27 * i + 24] == rec[i].astype("<f4").tobytes() and body[27 * i + 24:27 * i + 27] == rgb[i].tobytes()
    with pytest.raises(RuntimeError):
        write_ply(str(colour), rec, rgb[:2])
    with pytest.raises(RuntimeError):
        write_ply(str(colour), rec, rgb.astype(np.float32))


@pytest.fixture(scope="module")
def libpath():
    from estdepth_amd import build
    return build.build()


@pytest.mark.parametrize("mirror,struct", [("TsdfIntegrateColorDesc", "estd_tsdf_integrate_color_desc"), ("TsdfRaycastColorDesc", "estd_tsdf_raycast_color_desc")])
def test_colour_desc_struct_layout(libpath, tmp_path, mirror, struct):
    """sizeof / offsetof of the two new descriptors as the C compiler sees them == the ctypes mirrors; a descriptor without colour is a
    prefix of the one with; NULL and empty descriptors are argument errors (no GPU needed)"""
    from estdepth_amd import _native
    cls = getattr(_native, mirror)
    check_desc_layout(tmp_path, struct, cls)
    plain = _native.TsdfIntegrateDesc if "Integrate" in mirror else _native.TsdfRaycastDesc
    for f in plain._fields_:
        assert getattr(plain, f[0]).offset == getattr(cls, f[0]).offset, f[0]
    fn = getattr(_native.lib(), struct[:-len("_desc")])
    assert fn(None, None) == -1
    assert fn(ctypes.byref(cls()), None) == -1


def test_null_arguments_without_gpu(libpath):
    from estdepth_amd import _native
    lib = _native.lib()
    assert lib.estd_tsdf_edge_colors(None, None, 8, 8, 8, None, 0, None, None) == -1
    d = _native.TsdfIntegrateColorDesc()
    d.Z = d.Y = d.X = 8
    d.H, d.W, d.T = 6, 8, 1
    d.trunc, d.w_max = 0.1, 64.0
    d.tsdf = d.weight = d.color = 64                       # never dereferenced: the call fails on the null depth / image pointers
    assert lib.estd_tsdf_integrate_color(ctypes.byref(d), None) == -1
    d.depth[0] = 64
    assert lib.estd_tsdf_integrate_color(ctypes.byref(d), None) == -1     # image[0] is null
    d.image[0] = 64
    d.color = None
    assert lib.estd_tsdf_integrate_color(ctypes.byref(d), None) == -1
    d.color = 64
    d.T = 9
    assert lib.estd_tsdf_integrate_color(ctypes.byref(d), None) == -1
