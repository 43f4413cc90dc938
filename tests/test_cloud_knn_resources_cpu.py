"""The ledger of csrc/cloud/cloud_knn.hip (CPU; needs hipcc), as tests/test_mesh_simplify_resources_cpu.py keeps it for the simplifier:
the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it emits must EQUAL
the set claimed by the INSTANCES table of tests/test_gpu_cloud_knn_routes.py, and every instance must show no scratch and no spilled
vector or scalar register -- the neighbour list lives in LDS, 16 KiB per workgroup, precisely so that it does not become scratch
(DESIGN 3.18 records the figures this test pins).  The entry points' argument rules that need no device (a refusal comes before any
launch) are checked here too."""
import ctypes
import os
import re

import pytest

import test_gpu_cloud_knn_routes as GR
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("cloud", "cloud_knn.hip")
VGPRS = {"knn_search_kernel<false>": 44, "knn_search_kernel<true>": 45, "knn_normals_kernel": 56}          # as DESIGN 3.18 states them
LDS = {"knn_search_kernel<false>": 16384, "knn_search_kernel<true>": 16384, "knn_normals_kernel": 0}
OCCUPANCY = {"knn_search_kernel<false>": 3, "knn_search_kernel<true>": 3, "knn_normals_kernel": 8}


@pytest.fixture(scope="module")
def emitted():
    """{kernel name: the compiler's resource record}"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is not installed")
    kr = _tool()
    rec, _ = kr.resource_usage(os.path.join(kr.CSRC, SOURCE), isa=False)
    names = kr.demangle(list(rec))
    out = {}
    for mangled, d in rec.items():
        m = re.search(r"(\w+_kernel)(<[^>()]*>)?\(", names[mangled])
        assert m, names[mangled]
        inst = m.group(1) + (m.group(2) or "")
        assert inst not in out, inst
        out[inst] = d
    return out


def test_the_source_is_built_into_the_library():
    from estdepth_amd import build
    assert SOURCE.replace(os.sep, "/") in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, SOURCE))


def test_claimed_and_emitted_kernels_are_equal(emitted):
    named = [k for ks in GR.INSTANCES.values() for k in ks]
    assert len(named) == len(set(named)), sorted(named)
    assert set(named) == set(emitted), (sorted(set(named) ^ set(emitted)))
    assert not GR.NOT_ROUTES
    assert all(GR.KERNEL_RE.fullmatch(k) for k in named), named


def test_kernel_names_stay_clear_of_the_other_route_suites():
    """no other suite's profiler pattern may pick these kernels up, and this suite's picks up none of theirs"""
    import test_gpu_conv2d_routes as C2
    import test_gpu_glue2d_routes as G2
    import test_gpu_mesh_components_routes as GC
    import test_gpu_mesh_distance_routes as GD
    import test_gpu_mesh_raster_routes as GX
    import test_gpu_mesh_sample_routes as GS
    import test_gpu_mesh_simplify_routes as GP
    import test_gpu_recon3d_routes as R3
    import test_gpu_rigid_align_routes as RA
    import test_gpu_sweep_fusion_routes as SF
    import test_gpu_track_routes as GT
    import test_gpu_tsdf_mesh_routes as GM
    others = (C2, G2, GC, GD, GS, GX, GP, R3, RA, SF, GT, GM)
    for k in (k for ks in GR.INSTANCES.values() for k in ks):
        assert k.startswith("knn_") and not any(m.KERNEL_RE.search(k) for m in others), k
    for m in others:
        for k in (k for ks in getattr(m, "INSTANCES", {}).values() for k in ks):
            assert not GR.KERNEL_RE.search(k), k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("CLOUD-KNN-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
        assert d["AGPRs"] == 0, (inst, d)
        assert d["LDS Size [bytes/block]"] == LDS[inst], (inst, d)
        assert d["VGPRs"] == VGPRS[inst] and d["Occupancy [waves/SIMD]"] == OCCUPANCY[inst], (inst, d)


def test_the_descriptor_has_the_c_layout(tmp_path):
    from estdepth_amd import _native, ops
    from helpers import check_desc_layout
    assert check_desc_layout(tmp_path, "estd_cloud_knn_desc", _native.CloudKnnDesc, macros=["ESTD_CLOUD_KNN_MAX"]) == [ops.CLOUD_KNN_MAX]


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: negative sizes, nulls with work to do, k out of
    range, a grid estd_cloud_nearest would refuse, records that are not 16-byte aligned -> ESTD_ERR_ARG (-1); more than 2^31 - 1 rows ->
    ESTD_ERR_UNSUPPORTED (-3); nothing to do -> ESTD_OK without a launch"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_int * 64)()
    base = ctypes.addressof(buf)
    p = (base + 15) // 16 * 16                             # 16-byte aligned, inside the buffer

    def knn(**kw):
        d = _native.CloudKnnDesc()
        d.M, d.N, d.k = 4, 4, 8
        d.query = d.order = d.records = d.cell_start = d.dist = d.index = d.count = p
        d.cell, d.max_dist = 0.1, 1.0
        d.lo[:], d.dims[:] = (0.0, 0.0, 0.0), (4, 4, 4)
        for key, v in kw.items():
            if key in ("lo", "dims"):
                getattr(d, key)[:] = v
            else:
                setattr(d, key, v)
        return lib.estd_cloud_knn(ctypes.byref(d), None)

    assert lib.estd_cloud_knn(None, None) == -1
    for kw in (dict(M=-1), dict(N=-1), dict(k=0), dict(k=33), dict(k=-1), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")),
               dict(max_dist=float("inf")), dict(max_dist=1e20), dict(records=None), dict(records=p + 4), dict(cell_start=None), dict(query=None),
               dict(dist=None), dict(index=None), dict(count=None), dict(cell=0.0), dict(cell=float("nan")), dict(cell=1e-39), dict(lo=(0.0, float("inf"), 0.0)),
               dict(dims=(4, 0, 4)), dict(dims=(4, 1025, 4)), dict(dims=(1024, 1024, 17))):
        assert knn(**kw) == -1, kw
    for kw in (dict(M=2 ** 31), dict(N=2 ** 31)):
        assert knn(**kw) == -3, kw
    assert knn(M=0, query=None, dist=None, index=None, count=None) == 0

    def normals(points=p, n=4, query=p, m=4, index=p, count=p, k=8, toward=None, per=0, out=(p, p, p, p), cov=None):
        return lib.estd_cloud_normals(points, n, query, m, index, count, k, toward, per, *out, cov, None)

    for kw in (dict(n=-1), dict(m=-1), dict(k=0), dict(k=33), dict(points=None), dict(query=None), dict(index=None), dict(count=None),
               dict(out=(None, p, p, p)), dict(out=(p, None, p, p)), dict(out=(p, p, None, p)), dict(out=(p, p, p, None))):
        assert normals(**kw) == -1, kw
    for kw in (dict(n=2 ** 31), dict(m=2 ** 31)):
        assert normals(**kw) == -3, kw
    assert normals(m=0, query=None, index=None, count=None, out=(None, None, None, None)) == 0
    assert not any(buf)                              # nothing was written
    assert "estd_cloud_knn" in _native.EXPORTED_SYMBOLS and "estd_cloud_normals" in _native.EXPORTED_SYMBOLS
