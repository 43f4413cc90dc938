"""The ledger of csrc/cloud/cloud_cluster.hip (CPU; needs hipcc), as tests/test_cloud_knn_resources_cpu.py keeps it for the neighbour
search: the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it emits must
EQUAL the set claimed by the INSTANCES table of tests/test_gpu_cloud_cluster_routes.py, and every instance must show no scratch, no LDS
and no spilled vector or scalar register (DESIGN 3.20 records the figures this test pins).  The union-find these kernels share with
csrc/mesh/mesh_components.hip is written once, in csrc/estd_device.h.  The entry points' argument rules that need no device (a refusal
comes before any launch) are checked here too."""
import ctypes
import os
import re

import pytest

import test_gpu_cloud_cluster_routes as GR
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("cloud", "cloud_cluster.hip")
VGPRS = {"dbscan_count_kernel": 47, "dbscan_hook_kernel": 32, "dbscan_flatten_kernel": 6, "dbscan_border_kernel": 37}      # as DESIGN 3.20 states them
OCCUPANCY = {"dbscan_count_kernel": 8, "dbscan_hook_kernel": 8, "dbscan_flatten_kernel": 8, "dbscan_border_kernel": 8}


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
    import test_gpu_cloud_knn_routes as GK
    import test_gpu_conv2d_routes as C2
    import test_gpu_global_reg_routes as GG
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
    others = (GK, C2, GG, G2, GC, GD, GS, GX, GP, R3, RA, SF, GT, GM)
    for k in (k for ks in GR.INSTANCES.values() for k in ks):
        assert k.startswith("dbscan_") and not any(m.KERNEL_RE.search(k) for m in others), k
    for m in others:
        for k in (k for ks in getattr(m, "INSTANCES", {}).values() for k in ks):
            assert not GR.KERNEL_RE.search(k), k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("CLOUD-CLUSTER-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
        assert d["AGPRs"] == 0 and d["LDS Size [bytes/block]"] == 0, (inst, d)
        assert d["VGPRs"] == VGPRS[inst] and d["Occupancy [waves/SIMD]"] == OCCUPANCY[inst], (inst, d)


def test_the_union_find_is_written_once():
    """csrc/estd_device.h holds the four functions in the form tests/test_kernel_helpers_cpu.py parses; neither user defines one again"""
    import test_kernel_helpers_cpu as KH
    functions, _, _ = KH.header_names()
    moved = ("parent_load", "find_root", "find_root_halving", "unite")
    assert set(moved) <= set(functions)
    for rel in (SOURCE, os.path.join("mesh", "mesh_components.hip")):
        code = KH._code(os.path.join(KH.CSRC, rel))
        assert not [n for n in moved if KH._function_def(n).search(code)], rel
        assert re.search(r"\bunite\s*\(", code) and re.search(r"\bfind_root\s*\(", code), rel
    header = open(KH.HEADER, encoding="utf-8").read()
    assert header.count("Visibility.") == 1 and "Termination" in header                     # the argument moved with them


def test_the_descriptors_have_the_c_layout(tmp_path):
    from estdepth_amd import _native
    from helpers import check_desc_layout
    check_desc_layout(tmp_path, "estd_cloud_dbscan_desc", _native.CloudDbscanDesc)
    check_desc_layout(tmp_path, "estd_cloud_count_within_desc", _native.CloudCountWithinDesc)


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: negative sizes, nulls with work to do,
    min_points below 1, a grid estd_cloud_nearest would refuse, records that are not 16-byte aligned -> ESTD_ERR_ARG (-1); more than
    2^31 - 1 rows -> ESTD_ERR_UNSUPPORTED (-3); nothing to do -> ESTD_OK without a launch"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_int * 64)()
    base = ctypes.addressof(buf)
    p = (base + 15) // 16 * 16                             # 16-byte aligned, inside the buffer

    def fill(d, kw):
        d.cell = 0.1
        d.lo[:], d.dims[:] = (0.0, 0.0, 0.0), (4, 4, 4)
        for key, v in kw.items():
            if key in ("lo", "dims"):
                getattr(d, key)[:] = v
            else:
                setattr(d, key, v)
        return d

    def dbscan(**kw):
        d = _native.CloudDbscanDesc()
        d.N, d.min_points, d.eps = 4, 3, 1.0
        d.records = d.cell_start = d.count = d.parent = d.label = d.size = d.noise = p
        return lib.estd_cloud_dbscan(ctypes.byref(fill(d, kw)), None)

    def within(**kw):
        d = _native.CloudCountWithinDesc()
        d.M, d.N, d.radius = 4, 4, 1.0
        d.query = d.order = d.records = d.cell_start = d.count = p
        return lib.estd_cloud_count_within(ctypes.byref(fill(d, kw)), None)

    grid_bad = (dict(records=None), dict(records=p + 4), dict(cell_start=None), dict(cell=0.0), dict(cell=float("nan")), dict(cell=1e-39),
                dict(lo=(0.0, float("inf"), 0.0)), dict(dims=(4, 0, 4)), dict(dims=(4, 1025, 4)), dict(dims=(1024, 1024, 17)))
    assert lib.estd_cloud_dbscan(None, None) == -1 and lib.estd_cloud_count_within(None, None) == -1
    for kw in grid_bad + (dict(N=-1), dict(min_points=0), dict(min_points=-5), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
                          dict(eps=1e20), dict(count=None), dict(parent=None), dict(label=None), dict(size=None), dict(noise=None)):
        assert dbscan(**kw) == -1, kw
    assert dbscan(N=2 ** 31) == -3
    assert dbscan(N=0, records=None, cell_start=None, count=None, parent=None, label=None, size=None, noise=None) == 0
    for kw in grid_bad + (dict(M=-1), dict(N=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
                          dict(radius=1e20), dict(query=None), dict(count=None)):
        assert within(**kw) == -1, kw
    for kw in (dict(M=2 ** 31), dict(N=2 ** 31)):
        assert within(**kw) == -3, kw
    assert within(M=0, query=None, count=None) == 0
    assert not any(buf)                              # nothing was written
    assert "estd_cloud_dbscan" in _native.EXPORTED_SYMBOLS and "estd_cloud_count_within" in _native.EXPORTED_SYMBOLS
