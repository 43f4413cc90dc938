"""The ledger of csrc/mesh/mesh_simplify.hip (CPU; needs hipcc), as tests/test_mesh_raster_resources_cpu.py keeps it for the rasteriser:
the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it emits must EQUAL
the set claimed by the INSTANCES table of tests/test_gpu_mesh_simplify_routes.py, and every instance must show no scratch and no spilled
vector or scalar register (DESIGN 3.17 records the register counts this test prints).  The entry points' argument rules that need no
device (a refusal comes before any launch) are checked here too."""
import ctypes
import os
import re

import pytest

import test_gpu_mesh_simplify_routes as GR
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("mesh", "mesh_simplify.hip")
VGPRS = {"mesh_cluster_faces_kernel": 16, "mesh_cluster_quadric_kernel": 66}          # as DESIGN 3.17 states them
OCCUPANCY = {"mesh_cluster_faces_kernel": 8, "mesh_cluster_quadric_kernel": 7}


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
    import test_gpu_recon3d_routes as R3
    import test_gpu_rigid_align_routes as RA
    import test_gpu_sweep_fusion_routes as SF
    import test_gpu_track_routes as GT
    import test_gpu_tsdf_mesh_routes as GM
    others = (C2, G2, GC, GD, GS, GX, R3, RA, SF, GT, GM)
    for k in (k for ks in GR.INSTANCES.values() for k in ks):
        assert k.startswith("mesh_cluster_") and not any(m.KERNEL_RE.search(k) for m in others), k
    for m in others:
        for k in (k for ks in getattr(m, "INSTANCES", {}).values() for k in ks):
            assert not GR.KERNEL_RE.search(k), k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("MESH-SIMPLIFY-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
        assert d["LDS Size [bytes/block]"] == 0 and d["AGPRs"] == 0, (inst, d)
        assert d["VGPRs"] == VGPRS[inst] and d["Occupancy [waves/SIMD]"] == OCCUPANCY[inst], (inst, d)


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: negative sizes, more clusters than vertices,
    nulls with work to do, a grid estd_cloud_cell_keys would refuse, a reg that is negative or not finite -> ESTD_ERR_ARG (-1); more
    than 2^31 - 1 vertices or face indices -> ESTD_ERR_UNSUPPORTED (-3)"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    lo, dims = (ctypes.c_float * 3)(0.0, 0.0, 0.0), (ctypes.c_int * 3)(4, 4, 4)

    def faces(f=p, F=2, V=4, cluster=p, K=3, corner=p, triple=p, counts=p):
        return lib.estd_mesh_cluster_faces(f, F, V, cluster, K, corner, triple, counts, None)

    for kw in (dict(F=-1), dict(V=-1), dict(K=-1), dict(K=5), dict(f=None), dict(corner=None), dict(triple=None), dict(cluster=None), dict(counts=None),
               dict(F=0, f=None, counts=None), dict(V=0, K=1)):
        assert faces(**kw) == -1, kw
    for kw in (dict(V=2 ** 31, K=1), dict(F=(2 ** 31 - 1) // 3 + 1)):
        assert faces(**kw) == -3, kw

    def quadrics(xyz=p, V=4, f=p, F=2, order=p, segments=p, key=p, K=3, mean=p, lo=lo, cell=0.1, dims=dims, reg=2.0 ** -12, out=(p, p, p)):
        return lib.estd_mesh_cluster_quadrics(xyz, V, f, F, order, segments, key, K, mean, lo, cell, dims, reg, *out, None)

    nan_lo, big = (ctypes.c_float * 3)(0.0, float("nan"), 0.0), (ctypes.c_int * 3)(4, (1 << 20) + 1, 4)
    for kw in (dict(F=-1), dict(V=-1), dict(K=-1), dict(K=5), dict(xyz=None), dict(f=None), dict(order=None), dict(segments=None), dict(key=None),
               dict(mean=None), dict(out=(None, p, p)), dict(out=(p, None, p)), dict(out=(p, p, None)), dict(lo=None), dict(lo=nan_lo), dict(dims=None),
               dict(dims=big), dict(dims=(ctypes.c_int * 3)(4, 0, 4)), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")),
               dict(cell=1e-39), dict(reg=-1e-300), dict(reg=float("nan")), dict(reg=float("inf")), dict(reg=float("-inf"))):
        assert quadrics(**kw) == -1, kw
    for kw in (dict(V=2 ** 31, K=1), dict(F=(2 ** 31 - 1) // 3 + 1)):
        assert quadrics(**kw) == -3, kw
    # nothing to do: ESTD_OK without a launch (no device here), whatever the output pointers are
    assert quadrics(F=0, f=None, order=None) == 0 and quadrics(V=0, K=0, xyz=None, segments=None, key=None, mean=None, out=(None, None, None)) == 0
    assert quadrics(reg=0.0, F=0, f=None, order=None) == 0
    assert not any(buf)                              # nothing was written
    assert "estd_mesh_cluster_faces" in _native.EXPORTED_SYMBOLS and "estd_mesh_cluster_quadrics" in _native.EXPORTED_SYMBOLS
    assert _native.lib().estd_mesh_cluster_quadrics.argtypes[12] == ctypes.c_double      # the regularisation goes over as a double
