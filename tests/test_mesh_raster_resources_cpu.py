"""The ledger of csrc/mesh/mesh_raster.hip (CPU; needs hipcc), as tests/test_mesh_sample_resources_cpu.py keeps it for the sampling
source: the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it emits must
EQUAL the set claimed by the INSTANCES table of tests/test_gpu_mesh_raster_routes.py, and every instance must show no scratch, no
spilled vector or scalar register and full occupancy (DESIGN 3.14 records the register counts this test prints).  The entry points'
argument rules that need no device (a refusal comes before any launch) are checked here too."""
import ctypes
import os
import re

import pytest

import test_gpu_mesh_raster_routes as GR
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("mesh", "mesh_raster.hip")
VGPRS = {"mesh_raster_kernel<0>": 58, "mesh_raster_kernel<1>": 58, "mesh_resolve_kernel": 34}          # as DESIGN 3.14 states them


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
    import test_gpu_mesh_components_routes as GC
    import test_gpu_mesh_sample_routes as GS
    import test_gpu_recon3d_routes as R3
    import test_gpu_tsdf_mesh_routes as GM
    for k in (k for ks in GR.INSTANCES.values() for k in ks):
        assert not any(o.KERNEL_RE.search(k) for o in (R3, GM, GC, GS)) and "frame_align" not in k, k
    for other in (GC, GS, GM):
        for k in (k for ks in other.INSTANCES.values() for k in ks):
            assert not GR.KERNEL_RE.search(k), k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("MESH-RASTER-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
        assert d["Occupancy [waves/SIMD]"] == 8 and d["LDS Size [bytes/block]"] == 0, (inst, d)
        assert d["VGPRs"] == VGPRS[inst] and d["AGPRs"] == 0, (inst, d)


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: negative sizes, an empty image, nulls, a matrix
    or z_near that is not finite, an unknown flag, a face range outside [0, F] -> ESTD_ERR_ARG (-1); more than 2^31 - 1 pixels, vertices
    or face indices -> ESTD_ERR_UNSUPPORTED (-3)"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = (ctypes.c_double * 12)(*[1.0] * 12)
    nan = (ctypes.c_double * 12)(*([1.0] * 11 + [float("nan")]))
    inf = (ctypes.c_double * 12)(*([float("-inf")] + [1.0] * 11))

    def raster(xyz=p, V=4, faces=p, F=2, first=0, count=2, mat=good, H=4, W=4, zn=0.1, flags=0, keys=p, invalid=p):
        return lib.estd_mesh_raster(xyz, V, faces, F, first, count, mat, H, W, zn, flags, keys, invalid, None)

    for kw in (dict(F=-1), dict(V=-1), dict(H=0), dict(W=0), dict(H=-1), dict(xyz=None), dict(faces=None), dict(mat=None), dict(mat=nan), dict(mat=inf),
               dict(keys=None), dict(invalid=None), dict(zn=-0.5), dict(zn=float("nan")), dict(zn=float("inf")), dict(flags=4), dict(flags=-1),
               dict(first=-1), dict(count=-1), dict(first=3, count=0), dict(first=1, count=2), dict(count=3), dict(F=0, faces=None, count=1)):
        assert raster(**kw) == -1, kw
    for kw in (dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1), dict(H=65536, W=65536), dict(H=2 ** 31 - 1, W=2)):
        assert raster(**kw) == -3, kw

    def resolve(xyz=p, V=4, faces=p, F=2, mat=good, H=4, W=4, keys=p, out=(p, p, p, p)):
        return lib.estd_mesh_raster_resolve(xyz, V, faces, F, mat, H, W, keys, *out, None)

    for kw in (dict(F=-1), dict(V=-1), dict(H=0), dict(W=-2), dict(xyz=None), dict(faces=None), dict(mat=None), dict(mat=nan), dict(keys=None),
               dict(out=(None, p, p, p)), dict(out=(p, None, p, p)), dict(out=(p, p, None, p)), dict(out=(p, p, p, None))):
        assert resolve(**kw) == -1, kw
    for kw in (dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1), dict(H=65536, W=65536)):
        assert resolve(**kw) == -3, kw
    assert not any(buf)                              # nothing was written
    assert "estd_mesh_raster" in _native.EXPORTED_SYMBOLS and "estd_mesh_raster_resolve" in _native.EXPORTED_SYMBOLS
    assert _native.lib().estd_mesh_raster.argtypes[6] == ctypes.POINTER(ctypes.c_double)       # the matrix goes over as doubles
