"""The ledger of csrc/mesh/mesh_components.hip (CPU; needs hipcc), as tests/test_tsdf_mesh_resources_cpu.py keeps it for the surface-net
source: the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it emits must
EQUAL the set claimed by the INSTANCES table of tests/test_gpu_mesh_components_routes.py, and every instance must show no scratch, no
spilled vector or scalar register and full occupancy (DESIGN 3.12 records the register counts this test prints).  The entry point's
argument rules that need no device (a refusal comes before any launch) are checked here too."""
import ctypes
import os
import re

import pytest

import test_gpu_mesh_components_routes as GC
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("mesh", "mesh_components.hip")


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
    named = [k for ks in GC.INSTANCES.values() for k in ks]
    assert len(named) == len(set(named)), sorted(named)
    assert set(named) == set(emitted), (sorted(set(named) ^ set(emitted)))
    assert not GC.NOT_ROUTES
    assert all(GC.KERNEL_RE.fullmatch(k) for k in named), named


def test_kernel_names_stay_clear_of_the_other_route_suites():
    """no other suite's profiler pattern may pick these kernels up"""
    import test_gpu_recon3d_routes as R3
    import test_gpu_tsdf_mesh_routes as GM
    for k in (k for ks in GC.INSTANCES.values() for k in ks):
        assert not R3.KERNEL_RE.search(k) and not GM.KERNEL_RE.search(k) and "frame_align" not in k, k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("MESH-CC-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
        assert d["Occupancy [waves/SIMD]"] == 8, (inst, d)


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: negative sizes and nulls -> ESTD_ERR_ARG (-1);
    more than 2^31 - 1 vertices or face indices -> ESTD_ERR_UNSUPPORTED (-3)"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(faces=p, F=2, V=4, label=p, triangles=p, invalid=p):
        return lib.estd_mesh_components(faces, F, V, label, triangles, invalid, None)

    for kw in (dict(F=-1), dict(V=-1), dict(F=-1, V=0), dict(invalid=None), dict(faces=None), dict(label=None), dict(triangles=None),
               dict(faces=None, F=1, V=0), dict(label=None, F=0), dict(F=0, V=0, invalid=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1), dict(V=2 ** 40, F=0), dict(F=2 ** 62)):
        assert call(**kw) == -3, kw
    assert not any(buf)                              # nothing was written
    assert "estd_mesh_components" in _native.EXPORTED_SYMBOLS
