"""The ledger of csrc/mesh/mesh_sample.hip (CPU; needs hipcc), as tests/test_mesh_components_resources_cpu.py keeps it for the
components' source: the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it
emits must EQUAL the set claimed by the INSTANCES table of tests/test_gpu_mesh_sample_routes.py, and every instance must show no scratch,
no spilled vector or scalar register and full occupancy (DESIGN 3.13 records the register counts this test prints).  The entry points'
argument rules that need no device (a refusal comes before any launch) are checked here too."""
import ctypes
import os
import re

import pytest

import test_gpu_mesh_sample_routes as GS
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("mesh", "mesh_sample.hip")
VGPRS = {"mesh_face_area_kernel": 28, "mesh_sample_kernel": 24}          # as DESIGN 3.13 states them


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
    named = [k for ks in GS.INSTANCES.values() for k in ks]
    assert len(named) == len(set(named)), sorted(named)
    assert set(named) == set(emitted), (sorted(set(named) ^ set(emitted)))
    assert not GS.NOT_ROUTES
    assert all(GS.KERNEL_RE.fullmatch(k) for k in named), named


def test_kernel_names_stay_clear_of_the_other_route_suites():
    """no other suite's profiler pattern may pick these kernels up, and this suite's picks up none of theirs"""
    import test_gpu_mesh_components_routes as GC
    import test_gpu_recon3d_routes as R3
    import test_gpu_tsdf_mesh_routes as GM
    for k in (k for ks in GS.INSTANCES.values() for k in ks):
        assert not R3.KERNEL_RE.search(k) and not GM.KERNEL_RE.search(k) and not GC.KERNEL_RE.search(k) and "frame_align" not in k, k
    for k in (k for ks in GC.INSTANCES.values() for k in ks):
        assert not GS.KERNEL_RE.search(k), k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("MESH-SAMPLE-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
        assert d["Occupancy [waves/SIMD]"] == 8 and d["LDS Size [bytes/block]"] == 0, (inst, d)
        assert d["VGPRs"] == VGPRS[inst] and d["AGPRs"] == 0, (inst, d)


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: negative sizes, nulls, a stratum below 1 or too
    wide, C outside 0..6 -> ESTD_ERR_ARG (-1); more than 2^31 - 1 vertices, face indices or samples -> ESTD_ERR_UNSUPPORTED (-3); no
    samples -> 0 with nothing launched"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def area(xyz=p, V=4, faces=p, F=2, out=p, normal=p, invalid=p):
        return lib.estd_mesh_face_area(xyz, V, faces, F, out, normal, invalid, None)

    for kw in (dict(F=-1), dict(V=-1), dict(invalid=None), dict(xyz=None), dict(faces=None), dict(out=None), dict(normal=None),
               dict(F=0, V=0, invalid=None)):
        assert area(**kw) == -1, kw
    for kw in (dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1), dict(V=2 ** 40, F=0), dict(F=2 ** 62)):
        assert area(**kw) == -3, kw

    def sample(xyz=p, V=4, faces=p, F=2, attrs=None, C=0, cum=p, normal=p, n=8, first=0, w=1 << 20, out=(p, p, p, p, None)):
        return lib.estd_mesh_sample(xyz, V, faces, F, attrs, C, cum, normal, n, first, w, 0, *out, None)

    for kw in (dict(F=-1), dict(V=-1), dict(n=-1), dict(first=-1), dict(C=-1), dict(C=7), dict(C=1), dict(C=1, attrs=p), dict(w=0), dict(w=-1),
               dict(w=(1 << 59) + 1), dict(V=0), dict(F=0), dict(xyz=None), dict(faces=None), dict(cum=None), dict(normal=None),
               dict(out=(None, p, p, p, None)), dict(out=(p, None, p, p, None)), dict(out=(p, p, None, p, None)), dict(out=(p, p, p, None, None))):
        assert sample(**kw) == -1, kw
    for kw in (dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1), dict(n=2 ** 31), dict(first=2 ** 31 - 8), dict(n=0, first=2 ** 31)):
        assert sample(**kw) == -3, kw
    assert sample(n=0, xyz=None, faces=None, cum=None, normal=None, out=(None,) * 5) == 0
    assert not any(buf)                              # nothing was written
    assert "estd_mesh_face_area" in _native.EXPORTED_SYMBOLS and "estd_mesh_sample" in _native.EXPORTED_SYMBOLS
