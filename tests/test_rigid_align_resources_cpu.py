"""The ledger of csrc/track/rigid_align.hip (CPU; needs hipcc), as tests/test_mesh_distance_resources_cpu.py keeps it for the distance
source: the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it emits must
EQUAL the set claimed by the INSTANCES table of tests/test_gpu_rigid_align_routes.py, and every instance must show no scratch and no
spilled vector or scalar register; LDS is the four-wave join of the system kernel alone (DESIGN 3.16 records the register counts this
test prints).  The entry points' argument rules that need no device (a refusal comes before any launch) are checked here too, and the
descriptor's layout."""
import ctypes
import os
import re

import pytest

import test_gpu_rigid_align_routes as GR
from helpers import check_desc_layout
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("track", "rigid_align.hip")


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
    assert len(named) == len(set(named)) == 3, sorted(named)
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
    import test_gpu_sweep_fusion_routes as SF
    import test_gpu_track_routes as GT
    import test_gpu_tsdf_mesh_routes as GM
    others = (C2, G2, GC, GD, GS, GX, R3, SF, GT, GM)
    for k in (k for ks in GR.INSTANCES.values() for k in ks):
        assert k.startswith("rigid_") and not any(m.KERNEL_RE.search(k) for m in others), k
    for m in others:
        for k in (k for ks in getattr(m, "INSTANCES", {}).values() for k in ks):
            assert not GR.KERNEL_RE.search(k), k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("RIGID-ALIGN-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0 and d["AGPRs"] == 0, (inst, d)
        # LDS: the four-wave join only -- 4 waves x 29 terms x 8 bytes in the system kernel, none elsewhere
        assert d["LDS Size [bytes/block]"] == (4 * 29 * 8 if inst == "rigid_system_kernel" else 0), (inst, d)


def test_the_descriptor_layout(tmp_path):
    from estdepth_amd import _native, build, ops
    build.build()
    assert check_desc_layout(tmp_path, "estd_rigid_system_desc", _native.RigidSystemDesc,
                             macros=["ESTD_RIGID_SYSTEM_SUMS", "ESTD_RIGID_PLANE", "ESTD_RIGID_POINT"]) == \
        [ops.RIGID_SYSTEM_SUMS, ops.RIGID_METRICS["plane"], ops.RIGID_METRICS["point"]]


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: nulls, negative sizes, a dist_max whose square is
    not a positive finite fp32, a NaN cos_min together with normals, a matrix element that is not finite, an unknown metric ->
    ESTD_ERR_ARG (-1); N, Nt or Nn >= 2^31 -> ESTD_ERR_UNSUPPORTED (-3), after the argument errors; nothing is written"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")
    eye = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]

    def apply(src=p, normal=None, n=4, T=eye, moved=p, moved_normal=None):
        return lib.estd_rigid_apply(src, normal, n, (ctypes.c_float * 12)(*T) if T is not None else None, moved, moved_normal, None)

    for kw in (dict(n=-1), dict(T=None), dict(T=eye[:5] + [nan] + eye[6:]), dict(T=eye[:11] + [inf]), dict(src=None), dict(moved=None),
               dict(normal=p), dict(moved_normal=p), dict(n=2 ** 31, T=None)):
        assert apply(**kw) == -1, kw
    assert apply(n=2 ** 31) == -3 and apply(n=2 ** 31 - 1, src=None) == -1
    assert apply(n=0, src=None, moved=None) == 0

    def system(**kw):
        d = _native.RigidSystemDesc()
        d.N, d.Nt, d.Nn = kw.get("N", 4), kw.get("Nt", 4), kw.get("Nn", 4)
        d.metric, d.by_index, d.two_sided = kw.get("metric", 0), kw.get("by_index", 1), kw.get("two_sided", 0)
        d.dist_max, d.cos_min = kw.get("dist_max", 0.1), kw.get("cos_min", -inf)
        for k in ("moved", "index", "target", "normal", "residual", "match", "sums", "partials"):
            setattr(d, k, kw.get(k, p.value))
        d.moved_normal = kw.get("moved_normal", None)
        return lib.estd_rigid_system(ctypes.byref(d), None)

    assert lib.estd_rigid_system(None, None) == -1
    for kw in (dict(N=-1), dict(Nt=-1), dict(Nn=-1), dict(metric=2), dict(metric=-1), dict(dist_max=0.0), dict(dist_max=-1.0), dict(dist_max=nan),
               dict(dist_max=inf), dict(dist_max=1e30), dict(dist_max=1e-30), dict(moved_normal=p.value, cos_min=nan), dict(moved=None),
               dict(index=None), dict(target=None), dict(normal=None), dict(normal=None, metric=1, moved_normal=p.value, cos_min=0.5),
               dict(residual=None), dict(match=None), dict(sums=None), dict(partials=None), dict(by_index=0, Nt=3),
               dict(N=2 ** 31, dist_max=0.0), dict(N=0, sums=None)):
        assert system(**kw) == -1, kw
    for kw in (dict(N=2 ** 31, Nt=2 ** 31), dict(Nt=2 ** 31), dict(Nn=2 ** 31)):
        assert system(**kw) == -3, kw
    assert not any(buf)                              # nothing was written
    assert lib.estd_rigid_system_partials(1) == 29 * 8 == lib.estd_rigid_system_partials(256)
    assert lib.estd_rigid_system_partials(257) == 2 * 29 * 8 and lib.estd_rigid_system_partials(16641) == 66 * 29 * 8
    assert lib.estd_rigid_system_partials(0) == 0 == lib.estd_rigid_system_partials(-5) and lib.estd_rigid_system_partials(2 ** 31) == 0
    for name in ("estd_rigid_apply", "estd_rigid_system", "estd_rigid_system_partials"):
        assert name in _native.EXPORTED_SYMBOLS
