"""The ledger of csrc/mesh/mesh_distance.hip (CPU; needs hipcc), as tests/test_mesh_sample_resources_cpu.py keeps it for the sampling
source: the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it emits must
EQUAL the set claimed by the INSTANCES table of tests/test_gpu_mesh_distance_routes.py, and every instance must show no scratch, no
spilled vector or scalar register and no LDS (DESIGN 3.15 records the register counts this test prints).  The entry points' argument
rules that need no device (a refusal comes before any launch) are checked here too, and the descriptor's layout."""
import ctypes
import os
import re

import pytest

import test_gpu_mesh_distance_routes as GD
from helpers import check_desc_layout
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("mesh", "mesh_distance.hip")


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
    named = [k for ks in GD.INSTANCES.values() for k in ks]
    assert len(named) == len(set(named)), sorted(named)
    assert set(named) == set(emitted), (sorted(set(named) ^ set(emitted)))
    assert not GD.NOT_ROUTES
    assert all(GD.KERNEL_RE.fullmatch(k) for k in named), named


def test_kernel_names_stay_clear_of_the_other_route_suites():
    """no other suite's profiler pattern may pick these kernels up, and this suite's picks up none of theirs"""
    import test_gpu_mesh_components_routes as GC
    import test_gpu_mesh_sample_routes as GS
    import test_gpu_recon3d_routes as R3
    import test_gpu_tsdf_mesh_routes as GM
    for k in (k for ks in GD.INSTANCES.values() for k in ks):
        assert not any(m.KERNEL_RE.search(k) for m in (R3, GM, GC, GS)) and "frame_align" not in k, k
    for m in (GC, GS, GM):
        for k in (k for ks in m.INSTANCES.values() for k in ks):
            assert not GD.KERNEL_RE.search(k), k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("MESH-DISTANCE-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
        assert d["LDS Size [bytes/block]"] == 0 and d["AGPRs"] == 0, (inst, d)


def test_the_descriptor_layout(tmp_path):
    from estdepth_amd import _native, build, ops
    build.build()
    assert check_desc_layout(tmp_path, "estd_mesh_nearest_desc", _native.MeshNearestDesc,
                             macros=["ESTD_MESH_DISTANCE_MAX_PAIRS", "ESTD_MESH_DISTANCE_BIG_CELLS"]) == [ops.MESH_DISTANCE_MAX_PAIRS, ops.MESH_DISTANCE_BIG_CELLS]


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: negative sizes, nulls, a grid cloud_nearest would
    refuse, a misaligned record array, a max_dist without a finite square -> ESTD_ERR_ARG (-1); sizes beyond the limits ->
    ESTD_ERR_UNSUPPORTED (-3); nothing to do -> 0 with nothing launched"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    lo, dims = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4)
    grids = (dict(lo=None), dict(dims=None), dict(cell=0.0), dict(cell=float("inf")), dict(cell=float("nan")), dict(cell=1e-45),
             dict(lo=(ctypes.c_float * 3)(0, float("nan"), 0)), dict(dims=(ctypes.c_int * 3)(0, 1, 1)), dict(dims=(ctypes.c_int * 3)(1025, 1, 1)),
             dict(dims=(ctypes.c_int * 3)(512, 512, 512)))

    def bins(xyz=p, V=4, faces=p, F=2, lo=lo, cell=0.5, dims=dims, big=64, count=p, flag=p, invalid=p):
        return lib.estd_mesh_tri_bins(xyz, V, faces, F, lo, cell, dims, big, count, flag, invalid, None)

    for kw in (dict(F=-1), dict(V=-1), dict(big=-1), dict(invalid=None), dict(xyz=None), dict(faces=None), dict(count=None), dict(flag=None)) + grids:
        assert bins(**kw) == -1, kw
    for kw in (dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1)):
        assert bins(**kw) == -3, kw

    def fill(xyz=p, V=4, faces=p, F=2, lo=lo, cell=0.5, dims=dims, big=64, offset=p, n=8, keys=p, pair_face=p):
        return lib.estd_mesh_tri_fill(xyz, V, faces, F, lo, cell, dims, big, offset, n, keys, pair_face, None)

    for kw in (dict(F=-1), dict(V=-1), dict(big=-1), dict(n=-1), dict(xyz=None), dict(faces=None), dict(offset=None), dict(keys=None),
               dict(pair_face=None)) + grids:
        assert fill(**kw) == -1, kw
    for kw in (dict(V=2 ** 31), dict(F=(2 ** 31 - 1) // 3 + 1), dict(n=(1 << 23) + 1)):
        assert fill(**kw) == -3, kw
    assert fill(n=0, xyz=None, faces=None, offset=None, keys=None, pair_face=None) == 0
    assert fill(F=0, xyz=None, faces=None, offset=None, keys=None, pair_face=None) == 0

    def nearest(**kw):
        d = _native.MeshNearestDesc()
        d.M, d.B, d.P = kw.get("M", 4), kw.get("B", 1), kw.get("P", 1)
        for k in ("query", "order", "big_records", "records", "cell_start", "dist", "face", "bary", "closest"):
            setattr(d, k, kw.get(k, p.value))
        d.cell, d.max_dist = kw.get("cell", 0.5), kw.get("max_dist", 1.0)
        d.lo[:], d.dims[:] = kw.get("lo", (0, 0, 0)), kw.get("dims", (4, 4, 4))
        return lib.estd_mesh_nearest(ctypes.byref(d), None)

    assert lib.estd_mesh_nearest(None, None) == -1
    for kw in (dict(M=-1), dict(B=-1), dict(P=-1), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")),
               dict(max_dist=1e30), dict(big_records=None), dict(big_records=p.value + 4), dict(records=None), dict(records=p.value + 8),
               dict(cell_start=None), dict(cell=0.0), dict(cell=float("nan")), dict(lo=(0, float("inf"), 0)), dict(dims=(0, 1, 1)), dict(dims=(1025, 1, 1)),
               dict(dims=(512, 512, 512)), dict(query=None), dict(dist=None), dict(face=None)):
        assert nearest(**kw) == -1, kw
    for kw in (dict(M=2 ** 31), dict(B=(1 << 23) + 1), dict(P=(1 << 23) + 1)):
        assert nearest(**kw) == -3, kw
    assert nearest(M=0, query=None, dist=None, face=None) == 0
    assert not any(buf)                              # nothing was written
    for name in ("estd_mesh_tri_bins", "estd_mesh_tri_fill", "estd_mesh_nearest"):
        assert name in _native.EXPORTED_SYMBOLS
