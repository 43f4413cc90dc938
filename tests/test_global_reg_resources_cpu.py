"""The ledger of csrc/register/global_register.hip (CPU; needs hipcc), as tests/test_cloud_knn_resources_cpu.py keeps it for the neighbour
search: the file is cross-compiled with the library's flags (tools/kernel_resources.py), the set of ``*_kernel`` functions it emits must
EQUAL the set claimed by the INSTANCES table of tests/test_gpu_global_reg_routes.py, and every instance must show no scratch and no
spilled vector or scalar register -- the SPFH counters are bytes of six 64-bit registers and the FPFH accumulators 33 named doubles
precisely so that no per-lane array becomes scratch; only the matcher uses LDS, one tile of 128 rows (DESIGN 3.19 records the figures
this test pins)."""
import os
import re

import pytest

import test_gpu_global_reg_routes as GR
from test_tsdf_mesh_resources_cpu import _tool

SOURCE = os.path.join("register", "global_register.hip")
VGPRS = {"greg_spfh_kernel<true>": 68, "greg_spfh_kernel<false>": 64, "greg_fpfh_kernel": 122, "greg_match_kernel": 72, "greg_ransac_kernel": 95}
# the matcher: a tile of 128 rows of 36 floats, its 128 flags, and the four waves' partial (best, second, index) of 64 queries
LDS = {"greg_spfh_kernel<true>": 0, "greg_spfh_kernel<false>": 0, "greg_fpfh_kernel": 0, "greg_match_kernel": 128 * 36 * 4 + 128 * 4 + 3 * 4 * 64 * 4,
       "greg_ransac_kernel": 0}
OCCUPANCY = {"greg_spfh_kernel<true>": 7, "greg_spfh_kernel<false>": 8, "greg_fpfh_kernel": 4, "greg_match_kernel": 7, "greg_ransac_kernel": 5}


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
    others = (C2, G2, GC, GD, GK, GS, GX, GP, R3, RA, SF, GT, GM)
    for k in (k for ks in GR.INSTANCES.values() for k in ks):
        assert k.startswith("greg_") and not any(m.KERNEL_RE.search(k) for m in others), k
    for m in others:
        for k in (k for ks in getattr(m, "INSTANCES", {}).values() for k in ks):
            assert not GR.KERNEL_RE.search(k), k


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in sorted(emitted.items()):
        print("GLOBAL-REG-RESOURCES %s: %s" % (inst, d))
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
        assert d["AGPRs"] == 0, (inst, d)
        assert d["LDS Size [bytes/block]"] == LDS[inst], (inst, d)
        assert d["VGPRs"] == VGPRS[inst] and d["Occupancy [waves/SIMD]"] == OCCUPANCY[inst], (inst, d)


def test_the_mixer_is_shared_not_copied():
    """estd_ransac_pairs draws with estd_mesh_sample's mixer: one definition, in csrc/estd_device.h"""
    from estdepth_amd import build
    read = lambda *p: open(os.path.join(build.CSRC, *p), encoding="utf-8").read()              # noqa: E731
    assert len(re.findall(r"unsigned long long h64\(", read("estd_device.h"))) == 1
    for src in (("mesh", "mesh_sample.hip"), ("register", "global_register.hip")):
        text = read(*src)
        assert "h64(" in text and "0x9e3779b97f4a7c15" not in text and '#include "../estd_device.h"' in text, src
