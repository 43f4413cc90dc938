"""The ledger of csrc/mesh/tsdf_mesh.hip (CPU; needs hipcc).  tests/test_kernel_ledger_cpu.py walks ``csrc/*.hip`` only; this file gives the
same guarantee for the surface-net source: the file is cross-compiled with the library's flags (tools/kernel_resources.py: the demangled
names and the compiler's resource remarks, nothing else), the set of ``*_kernel`` functions it emits must EQUAL the set claimed by the
INSTANCES table of tests/test_gpu_tsdf_mesh_routes.py -- a kernel added to the source cannot ship without a case that names it, and
nothing claimed may be absent -- and every instance must show no scratch, no spilled vector register and no spilled scalar register.
The entry points' argument rules that need no device (a refusal comes before any launch) are checked here too."""
import ctypes
import importlib.util
import os
import re

import pytest

import test_gpu_tsdf_mesh_routes as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join("mesh", "tsdf_mesh.hip")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def emitted():
    """{instance name (template arguments included): the compiler's resource record}"""
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
    named = [k for ks in GM.INSTANCES.values() for k in ks]
    assert len(named) == len(set(named)), sorted(named)
    assert set(named) == set(emitted), (sorted(set(named) ^ set(emitted)))
    assert not GM.NOT_ROUTES


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in emitted.items():
        print(inst, d)
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)


def test_argument_rules_without_a_device():
    """every refusal returns before a launch, so host memory stands in for the pointers: nulls, sizes, scalars -> ESTD_ERR_ARG (-1); more
    than 2^31 - 1 voxels or a dimension past the launch grid -> ESTD_ERR_UNSUPPORTED (-3); a dimension of 1 -> ESTD_OK, nothing launched"""
    from estdepth_amd import _native, build
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    org = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")

    def vertices(tsdf=p, weight=p, color=None, dims=(4, 4, 4), voxel=0.03, origin=org, w_min=1.0, counter=p, cap=2, cell=p, xyz=p, normal=p, vw=p, vc=None):
        return lib.estd_tsdf_mesh_vertices(tsdf, weight, color, dims[0], dims[1], dims[2], voxel, origin, w_min, counter, cap, cell, xyz, normal, vw, vc, None)

    def faces(tsdf=p, weight=p, dims=(4, 4, 4), w_min=1.0, counter=p, cap=2, edge=p, quad=p):
        return lib.estd_tsdf_mesh_faces(tsdf, weight, dims[0], dims[1], dims[2], w_min, counter, cap, edge, quad, None)

    for kw in (dict(tsdf=None), dict(weight=None), dict(origin=None), dict(counter=None), dict(cap=-1), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=inf),
               dict(voxel=nan), dict(w_min=nan), dict(cell=None), dict(xyz=None), dict(normal=None), dict(vw=None), dict(color=p, vc=None),
               dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(4, 4, 0))):
        assert vertices(**kw) == -1, kw
    for kw in (dict(tsdf=None), dict(weight=None), dict(counter=None), dict(cap=-1), dict(w_min=nan), dict(edge=None), dict(quad=None), dict(dims=(4, 0, 4))):
        assert faces(**kw) == -1, kw
    for dims in ((2048, 1024, 1024), (65536, 2, 2), (2, 65535 * 4 + 1, 2), (2, 2, (1 << 20) + 1)):
        assert vertices(dims=dims) == -3 and faces(dims=dims) == -3, dims
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (1, 1, 1)):
        assert vertices(dims=dims) == 0 and faces(dims=dims) == 0, dims
    assert not any(buf)                              # nothing was written
