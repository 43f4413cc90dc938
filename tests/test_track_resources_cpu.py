"""The ledger of csrc/track/frame_align.hip (CPU; needs hipcc).  tests/test_kernel_ledger_cpu.py walks ``csrc/*.hip`` only; this file gives the
same guarantee for the tracking source: the file is cross-compiled with the library's flags (tools/kernel_resources.py: the demangled names
and the compiler's resource remarks, nothing else), the set of ``*_kernel`` functions it emits must EQUAL the set claimed by the INSTANCES
table of tests/test_gpu_track_routes.py -- a kernel added to the source cannot ship without a case that names it, and nothing claimed may
be absent -- and every instance must show no scratch, no spilled vector register and no spilled scalar register."""
import importlib.util
import os
import re

import pytest

import test_gpu_track_routes as GT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join("track", "frame_align.hip")


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
    named = [k for ks in GT.INSTANCES.values() for k in ks]
    assert len(named) == len(set(named)), sorted(named)
    assert set(named) == set(emitted), (sorted(set(named) ^ set(emitted)))
    assert not GT.NOT_ROUTES


def test_instances_use_no_scratch_and_spill_nothing(emitted):
    assert emitted
    for inst, d in emitted.items():
        print(inst, d)
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (inst, d)
