"""The LDS-tiled 1x1 kernel (csrc/conv1x1.hip, conv1x1_lds_kernel) synchronises its stage ring with hand-counted ``s_waitcnt vmcnt(N)`` and a
raw ``s_barrier``: the counts hold only while no instance touches scratch memory (a spill is a vector-memory access the counts do not know
about).  The compiler's resource account, with the library's flags, must show no scratch and no spills for every instance."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv1x1_lds_instances_use_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is not installed")
    kr = _tool()
    rec, _ = kr.resource_usage(os.path.join(kr.CSRC, "conv1x1.hip"), isa=False)
    names = kr.demangle(list(rec))
    lds = {names.get(k, k): v for k, v in rec.items() if "conv1x1_lds_kernel" in names.get(k, k)}
    assert len(lds) == 11, sorted(lds)                 # every instance of the dispatcher's switch
    for name, d in sorted(lds.items()):
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d, (name, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (name, d)
