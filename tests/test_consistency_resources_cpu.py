"""The consistency kernel (csrc/depth_consistency.hip depth_consistency_kernel) keeps its source loop rolled and reads the 8 x 24 matrix
values from the launch arguments at the loop's index: the compiler's resource account, with the library's flags, must show no scratch and no
spilled register for every instance of it."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_consistency_kernel_uses_no_scratch_and_spills_nothing():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is not installed")
    kr = _tool()
    rec, _ = kr.resource_usage(os.path.join(kr.CSRC, "depth_consistency.hip"), isa=False)
    names = kr.demangle(list(rec))
    inst = {names.get(k, k): v for k, v in rec.items() if "depth_consistency_kernel" in names.get(k, k)}
    assert len(inst) >= 1, sorted(names.values())
    for name, d in inst.items():
        print(name, d)
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d, (name, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (name, d)
