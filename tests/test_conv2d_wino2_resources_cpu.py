"""The F(2x2, 3x3) kernel (csrc/conv2d_wino2.hip) keeps its accumulators, weight ring and brick prefetch in registers at two waves per SIMD
in both work decompositions: the compiler's resource account, with the library's flags, must show no scratch and no spilled VGPRs for every
instance of ``conv2d_wino2_kernel`` -- the default build (operand-reuse items for Cout % 64 == 0), the round-6 decomposition alone
(-DESTD_C2W2_SPLIT=0) and the operand-reuse form for every Cout (-DESTD_C2W2_SPLIT=2)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("split", [None, 0, 2])
def test_conv2d_wino2_instances_use_no_scratch(split, monkeypatch):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is not installed")
    kr = _tool()
    if split is not None:
        monkeypatch.setattr(kr, "FLAGS", kr.FLAGS + ["-DESTD_C2W2_SPLIT=%d" % split])
    rec, _ = kr.resource_usage(os.path.join(kr.CSRC, "conv2d_wino2.hip"), isa=False)
    names = kr.demangle(list(rec))
    inst = {names.get(k, k): v for k, v in rec.items() if "conv2d_wino2_kernel" in names.get(k, k)}
    assert sorted(n.split("::")[-1].split("(")[0] for n in inst) == ["conv2d_wino2_kernel<1>", "conv2d_wino2_kernel<2>"], sorted(inst)
    for name, d in sorted(inst.items()):
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "Occupancy [waves/SIMD]" in d, (name, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0, (name, d)
        assert d["Occupancy [waves/SIMD]"] >= 2, (name, d)
