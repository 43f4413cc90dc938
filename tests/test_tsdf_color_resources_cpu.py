"""The colour instances of the TSDF kernels (csrc/tsdf.hip tsdf_integrate_kernel<*, true> and tsdf_edge_colors_kernel, csrc/tsdf_raycast.hip
tsdf_raycast_kernel<*, true>) hold per-frame state in registers -- (tsdf, w, pixel) for 8 frames x 4 voxels in the integrate kernel, the
previous sample's cell in the ray caster: the compiler's resource account, with the library's flags, must show no scratch and no spilled
register for every one of them, and no scratch for the instances that existed before."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _instances(kr, source):
    rec, _ = kr.resource_usage(os.path.join(kr.CSRC, source), isa=False)
    names = kr.demangle(list(rec))
    return {names.get(k, k): v for k, v in rec.items()}


@pytest.mark.parametrize("source,kernel,colour,plain", [("tsdf.hip", "tsdf_integrate_kernel", ("<false, true>", "<true, true>"), ("<false, false>", "<true, false>")),
                                                        ("tsdf_raycast.hip", "tsdf_raycast_kernel", ("<false, true>", "<true, true>"), ("<false, false>", "<true, false>"))])
def test_colour_instances_use_no_scratch_and_spill_nothing(source, kernel, colour, plain):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is not installed")
    inst = _instances(_tool(), source)
    for tag in colour + plain:
        hits = {n: d for n, d in inst.items() if kernel + tag in n}
        assert len(hits) == 1, (tag, sorted(inst))
        (name, d), = hits.items()
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d, (name, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0, (name, d)
        if tag in colour:
            assert d["SGPRs Spill"] == 0, (name, d)
    if source == "tsdf.hip":
        (name, d), = {n: d for n, d in inst.items() if "tsdf_edge_colors_kernel" in n}.items()
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0 and d["SGPRs Spill"] == 0, (name, d)
