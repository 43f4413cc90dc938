"""One ledger of every kernel the library emits (CPU; needs hipcc): each ``csrc/*.hip`` is cross-compiled with the library's flags
(tools/kernel_resources.py: the demangled names and the compiler's resource remarks, nothing else) and every ``*_kernel`` function must be
claimed by exactly one GPU route suite's table -- or by a NOT_ROUTES entry that says why it is no route:

    tests/test_gpu_conv3d_routes.py        INSTANCES        per instance, template arguments included (tests/conv3d_instances.py)
    tests/test_gpu_conv2d_routes.py        ROUTES           by name prefix (the instance is predicted per case by the dispatcher copies)
    tests/test_gpu_sweep_fusion_routes.py  INSTANCES        per instance, template arguments included
    tests/test_gpu_glue2d_routes.py        INSTANCES        per instance
    tests/test_gpu_recon3d_routes.py       INSTANCES        per instance

so a kernel -- for the per-instance suites: a template instance -- added to a source cannot ship without a test that names it.  For the
four per-instance tables nothing claimed may be absent from the emitted set either.  The 25 instances of the glue and reconstruction suites hold no array the compiler could not keep in
registers: no scratch, no spilled vector register, and no spilled scalar register either -- but for the two plain integrate instances,
whose known counts are pinned (SGPR_IN_LANES)."""
import glob
import importlib.util
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

import test_gpu_conv2d_routes as G2
import test_gpu_conv3d_routes as G3
import test_gpu_glue2d_routes as GG
import test_gpu_recon3d_routes as GR
import test_gpu_sweep_fusion_routes as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKERS = 8                     # compiler processes at a time

# kernels no route suite claims, with the reason
NOT_ROUTES = {
    "conv3d_wino_kernel": "superseded A/B kernel (ESTD_BUILD_AB=1 builds only): tests/test_gpu_wino.py under the ab mark",
    "conv3d_wino2x_kernel": "superseded A/B kernel (ESTD_BUILD_AB=1 builds only): tests/test_gpu_wino.py under the ab mark",
    "conv3d_k3_split_kernel": "superseded A/B kernel (ESTD_BUILD_AB=1 builds only): tests/test_gpu_split_conv.py under the ab mark",
}
PER_INSTANCE = (("conv3d", G3), ("sweep_fusion", GS), ("glue2d", GG), ("recon3d", GR))
# Scalar registers the compiler parks in VGPR lanes (v_writelane / v_readlane: no scratch, no memory traffic), at most.  The plain integrate
# instances take the per-frame arguments of eight frames (128 SGPRs) by value and the scalar file cannot hold them beside the rest.  That
# is accepted there: the kernel is bound by the projection arithmetic of every voxel (profiles/tsdf_bench.txt: 0.150 ms for
# three 640 x 480 frames into 256^3), the lane traffic sits outside the per-voxel work, and the instances hold 99 / 100 VGPRs with no
# scratch (tests/test_tsdf_color_resources_cpu.py).  The colour instances fetch the arguments where they are used and spill nothing; doing
# the same here (93 VGPRs, no spill) is open until it is timed against these figures.  The counts are pinned so that they cannot grow
# unnoticed; every other instance must show 0.
SGPR_IN_LANES = {"tsdf_integrate_kernel<false, false>": 182, "tsdf_integrate_kernel<true, false>": 204}


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def emitted():
    """{instance name (template arguments included): (source file, the compiler's resource record)} over every csrc/*.hip"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc is not installed")
    kr = _tool()
    files = sorted(glob.glob(os.path.join(kr.CSRC, "*.hip")))
    assert files
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        recs = list(ex.map(lambda f: kr.resource_usage(f, isa=False)[0], files))
    out = {}
    for f, rec in zip(files, recs):
        names = kr.demangle(list(rec))
        for mangled, d in rec.items():
            m = re.search(r"(\w+_kernel)(<[^>()]*>)?\(", names[mangled])
            assert m, (f, names[mangled])
            inst = m.group(1) + (m.group(2) or "")
            assert inst not in out, "%s is emitted by %s and %s" % (inst, out[inst][0], os.path.basename(f))
            out[inst] = (os.path.basename(f), d)
    return out


def _base(inst):
    return inst.split("<")[0]


def _claims(inst):
    """the suites (or NOT_ROUTES tables) that claim an emitted instance"""
    base, who = _base(inst), []
    if any(base.startswith(prefix) for prefix, _ in G2.ROUTES):
        who.append("conv2d")
    for name, mod in PER_INSTANCE:
        if any(inst in ks for ks in mod.INSTANCES.values()):
            who.append(name)
        if inst in mod.NOT_ROUTES or base in mod.NOT_ROUTES:
            who.append(name + ".NOT_ROUTES")
    if base in NOT_ROUTES:
        who.append("ledger.NOT_ROUTES")
    return who


def test_every_emitted_kernel_is_claimed_by_exactly_one_suite(emitted):
    claims = {inst: _claims(inst) for inst in emitted}
    unclaimed = sorted(i for i, w in claims.items() if not w)
    twice = {i: w for i, w in claims.items() if len(w) > 1}
    assert not unclaimed, "no GPU suite names %s" % unclaimed
    assert not twice, "claimed more than once: %s" % twice
    for table in [NOT_ROUTES] + [mod.NOT_ROUTES for _, mod in PER_INSTANCE]:
        assert all(isinstance(r, str) and len(r) > 10 for r in table.values()), table


def test_per_instance_tables_claim_nothing_that_is_not_emitted(emitted):
    bases = {_base(i) for i in emitted}
    for name, mod in PER_INSTANCE:
        named = [k for ks in mod.INSTANCES.values() for k in ks]
        assert len(named) == len(set(named)), (name, sorted(named))
        assert not set(named) - set(emitted), (name, sorted(set(named) - set(emitted)))
        assert not {k for k in mod.NOT_ROUTES if k not in emitted and k not in bases}, (name, sorted(mod.NOT_ROUTES))
    assert set(NOT_ROUTES) <= bases, sorted(set(NOT_ROUTES) - bases)
    assert not {k for ks in G3.KERNELS.values() for k in ks} - bases
    assert all(any(b.startswith(prefix) for b in bases) for prefix, _ in G2.ROUTES)


def test_glue_and_reconstruction_instances_use_no_scratch_and_spill_nothing(emitted):
    insts = [k for mod in (GG, GR) for ks in mod.INSTANCES.values() for k in ks]
    assert len(insts) == 25, sorted(insts)
    for inst in insts:
        src, d = emitted[inst]
        assert "ScratchSize [bytes/lane]" in d and "VGPRs Spill" in d and "SGPRs Spill" in d, (inst, d)
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0, (src, inst, d)
        assert d["SGPRs Spill"] <= SGPR_IN_LANES.get(inst, 0), (src, inst, d)
