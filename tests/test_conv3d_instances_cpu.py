"""CPU: tests/conv3d_instances.py, the copy of the 3x3x3 launchers' instance choice that tests/test_gpu_conv3d_routes.py asserts on the
device, over the whole argument grid -- every plan of ``_plan_args``, with and without tanh, under every switch setting the GPU suite uses,
every subset of {res, res2, scale, acc, stats, gate, head}, four and eight waves.  The route of a combination is the one
ops.Conv3dPlan.route gives (pure: a plan on the CPU answers).  Every prediction lies in the claim table INSTANCES, and every entry of
INSTANCES is predicted by some combination: neither the table nor the predictor can drift alone."""
import itertools

import pytest

import conv3d_instances as CI
import test_gpu_conv3d_routes as G3
from estdepth_amd import ops
from test_conv_routes_cpu import _call, _plan3d, build, switches      # noqa: F401 (fixtures)

SWITCH_SETS = ({}, G3.DIRECT, G3.W2, G3.W2XOUT, dict(W3_EXTRA=False))


def _subsets(names):
    return [set(c) for n in range(len(names) + 1) for c in itertools.combinations(names, n)]


def _grid():
    """(plan, activations, switches)"""
    for name, acts in itertools.product(CI.PLANS, (("relu",), ("tanh",))):
        for sw in SWITCH_SETS:
            yield name, acts, sw


def _epilogues(name):
    """every subset the plan can be called with: only 16>16h has a head, and without "head" it is asked for its 16 -> 16 volume"""
    for epi in _subsets(CI.EPILOGUE):
        if name != "16>16h":
            if "head" not in epi:
                yield epi
        else:
            yield epi | {"main"}
            if "head" in epi:
                yield epi


def test_readback_kind_is_the_launchers():
    # csrc/estd_common.h: (!res_any && !accumulate) ? 0 : (!res_any ? 1 : (!accumulate ? 2 : 3))
    assert [CI.readback_kind(r, a) for r in (False, True) for a in (False, True)] == [0, 1, 2, 3]


def test_predictor_over_the_whole_grid(build, switches):
    build(False)
    seen = {route: set() for route in CI.INSTANCES}
    refused, n = set(), 0
    for name, acts, sw in _grid():
        switches(**sw)
        plan = _plan3d(name, acts)
        for epi in _epilogues(name):
            try:
                route = plan.route(**_call(plan, epi))
            except RuntimeError:                             # (the reset gate on a route other than the 32 -> 16 instance's)
                assert "gate" in epi, (name, epi)
                continue
            for waves in (4, 8):
                try:
                    got = CI.instance(route, name, epi, waves)
                except CI.Refused:
                    refused.add((route, name, frozenset(epi)))
                    continue
                n += 1
                assert got <= CI.reach(route), (route, name, sorted(epi), waves, sorted(got))
                assert len(got) == len(ops.CONV3D_ROUTES[route]), (route, sorted(got))
                seen[route] |= got
    assert n > 1000
    for route in CI.INSTANCES:
        assert seen[route] == CI.reach(route), (route, sorted(CI.reach(route) - seen[route]))
    # the one call a route lets through and its launcher refuses: the reset gate next to a read-back stream
    assert refused and all(route == "wino2_o16" and "gate" in epi and epi & {"res", "res2", "scale", "acc"} for route, _, epi in refused), refused


def test_instances_is_a_partition_of_25():
    named = [k for ks in CI.INSTANCES.values() for k in ks]
    assert len(named) == len(set(named)) == 25
    assert all(k in CI.ALL for ks in CI.SHARED.values() for k in ks)
    assert CI.KERNELS["wino3+xout"] == {"conv3d_wino3_kernel", "conv3d_xout_kernel"}


@pytest.mark.parametrize("route,plan,epi,waves,want", [
    ("wino2", "32>32", (), 8, "conv3d_wino2_kernel<8, 0, false, false, false, false>"),
    ("wino2", "32>32", ("acc",), 8, "conv3d_wino2_kernel<8, 1, false, false, false, false>"),
    ("wino2", "32>32", ("scale",), 8, "conv3d_wino2_kernel<8, 2, false, false, false, false>"),
    ("wino2", "32>32", ("res2", "acc"), 8, "conv3d_wino2_kernel<8, 3, false, false, false, false>"),
    ("wino2", "32>32", ("acc",), 4, "conv3d_wino2_kernel<4, 3, false, false, false, false>"),
    ("wino2", "32>32", ("stats",), 4, "conv3d_wino2_kernel<4, 0, false, false, false, false>"),
    ("wino2", "33>32", ("res",), 4, "conv3d_wino2_kernel<8, 3, true, false, false, false>"),
    ("wino2_o16", "32>16", ("acc",), 8, "conv3d_wino2_kernel<8, 3, false, true, false, false>"),
    ("wino2_o16", "32>16", ("gate", "stats"), 4, "conv3d_wino2_kernel<8, 0, false, true, false, true>"),
    ("wino2_xout", "33>33", (), 4, "conv3d_wino2_kernel<8, 0, true, false, true, false>"),
    ("wino3", "32>32", ("stats",), 8, "conv3d_wino3_kernel<0, true, false>"),
    ("wino3", "32>32", ("res", "scale"), 8, "conv3d_wino3_kernel<2, false, false>"),
    ("wino3", "33>32", (), 8, "conv3d_wino3_kernel<0, false, true>"),
    ("direct", "33>33", ("res",), 8, "conv3d_k3_kernel<32, 2, true, true>"),
    ("direct", "16>16h", ("head",), 8, "conv3d_k3_kernel<16, 1, false, false>"),
])
def test_known_launches(route, plan, epi, waves, want):
    """launcher lines read off the sources, spelled out"""
    assert CI.instance(route, plan, epi, waves) == {want}


def test_every_gpu_case_has_a_prediction():
    """each case of the GPU suite names an instance set of its route's row (or is one the launcher refuses, and says so in its id)"""
    for p in G3.CASES + G3.READBACK:
        case = p.values[0]
        for waves in (4, 8):
            try:
                got = CI.instance(case["route"], case["plan"], case["epi"], waves)
            except CI.Refused:
                assert p.id.startswith("refused-"), p.id
                continue
            assert got and got <= CI.reach(case["route"]) and not p.id.startswith("refused-"), (p.id, sorted(got))
