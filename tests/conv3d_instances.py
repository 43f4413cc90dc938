"""Which template instance of the 3x3x3 kernels a launch runs: a plain-Python copy of the instance choice of the five launchers
(csrc/conv3d_mfma.hip ``estd_conv3d_k3``, csrc/conv3d_wino3.hip, csrc/conv3d_wino2.hip ``estd_conv3d_k3_wino2``, csrc/conv3d_xout.hip,
csrc/conv3d_wino2_c16.hip), for the routes of ops.CONV3D_ROUTES that the default build carries.  No torch, no GPU.

The names are spelled as the demangler and torch.profiler print them: ``conv3d_wino2_kernel<8, 3, true, false, false, false>``.

    conv3d_k3_kernel<CM, NT, EXTRA, XOUT>                    by the plan's shape alone: every epilogue is a run-time flag
    conv3d_wino3_kernel<RBK, STATS, EXTRA>                   RBK of the call; STATS / EXTRA only at RBK 0
    conv3d_wino2_kernel<NW, RBK, EXTRA, O16, XOUT, GATE>     RBK of the call in the plain eight-wave form; the scalar-channel (EXTRA),
                                                             32 -> 16 (O16) and four-wave (NW = 4, ESTD_WINO2_WAVES=4) forms have the
                                                             instances RBK 0 and 3 only: every call with a read-back stream runs <.., 3, ..>
RBK (csrc/estd_common.h estd_conv3d_readback_kind): 0 none, 1 running sum only, 2 residual(s) and / or out_scale != 1, 3 both."""

PLANS = {                   # plan (tests/test_gpu_conv3d_routes.py _plan_args) -> (main input channels, n_tiles, scalar input channel)
    "32>32": (32, 2, False), "33>32": (32, 2, True), "33>33": (32, 3, True), "32>16": (32, 1, False), "16>16": (16, 1, False),
    "16>16h": (16, 1, False),
}
EPILOGUE = ("res", "res2", "scale", "acc", "stats", "gate", "head")      # (+ "main": the 16 -> 16 volume next to the head's)


class Refused(ValueError):
    """the launcher returns an error before any launch"""


def readback_kind(res_any, accumulate):
    return (2 if res_any else 0) + (1 if accumulate else 0)


def _b(*flags):
    return ", ".join("true" if f else "false" for f in flags)


def _wino2(nw, rbk, extra, o16, xout=False, gate=False):
    return "conv3d_wino2_kernel<%d, %d, %s>" % (nw, rbk, _b(extra, o16, xout, gate))


def _wino3(rbk, stats, extra):
    return "conv3d_wino3_kernel<%d, %s>" % (rbk, _b(stats, extra))


def _k3(cm, nt, extra, xout):
    return "conv3d_k3_kernel<%d, %d, %s>" % (cm, nt, _b(extra, xout))


def instance(route, plan, epi, waves=8):
    """the kernel instances (a set of "name<args>") one Conv3dPlan.run of ``plan`` with the epilogue ``epi`` launches on ``route`` (the
    name Conv3dPlan.route returned) in a process whose ESTD_WINO2_WAVES latched ``waves``; Refused where the launcher takes no such call"""
    cin, nt, extra = PLANS[plan]
    epi = set(epi)
    assert epi <= set(EPILOGUE) | {"main"} and waves in (4, 8), (epi, waves)
    rbk = readback_kind(bool(epi & {"res", "res2", "scale"}), "acc" in epi)
    stats, gate = "stats" in epi, "gate" in epi
    if route == "direct":                                 # launch<CM, NT, EXTRA, XOUT>
        if cin == 32 and nt == 2:
            return {_k3(32, 2, extra, False)}
        if cin == 32 and nt == 3 and extra:
            return {_k3(32, 2, True, True)}
        if nt == 1 and not extra:
            return {_k3(cin, 1, False, False)}
        raise Refused("no instance of the direct kernel for %s" % plan)
    if route in ("wino3", "wino3+xout"):
        if cin != 32 or gate or "head" in epi:
            raise Refused("conv3d_wino3: 32 main input channels, no gate, no head")
        if route == "wino3+xout":                         # the first launch is a plain 33 -> 32 call, the second has one kernel
            if nt != 3 or not extra or rbk or stats:
                raise Refused("33 -> 33 in two launches: no read-back stream, no statistics")
            return {_wino3(0, False, True), "conv3d_xout_kernel"}
        if nt != 2 or (stats and rbk) or (extra and (rbk or stats)):
            raise Refused("conv3d_wino3: statistics / the scalar channel only without read-back streams")
        return {_wino3(rbk, stats and rbk == 0, extra and rbk == 0)}
    if route == "wino2_c16":
        if cin != 16 or "head" not in epi or "main" in epi or rbk or stats or gate:
            raise Refused("conv3d_wino2_c16: the head's volume only, plain epilogue")
        return {"conv3d_wino2_c16_kernel"}
    if route in ("wino2", "wino2_xout", "wino2_o16"):
        o16, xout = nt == 1, nt == 3
        if cin != 32 or "head" in epi or (route == "wino2_o16") != o16 or (route == "wino2_xout") != xout:
            raise Refused("%s does not take %s" % (route, plan))
        if (xout and (rbk or stats)) or (o16 and extra) or (extra and stats) or (gate and (not o16 or rbk)):
            raise Refused("conv3d_wino2: %s with %s" % (plan, sorted(epi)))
        wide = 3 if rbk else 0                            # the forms without an instance per kind
        if gate:
            return {_wino2(8, 0, False, True, False, True)}
        if o16:
            return {_wino2(8, wide, False, True)}
        if xout:
            return {_wino2(8, 0, True, False, True)}
        if extra:
            return {_wino2(8, wide, True, False)}
        return {_wino2(8, rbk, False, False)} if waves == 8 else {_wino2(4, wide, False, False)}
    raise KeyError(route)


# route -> the instances it launches; every instance the default library emits, once
INSTANCES = {
    "direct": [_k3(16, 1, False, False), _k3(32, 1, False, False), _k3(32, 2, False, False), _k3(32, 2, True, False), _k3(32, 2, True, True)],
    "wino3": [_wino3(0, False, False), _wino3(0, True, False), _wino3(0, False, True), _wino3(1, False, False), _wino3(2, False, False),
              _wino3(3, False, False)],
    "wino2": [_wino2(8, 0, False, False), _wino2(8, 1, False, False), _wino2(8, 2, False, False), _wino2(8, 3, False, False),
              _wino2(8, 0, True, False), _wino2(8, 3, True, False), _wino2(4, 0, False, False), _wino2(4, 3, False, False)],
    "wino2_xout": [_wino2(8, 0, True, False, True)],
    "wino2_o16": [_wino2(8, 0, False, True), _wino2(8, 3, False, True), _wino2(8, 0, False, True, False, True)],
    "wino2_c16": ["conv3d_wino2_c16_kernel"],
    "wino3+xout": ["conv3d_xout_kernel"],
}
# ... and the instances a route launches that another route's row claims (its first launch is the three-axis kernel's 33 -> 32 call)
SHARED = {"wino3+xout": [_wino3(0, False, True)]}
ALL = {k for ks in INSTANCES.values() for k in ks}


def reach(route):
    """every instance the route can launch"""
    return set(INSTANCES[route]) | set(SHARED.get(route, ()))


KERNELS = {route: {k.split("<")[0] for k in reach(route)} for route in INSTANCES}      # by kernel name, for the messages
