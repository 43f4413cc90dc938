"""CPU: every refusal of the global-registration entry points that needs no device.  The C ABI (include/estd_hip.h: estd_cloud_spfh,
estd_cloud_fpfh, estd_feature_match, estd_ransac_pairs) refuses before any launch, so host memory stands in for the pointers: negative
sizes, nulls with work to do, k out of range, a dist_max or an edge_ratio out of range -> ESTD_ERR_ARG (-1); 2^31 rows or more ->
ESTD_ERR_UNSUPPORTED (-3); nothing to do -> ESTD_OK without a launch.  The operators (estdepth_amd/ops.py, either binding) and the Python
entry points (estdepth_amd/registration.py) refuse host tensors, wrong types and shapes and values out of range with a RuntimeError that
names the operator and the argument."""
import ctypes

import pytest
import torch

from estdepth_amd import ops, registration

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from estdepth_amd import _native, build
    build.build()
    return _native.lib()


def test_c_abi_refusals(lib):
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)

    def spfh(points=p, normal=p, n=4, index=p, count=p, k=8, oriented=1, hist=p, pairs=p):
        return lib.estd_cloud_spfh(points, normal, n, index, count, k, oriented, hist, pairs, None)

    for kw in (dict(n=-1), dict(k=0), dict(k=33), dict(k=-1), dict(points=None), dict(normal=None), dict(index=None), dict(count=None), dict(hist=None),
               dict(pairs=None)):
        assert spfh(**kw) == -1, kw
    assert spfh(n=2 ** 31) == -3
    assert spfh(n=0, points=None, normal=None, index=None, count=None, hist=None, pairs=None) == 0

    def fpfh(points=p, normal=p, n=4, index=p, count=p, k=8, hist=p, pairs=p, desc=p, valid=p, invalid=p):
        return lib.estd_cloud_fpfh(points, normal, n, index, count, k, hist, pairs, desc, valid, invalid, None)

    for kw in (dict(n=-1), dict(k=0), dict(k=33), dict(points=None), dict(normal=None), dict(index=None), dict(count=None), dict(hist=None), dict(pairs=None),
               dict(desc=None), dict(valid=None), dict(invalid=None)):
        assert fpfh(**kw) == -1, kw
    assert fpfh(n=2 ** 31) == -3
    assert fpfh(n=0, points=None, desc=None, valid=None, invalid=None) == 0

    def match(a=p, m=4, b=p, n=4, av=None, bv=None, index=p, d2=p, second=p):
        return lib.estd_feature_match(a, m, b, n, av, bv, index, d2, second, None)

    for kw in (dict(m=-1), dict(n=-1), dict(a=None), dict(b=None), dict(index=None), dict(d2=None), dict(second=None)):
        assert match(**kw) == -1, kw
    for kw in (dict(m=2 ** 31), dict(n=2 ** 31)):
        assert match(**kw) == -3, kw
    assert match(m=0, a=None, index=None, d2=None, second=None) == 0

    def ransac(P=p, Q=p, c=4, H=4, seed=0, dist_max=0.1, edge_ratio=0.9, count=p, status=p, ssq=p, T=p, best=p):
        return lib.estd_ransac_pairs(P, Q, c, H, seed, dist_max, edge_ratio, count, status, ssq, T, best, None)

    for kw in (dict(c=-1), dict(H=-1), dict(dist_max=-1.0), dict(dist_max=NAN), dict(dist_max=INF), dict(edge_ratio=-0.1), dict(edge_ratio=1.5),
               dict(edge_ratio=NAN), dict(P=None), dict(Q=None), dict(count=None), dict(status=None), dict(ssq=None), dict(T=None), dict(best=None)):
        assert ransac(**kw) == -1, kw
    for kw in (dict(c=2 ** 31), dict(H=2 ** 31)):
        assert ransac(**kw) == -3, kw
    assert ransac(H=0, count=None, status=None, ssq=None, T=None, best=None) == 0
    assert not any(buf)                              # nothing was written
    from estdepth_amd import _native
    assert {"estd_cloud_spfh", "estd_cloud_fpfh", "estd_feature_match", "estd_ransac_pairs"} <= set(_native.EXPORTED_SYMBOLS)


def _ops_calls():
    z3, zi, zc = torch.zeros((4, 3)), torch.zeros((4, 8), dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    zd, zh = torch.zeros((4, 33)), torch.zeros((4, 33), dtype=torch.int32)
    return ((ops.cloud_spfh, (z3, z3, zi, zc, True)), (ops.cloud_fpfh, (z3, z3, zi, zc, zh, zc)), (ops.feature_match, (zd, zd)),
            (ops.ransac_pairs, (z3, z3, 4, 0, 0.1, 0.9)))


@pytest.mark.parametrize("binding", ["ctypes", "torch"])
def test_the_operators_refuse_host_tensors(binding, monkeypatch, lib):
    monkeypatch.setattr(ops, "BINDING", binding)
    for op, args in _ops_calls():
        with pytest.raises(RuntimeError):
            op(*args)
        with pytest.raises(RuntimeError):
            op(None, *args[1:])


@pytest.mark.parametrize("binding", ["ctypes", "torch"])
def test_ransac_pairs_takes_whole_numbers_only(binding, monkeypatch):
    """4.7 hypotheses are not silently 4, True is not 1: refused before either binding sees the call"""
    monkeypatch.setattr(ops, "BINDING", binding)
    z3 = torch.zeros((4, 3))
    for bad in (4.7, True, "3", None):
        with pytest.raises(RuntimeError, match="ransac_pairs: hypotheses must be an integer"):
            ops.ransac_pairs(z3, z3, bad, 0, 0.1, 0.9)
        with pytest.raises(RuntimeError, match="ransac_pairs: seed must be an integer"):
            ops.ransac_pairs(z3, z3, 4, bad, 0.1, 0.9)


def test_the_ctypes_front_end_names_operator_and_argument(monkeypatch):
    monkeypatch.setattr(ops, "BINDING", "ctypes")
    for op, args in _ops_calls():
        with pytest.raises(RuntimeError, match="ROCm device"):
            op(*args)
    dev = torch.device("cpu")
    good = torch.zeros((4, 33), dtype=torch.int32)
    ops._table(good, "some_op", "some_arg", dev, 4, 33, torch.int32, "int32")
    ops._table(good, "some_op", "some_arg", dev, None, 33, torch.int32, "int32")
    for bad, rows, cols, dt in ((good, 5, 33, torch.int32), (good, 4, 32, torch.int32), (good, 4, 0, torch.int32), (good, 4, 33, torch.int64),
                                (good.t(), 33, 4, torch.int32), (None, 4, 33, torch.int32), (good[:, 0], 4, 33, torch.int32)):
        with pytest.raises(RuntimeError, match=r"some_op: some_arg must be a contiguous int32 \["):
            ops._table(bad, "some_op", "some_arg", dev, rows, cols, dt, "int32")
    with pytest.raises(RuntimeError, match=r"\[n,32\]"):
        ops._table(good, "some_op", "some_arg", dev, None, 32, torch.int32, "int32")


def test_the_python_entry_points_refuse_before_the_device():
    z = torch.zeros((4, 3))
    for k in (0, 33, 2.0, True):
        with pytest.raises(RuntimeError, match="fpfh: k"):
            registration.fpfh(z, z, k=k, radius=0.1)
    with pytest.raises(RuntimeError, match="fpfh: radius"):
        registration.fpfh(z, z)
    for radius in (0.0, -1.0, NAN, INF, 1e20):
        with pytest.raises(RuntimeError, match="max_dist"):
            registration.fpfh(z, z, radius=radius)
    with pytest.raises(RuntimeError, match="ROCm device"):
        registration.fpfh(z, z, radius=0.1)
    with pytest.raises(RuntimeError, match="fpfh: grid"):
        registration.fpfh(z, z, grid="grid")
    for ratio in (0.0, -0.5, 1.5, "x"):
        with pytest.raises(RuntimeError, match="match_features: ratio"):
            registration.match_features(torch.zeros((4, 33)), torch.zeros((4, 33)), ratio=ratio)
    with pytest.raises(RuntimeError, match="ransac_pairs: src_xyz"):
        registration.ransac_pairs(z, z, torch.zeros((2, 2), dtype=torch.int64), 0.1)
    for voxel in (0.0, -1.0, NAN, INF, "v"):
        with pytest.raises(RuntimeError, match="register_global: voxel"):
            registration.register_global(z, z, voxel)
    for mc in (2, 0, 3.0):
        with pytest.raises(RuntimeError, match="register_global: min_count"):
            registration.register_global(z, z, 0.1, min_count=mc)
    with pytest.raises(RuntimeError, match="register_global: refine"):
        registration.register_global(z, z, 0.1, refine="plane")
    with pytest.raises(RuntimeError, match="ROCm device"):
        registration.register_global(z, z, 0.1)
