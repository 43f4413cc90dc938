"""CPU: the argument checks of the reconstruction operators' ctypes front ends that need no device (estdepth_amd/ops.py): the host-values
helper, the four fp32 scalar rules and the grid-cell rule, at the fp32 edges the GPU suites reach only through whole operator calls.  The
verdicts are the operators' under both bindings (csrc/torch_ops.cpp applies the same rules); a refused value raises RuntimeError with the
operator's and the argument's name in the message."""
import ctypes
import math

import pytest
import torch

from estdepth_amd import ops

NAN, INF = float("nan"), float("inf")


def _refused(rule, value, **kw):
    with pytest.raises(RuntimeError) as e:
        rule(value, "some_op", "some_arg", **kw)
    assert "some_op" in str(e.value) and "some_arg" in str(e.value), str(e.value)


def test_the_edges_are_where_fp32_puts_them():
    f32 = lambda v: ctypes.c_float(v).value                                              # noqa: E731
    assert f32(1e-46) == 0.0 and f32(1e-45) > 0.0
    assert math.isinf(f32(f32(1e20) ** 2)) and math.isfinite(f32(f32(1.8e19) ** 2))
    assert f32(f32(1e-23) ** 2) == 0.0 and f32(f32(1e-20) ** 2) > 0.0
    assert math.isinf(f32(1.0 / f32(1e-39))) and math.isfinite(f32(1.0 / f32(1e-38)))


@pytest.mark.parametrize("v", [NAN, INF, 0.0, -0.0, -1.0, 1e-46])
def test_positive_refuses(v):
    _refused(ops._positive, v)


@pytest.mark.parametrize("v", [1e-45, 1.0])
def test_positive_accepts(v):
    ops._positive(v, "some_op", "some_arg")


@pytest.mark.parametrize("v", [NAN, INF, -1e-30])
def test_not_negative_refuses(v):
    _refused(ops._not_negative, v)


@pytest.mark.parametrize("v", [0.0, -0.0])
def test_not_negative_accepts(v):
    ops._not_negative(v, "some_op", "some_arg")


def test_not_nan():
    _refused(ops._not_nan, NAN)
    ops._not_nan(-INF, "some_op", "some_arg")


def test_positive_with_a_finite_square():
    """cloud_nearest's max_dist: the square may round to 0, it may not overflow"""
    for v in (NAN, INF, 0.0, -1.0, 1e20):
        _refused(ops._positive_square, v)
    for v in (1.8e19, 1e-23):
        ops._positive_square(v, "some_op", "some_arg")


def test_positive_with_a_finite_positive_square():
    """frame_align's dist_max: the square may neither overflow nor round to 0"""
    for v in (NAN, INF, 0.0, -1.0, 1e20, 1e-23):
        _refused(ops._positive_square, v, square_positive=True)
    for v in (1e-20, 1.8e19):
        ops._positive_square(v, "some_op", "some_arg", square_positive=True)


def test_grid_cell_needs_a_finite_fp32_reciprocal():
    lo = torch.zeros(3)
    for cell in (1e-39, NAN, INF, 0.0, -1.0):
        with pytest.raises(RuntimeError, match="some_op.*cell"):
            ops._cloud_grid(lo, cell, (4, 4, 4), "some_op", ops.CLOUD_MAX_DIM)
    assert ops._cloud_grid(lo, 1e-38, (4, 5, 6), "some_op", ops.CLOUD_MAX_DIM) == ([0.0, 0.0, 0.0], (4, 5, 6))
    with pytest.raises(RuntimeError, match="some_op.*lo"):
        ops._cloud_grid(torch.tensor([0.0, INF, 0.0]), 0.1, (4, 4, 4), "some_op", ops.CLOUD_MAX_DIM)
    with pytest.raises(RuntimeError, match="some_op.*dims"):
        ops._cloud_grid(lo, 0.1, (4, 4, ops.CLOUD_MAX_DIM + 1), "some_op", ops.CLOUD_MAX_DIM)


@pytest.mark.parametrize("bad", [torch.zeros(12, dtype=torch.float64), torch.zeros(12, 2)[:, 0], torch.zeros(11), torch.zeros(13), [0.0] * 12, None],
                         ids=["float64", "strided", "short", "long", "list", "none"])
def test_host_values_refuses(bad):
    with pytest.raises(RuntimeError) as e:
        ops._host_values(bad, 12, "some_op", "some_arg", "[12]")
    assert "some_op" in str(e.value) and "some_arg" in str(e.value) and "[12]" in str(e.value)


def test_host_values_and_the_finite_flag():
    t = torch.arange(24, dtype=torch.float32).reshape(2, 12)
    assert ops._host_values(t, 24, "some_op", "some_arg", "[T,12]") == [float(i) for i in range(24)]
    for bad in (NAN, INF, -INF):
        t[1, 3] = bad
        got = ops._host_values(t, 24, "some_op", "some_arg", "[T,12]")                 # not checked unless asked for
        assert len(got) == 24 and (got[15] == bad or bad != bad)
        with pytest.raises(RuntimeError, match="some_op.*some_arg.*not finite"):
            ops._host_values(t, 24, "some_op", "some_arg", "[T,12]", finite=True)
