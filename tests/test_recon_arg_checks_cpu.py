"""CPU: the argument checks of the ctypes front ends that need no device (estdepth_amd/ops.py; the file keeps the name it got when the
helpers served the reconstruction operators only): the host-values helper, the four fp32 scalar rules and the grid-cell rule, at the fp32
edges the GPU suites reach only through whole operator calls, and the network operators' count rule, list rule and non-tensor refusals.
The verdicts are the operators' under both bindings (csrc/torch_ops.cpp applies the same rules); a refused value raises RuntimeError with
the operator's and the argument's name in the message."""
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


# ------------------------------------------------------------------------------------------------- the network operators' helpers
def _raises(call):
    with pytest.raises(RuntimeError) as e:
        call()
    assert "some_op" in str(e.value) and "some_arg" in str(e.value), str(e.value)


@pytest.mark.parametrize("lo,hi", [(1, 16), (1, 4), (0, 32), (3, 3)])
def test_count_at_its_edges(lo, hi):
    for v in (lo, hi):
        ops._count(v, lo, hi, "some_op", "some_arg")
    for v in (lo - 1, hi + 1):
        _raises(lambda: ops._count(v, lo, hi, "some_op", "some_arg"))
    with pytest.raises(RuntimeError, match="at most %d" % hi):
        ops._count(hi + 1, lo, hi, "some_op", "some_arg")


def test_count_with_an_empty_range_refuses_everything():
    """avgpool_nhwc on an empty map (1..min(H, W) = 1..0), cdhw_to_vol with a negative stride (0..dst_stride)"""
    for v in (-1, 0, 1):
        _raises(lambda: ops._count(v, 1, 0, "some_op", "some_arg"))


NOT_TENSORS = [None, [0.0] * 16, 1.0, "x"]


@pytest.mark.parametrize("bad", NOT_TENSORS, ids=["none", "list", "float", "str"])
def test_a_non_tensor_is_refused_by_every_tensor_helper(bad):
    """RuntimeError, never the AttributeError / TypeError of the first attribute access"""
    calls = [lambda: ops._floats(bad, 16, "some_op", "some_arg"),
             lambda: ops._floats(bad, 16, "some_op", "some_arg", at_least=True, strided=True),
             lambda: ops._map(bad, (-1, -1), "some_op", "some_arg"),
             lambda: ops._records(bad, "some_op", "some_arg"),
             lambda: ops._channels_last(bad, "some_op", "some_arg"),
             lambda: ops._like([bad], torch.zeros(2, 3), "some_op", "some_arg", None)]
    if bad is not None:                                  # (None is the optional vector that is not there)
        calls.append(lambda: ops._opt_floats(bad, 16, "some_op", "some_arg", None))
    for call in calls:
        with pytest.raises(RuntimeError, match="some_op.*some_arg.*must be a tensor"):
            call()
    assert ops._opt_floats(None, 16, "some_op", "some_arg", None) is None


def test_a_cpu_tensor_is_refused_by_every_tensor_helper():
    t = torch.zeros(1, 4, 2, 2)
    for call in (lambda: ops._floats(t, 16, "some_op", "some_arg"), lambda: ops._map(t, (-1, -1), "some_op", "some_arg"),
                 lambda: ops._records(torch.zeros(2, 32), "some_op", "some_arg"), lambda: ops._opt_floats(t, 16, "some_op", "some_arg", None),
                 lambda: ops._channels_last(t.contiguous(memory_format=torch.channels_last), "some_op", "some_arg"),
                 lambda: ops._like([t], t, "some_op", "some_arg", None)):
        with pytest.raises(RuntimeError, match="some_op.*some_arg.*ROCm device"):
            call()


@pytest.fixture
def any_device(monkeypatch):
    """the shape rules of the helpers on CPU tensors: _chk's rules are switched off but for 'is a tensor' (they need a device to pass)"""
    def chk(t, name, dtype=torch.float32, op=None, dev=None, contiguous=True):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("%s: %s must be a tensor" % (op, name))
        return t
    monkeypatch.setattr(ops, "_chk", chk)


def test_a_list_with_one_odd_shape(any_device):
    first = torch.zeros(2, 3, 5, 32)
    same = [torch.zeros(2, 3, 5, 32) for _ in range(3)]
    assert len(ops._like(same, first, "some_op", "some_arg", None)) == 3
    assert len(ops._like([], first, "some_op", "some_arg", None)) == 0           # (the count rule is _count's)
    for i, odd in ((0, torch.zeros(2, 3, 32, 5)), (1, torch.zeros(2, 5, 3, 32)), (2, torch.zeros(2 * 3 * 5 * 32)), (2, torch.zeros(2, 3, 5, 31))):
        ts = list(same)
        ts[i] = odd
        with pytest.raises(RuntimeError, match=r"some_op.*some_arg\[%d\].*another shape" % i):
            ops._like(ts, first, "some_op", "some_arg", None)
    with pytest.raises(RuntimeError, match=r"some_op.*some_arg\[1\].*must be a tensor"):
        ops._like([first, None], first, "some_op", "some_arg", None)


def test_floats_exactly_and_at_least(any_device):
    t = torch.zeros(3, 4)
    assert ops._floats(t, 12, "some_op", "some_arg") is t
    assert ops._floats(t, 12, "some_op", "some_arg", at_least=True) is t and ops._floats(t, 5, "some_op", "some_arg", at_least=True) is t
    for n in (11, 13):
        _raises(lambda: ops._floats(t, n, "some_op", "some_arg"))
    _raises(lambda: ops._floats(t, 13, "some_op", "some_arg", at_least=True))
    assert ops._opt_floats(t, 12, "some_op", "some_arg", None) is t
    _raises(lambda: ops._opt_floats(t, 11, "some_op", "some_arg", None))


def test_whole_records(any_device):
    assert ops._records(torch.zeros(2, 3, 32), "some_op", "some_arg") == 6 and ops._records(torch.zeros(64), "some_op", "some_arg") == 2
    for n in (31, 33, 65):
        _raises(lambda: ops._records(torch.zeros(n), "some_op", "some_arg"))


def test_channels_last_rule(any_device):
    x = torch.zeros(2, 4, 3, 5).contiguous(memory_format=torch.channels_last)
    assert ops._channels_last(x, "some_op", "some_arg") == (2, 4, 3, 5)
    assert ops._channels_last(x.clone(memory_format=torch.channels_last), "some_op", "some_arg", like=x) == (2, 4, 3, 5)
    for bad in (torch.zeros(2, 4, 3, 5), torch.zeros(4, 3, 5), x[:, :, :, ::2]):
        with pytest.raises(RuntimeError, match="some_op.*some_arg.*channels_last"):
            ops._channels_last(bad, "some_op", "some_arg")
    other = torch.zeros(2, 4, 5, 3).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="some_op.*some_arg.*shape"):
        ops._channels_last(other, "some_op", "some_arg", like=x)


def test_map_tail_rule(any_device):
    """a transposed size, a missing axis and extra leading sizes other than 1 are refused; leading 1s pass"""
    t = torch.zeros(3, 5, 32)
    assert ops._map(t, (-1, -1, 32), "some_op", "some_arg") == (3, 5, 32)
    assert ops._map(t[None], (3, 5, 32), "some_op", "some_arg") == (3, 5, 32)
    for bad, tail in ((torch.zeros(3, 32, 5), (-1, -1, 32)), (torch.zeros(5, 32), (-1, -1, 32)), (torch.zeros(2, 3, 5, 32), (-1, -1, 32)),
                      (t, (5, 3, 32))):
        with pytest.raises(RuntimeError, match="some_op.*some_arg.*must end in the sizes"):
            ops._map(bad, tail, "some_op", "some_arg")
