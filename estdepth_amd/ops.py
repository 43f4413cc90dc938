"""Torch-tensor front-end of the C ABI (device memory, streams and allocation are PyTorch-ROCm's;
the arithmetic is libestd_hip.so's).  Every function enqueues on the current HIP stream and
returns tensors owned by the caching allocator.  CUDA(ROCm)-only: CPU tensors raise RuntimeError.

Arguments are checked before anything is launched, by one helper per kind of rule ("argument checks" below); csrc/torch_ops.cpp has the
same helpers and every operator outside the convolution plans calls them in the same order under both bindings, so a call either runs
under both or raises RuntimeError, naming the operator and the argument, under both.  Value rules the C ABI enforces itself (strides,
channel multiples, 32-bit limits) come back as its status, a RuntimeError as well.
"""
import collections
import ctypes
import math
import numbers
import os

import torch

from . import _native as N
from . import packing

# Binding of the hot-path operators:
#   "torch"  (default) -- PyTorch custom operators torch.ops.estdepth_hip.* registered with TORCH_LIBRARY by
#             csrc/torch_ops.cpp (libestd_torch_ops.so): dispatcher, argument checks and at::empty outputs in C++, on the current
#             HIP stream of the first tensor's device;
#   "ctypes" -- the torch-free C ABI of libestd_hip.so called directly with raw device pointers (what a non-PyTorch host
#             would bind; kept as the second test path: ESTD_BINDING=ctypes), after the same argument checks in Python, under
#             torch.cuda.device(<the first tensor's device>).
# Both end in the same extern "C" entry points; there is no CPU / eager fallback under either.
BINDING = os.environ.get("ESTD_BINDING", "torch")
_TORCH_OPS_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libestd_torch_ops.so")
_torch_ops = None


def T():
    """torch.ops.estdepth_hip (loads libestd_torch_ops.so once; RuntimeError when it has not been built)."""
    global _torch_ops
    if _torch_ops is None:
        if BINDING not in ("torch", "ctypes"):
            raise RuntimeError("ESTD_BINDING must be 'torch' or 'ctypes', got %r" % (BINDING,))
        if not os.path.exists(_TORCH_OPS_LIB):
            raise RuntimeError("libestd_torch_ops.so not found at %s -- build it with `python -m estdepth_amd.build` "
                               "(there is no CPU/eager fallback)" % _TORCH_OPS_LIB)
        N.lib()                                   # libestd_hip.so first: the operator library links against it
        torch.ops.load_library(_TORCH_OPS_LIB)
        _torch_ops = torch.ops.estdepth_hip
    return _torch_ops


def _use_torch():
    return BINDING == "torch"

ACT = {"none": 0, "relu": 1, "tanh": 2}
MAX_ATTENTION_SOURCES = 16      # ESTD_MAX_ATTENTION_SOURCES (include/estd_hip.h)

# bench.py sets this to a list to collect (group, amount, start_event, end_event) around every launch of the hot-path
# kernels on the stream they are launched on: amount = algorithmic FLOPs (groups "conv3d:<Cin>-><Cout>[+x]") or
# algorithmic bytes (SURVEY §8d figures; groups "homo_warp_costvol", "warp_attention", "gru_elementwise", "softargmin").
PROFILE = None


class _Prof:
    """HIP-event pair around one launch (events are recorded on torch's CURRENT stream = the launch stream).  ``amount``: a number, or
    a function that gives it once the launch has returned (it may read shapes the operator has checked by then)."""
    __slots__ = ("group", "amount", "e0")

    def __init__(self, group, amount):
        self.group, self.amount, self.e0 = group, amount, None

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if self.e0 is not None and PROFILE is not None and exc[0] is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(torch.cuda.current_stream())
            PROFILE.append((self.group, float(self.amount() if callable(self.amount) else self.amount), self.e0, e1))
        return False

# Arithmetic of the plain 32->32 3x3x3 convolutions: "f32" = v_mfma_f32_16x16x4_f32 (csrc/conv3d_mfma.hip),
# "bf16x3" = exact 3-way bf16 operand split, six bf16 MFMAs per product block (csrc/conv3d_split_bf16.hip).
CONV3D_ARITH = os.environ.get("ESTD_CONV3D_ARITH", "f32")
CONV2D_ARITH = os.environ.get("ESTD_CONV2D_ARITH", "f32")     # same choice for the 3x3 / dilation-1 NHWC convolutions
# Algorithm of the plain 32->32 3x3x3 convolutions under CONV3D_ARITH == "f32" (every product an fp32 MFMA either way):
# "wino2" = depth AND row axis in Winograd F(2,3) form for the plain 32 -> 32 instance, 0.444 of the products
# (csrc/conv3d_wino2.hip, every 3x3x3 instance of the step); "wino" = depth axis only, 2/3 of the products
# (csrc/conv3d_wino.hip); "direct" = 27 taps (csrc/conv3d_mfma.hip)
CONV3D_ALGO = os.environ.get("ESTD_CONV3D_ALGO", "wino2")
# A/B: "0" sends the 33 -> 33 convolution (dres2) to the depth-only Winograd kernel as in round 3
W2_XOUT = os.environ.get("ESTD_W2_XOUT", "1") != "0"
# the plain 32 -> 32 instances of the two-axis Winograd kernel on the operand-reuse form (csrc/conv3d_wino2x.hip: one wave per SIMD,
# 32x32x2 MFMAs, transforms in front of the LDS); opt-in ("1"): at parity with the 8-wave kernel of csrc/conv3d_wino2.hip, not faster (profiles/r5_wino2x_table.txt)
W2X = os.environ.get("ESTD_W2X", "0") != "0"
# the 32 -> 32 instances without a scalar channel (BN / activation / residuals / running sum / GroupNorm partials) with ALL THREE axes in Winograd form
# (csrc/conv3d_wino3.hip: F(2x2x2, 3x3x3), 8/27 of the direct products; default since round 5: 0.65 vs 0.81 ms for 3 volumes, Joint step 16.9 -> 15.8 ms; "0": two-axis kernel)
W3 = os.environ.get("ESTD_W3", "1") != "0"
# the key || value convolution (33 -> 32) on the three-axis kernel's scalar-channel instance as well (0.73 vs 0.85 ms for 3 volumes; "0": two-axis kernel)
W3_EXTRA = os.environ.get("ESTD_W3_EXTRA", "1") != "0"
# dres2 (33 -> 33): the 32 main output channels on the three-axis kernel's scalar-channel instance + output channel 32 as a pass of its own
# (csrc/conv3d_xout.hip: taps as matrix rows) instead of the two-axis kernel's 33 -> 33 instance ("0")
W3_XOUT = os.environ.get("ESTD_W3_XOUT", "1") != "0"
# same choice for the 3x3 / dilation-1 NHWC convolutions: row axis in Winograd F(2,3) form (csrc/conv2d_wino.hip) or direct
CONV2D_ALGO = os.environ.get("ESTD_CONV2D_ALGO", "wino2")
CONV2D_NT = os.environ.get("ESTD_CONV2D_NT", "auto")
C2W2_DIL2 = os.environ.get("ESTD_C2W2_DIL2", "1") == "1"      # A/B switch: dilation-2 convolutions on the F(2x2,3x3) kernel too (0: row-only kernel)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name, dtype=torch.float32, op=None, dev=None, contiguous=True):
    """``t`` is a contiguous ``dtype`` tensor on a device (``dev``: on that one) -> t; ``op``: the operator's name, put in front of the
    message (the helpers of the argument checks pass it).  csrc/torch_ops.cpp: fptr()."""
    if op is not None:
        name = "%s: %s" % (op, name)
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s must be a tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on a ROCm device (estdepth_amd has no CPU path); got %s" % (name, t.device))
    if dev is not None and t.device != dev:
        raise RuntimeError("%s is on %s but the operator runs on %s" % (name, t.device, dev))
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if contiguous and not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _need(ok, msg):
    """the ctypes front end's argument checks (the torch binding's TORCH_CHECKs): raise before anything is launched"""
    if not ok:
        raise RuntimeError(msg)


def set_reserved_cus(n):
    """Compute units the persistent convolution grids leave free for a concurrent collective (include/estd_hip.h)."""
    if _use_torch():
        return int(T().set_reserved_cus(int(n)))
    return int(N.lib().estd_set_reserved_cus(int(n)))


def get_reserved_cus():
    return int(N.lib().estd_get_reserved_cus())


def profile_mark(idx):
    if _use_torch():
        return T().profile_mark(int(idx))
    N.check(N.lib().estd_profile_mark(int(idx), _stream()), "estd_profile_mark")


# ---------------------------------------------------------------------------------- argument checks
# One helper per kind of check for the ctypes front ends of every operator but the convolution plans' (csrc/torch_ops.cpp has the same
# set for the torch binding, and each operator calls them in the same order there); each takes the operator's and the argument's name
# for its message.
def _volume(volume, op, any_x=False):
    """the volume argument: two float32 planes (D, weight), contiguous, on a device, X % 4 == 0 (``any_x``: the mesh kernels move one
    voxel per lane and take any X) -> (Z, Y, X, address of the weight plane)"""
    _need(isinstance(volume, torch.Tensor) and volume.dim() == 4 and volume.shape[0] == 2, "%s: volume must be [2,Z,Y,X] (D plane, weight plane)" % op)
    _chk(volume, "volume", op=op)
    Z, Y, X = volume.shape[1:]
    _need(any_x or X % 4 == 0, "%s: X must be a multiple of 4, got %d" % (op, X))
    return Z, Y, X, volume.data_ptr() + 4 * Z * Y * X


def _color_planes(color, volume, op):
    _need(isinstance(color, torch.Tensor) and color.dim() == 4 and color.shape[0] == 3 and tuple(color.shape[1:]) == tuple(volume.shape[1:]),
          "%s: color must be [3,Z,Y,X] with the volume's Z, Y, X" % op)
    _chk(color, "color", op=op)
    _need(color.device == volume.device, "%s: color is on %s but the volume on %s" % (op, color.device, volume.device))


def _host_values(t, n, op, name, shape, finite=False):
    """host values of the launch arguments: exactly ``n`` of them (``finite``: none NaN or infinite) -> the values as a list"""
    _need(isinstance(t, torch.Tensor) and not t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n,
          "%s: %s must be a contiguous CPU float32 tensor %s" % (op, name, shape))
    flat = t.reshape(-1).tolist()
    _need(not finite or all(math.isfinite(v) for v in flat), "%s: %s holds a value that is not finite" % (op, name))
    return flat


def _map(t, tail, op, name, dev=None):
    """``t`` is a float32 device map whose last sizes are ``tail`` (-1: any size), leading 1s allowed, on ``dev`` -> its last sizes"""
    _chk(t, name, op=op, dev=dev)
    got = tuple(t.shape[-len(tail):])
    _need(t.dim() >= len(tail) and all(w < 0 or w == g for w, g in zip(tail, got)) and t.numel() == math.prod(got),
          "%s: %s must end in the sizes %s (-1: any; leading 1s allowed), got %s" % (op, name, tail, tuple(t.shape)))
    return got


def _map_size(H, W, op, name, least=1):
    _need(H >= least and W >= least and H * W <= 0x7fffffff, "%s: %s must be at least %d x %d (and H * W < 2^31), got %d x %d" % (op, name, least, least, H, W))


def _floats(t, n, op, name, dev=None, at_least=False, strided=False):
    """``t`` is a float32 tensor on ``dev`` that holds exactly (``at_least``: at least) ``n`` floats, whatever its shape; ``strided``: the
    base of wider records, which need not be contiguous -> t"""
    _chk(t, name, op=op, dev=dev, contiguous=not strided)
    _need(t.numel() >= n if at_least else t.numel() == n,
          "%s: %s must hold %s %d floats, got %d" % (op, name, "at least" if at_least else "exactly", n, t.numel()))
    return t


def _records(t, op, name):
    """``t`` is a float32 device tensor of whole 32-float records (voxels) and nothing else -> their number"""
    n_vox = t.numel() // 32 if isinstance(t, torch.Tensor) else 0
    _floats(t, n_vox * 32, op, name)
    return n_vox


def _opt_floats(t, n, op, name, dev):
    """an optional vector (a per-channel scale, shift or bias; a second pose): None, or exactly ``n`` floats -> t"""
    return None if t is None else _floats(t, n, op, name, dev)


def _like(ts, first, op, name, dev):
    """a list of float32 tensors on ``dev``, each of ``first``'s shape -> their addresses"""
    for i, t in enumerate(ts):
        _chk(t, "%s[%d]" % (name, i), op=op, dev=dev)
        _need(t.shape == first.shape, "%s: %s[%d] has another shape than the first tensor: %s for %s" % (op, name, i, tuple(t.shape), tuple(first.shape)))
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _channels_last(t, op, name, dev=None, like=None):
    """bn_act_nhwc_'s tensors: float32 [N,C,H,W] in channels_last memory on ``dev`` (``like``: and of that tensor's shape) -> (N, C, H, W)"""
    _chk(t, name, op=op, dev=dev, contiguous=False)
    _need(t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last),
          "%s: %s must be [N,C,H,W] in channels_last memory, got %s with the strides %s" % (op, name, tuple(t.shape), t.stride()))
    _need(like is None or t.shape == like.shape, "%s: %s must have the shape %s, got %s" % (op, name, like is not None and tuple(like.shape), tuple(t.shape)))
    return tuple(t.shape)


def _count(v, lo, hi, op, name):
    """a count (tensors of a list, a window, a stride the front end divides by) within lo..hi"""
    _need(lo <= v <= hi, "%s: %s: at least %d and at most %d expected, got %r" % (op, name, lo, hi, v))


def _ivec(t, op, name, dev, size=None, dtype=torch.int64):
    _need(isinstance(t, torch.Tensor) and t.dim() == 1 and t.dtype == dtype and t.is_contiguous() and t.device == dev
          and (size is None or t.shape[0] == size),
          "%s: %s must be a contiguous %s vector%s on the operator's device" % (op, name, dtype, "" if size is None else " [%d]" % size))


# the four rules for a scalar that a kernel takes as fp32
def _positive(v, op, name):
    _need(math.isfinite(v) and ctypes.c_float(v).value > 0, "%s: %s must be positive and finite, got %r" % (op, name, v))


def _not_negative(v, op, name):
    _need(math.isfinite(v) and v >= 0, "%s: %s must be finite and not negative, got %r" % (op, name, v))


def _not_nan(v, op, name):
    _need(v == v, "%s: %s must not be NaN" % (op, name))


def _positive_square(v, op, name, square_positive=False):
    """positive and finite, and its square finite in fp32 (``square_positive``: and not rounded to 0)"""
    v32 = ctypes.c_float(v).value if math.isfinite(v) else float("nan")
    sq = ctypes.c_float(v32 * v32).value
    _need(v32 > 0 and math.isfinite(sq) and (sq > 0 or not square_positive),
          "%s: %s (and its square in fp32) must be positive and finite, got %r" % (op, name, v))


def _launch(dev, entry, *args):
    """Every entry point takes the stream last: one launch of ``entry`` (a function of N.lib()) on the current stream of ``dev``, the
    operator's device (not of whatever device is current), its status translated."""
    with torch.cuda.device(dev):
        N.check(entry(*args, _stream()), entry.__name__)


# ---------------------------------------------------------------------------------- camera algebra
def cam_pair_proj(src_proj, ref_proj):
    """rot|trans of src_proj @ inverse(ref_proj) for one batch element -> [12]."""
    if _use_torch():
        return T().cam_pair_proj(src_proj, ref_proj)
    op = "cam_pair_proj"
    dev = _floats(src_proj, 16, op, "src_proj").device
    _floats(ref_proj, 16, op, "ref_proj", dev)
    out = torch.empty(12, device=dev)
    _launch(dev, N.lib().estd_cam_pair_proj, _p(src_proj), _p(ref_proj), _p(out))
    return out


def cam_sweep_proj(ref_pose, src_pose, intr):
    if _use_torch():
        return T().cam_sweep_proj(ref_pose, src_pose, intr)
    op = "cam_sweep_proj"
    dev = _floats(ref_pose, 16, op, "ref_pose").device
    _floats(src_pose, 16, op, "src_pose", dev)
    _floats(intr, 9, op, "intr", dev)
    out = torch.empty(12, device=dev)
    _launch(dev, N.lib().estd_cam_sweep_proj, _p(ref_pose), _p(src_pose), _p(intr), _p(out))
    return out


def cam_volume_mats(pose_j, pose_i, intr, out=None):
    op = "cam_volume_mats"
    if out is None:
        out = torch.empty(30, device=_chk(pose_j, "pose_j", op=op).device)
    if _use_torch():
        T().cam_volume_mats(pose_j, pose_i, intr, out)
        return out
    dev = _floats(pose_j, 16, op, "pose_j").device
    _opt_floats(pose_i, 16, op, "pose_i", dev)
    _floats(intr, 9, op, "intr", dev)
    _floats(out, 30, op, "out", dev)
    _launch(dev, N.lib().estd_cam_volume_mats, _p(pose_j), _p(pose_i), _p(intr), _p(out))
    return out


# ---------------------------------------------------------------------------------- plane sweep
def _homo_warp(op, entry, src_chw, proj12, depth, per_pixel, D):
    """homo_warping_chw (``depth``: at least D plane depths) and homo_warping_px_chw (``per_pixel``: ``depth`` is [D,H,W], which gives D)
    under the ctypes binding"""
    C, H, W = _map(src_chw, (-1, -1, -1), op, "src_chw")
    dev = src_chw.device
    _floats(proj12, 12, op, "proj12", dev)
    if per_pixel:
        D = _map(depth, (-1, H, W), op, "depth_dhw", dev)[0]
    else:
        _floats(depth, D, op, "depth_values", dev, at_least=True)
    out = torch.empty((C, D, H, W), device=dev)
    _launch(dev, entry, _p(src_chw), _p(proj12), _p(depth), _p(out), C, D, H, W)
    return out


def homo_warping_chw(src_chw, proj12, depth_values, D):
    if _use_torch():
        return T().homo_warping(src_chw, proj12, depth_values, D)
    return _homo_warp("homo_warping", N.lib().estd_homo_warping, src_chw, proj12, depth_values, False, D)


def homo_warping_px_chw(src_chw, proj12, depth_dhw):
    """per-pixel depth hypotheses [D,H,W] (homo_utils.py:462)."""
    if _use_torch():
        return T().homo_warping_px(src_chw, proj12, depth_dhw)
    return _homo_warp("homo_warping_px", N.lib().estd_homo_warping_px, src_chw, proj12, depth_dhw, True, 0)


def mix1x1(in_chw, w, bias):
    """[Cin,H,W] -> [H,W,Cout] channel mix."""
    if _use_torch():
        return T().mix1x1(in_chw, w, bias)
    op = "mix1x1"
    Cin, H, W = _map(in_chw, (-1, -1, -1), op, "in_chw")
    dev = in_chw.device
    Cout = _map(w, (-1, Cin), op, "w", dev)[0]
    _opt_floats(bias, Cout, op, "bias", dev)
    out = torch.empty((H, W, Cout), device=dev)
    _launch(dev, N.lib().estd_mix1x1_chw_to_hwc, _p(in_chw), _p(w), _p(bias), _p(out), Cin, Cout, H * W)
    return out


def homo_warp_costvol(src_mix, ref_mix, proj12, depth_values, D, out=None):
    op = "homo_warp_costvol"
    if out is None:
        H, W, _ = _map(src_mix, (-1, -1, 32), op, "src_mix")
        out = torch.empty((D, H, W, 32), device=src_mix.device)
    with _Prof(op, lambda: 4.0 * src_mix.numel() * (2 + D)):          # src map + ref map + one volume
        if _use_torch():
            T().homo_warp_costvol(src_mix, ref_mix, proj12, depth_values, D, out)
            return out
        H, W, _ = _map(src_mix, (-1, -1, 32), op, "src_mix")
        dev = src_mix.device
        _map(ref_mix, (H, W, 32), op, "ref_mix", dev)
        _floats(proj12, 12, op, "proj12", dev)
        _floats(depth_values, D, op, "depth_values", dev, at_least=True)
        _floats(out, D * H * W * 32, op, "out", dev)
        _launch(dev, N.lib().estd_homo_warp_costvol, _p(src_mix), _p(ref_mix), _p(proj12), _p(depth_values), _p(out), D, H, W)
    return out


# ---------------------------------------------------------------------------------- conv3d
# One kernel launch of a route: the C entry point, the torch operator's ``variant``, {descriptor weight field: plan weight form} (a form the
# plan's shape does not define arrives as NULL), the descriptor fields that differ from the call's, and the number of output channels its
# ops.PROFILE group counts (None: the plan's).
_Launch = collections.namedtuple("_Launch", "entry variant weights overrides n_out", defaults=({}, None))

# route name (Conv3dPlan.route) -> its launches, in order
CONV3D_ROUTES = {
    "direct": (_Launch("estd_conv3d_k3", 0, dict(w_main="w_main", w_extra="w_extra", w_xout="w_xout")),),
    # (the operand-split kernel reads the direct form's scalar-channel / 33rd-output weights)
    "split": (_Launch("estd_conv3d_k3_split", 1, dict(w_main="w_main", w_extra="w_extra", w_xout="w_xout", w_split="w_split")),),
    "wino": (_Launch("estd_conv3d_k3_wino", 2, dict(w_wino="w_wino", w_extra="w_wino_extra", w_xout="w_wino_xout")),),
    "wino2": (_Launch("estd_conv3d_k3_wino2", 3, dict(w_wino2="w_wino2", w_extra="w_wino2_extra")),),
    "wino2_xout": (_Launch("estd_conv3d_k3_wino2", 3, dict(w_wino2="w_wino2", w_extra="w_wino2_extra", w_xout="w_wino2_xout")),),
    "wino2_o16": (_Launch("estd_conv3d_k3_wino2", 3, dict(w_wino2="w_wino2_o16")),),
    "wino2_c16": (_Launch("estd_conv3d_k3_wino2", 3, dict(w_wino2="w_wino2_c16")),),
    "wino2x": (_Launch("estd_conv3d_k3_wino2x", 4, dict(w_wino2="w_wino2x")),),
    "wino3": (_Launch("estd_conv3d_k3_wino3", 5, dict(w_wino2="w_wino3", w_extra="w_wino3_extra")),),
    # the 33 -> 33 instance as two launches: 33 -> 32 (the main output channels) + 33 -> 1 (csrc/conv3d_xout.hip); two profile groups,
    # the launches belong to two kernel families of the replay trace.  (The second kernel reads w_xout only; w_extra is there because the
    # torch operator refuses a scalar input channel without extra-channel weights.)
    "wino3+xout": (_Launch("estd_conv3d_k3_wino3", 5, dict(w_wino2="w_wino3", w_extra="w_wino3_extra"),
                           dict(n_tiles=2, out_channels=32, out_extra=None), n_out=32),
                   _Launch("estd_conv3d_k3_xout", 6, dict(w_extra="w_wino3_extra", w_xout="w_xout_taps"),
                           dict(n_tiles=3, out_main=None), n_out=1)),
}
# route name (Conv2dPlan.route) -> its launch; {nt}: the work-item width the route function returns next to the name
CONV2D_ROUTES = {
    "k3": (_Launch("estd_conv2d_k3", 0, dict(w="w_nt{nt}")),),
    "k3_split": (_Launch("estd_conv2d_k3_split", 1, dict(w="w_nt{nt}", w_split="w_split")),),       # (validates d.w as well)
    "wino": (_Launch("estd_conv2d_k3_wino", 2, dict(w_wino="w_wino_nt{nt}")),),
    "wino2": (_Launch("estd_conv2d_k3_wino2", 3, dict(w_wino="w_wino2")),),
}
# the descriptor field the torch operators fill from their ``w_alt`` argument, by variant (csrc/torch_ops.cpp)
_CONV3D_ALT = (None, "w_split", "w_wino", "w_wino2", "w_wino2", "w_wino2", "w_xout")
_CONV2D_ALT = (None, "w_split", "w_wino", "w_wino")


def _conv3d_torch_args(f, variant):
    alt = _CONV3D_ALT[variant]
    return (f["in_main"], f["in_extra"], f["w_main"], f["w_extra"], None if alt == "w_xout" else f["w_xout"], f[alt] if alt else None,
            f["scale"], f["shift"], (f["N"], f["D"], f["H"], f["W"]), f["cin_main"], f["in_stride"], f["n_tiles"], f["act_a"], f["act_b"],
            f["act_split"], f["out_main"], f["out_stride"], f["out_channels"], f["residual"], f["residual2"], f["out_scale"],
            bool(f["accumulate"]), f["out_extra"], f["head_w"], f["head_b"], f["out_head"], f["stats_partials"], variant,
            f["gate_r"], f["gate_stats"], f["gate_gamma"], f["gate_beta"])


def _conv2d_torch_args(f, variant):
    alt = _CONV2D_ALT[variant]
    return (f["in_"], f["w"], f[alt] if alt else None, f["scale"], f["shift"], f["cout"], f["dilation"], f["group_tiles"],
            bool(f["relu_before_residual"]), bool(f["relu_after_residual"]), f["residual"], variant)


_CONV_BINDINGS = {"conv3d_k3": (_conv3d_torch_args, N.Conv3dDesc), "conv2d_k3": (_conv2d_torch_args, N.Conv2dDesc)}


def _launch_conv(op, launch, fields, weights):
    """One launch of a route under the current binding: ``fields`` are the descriptor's fields (tensors where it holds a pointer),
    ``weights`` the launch's {descriptor field: packed tensor or None}.  The torch operator ``op`` takes them as positional arguments
    (its result is returned), the C entry point as the descriptor."""
    torch_args, desc = _CONV_BINDINGS[op]
    f = dict(fields, **launch.overrides)
    f.update(weights)
    if _use_torch():
        return getattr(T(), op)(*torch_args(f, launch.variant))
    d = desc()
    for k, v in f.items():
        if v is not None:                             # (a fresh descriptor is all zeros / NULL)
            setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    N.check(getattr(N.lib(), launch.entry)(ctypes.byref(d), _stream()), launch.entry)


def _need_ab(has_ab, switches):
    """``switches``: (set?, what) of the switches that select a superseded A/B kernel (raises as _native.require_ab does, from the plan's own fact)"""
    for on, what in switches:
        if on and not has_ab:
            raise RuntimeError("%s needs the A/B kernels: rebuild the library with ESTD_BUILD_AB=1 (python -m estdepth_amd.build)" % what)


class _Packs:
    """Weight forms of a plan, packed and uploaded on first use (``define`` registers how, ``has`` says whether the plan's shape admits the
    form, ``get`` packs once).  Shared by the copies ``with_shift_scaled`` makes."""

    def __init__(self, device):
        self.device, self._fns, self._vals = device, {}, {}

    def define(self, name, fn):
        self._fns[name] = fn

    def has(self, name):
        return name in self._fns

    def get(self, name):
        if name not in self._vals:
            fn = self._fns.get(name)
            self._vals[name] = fn().to(self.device) if fn is not None else None
        return self._vals[name]

    def packed(self):
        """names of the forms that have been packed so far"""
        return sorted(k for k, v in self._vals.items() if v is not None)


class Conv3dPlan:
    """Packed weights + epilogue constants of one 3x3x3 convolution, resident on a device."""

    def __getattr__(self, name):                     # self.w_<form>: packed on first use (None when the plan's shape has no such form)
        if name.startswith("w_") and "_packs" in self.__dict__:
            return self._packs.get(name)
        raise AttributeError(name)

    def __init__(self, weight, main_idx, extra_idx, out_idx, n_tiles, scale, shift, act_a="none", act_b=None,
                 act_split=0, head_w=None, head_b=None, device="cuda"):
        self.cin_main = len(main_idx)
        self.n_tiles = n_tiles
        self.n_out = len(out_idx)
        self.has_extra = extra_idx is not None
        weight = weight.detach()
        # Weight forms are packed ON FIRST USE (``self.w_<form>``, ``_Packs``): a plan carries only what the kernels it is actually run on
        # read -- under the default switches one Winograd form per plan, the direct kernel's ``w_main`` only where a launch falls back to it.
        # (Every launch of a captured forward has run eagerly first: GraphedForward warms up before it captures.)
        P = self._packs = _Packs(device)
        P.define("w_main", lambda: packing.pack_conv3d(weight, main_idx, extra_idx, out_idx, n_tiles)[0])
        if extra_idx is not None:
            P.define("w_extra", lambda: packing.pack_conv3d(weight, main_idx, extra_idx, out_idx, n_tiles)[1])
        if n_tiles == 3:
            P.define("w_xout", lambda: packing.pack_xout(weight, main_idx, extra_idx, out_idx[32]))
        splittable = len(main_idx) == 32 and head_w is None and \
            (n_tiles == 2 or (n_tiles == 3 and extra_idx is not None) or (n_tiles == 1 and extra_idx is None))
        # the superseded A/B kernels (bf16 operand split, depth-only Winograd, operand-reuse wino2x): only in a library built with ESTD_BUILD_AB=1
        ab = self.has_ab = N.has_ab()
        if splittable and ab:
            P.define("w_split", lambda: packing.pack_conv3d_split(weight, main_idx, out_idx, extra_idx, n_tiles))
        wino_ok = len(main_idx) == 32 and head_w is None and \
            ((n_tiles == 2 and len(out_idx) == 32) or (n_tiles == 3 and len(out_idx) == 33 and extra_idx is not None))
        self.wino_ok = wino_ok
        if wino_ok and ab:
            P.define("w_wino", lambda: packing.pack_conv3d_wino(weight, main_idx, out_idx[:32]))
            if extra_idx is not None:
                P.define("w_wino_extra", lambda: packing.pack_conv3d_wino_extra(weight, extra_idx, out_idx[:32]))
            if n_tiles == 3:
                P.define("w_wino_xout", lambda: packing.pack_conv3d_wino_xout(weight, main_idx, extra_idx, out_idx[32]))
            if n_tiles == 2 and extra_idx is None:
                P.define("w_wino2x", lambda: packing.pack_conv3d_wino2x(weight, main_idx, out_idx[:32]))
        if wino_ok:
            P.define("w_wino2", lambda: packing.pack_conv3d_wino2(weight, main_idx, out_idx[:32]))
            if n_tiles == 2 or (n_tiles == 3 and extra_idx is not None):
                P.define("w_wino3", lambda: packing.pack_conv3d_wino3(weight, main_idx, out_idx[:32]))
                if extra_idx is not None:
                    P.define("w_wino3_extra", lambda: packing.pack_conv3d_wino3_extra(weight, extra_idx, out_idx[:32]))
            if n_tiles == 3 and extra_idx is not None:      # ... + output channel 32 as a pass of its own (csrc/conv3d_xout.hip)
                P.define("w_xout_taps", lambda: packing.pack_conv3d_xout_taps(weight, main_idx, extra_idx, out_idx[32]))
            if extra_idx is not None:
                P.define("w_wino2_extra", lambda: packing.pack_conv3d_wino2_extra(weight, extra_idx, out_idx[:32]))
            if n_tiles == 3:       # 33 -> 33 (dres2): the 33rd output channel of the wino2 kernel's XOUT instance
                P.define("w_wino2_xout", lambda: packing.pack_conv3d_wino2_xout(weight, main_idx, extra_idx, out_idx[32]))
        # 32 -> 16 (the GRU output convolution): the wino2 kernel's 16-output-channel instance
        if len(main_idx) == 32 and n_tiles == 1 and len(out_idx) == 16 and extra_idx is None and head_w is None:
            P.define("w_wino2_o16", lambda: packing.pack_conv3d_wino2(weight, main_idx, out_idx[:16]))
        # 16 -> 16 + 1x1x1 head (the stereo heads): csrc/conv3d_wino2_c16.hip
        if len(main_idx) == 16 and n_tiles == 1 and len(out_idx) == 16 and extra_idx is None and head_w is not None:
            P.define("w_wino2_c16", lambda: packing.pack_conv3d_wino2_c16(weight, main_idx, out_idx[:16]))
        self.scale = scale.float().contiguous().to(device)
        self.shift = shift.float().contiguous().to(device)
        self.act_a = ACT[act_a]
        self.act_b = ACT[act_b if act_b is not None else act_a]
        self.act_split = act_split if act_b is not None else 0
        self.head_w = head_w.float().contiguous().to(device) if head_w is not None else None
        self.head_b = head_b.float().contiguous().to(device) if head_b is not None else None

    def with_shift_scaled(self, k):
        """same packed weights, BN shift multiplied by k: sum of k conv+BN results of a LINEAR layer computed as ONE
        convolution of the summed inputs (conv is linear, the shift is counted k times)."""
        import copy
        other = copy.copy(self)
        other.shift = (self.shift * float(k)).contiguous()
        return other

    def route(self, out=True, in_extra=False, out_extra=False, out_head=False, residual=False, residual2=False, stats_partials=False,
              gate=False, out_channels=None, accumulate=False, out_scale=1.0):
        """The route (a key of CONV3D_ROUTES) ``run`` takes for a call under the current module switches.  The first eight arguments say
        whether the call passes that tensor; ``out_channels`` / ``accumulate`` / ``out_scale`` are ``run``'s.  Pure (nothing is packed or
        loaded, a plan on any device answers); RuntimeError for a call or a switch setting ``run`` refuses."""
        _need(in_extra == self.has_extra, "conv3d plan/extra-channel mismatch")
        if CONV3D_ARITH not in ("f32", "bf16x3"):
            raise RuntimeError("ESTD_CONV3D_ARITH must be f32 or bf16x3, got %r" % (CONV3D_ARITH,))
        if CONV3D_ALGO not in ("wino2", "wino", "direct"):
            raise RuntimeError("ESTD_CONV3D_ALGO must be wino2, wino or direct, got %r" % (CONV3D_ALGO,))
        _need_ab(self.has_ab, ((CONV3D_ARITH == "bf16x3", "ESTD_CONV3D_ARITH=bf16x3 (csrc/conv3d_split_bf16.hip)"),
                               (CONV3D_ALGO == "wino", "ESTD_CONV3D_ALGO=wino (csrc/conv3d_wino.hip)"), (W2X, "ESTD_W2X=1 (csrc/conv3d_wino2x.hip)")))
        has, nt, stats = self._packs.has, self.n_tiles, stats_partials
        if out_channels is None:
            out_channels = 16 * min(nt, 2)
        tanh = ACT["tanh"] in ((self.act_a if self.act_split > 0 else self.act_b), self.act_b)
        plain_epi = not (residual or residual2 or accumulate) and float(out_scale) == 1.0      # no read-back stream
        # instances of the split kernel (csrc/conv3d_split_bf16.hip dispatch): plain [+stats], extra input [tanh|relu], 33 -> 33
        split_inst = (not tanh and not stats) if nt == 3 else (not tanh and not in_extra) if nt == 1 else (not stats) if in_extra else not tanh
        wino2_algo = CONV3D_ALGO == "wino2"
        # the 32 -> 32 / 33 -> 32 / 33 -> 33 shapes of the Winograd kernels ...
        wino_shape = CONV3D_ALGO in ("wino", "wino2") and self.wino_ok and out and out_extra == (nt == 3) and not out_head \
            and out_channels == 32 and not (stats and in_extra)
        # ... on the two-axis kernel (its 33 -> 33 instance has no read-back streams / statistics: dres2 needs none) or one that builds on it
        two_axis = wino_shape and wino2_algo and has("w_wino2") and (nt == 2 or (W2_XOUT and plain_epi and not stats))
        routes = (                                        # the first route whose condition holds
            ("split", CONV3D_ARITH == "bf16x3" and has("w_split") and out and split_inst),
            # the stereo heads: only the head's logit volume leaves the kernel, no tanh
            ("wino2_c16", wino2_algo and has("w_wino2_c16") and not out and out_head and not in_extra and not out_extra and plain_epi
             and not stats and not tanh),
            ("wino2_o16", wino2_algo and has("w_wino2_o16") and out and not out_head and not in_extra and not out_extra and out_channels == 16),
            # 33 -> 33 (dres2): 32 outputs on the three-axis kernel's 33 -> 32 instance, then output channel 32 alone (that pass has no
            # tanh: the two-axis kernel's 33 -> 33 instance does)
            ("wino3+xout", two_axis and nt == 3 and W3 and W3_EXTRA and W3_XOUT and has("w_wino3") and has("w_wino3_extra")
             and has("w_xout_taps") and not tanh),
            # GroupNorm partials only without read-back streams; the scalar-channel instance has neither
            ("wino3", two_axis and nt == 2 and W3 and has("w_wino3") and (plain_epi or not stats)
             and (not in_extra or (W3_EXTRA and has("w_wino3_extra") and plain_epi and not stats))),
            # 32 -> 32 without a scalar channel and without tanh: the operand-reuse kernel (GroupNorm partials only without read-back streams)
            ("wino2x", two_axis and nt == 2 and W2X and has("w_wino2x") and not in_extra and not tanh and (plain_epi or not stats)),
            ("wino2_xout", two_axis and nt == 3),
            ("wino2", two_axis),
            # the depth-only kernel: ESTD_CONV3D_ALGO=wino, or dres2 with ESTD_W2_XOUT=0 -- where the library carries it
            ("wino", wino_shape and has("w_wino")),
            ("direct", True))
        name = next(r for r, ok in routes if ok)
        _need(not gate or name == "wino2_o16", "the reset gate is folded into the 32 -> 16 instance of the two-axis Winograd kernel only")
        return name

    def run(self, x, dims, in_stride=None, in_extra=None, out=None, out_stride=None, out_channels=None,
            residual=None, residual2=None, out_scale=1.0, accumulate=False, out_extra=None, out_head=None, stats_partials=None, gate=None):
        """x: channels-last volume(s) [N,D,H,W,in_stride] (or a base view of it); dims = (N,D,H,W).
        ``gate`` = (ru [N,D,H,W,32], statistics [4], gamma [16], beta [16]): the ConvGRU's reset gate applied to input channels 16..31 in the
        convolution's own loads (32 -> 16 instance of the two-axis Winograd kernel only; include/estd_hip.h ``gate_r``)."""
        Nn, D, H, W = dims
        out_channels = out_channels if out_channels is not None else 16 * min(self.n_tiles, 2)
        name = self.route(out is not None, in_extra is not None, out_extra is not None, out_head is not None, residual is not None,
                          residual2 is not None, stats_partials is not None, gate is not None, out_channels, accumulate, out_scale)
        g_r, g_st, g_ga, g_be = gate if gate is not None else (None, None, None, None)
        fields = dict(
            N=Nn, D=D, H=H, W=W, cin_main=self.cin_main, in_stride=in_stride if in_stride is not None else self.cin_main, n_tiles=self.n_tiles,
            in_main=x, in_extra=in_extra, w_main=None, w_extra=None, w_xout=None, scale=self.scale, shift=self.shift,
            act_a=self.act_a, act_b=self.act_b, act_split=self.act_split,
            out_main=out, out_stride=out_stride if out_stride is not None else 16 * min(self.n_tiles, 2), out_channels=out_channels,
            residual=residual, residual2=residual2, out_scale=float(out_scale), accumulate=int(bool(accumulate)), out_extra=out_extra,
            head_w=self.head_w if out_head is not None else None, head_b=self.head_b if out_head is not None else None, out_head=out_head,
            stats_partials=stats_partials, w_split=None, w_wino=None, w_wino2=None, gate_r=g_r, gate_stats=g_st, gate_gamma=g_ga, gate_beta=g_be)
        # (the route's weight forms, packed on first use, before the first launch)
        launches = [(la, {fld: self._packs.get(form) for fld, form in la.weights.items()}) for la in CONV3D_ROUTES[name]]
        cin = self.cin_main + (1 if self.has_extra else 0)
        for la, weights in launches:
            n_out = la.n_out if la.n_out is not None else self.n_out
            with _Prof("conv3d:%d->%d" % (cin, n_out), 2.0 * 27 * cin * n_out * Nn * D * H * W):
                _launch_conv("conv3d_k3", la, fields, weights)


class Conv2dPlan:
    """3x3 Conv2d (stride 1, dilation 1|2) + folded BatchNorm2d [+ReLU] [+residual] on NHWC tensors
    (csrc/conv2d_mfma.hip).  ``conv`` / ``bn`` are the torch modules holding the parameters."""

    def __init__(self, conv, bn, relu_before=False, relu_after=False):
        if conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.groups != 1 or conv.bias is not None:
            raise RuntimeError("Conv2dPlan: 3x3 / stride 1 / bias-free convolutions only")
        if conv.dilation not in ((1, 1), (2, 2)) or conv.padding != conv.dilation:
            raise RuntimeError("Conv2dPlan: dilation 1 or 2 with padding = dilation only")
        if conv.in_channels % 32 or conv.out_channels % 32:
            raise RuntimeError("Conv2dPlan: channel counts must be multiples of 32")
        dev = conv.weight.device
        self.cin, self.cout, self.dil = conv.in_channels, conv.out_channels, conv.dilation[0]
        # output channels per work item: 64 (NT = 4: the input brick feeds twice the MFMAs) unless that leaves the 512 resident
        # workgroups badly balanced (e.g. 64 -> 64 on 5 x 120x160: 750 items = 1.46 rounds, 87 TFLOP/s; NT = 2: 1500 items, 103)
        # weight forms packed on first use (see Conv3dPlan): the default path reads w_wino2 only
        w = conv.weight.detach()
        P = self._packs = _Packs(dev)
        self.nts = (2, 4) if self.cout % 64 == 0 else (2,)
        for nt in self.nts:
            P.define("w_nt%d" % nt, lambda nt=nt: packing.pack_conv2d(w, nt))
        self.has_ab = N.has_ab()
        if self.has_ab:      # row-only Winograd / bf16 operand split: only in a library built with ESTD_BUILD_AB=1
            P.define("w_split", lambda: packing.pack_conv2d_split(w))
            for nt in self.nts:
                P.define("w_wino_nt%d" % nt, lambda nt=nt: packing.pack_conv2d_wino(w, nt))
        P.define("w_wino2", lambda: packing.pack_conv2d_wino2(w))      # F(2x2, 3x3): csrc/conv2d_wino2.hip (dilation 1 and 2)
        sc, sh = packing.fold_bn_fp32(bn, list(range(self.cout)))
        self.scale, self.shift = sc.to(dev), sh.to(dev)
        self.relu_before, self.relu_after = int(relu_before), int(relu_after)

    def __getattr__(self, name):                     # self.w_<form>: packed on first use (None when the plan has no such form)
        if name.startswith("w_") and "_packs" in self.__dict__:
            return self._packs.get(name)
        raise AttributeError(name)

    def _pick_nt(self, n, h, w):
        if 4 not in self.nts:
            return 2
        if CONV2D_NT in ("2", "4"):               # A/B switch (ESTD_CONV2D_NT): force the work-item width
            return int(CONV2D_NT)
        tiles = n * ((h + 7) // 8) * ((w + 15) // 16)
        def balance(items):                       # fraction of the persistent grid's rounds that does useful work
            return items / (512.0 * ((items + 511) // 512))
        return 2 if 0.93 * balance(tiles * (self.cout // 32)) > balance(tiles * (self.cout // 64)) else 4

    def route(self, n, h, w):
        """-> (a key of CONV2D_ROUTES, the work-item width nt) for an [n, h, w, cin] input under the current module switches.  Pure, like
        Conv3dPlan.route; RuntimeError for a switch setting ``run`` refuses."""
        if CONV2D_ARITH not in ("f32", "bf16x3"):
            raise RuntimeError("ESTD_CONV2D_ARITH must be f32 or bf16x3, got %r" % (CONV2D_ARITH,))
        if CONV2D_ALGO not in ("wino2", "wino", "direct"):
            raise RuntimeError("ESTD_CONV2D_ALGO must be wino2, wino or direct, got %r" % (CONV2D_ALGO,))
        _need_ab(self.has_ab, ((CONV2D_ARITH == "bf16x3", "ESTD_CONV2D_ARITH=bf16x3 (csrc/conv2d_split_bf16.hip)"),
                               (CONV2D_ALGO == "wino", "ESTD_CONV2D_ALGO=wino (csrc/conv2d_wino.hip)")))
        has = self._packs.has
        split = CONV2D_ARITH == "bf16x3" and has("w_split")
        nt = self._pick_nt(n, h, w)
        if self.dil == 2 and not split and CONV2D_ALGO in ("wino", "wino2"):
            nt = 2        # the 64-channel work item of the dilated Winograd kernel spills registers into its MFMA loop (5x slower)
        routes = (                                        # the first route whose condition holds
            ("k3_split", split),
            ("wino2", CONV2D_ALGO == "wino2" and (self.dil == 1 or C2W2_DIL2)),
            ("wino", CONV2D_ALGO in ("wino", "wino2") and has("w_wino_nt%d" % nt)),      # (where the library carries it)
            ("k3", True))
        return next(r for r, ok in routes if ok), nt

    def run(self, x_nhwc, residual=None):
        """x_nhwc [N,H,W,Cin] contiguous -> [N,H,W,Cout]."""
        Nn, H, W, C = x_nhwc.shape
        if C != self.cin or not x_nhwc.is_contiguous():
            raise RuntimeError("Conv2dPlan.run: expected contiguous NHWC input with %d channels" % self.cin)
        if residual is not None and (tuple(residual.shape) != (Nn, H, W, self.cout) or not residual.is_contiguous()):
            raise RuntimeError("Conv2dPlan.run: residual must be contiguous NHWC of the output shape")
        name, nt = self.route(Nn, H, W)
        la, = CONV2D_ROUTES[name]
        weights = {fld: self._packs.get(form.format(nt=nt)) for fld, form in la.weights.items()}
        out = None         # (the torch operator allocates its own)
        if not _use_torch():
            _chk(x_nhwc, "conv2d input")
            out = torch.empty((Nn, H, W, self.cout), device=x_nhwc.device, dtype=torch.float32)
        fields = dict(N=Nn, H=H, W=W, cin=self.cin, cout=self.cout, dilation=self.dil, group_tiles=nt, in_=x_nhwc, w=None,
                      scale=self.scale, shift=self.shift, relu_before_residual=self.relu_before, relu_after_residual=self.relu_after,
                      residual=residual, out=out, w_split=None, w_wino=None)
        res = _launch_conv("conv2d_k3", la, fields, weights)
        return res if _use_torch() else out


def conv3d_grid(Nn, D, H, W):
    g = N.lib().estd_conv3d_k3_grid(Nn, D, H, W)
    if g < 0:
        N.check(g, "estd_conv3d_k3_grid")
    return g


def groupnorm_finalize(partials, n_blocks, count, eps=1e-5):
    if _use_torch():
        return T().groupnorm_finalize(partials, n_blocks, float(count), float(eps))
    _need(_chk(partials, "partials", torch.float64, op="groupnorm_finalize").numel() >= n_blocks * 4,
          "groupnorm_finalize: partials must be a contiguous float64 ROCm tensor with 4 doubles per block")
    out = torch.empty(4, device=partials.device, dtype=torch.float32)
    _launch(partials.device, N.lib().estd_groupnorm_finalize, _p(partials), n_blocks, float(count), float(eps), _p(out))
    return out


# ---------------------------------------------------------------------------------- soft-argmin
def softargmin_up(logits, depth_values, scale=4):
    """logits [N,D,H,W] -> (depth, prob) each [N,1,scale*H,scale*W]."""
    op = "softargmin_up"
    with _Prof("softargmin", lambda: 4.0 * (logits.numel() // logits.shape[-3]) * (logits.shape[-3] + 2 * scale * scale)):   # logits in, depth + prob maps out
        if _use_torch():
            return T().softargmin_up(logits, depth_values, scale)
        Nn, D, H, W = _map(logits, (-1, -1, -1, -1), op, "logits")
        dev = logits.device
        _floats(depth_values, D, op, "depth_values", dev, at_least=True)
        depth = torch.empty((Nn, 1, H * scale, W * scale), device=dev)
        prob = torch.empty_like(depth)
        _launch(dev, N.lib().estd_softargmin_up, _p(logits), _p(depth_values), _p(depth), _p(prob), Nn, D, H, W, scale)
    return depth, prob


# ---------------------------------------------------------------------------------- EST fusion
def _warp_vol(op, entry, vol, mats30, depth, depth_per_voxel, *scalars):
    """warp_volume_cdhw and warp_volume_ex_cdhw under the ctypes binding; ``scalars``: the entry point's own arguments between the depths
    and the output"""
    C, D, H, W = _map(vol, (-1, -1, -1, -1), op, "vol")
    dev = vol.device
    _floats(mats30, 30, op, "mats30", dev)
    _floats(depth, D * H * W if depth_per_voxel else D, op, "depth", dev, at_least=True)
    out = torch.empty_like(vol)
    _launch(dev, entry, _p(vol), _p(mats30), _p(depth), *scalars, _p(out), C, D, H, W)
    return out


def warp_volume_cdhw(vol, mats30, depth_values, depth_min, depth_interval):
    if _use_torch():
        return T().warp_volume(vol, mats30, depth_values, float(depth_min), float(depth_interval))
    return _warp_vol("warp_volume", N.lib().estd_warp_volume, vol, mats30, depth_values, False, float(depth_min), float(depth_interval))


def warp_volume_ex_cdhw(vol, mats30, depth, depth_per_voxel, depth_min, depth_interval, disp_min=None, disp_interval=None,
                        border=False, padding_value=0.0):
    """every branch of the reference's warp_volume() signature (include/estd_hip.h::estd_warp_volume_ex)."""
    use_disp = disp_min is not None
    # values are passed through as given: a zero interval reaches the native check (ESTD_ERR_ARG / RuntimeError) instead of being
    # replaced silently -- the reference divides by it (homo_utils.py:187-190).  Placeholders only when disparity planes are off.
    dmin_ = float(disp_min) if use_disp else 0.0
    dint_ = float(disp_interval) if (use_disp and disp_interval is not None) else (0.0 if use_disp else 1.0)
    if _use_torch():
        return T().warp_volume_ex(vol, mats30, depth, bool(depth_per_voxel), float(depth_min), float(depth_interval), use_disp,
                                  dmin_, dint_, bool(border), float(padding_value))
    o = N.WarpVolumeOpts(int(bool(depth_per_voxel)), int(use_disp), int(bool(border)), float(depth_min), float(depth_interval),
                         dmin_, dint_, float(padding_value))
    return _warp_vol("warp_volume_ex", N.lib().estd_warp_volume_ex, vol, mats30, depth, depth_per_voxel, ctypes.byref(o))


def warp_attention(kv_target, kv_sources, mats, depth_values, depth_min, depth_interval):
    """kv_target [D,H,W,32]; kv_sources list of the same; mats [n,30] -> xh [D,H,W,32] = [V_t | h]."""
    op = "warp_attention"
    kv_sources = list(kv_sources)
    with _Prof(op, lambda: 4.0 * 16 * (kv_target.numel() // 32) * (2 + 2 * len(kv_sources))):   # K_t, h out, K_j and V_j of every source
        if _use_torch():
            return T().warp_attention(kv_target, kv_sources, mats, depth_values, float(depth_min), float(depth_interval))
        D, H, W, _ = _map(kv_target, (-1, -1, -1, 32), op, "kv_target")
        dev, n = kv_target.device, len(kv_sources)
        _count(n, 1, MAX_ATTENTION_SOURCES, op, "kv_sources")
        srcs = _like(kv_sources, kv_target, op, "kv_sources", dev)
        _floats(mats, n * 30, op, "mats", dev)
        _floats(depth_values, D, op, "depth_values", dev, at_least=True)
        xh = torch.empty_like(kv_target)
        _launch(dev, N.lib().estd_warp_attention, _p(kv_target), srcs, _p(mats), n, _p(depth_values), float(depth_min), float(depth_interval),
                _p(xh), D, H, W)
    return xh


def attention_prewarped(kv_target, kv_sources):
    kv_sources = list(kv_sources)
    if _use_torch():
        return T().attention_prewarped(kv_target, kv_sources)
    op = "attention_prewarped"
    n_vox = _records(kv_target, op, "kv_target")
    dev, n = kv_target.device, len(kv_sources)
    _count(n, 1, MAX_ATTENTION_SOURCES, op, "kv_sources")
    srcs = _like(kv_sources, kv_target, op, "kv_sources", dev)
    xh = torch.empty_like(kv_target)
    _launch(dev, N.lib().estd_attention_prewarped, _p(kv_target), srcs, n, _p(xh), n_vox)
    return xh


def gru_reset_apply(xh, ru, stats4, gamma_r, beta_r):
    op = "gru_reset_apply"
    with _Prof("gru_elementwise", lambda: 4.0 * 16 * (xh.numel() // 32) * 2):       # SURVEY §8d K11+K13 = 5 x 16 channels per voxel: r, h here
        if _use_torch():
            return T().gru_reset_apply(xh, ru, stats4, gamma_r, beta_r)
        n_vox = _records(xh, op, "xh")
        dev = xh.device
        _floats(ru, n_vox * 32, op, "ru", dev)
        _floats(stats4, 4, op, "stats4", dev)
        _floats(gamma_r, 16, op, "gamma_r", dev)
        _floats(beta_r, 16, op, "beta_r", dev)
        xrh = torch.empty_like(xh)
        _launch(dev, N.lib().estd_gru_reset_apply, _p(xh), _p(ru), _p(stats4), _p(gamma_r), _p(beta_r), _p(xrh), n_vox)
    return xrh


def gru_blend(xh, ru, o_raw, stats_ru, stats_o, gamma_u, beta_u, gamma_o, beta_o, out_value, out_stride):
    op = "gru_blend"
    with _Prof("gru_elementwise", lambda: 4.0 * 16 * (xh.numel() // 32) * 3):       # ... u, o_raw, out here (h counted once, in the reset pass)
        if _use_torch():
            return T().gru_blend(xh, ru, o_raw, stats_ru, stats_o, gamma_u, beta_u, gamma_o, beta_o, out_value, out_stride)
        n_vox = _records(xh, op, "xh")
        dev = xh.device
        _floats(ru, n_vox * 32, op, "ru", dev)
        _floats(o_raw, n_vox * 16, op, "o_raw", dev)
        for name, t in (("stats_ru", stats_ru), ("stats_o", stats_o)):
            _floats(t, 4, op, name, dev)
        for name, t in (("gamma_u", gamma_u), ("beta_u", beta_u), ("gamma_o", gamma_o), ("beta_o", beta_o)):
            _floats(t, 16, op, name, dev)
        _floats(out_value, (n_vox - 1) * out_stride + 16, op, "out_value", dev, at_least=True, strided=True)
        _launch(dev, N.lib().estd_gru_blend, _p(xh), _p(ru), _p(o_raw), _p(stats_ru), _p(stats_o), _p(gamma_u), _p(beta_u), _p(gamma_o), _p(beta_o),
                _p(out_value), out_stride, n_vox)


# ---------------------------------------------------------------------------------- 2D backbone epilogues
def bn_act_nhwc_(x, scale, shift, relu, residual=None):
    """in place on an NCHW-shaped tensor in channels_last memory: x = act(x*scale[c] + shift[c] (+ residual))."""
    if _use_torch():
        return T().bn_act_nhwc_(x, scale, shift, bool(relu), residual)
    op = "bn_act_nhwc_"
    n, c, h, w = _channels_last(x, op, "x")
    dev = x.device
    _floats(scale, c, op, "scale", dev)
    _floats(shift, c, op, "shift", dev)
    if residual is not None:
        _channels_last(residual, op, "residual", dev, like=x)
    _launch(dev, N.lib().estd_bn_act_nhwc, _p(x), _p(scale), _p(shift), _p(residual), 1 if relu else 0, n * h * w, c)
    return x


def spp_upsample_cat(raw, skip, branches):
    """NHWC tensors: raw [N,H,W,Cr], skip [N,H,W,Cs], branches [N,hk,wk,Cb] -> [N,H,W,Cr+Cs+nb*Cb] =
    cat(raw, skip, bilinear_up(branches...)) in one pass (psm_submodule.py:100-116)."""
    branches = list(branches)
    if _use_torch():
        return T().spp_upsample_cat(raw, skip, branches)
    op = "spp_upsample_cat"
    n, h, w, cr = _map(raw, (-1, -1, -1, -1), op, "raw")
    dev, nb = raw.device, len(branches)
    cs = _map(skip, (n, h, w, -1), op, "skip", dev)[3]
    _count(nb, 1, 4, op, "branches")
    bh, bw, cb = [], [], -1                                   # the first branch's channel count is every branch's
    for k, b in enumerate(branches):
        _, hk, wk, cb = _map(b, (n, -1, -1, cb), op, "branches[%d]" % k, dev)
        bh.append(hk)
        bw.append(wk)
    out = torch.empty((n, h, w, cr + cs + nb * cb), device=dev)
    _launch(dev, N.lib().estd_spp_upsample_cat, _p(raw), cr, _p(skip), cs, (ctypes.c_void_p * nb)(*[b.data_ptr() for b in branches]),
            (ctypes.c_int * nb)(*bh), (ctypes.c_int * nb)(*bw), nb, cb, _p(out), n, h, w)
    return out


def _desc_conv(op, entry, d, x, w, w_tail, ho, wo, scale, shift, relu, residual):
    """conv1x1_nhwc and conv2d_taps_nhwc under the ctypes binding: ``d`` arrives with the operator's own fields (stride; ksize, pad) set,
    ``w_tail`` are the weight's sizes around cout ([cout,cin] / [k*k,cout,cin]), ho x wo the output map."""
    n, h, wd, cin = x.shape[-4:]
    dev = x.device
    cout = _map(w, w_tail, op, "w", dev)[-2]
    d.N, d.H, d.W, d.cin, d.cout, d.relu = n, h, wd, cin, cout, int(bool(relu))
    d.in_, d.w = x.data_ptr(), w.data_ptr()
    d.scale, d.shift = _p(_opt_floats(scale, cout, op, "scale", dev)), _p(_opt_floats(shift, cout, op, "shift", dev))
    if residual is not None:
        _map(residual, (n, ho, wo, cout), op, "residual", dev)
        d.residual = residual.data_ptr()
    out = torch.empty((n, ho, wo, cout), device=dev)
    d.out = out.data_ptr()
    _launch(dev, entry, ctypes.byref(d))
    return out


def conv1x1_nhwc(x, w2, scale, shift, stride=1, relu=False, residual=None):
    """1x1 convolution (stride 1|2) + folded BN [+ residual] [+ ReLU] of an NHWC map in one launch (csrc/conv1x1.hip).
    x [N,H,W,cin]; w2 [cout,cin] (the Conv2d weight as it lies); scale / shift [cout] or None -> NHWC [N,Ho,Wo,cout]."""
    if _use_torch():
        return T().conv1x1_nhwc(x, w2, scale, shift, int(stride), bool(relu), residual)
    op = "conv1x1_nhwc"
    n, h, w, c = _map(x, (-1, -1, -1, -1), op, "x")
    _count(stride, 1, 2, op, "stride")
    d = N.Conv1x1Desc()
    d.stride = int(stride)
    return _desc_conv(op, N.lib().estd_conv1x1_nhwc, d, x, w2, (-1, c), (h - 1) // stride + 1, (w - 1) // stride + 1, scale, shift, relu, residual)


def conv2d_taps_nhwc(x, w_taps, scale, shift, ksize, stride=1, pad=None, relu=False, residual=None):
    """k x k convolution (k = 1|3|5, stride 1|2, zero padding) + folded BN [+ residual] [+ ReLU] of an NHWC map in one launch
    (csrc/conv2d_taps.hip).  x [N,H,W,cin]; w_taps [k*k,cout,cin] (packing.pack_conv2d_taps) -> NHWC [N,Ho,Wo,cout]."""
    pad = ksize // 2 if pad is None else pad
    if _use_torch():
        return T().conv2d_taps_nhwc(x, w_taps, scale, shift, int(ksize), int(stride), int(pad), bool(relu), residual)
    op = "conv2d_taps_nhwc"
    n, h, w, c = _map(x, (-1, -1, -1, -1), op, "x")
    _count(stride, 1, 2, op, "stride")
    d = N.Conv2dTapsDesc()
    d.ksize, d.stride, d.pad = int(ksize), int(stride), int(pad)
    return _desc_conv(op, N.lib().estd_conv2d_taps_nhwc, d, x, w_taps, (ksize * ksize, -1, c), (h + 2 * pad - ksize) // stride + 1,
                      (w + 2 * pad - ksize) // stride + 1, scale, shift, relu, residual)


def _packed_conv(op, entry, x, w, scale, shift, out_shape, *sizes):
    """the four "NHWC in, packed weights, scale / shift [cout], NHWC out" convolutions under the ctypes binding: x and the weights ``w``
    have been checked, ``sizes`` are the entry point's own arguments after the five pointers"""
    dev = x.device
    _floats(scale, out_shape[3], op, "scale", dev)
    _floats(shift, out_shape[3], op, "shift", dev)
    out = torch.empty(out_shape, device=dev)
    _launch(dev, entry, _p(x), _p(w), _p(scale), _p(shift), _p(out), *sizes)
    return out


def stem7x7s2_nhwc(x, w_packed, scale, shift):
    """Conv2d(3, 64, 7, stride 2, padding 3) + folded BatchNorm2d + ReLU on an NHWC image batch [N,H,W,3] -> [N,Ho,Wo,64]
    (torchvision ResNet conv1 / bn1 / relu, hybrid_models/resnet_encoder.py:42-44); w_packed: packing.pack_stem7x7."""
    if _use_torch():
        return T().stem7x7s2_nhwc(x, w_packed, scale, shift)
    op = "stem7x7s2_nhwc"
    n, h, w, _ = _map(x, (-1, -1, -1, 3), op, "x")
    _floats(w_packed, 7 * 6 * 4 * 64, op, "w_packed", x.device)
    return _packed_conv(op, N.lib().estd_stem7x7s2_nhwc, x, w_packed, scale, shift, (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64), n, h, w)


def stem3x3s2_nhwc(x, weight, scale, shift):
    """Conv2d(3, 32, 3, stride 2, padding 1) + folded BatchNorm2d + ReLU on an NHWC image batch [N,H,W,3] -> [N,Ho,Wo,32]
    (networks/psm_submodule.py:47)."""
    if _use_torch():
        return T().stem3x3s2_nhwc(x, weight, scale, shift)
    op = "stem3x3s2_nhwc"
    n, h, w, _ = _map(x, (-1, -1, -1, 3), op, "x")
    _map(weight, (32, 3, 3, 3), op, "weight", x.device)
    return _packed_conv(op, N.lib().estd_stem3x3s2_nhwc, x, weight, scale, shift, (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 32), n, h, w)


SMALL_CONV_SHAPES = {(32, 3, 2), (32, 1, 2), (32, 1, 1), (64, 1, 1), (128, 1, 1)}      # (cin, ksize, stride) instances of estd_conv2d_small_nhwc


def conv2d_small_nhwc(x, w_packed, scale, shift, cout, ksize, stride, relu):
    """small PSM convolutions (3x3 stride 2, 1x1 stride 1|2) + folded BN [+ ReLU] on an NHWC map -> NHWC [N,Ho,Wo,cout]."""
    if _use_torch():
        return T().conv2d_small_nhwc(x, w_packed, scale, shift, int(cout), int(ksize), int(stride), bool(relu))
    op = "conv2d_small_nhwc"
    n, h, w, c = _map(x, (-1, -1, -1, -1), op, "x")
    # (the weight count below divides by these)
    _need(ksize in (1, 3) and stride in (1, 2) and cout > 0 and cout % 16 == 0 and c % 16 == 0,
          "conv2d_small_nhwc: ksize 1|3, stride 1|2, the channel counts of x and cout multiples of 16")
    _floats(w_packed, cout // 16 * ksize * ksize * (c // 16) * 256, op, "w_packed", x.device)
    pad = ksize // 2
    return _packed_conv(op, N.lib().estd_conv2d_small_nhwc, x, w_packed, scale, shift,
                        (n, (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1, cout),
                        n, h, w, c, int(cout), int(ksize), int(stride), int(bool(relu)))


def conv2d_k3_to16_nhwc(x, w_packed, scale, shift, upsample=False):
    """3x3 conv (cin 16|32 -> 16) + folded BN + ReLU on an NHWC map, optionally on its nearest-x2 upsampling (never materialised)."""
    if _use_torch():
        return T().conv2d_k3_to16_nhwc(x, w_packed, scale, shift, bool(upsample))
    op = "conv2d_k3_to16_nhwc"
    n, h, w, c = _map(x, (-1, -1, -1, -1), op, "x")
    _need(c in (16, 32), "conv2d_k3_to16_nhwc: x must have 16 or 32 channels, got %d" % c)      # (the weight count depends on it)
    _floats(w_packed, 9 * (c // 16) * 256, op, "w_packed", x.device)
    u = 2 if upsample else 1
    return _packed_conv(op, N.lib().estd_conv2d_k3_to16_nhwc, x, w_packed, scale, shift, (n, u * h, u * w, 16), n, u * h, u * w, c, int(bool(upsample)))


def maxpool3x3s2_nhwc(x):
    """MaxPool2d(3, 2, 1) of an NHWC map [N,H,W,C] (C % 4 == 0) -> [N,(H-1)//2+1,(W-1)//2+1,C]."""
    if _use_torch():
        return T().maxpool3x3s2_nhwc(x)
    n, h, w, c = _map(x, (-1, -1, -1, -1), "maxpool3x3s2_nhwc", "x")
    out = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), device=x.device)
    _launch(x.device, N.lib().estd_maxpool3x3s2_nhwc, _p(x), _p(out), n, h, w, c)
    return out


def avgpool_nhwc(x, k):
    """AvgPool2d(k, k) of an NHWC map [N,H,W,C] (C % 4 == 0) -> [N,H//k,W//k,C]."""
    if _use_torch():
        return T().avgpool_nhwc(x, int(k))
    n, h, w, c = _map(x, (-1, -1, -1, -1), "avgpool_nhwc", "x")
    _count(k, 1, min(h, w), "avgpool_nhwc", "k")                      # (the output size divides by it)
    out = torch.empty((n, h // k, w // k, c), device=x.device)
    _launch(x.device, N.lib().estd_avgpool_nhwc, _p(x), _p(out), n, h, w, c, int(k))
    return out


def normalise_nhwc(imgs):
    """[N,3,H,W] images in 0..255 -> 2 * (imgs / 255) - 1 as an NHWC batch [N,H,W,3] (model_hybrid.py:119)."""
    if _use_torch():
        return T().normalise_nhwc(imgs)
    n, _, h, w = _map(imgs, (-1, 3, -1, -1), "normalise_nhwc", "imgs")
    out = torch.empty((n, h, w, 3), device=imgs.device)
    _launch(imgs.device, N.lib().estd_normalise_nhwc, _p(imgs), _p(out), n, h * w)
    return out


def nhwc_to_planes(x):
    """NHWC map [N,H,W,C] -> contiguous NCHW planes [N,C,H,W] (hybrid_depth_decoder.py:162-184: the plane scores as scalar volumes)."""
    if _use_torch():
        return T().nhwc_to_planes(x)
    n, h, w, c = _map(x, (-1, -1, -1, -1), "nhwc_to_planes", "x")
    out = torch.empty((n, c, h, w), device=x.device)
    _launch(x.device, N.lib().estd_nhwc_to_planes, _p(x), c, _p(out), n, h * w)
    return out


def planes_cat_nhwc(a, b, relu_b=False):
    """torch.cat([a, relu?(b)], 1) of NCHW stacks -> NHWC map [N,H,W,Ca+Cb] (hybrid_depth_decoder.py:268)."""
    if _use_torch():
        return T().planes_cat_nhwc(a, b, bool(relu_b))
    op = "planes_cat_nhwc"
    n, ca, h, w = _map(a, (-1, -1, -1, -1), op, "a")
    cb = _map(b, (n, -1, h, w), op, "b", a.device)[1]
    out = torch.empty((n, h, w, ca + cb), device=a.device)
    _launch(a.device, N.lib().estd_planes_cat_nhwc, _p(a), ca, _p(b), cb, int(bool(relu_b)), _p(out), n, h * w)
    return out


def upsample2_cat_nhwc(x, skip):
    """torch.cat([nearest_x2(x), skip], 1) on NHWC maps: x [N,H/2,W/2,Cx], skip [N,H,W,Cs] -> [N,H,W,Cx+Cs] (:269-272)."""
    if _use_torch():
        return T().upsample2_cat_nhwc(x, skip)
    op = "upsample2_cat_nhwc"
    n, hx, wx, cx = _map(x, (-1, -1, -1, -1), op, "x")
    h, w = 2 * hx, 2 * wx
    cs = _map(skip, (n, h, w, -1), op, "skip", x.device)[3]
    out = torch.empty((n, h, w, cx + cs), device=x.device)
    _launch(x.device, N.lib().estd_upsample2_cat_nhwc, _p(x), cx, _p(skip), cs, _p(out), n, h, w)
    return out


def disp_head_nhwc(x, weight, bias, depth_max, upscale=1):
    """depth_max * sigmoid(Conv2d(C,1,3,padding=1,bias)(x)) on an NHWC map, optionally nearest x2 -> [N,1,uH,uW] (:274, :279)."""
    if _use_torch():
        return T().disp_head_nhwc(x, weight, bias, float(depth_max), int(upscale))
    op = "disp_head_nhwc"
    n, h, w, c = _map(x, (-1, -1, -1, -1), op, "x")
    _map(weight, (1, c, 3, 3), op, "weight", x.device)
    _floats(bias, 1, op, "bias", x.device)
    out = torch.empty((n, 1, upscale * h, upscale * w), device=x.device)
    _launch(x.device, N.lib().estd_disp_head_nhwc, _p(x), _p(weight), _p(bias), float(depth_max), _p(out), n, h, w, c, int(upscale))
    return out


# ---------------------------------------------------------------------------------- layout converters
def cdhw_to_vol(src, dst, dst_stride, dst_off):
    """src [C,D,H,W] contiguous -> channels dst_off.. of the channels-last records of dst."""
    if _use_torch():
        return T().cdhw_to_vol(src, dst, dst_stride, dst_off)
    op = "cdhw_to_vol"
    _chk(src, "src", op=op)
    _need(src.dim() >= 2 and src.shape[0] >= 1, "%s: src must be [C, ...] with C >= 1, got %s" % (op, tuple(src.shape)))
    C = src.shape[0]
    S = src.numel() // C
    _count(dst_off, 0, dst_stride, op, "dst_off")                      # (estd_cdhw_to_vol checks its upper end only)
    _floats(dst, S * dst_stride, op, "dst", src.device, at_least=True, strided=True)
    _launch(src.device, N.lib().estd_cdhw_to_vol, _p(src), _p(dst), C, S, dst_stride, dst_off)


def vol_to_cdhw(src, C, dims, src_stride, src_off):
    dims = list(dims)
    if _use_torch():
        return T().vol_to_cdhw(src, C, dims, src_stride, src_off)
    op = "vol_to_cdhw"
    _count(len(dims), 3, 3, op, "dims")
    D, H, W = dims
    _count(src_off, 0, src_stride, op, "src_off")                      # (estd_vol_to_cdhw checks its upper end only)
    _floats(src, D * H * W * src_stride, op, "src", at_least=True, strided=True)
    out = torch.empty((C, D, H, W), device=src.device)
    _launch(src.device, N.lib().estd_vol_to_cdhw, _p(src), _p(out), C, D * H * W, src_stride, src_off)
    return out


# ---------------------------------------------------------------------------------- TSDF fusion (csrc/tsdf.hip)
TSDF_MAX_FRAMES = N.TSDF_MAX_FRAMES


def _tsdf_integrate(op, volume, color, depths, confs, images, mats, trunc, z_near, conf_min, weighted, w_max, no_skip):
    """tsdf_integrate_ (``color`` and ``images`` None) and tsdf_integrate_color_ under the ctypes binding"""
    Z, Y, X, weight = _volume(volume, op)
    n = len(depths)
    _need(1 <= n <= TSDF_MAX_FRAMES, "%s: 1..%d frames per call, got %d" % (op, TSDF_MAX_FRAMES, n))
    _need(len(confs) in (0, n), "%s: one confidence map per depth map (or none)" % op)
    _need(not weighted or confs, "%s: weighted fusion needs confidence maps" % op)
    flat = _host_values(mats, n * 12, op, "mats", "[T,12]")
    dev = volume.device
    H, W = _map(depths[0], (-1, -1), op, "depth map 0", dev)
    for name, maps in (("depth map", depths), ("confidence map", confs)):
        for i, t in enumerate(maps):
            _map(t, (H, W), op, "%s %d" % (name, i), dev)
    d = N.TsdfIntegrateDesc() if color is None else N.TsdfIntegrateColorDesc()
    d.Z, d.Y, d.X, d.T, d.H, d.W = Z, Y, X, n, H, W
    d.weighted, d.no_skip = int(bool(weighted)), int(bool(no_skip))
    d.trunc, d.z_near, d.conf_min, d.w_max = float(trunc), float(z_near), float(conf_min), float(w_max)
    d.tsdf, d.weight = volume.data_ptr(), weight
    for t in range(n):
        d.depth[t] = depths[t].data_ptr()
        d.conf[t] = confs[t].data_ptr() if confs else None
        d.mats[t][:] = flat[t * 12:t * 12 + 12]
    launch, what = N.lib().estd_tsdf_integrate, "estd_tsdf_integrate"
    if color is not None:
        _color_planes(color, volume, op)
        _need(len(images) == n, "%s: one image per depth map, got %d for %d" % (op, len(images), n))
        d.color = color.data_ptr()
        for t in range(n):
            _map(images[t], (3, H, W), op, "image %d" % t, dev)
            d.image[t] = images[t].data_ptr()
        launch, what = N.lib().estd_tsdf_integrate_color, "estd_tsdf_integrate_color"
    with torch.cuda.device(dev):
        N.check(launch(ctypes.byref(d), _stream()), what)
    return volume


def tsdf_integrate_(volume, depths, confs, mats, trunc, z_near, conf_min, weighted, w_max, no_skip=False):
    """In place on ``volume`` [2,Z,Y,X] (D plane, weight plane): fuse the depth maps ``depths`` (list of [H,W] device tensors, 1..8) with the
    host matrices ``mats`` (CPU float32 [T,12], camera.tsdf_matrices) in one pass over the voxels; ``confs``: a list of the same length or
    empty.  The contract is spelled out in include/estd_hip.h."""
    depths, confs = list(depths), list(confs) if confs is not None else []
    if _use_torch():
        return T().tsdf_integrate_(volume, depths, confs, mats, float(trunc), float(z_near), float(conf_min), bool(weighted), float(w_max), bool(no_skip))
    return _tsdf_integrate("tsdf_integrate_", volume, None, depths, confs, None, mats, trunc, z_near, conf_min, weighted, w_max, no_skip)


def tsdf_integrate_color_(volume, color, depths, confs, images, mats, trunc, z_near, conf_min, weighted, w_max, no_skip=False):
    """tsdf_integrate_ with colour, in place on ``volume`` [2,Z,Y,X] and ``color`` [3,Z,Y,X]: ``images`` is one [3,H,W] device tensor per depth
    map (the frame the map belongs to, at the map's size).  D and the weight come out as from tsdf_integrate_; the colour planes share the
    weight plane.  The contract is spelled out in include/estd_hip.h (estd_tsdf_integrate_color)."""
    depths, confs, images = list(depths), list(confs) if confs is not None else [], list(images)
    if _use_torch():
        return T().tsdf_integrate_color_(volume, color, depths, confs, images, mats, float(trunc), float(z_near), float(conf_min), bool(weighted),
                                         float(w_max), bool(no_skip))
    _need(color is not None, "tsdf_integrate_color_: color must be a tensor")
    return _tsdf_integrate("tsdf_integrate_color_", volume, color, depths, confs, images, mats, trunc, z_near, conf_min, weighted, w_max, no_skip)


def tsdf_extract_points(volume, voxel_size, origin, w_min, capacity):
    """Zero crossings of ``volume`` [2,Z,Y,X] -> (count [1] int64 on the device: the TOTAL number of crossings, xyz [capacity,3],
    normal [capacity,3], weight [capacity], edge [capacity] int64); ``capacity`` 0 counts only.  ``origin``: CPU float32 [3]."""
    if _use_torch():
        return T().tsdf_extract_points(volume, float(voxel_size), origin, float(w_min), int(capacity))
    Z, Y, X, weight = _volume(volume, "tsdf_extract_points")
    _need(capacity >= 0, "tsdf_extract_points: capacity must not be negative")
    org = (ctypes.c_float * 3)(*_host_values(origin, 3, "tsdf_extract_points", "origin", "[3]"))
    dev = volume.device
    with torch.cuda.device(dev):
        count = torch.zeros(1, device=dev, dtype=torch.int64)
        xyz, normal = torch.empty((capacity, 3), device=dev), torch.empty((capacity, 3), device=dev)
        weight_out, edge = torch.empty(capacity, device=dev), torch.empty(capacity, device=dev, dtype=torch.int64)
        pp = (lambda t: _p(t)) if capacity else (lambda t: None)
        N.check(N.lib().estd_tsdf_extract_points(_p(volume), ctypes.c_void_p(weight), Z, Y, X, float(voxel_size), org, float(w_min), _p(count),
                                                 int(capacity), pp(xyz), pp(normal), pp(weight_out), pp(edge), _stream()),
                "estd_tsdf_extract_points")
    return count, xyz, normal, weight_out, edge


def _tsdf_raycast(op, volume, color, mat, H, W, t_min, dt, n_steps, w_min, stats):
    """tsdf_raycast (``color`` None) and tsdf_raycast_color under the ctypes binding -> (depth, normal, weight, stats or None, colour map or
    None).  n_steps is in 1..2^24, dt must be positive and finite as fp32, t_min finite and not negative, w_min not NaN."""
    Z, Y, X, weight = _volume(volume, op)
    m = _host_values(mat, 12, op, "mat", "[12] (3x4 row-major)")
    _map_size(H, W, op, "the image")
    _need(0 < n_steps <= 1 << 24, "%s: n_steps must be in 1..2^24, got %d" % (op, n_steps))
    _positive(dt, op, "dt")
    _not_negative(t_min, op, "t_min")
    _not_nan(w_min, op, "w_min")
    dev = volume.device
    with torch.cuda.device(dev):
        depth, normal, out_weight = torch.empty((H, W), device=dev), torch.empty((H, W, 3), device=dev), torch.empty((H, W), device=dev)
        st = torch.empty((H, W, 2), device=dev, dtype=torch.int32) if stats else None
        d = N.TsdfRaycastDesc() if color is None else N.TsdfRaycastColorDesc()
        d.Z, d.Y, d.X, d.H, d.W, d.n_steps = Z, Y, X, H, W, n_steps
        d.t_min, d.dt, d.w_min = t_min, dt, w_min
        d.tsdf, d.weight = volume.data_ptr(), weight
        d.depth, d.normal, d.out_weight = depth.data_ptr(), normal.data_ptr(), out_weight.data_ptr()
        d.stats = st.data_ptr() if stats else None
        d.mat[:] = m
        launch, what, rgb = N.lib().estd_tsdf_raycast, "estd_tsdf_raycast", None
        if color is not None:
            _color_planes(color, volume, op)
            rgb = torch.empty((H, W, 3), device=dev)
            d.color, d.out_color = color.data_ptr(), rgb.data_ptr()
            launch, what = N.lib().estd_tsdf_raycast_color, "estd_tsdf_raycast_color"
        N.check(launch(ctypes.byref(d), _stream()), what)
    return depth, normal, out_weight, st, rgb


def tsdf_raycast(volume, mat, H, W, t_min, dt, n_steps, w_min, stats=False):
    """Ray-cast ``volume`` [2,Z,Y,X] with the host matrix ``mat`` (CPU float32 [12], camera.tsdf_ray_matrix): ``n_steps`` samples per pixel at
    z-depths t_min + k dt -> (depth [H,W], normal [H,W,3], weight [H,W]) on the volume's device; zeros where a ray finds no surface.
    ``stats=True`` (measurement only) appends an int32 [H,W,2] tensor: samples whose weights / whose D values were read.  The contract
    is spelled out in include/estd_hip.h (csrc/tsdf_raycast.hip)."""
    H, W, n_steps, t_min, dt, w_min = int(H), int(W), int(n_steps), float(t_min), float(dt), float(w_min)
    if _use_torch():
        out = T().tsdf_raycast(volume, mat, H, W, t_min, dt, n_steps, w_min, bool(stats))
    else:
        out = _tsdf_raycast("tsdf_raycast", volume, None, mat, H, W, t_min, dt, n_steps, w_min, stats)
    return tuple(out[:4 if stats else 3])


def tsdf_edge_colors(volume, color, edge):
    """The colour at the crossings ``edge`` [N] int64 (the ids tsdf_extract_points returns) of ``volume`` [2,Z,Y,X] / ``color`` [3,Z,Y,X]
    -> [N,3] on the device; an id outside the volume gives zeros (include/estd_hip.h, estd_tsdf_edge_colors)."""
    if _use_torch():
        return T().tsdf_edge_colors(volume, color, edge)
    Z, Y, X, _ = _volume(volume, "tsdf_edge_colors")
    _color_planes(color, volume, "tsdf_edge_colors")
    _ivec(edge, "tsdf_edge_colors", "edge", volume.device)
    n = edge.shape[0]
    with torch.cuda.device(volume.device):
        out = torch.empty((n, 3), device=volume.device)
        if n:
            N.check(N.lib().estd_tsdf_edge_colors(_p(volume), _p(color), Z, Y, X, ctypes.c_void_p(edge.data_ptr()), n, _p(out), _stream()),
                    "estd_tsdf_edge_colors")
    return out


def tsdf_raycast_color(volume, color, mat, H, W, t_min, dt, n_steps, w_min):
    """tsdf_raycast with a colour map: -> (depth [H,W], normal [H,W,3], weight [H,W], color [H,W,3]); the first three as from tsdf_raycast,
    the colour blended from ``color`` [3,Z,Y,X] at the hit, zeros without one (include/estd_hip.h, estd_tsdf_raycast_color)."""
    H, W, n_steps, t_min, dt, w_min = int(H), int(W), int(n_steps), float(t_min), float(dt), float(w_min)
    if _use_torch():
        return tuple(T().tsdf_raycast_color(volume, color, mat, H, W, t_min, dt, n_steps, w_min))
    _need(color is not None, "tsdf_raycast_color: color must be a tensor")
    out = _tsdf_raycast("tsdf_raycast_color", volume, color, mat, H, W, t_min, dt, n_steps, w_min, False)
    return out[:3] + out[4:]


# ---------------------------------------------------------------------------------- surface nets (csrc/mesh/tsdf_mesh.hip)
def tsdf_mesh_vertices(volume, color, voxel_size, origin, w_min, capacity):
    """The surface-net vertices of ``volume`` [2,Z,Y,X] (any X), one per active cell -> (count [1] int64 on the device: the TOTAL number,
    cell [capacity] int64, xyz [capacity,3], normal [capacity,3], weight [capacity], color [capacity,3] or None); ``color``: the colour
    planes [3,Z,Y,X] or None; ``capacity`` 0 counts only; records come in no fixed order (sort by ``cell``).  ``origin``: CPU float32
    [3].  The contract is spelled out in include/estd_hip.h (estd_tsdf_mesh_vertices)."""
    capacity = int(capacity)
    if _use_torch():
        out = T().tsdf_mesh_vertices(volume, color, float(voxel_size), origin, float(w_min), capacity)
        return tuple(out[:5]) + (out[5] if color is not None else None,)
    op = "tsdf_mesh_vertices"
    Z, Y, X, weight = _volume(volume, op, any_x=True)
    if color is not None:
        _color_planes(color, volume, op)
    _need(capacity >= 0, "%s: capacity must not be negative" % op)
    _positive(voxel_size, op, "voxel_size")
    _not_nan(w_min, op, "w_min")
    org = (ctypes.c_float * 3)(*_host_values(origin, 3, op, "origin", "[3]", True))
    dev = volume.device
    with torch.cuda.device(dev):
        count = torch.zeros(1, device=dev, dtype=torch.int64)
        cell = torch.empty(capacity, device=dev, dtype=torch.int64)
        xyz, normal, weight_out = torch.empty((capacity, 3), device=dev), torch.empty((capacity, 3), device=dev), torch.empty(capacity, device=dev)
        rgb = torch.empty((capacity, 3), device=dev) if color is not None else None
        pp = (lambda t: _p(t)) if capacity else (lambda t: None)
        N.check(N.lib().estd_tsdf_mesh_vertices(_p(volume), ctypes.c_void_p(weight), _p(color), Z, Y, X, float(voxel_size), org, float(w_min),
                                                _p(count), capacity, pp(cell), pp(xyz), pp(normal), pp(weight_out), pp(rgb), _stream()),
                "estd_tsdf_mesh_vertices")
    return count, cell, xyz, normal, weight_out, rgb


def tsdf_mesh_faces(volume, w_min, capacity):
    """The surface-net quads of ``volume`` [2,Z,Y,X] (any X), one per crossing edge whose four cells exist and are observed -> (count [1]
    int64 on the device: the TOTAL number, edge [capacity] int64 = 3 * voxel + axis, quad [capacity,4] int32: the four cell ids in winding
    order, triangles (0, 1, 2) and (0, 2, 3)); ``capacity`` 0 counts only; no fixed order (sort by ``edge``).  include/estd_hip.h,
    estd_tsdf_mesh_faces."""
    capacity = int(capacity)
    if _use_torch():
        return tuple(T().tsdf_mesh_faces(volume, float(w_min), capacity))
    op = "tsdf_mesh_faces"
    Z, Y, X, weight = _volume(volume, op, any_x=True)
    _need(capacity >= 0, "%s: capacity must not be negative" % op)
    _not_nan(w_min, op, "w_min")
    dev = volume.device
    with torch.cuda.device(dev):
        count = torch.zeros(1, device=dev, dtype=torch.int64)
        edge = torch.empty(capacity, device=dev, dtype=torch.int64)
        quad = torch.empty((capacity, 4), device=dev, dtype=torch.int32)
        pp = (lambda t: _p(t)) if capacity else (lambda t: None)
        N.check(N.lib().estd_tsdf_mesh_faces(_p(volume), ctypes.c_void_p(weight), Z, Y, X, float(w_min), _p(count), capacity, pp(edge), pp(quad),
                                             _stream()), "estd_tsdf_mesh_faces")
    return count, edge, quad


# ---------------------------------------------------------------------------------- mesh components (csrc/mesh/mesh_components.hip)
def _faces(t, op, name):
    """a triangle list: int32 [F,3], contiguous, on a device -> F"""
    _need(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous(),
          "%s: %s must be a contiguous int32 tensor [F,3] on a ROCm device" % (op, name))
    return t.shape[0]


def mesh_components(faces, n_vertices):
    """The connected components of the triangles ``faces`` [F,3] int32 over ``n_vertices`` vertices -> (label [V] int32: the smallest
    vertex index of the vertex's component, triangles [V] int32: at a root the component's triangles, 0 elsewhere, invalid [1] int64 on
    the device: the triangles with an index outside [0, V), which are ignored).  include/estd_hip.h, estd_mesh_components."""
    n_vertices = int(n_vertices)
    if _use_torch():
        return tuple(T().mesh_components(faces, n_vertices))
    op = "mesh_components"
    n_faces = _faces(faces, op, "faces")
    _count(n_vertices, 0, 0x7fffffff, op, "n_vertices")
    dev = faces.device
    with torch.cuda.device(dev):
        label = torch.empty(n_vertices, device=dev, dtype=torch.int32)
        triangles = torch.empty(n_vertices, device=dev, dtype=torch.int32)
        invalid = torch.empty(1, device=dev, dtype=torch.int64)
        pp = (lambda t: _p(t)) if n_vertices else (lambda t: None)
        N.check(N.lib().estd_mesh_components(_p(faces) if n_faces else None, n_faces, n_vertices, pp(label), pp(triangles), _p(invalid), _stream()),
                "estd_mesh_components")
    return label, triangles, invalid


# ---------------------------------------------------------------------------------- mesh sampling (csrc/mesh/mesh_sample.hip)
MESH_SAMPLE_MIN_STRATUM = 1 << 20      # ESTD_MESH_SAMPLE_MIN_STRATUM (include/estd_hip.h)


def _mesh(xyz, faces, op):
    """the vertices float32 [V,3] and the triangles int32 [F,3] of one mesh on one device -> (V, F)"""
    n_faces = _faces(faces, op, "faces")
    _cloud(xyz, op, "xyz")
    _need(xyz.device == faces.device, "%s: xyz is on %s but faces on %s" % (op, xyz.device, faces.device))
    return xyz.shape[0], n_faces


def mesh_sample_scale(n_faces, area_max):
    """The exponent e of the power of two that quantises the areas (include/estd_hip.h, "The glue"): with ``area_max`` = m 2^k,
    0.5 <= m < 1, e = 62 - ceil(log2 n_faces) - k, so that the sum of the n_faces values floor(area 2^e) stays below 2^62.  Needs no
    device.  A largest area that is not finite means a vertex that is not: refused."""
    _need(math.isfinite(area_max) and area_max >= 0, "mesh_sample: xyz holds a coordinate that is not finite (the largest area is %r)" % (area_max,))
    if n_faces <= 0 or area_max == 0:
        return 0
    return min(1000, 62 - (int(n_faces) - 1).bit_length() - math.frexp(area_max)[1])


def mesh_sample_stratum(total, n_samples):
    """The stratum w = total // n_samples of ``n_samples`` > 0 samples over ``total`` units of quantised area; refused without area and
    below 2^20 units.  Needs no device."""
    _need(total > 0, "mesh_sample: the mesh has no area to put n_samples = %d samples on" % n_samples)
    w = int(total) // int(n_samples)
    _need(w >= MESH_SAMPLE_MIN_STRATUM, "mesh_sample: n_samples = %d leaves strata of %d units of area, fewer than %d: too many samples for this mesh"
          % (n_samples, w, MESH_SAMPLE_MIN_STRATUM))
    return w


def mesh_face_area(xyz, faces):
    """Per-triangle areas of the mesh ``xyz`` [V,3] float32 / ``faces`` [F,3] int32 -> (area [F] float64, face_normal [F,3] float32,
    invalid [1] int64 on the device: the triangles with an index outside [0, V), whose area is 0).  include/estd_hip.h,
    estd_mesh_face_area."""
    if _use_torch():
        return tuple(T().mesh_face_area(xyz, faces))
    n_vertices, n_faces = _mesh(xyz, faces, "mesh_face_area")
    dev = faces.device
    with torch.cuda.device(dev):
        area = torch.empty(n_faces, device=dev, dtype=torch.float64)
        normal = torch.empty((n_faces, 3), device=dev)
        invalid = torch.empty(1, device=dev, dtype=torch.int64)
        pp = (lambda t: _p(t)) if n_faces else (lambda t: None)
        N.check(N.lib().estd_mesh_face_area(_p(xyz) if n_vertices else None, n_vertices, pp(faces), n_faces, pp(area), pp(normal), _p(invalid),
                                            _stream()), "estd_mesh_face_area")
    return area, normal, invalid


def mesh_sample(xyz, faces, attrs, n_samples, seed=0):
    """``n_samples`` points spread evenly by area over the mesh ``xyz`` [V,3] float32 / ``faces`` [F,3] int32, with the vertex attributes
    ``attrs`` [V,C] (1 <= C <= 6, or None) interpolated -> (xyz [N,3], face [N] int32, bary [N,2], normal [N,3] (the triangle's), attrs
    [N,C] or None, area [F] float64, invalid [1] int64).  Stratified along the cumulative area, a function of (mesh, n_samples, seed) alone;
    ``seed``: any integer, taken modulo 2^64.  Without faces or with n_samples = 0 the sample arrays are empty.  The contract:
    include/estd_hip.h (estd_mesh_face_area, the glue, estd_mesh_sample)."""
    n_samples, seed = int(n_samples), int(seed) & 0xffffffffffffffff
    if _use_torch():
        out = list(T().mesh_sample(xyz, faces, attrs, n_samples, seed - (1 << 64) if seed >> 63 else seed))
        out[4] = out[4] if attrs is not None else None
        return tuple(out)
    op = "mesh_sample"
    n_vertices, n_faces = _mesh(xyz, faces, op)
    dev = faces.device
    C = 0
    if attrs is not None:
        _chk(attrs, "attrs", op=op, dev=dev)
        _need(attrs.dim() == 2 and attrs.shape[0] == n_vertices and 1 <= attrs.shape[1] <= CLOUD_MAX_ATTRS,
              "%s: attrs must be [%d,C] with 1 <= C <= %d" % (op, n_vertices, CLOUD_MAX_ATTRS))
        C = attrs.shape[1]
    _count(n_samples, 0, 0x7fffffff, op, "n_samples")
    area, face_normal, invalid = mesh_face_area(xyz, faces)
    n = n_samples if n_faces else 0
    w = 0
    if n:
        scale = 2.0 ** mesh_sample_scale(n_faces, float(area.max().item()))
        cum = torch.cumsum(torch.floor(area * scale).to(torch.int64), 0)
        w = mesh_sample_stratum(int(cum[-1].item()), n)
    with torch.cuda.device(dev):
        out_xyz, face, bary = torch.empty((n, 3), device=dev), torch.empty(n, device=dev, dtype=torch.int32), torch.empty((n, 2), device=dev)
        normal = torch.empty((n, 3), device=dev)
        out_attrs = torch.empty((n, C), device=dev) if C else None
        if n:
            N.check(N.lib().estd_mesh_sample(_p(xyz), n_vertices, _p(faces), n_faces, _p(attrs) if C else None, C, _p(cum), _p(face_normal), n, 0, w,
                                             seed, _p(out_xyz), _p(face), _p(bary), _p(normal), _p(out_attrs) if C else None, _stream()),
                    "estd_mesh_sample")
    return out_xyz, face, bary, normal, out_attrs, area, invalid


# ---------------------------------------------------------------------------------- mesh rasteriser (csrc/mesh/mesh_raster.hip)
MESH_RASTER_PRELOAD, MESH_RASTER_CLEAR = 1, 2      # ESTD_MESH_RASTER_PRELOAD, ESTD_MESH_RASTER_CLEAR (include/estd_hip.h)


def _host_doubles(t, n, op, name, shape):
    """host values a kernel takes as float64: exactly ``n`` of them, all finite -> a ctypes array"""
    _need(isinstance(t, torch.Tensor) and not t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n,
          "%s: %s must be a contiguous CPU float64 tensor %s" % (op, name, shape))
    flat = t.reshape(-1).tolist()
    _need(all(math.isfinite(v) for v in flat), "%s: %s holds a value that is not finite" % (op, name))
    return (ctypes.c_double * n)(*flat)


def mesh_raster(xyz, faces, mat, H, W, z_near, preload=False):
    """Rasterise the mesh ``xyz`` [V,3] float32 / ``faces`` [F,3] int32 with the host matrix ``mat`` (CPU float64 [12],
    camera.mesh_raster_matrix) into an ``H`` x ``W`` image -> (depth [H,W] float32: the z-depth of the nearest triangle, 0 = nothing; face
    [H,W] int32: its index, -1 = nothing; bary [H,W,2]: the perspective-correct weights of its second and third vertex; facing [H,W]
    int32: +1 counter-clockwise seen from the camera, -1 clockwise, 0 = nothing; invalid [1] int64 on the device: the triangles with an
    index outside [0, V), which cover nothing).  Defined to the bit: include/estd_hip.h (estd_mesh_raster, estd_mesh_raster_resolve).
    ``preload=True`` puts a load in front of the atomic minimum (faster where thousands of triangles share pixels; the same bits).  The key buffer is
    allocated here and cleared by the first entry point with a memset on the stream (ESTD_MESH_RASTER_CLEAR)."""
    H, W, z_near = int(H), int(W), float(z_near)
    if _use_torch():
        return tuple(T().mesh_raster(xyz, faces, mat, H, W, z_near, bool(preload)))
    op = "mesh_raster"
    n_vertices, n_faces = _mesh(xyz, faces, op)
    m = _host_doubles(mat, 12, op, "mat", "[12] (3x4 row-major)")
    _map_size(H, W, op, "the image")
    _not_negative(z_near, op, "z_near")
    dev = faces.device
    with torch.cuda.device(dev):
        keys = torch.empty((H, W), device=dev, dtype=torch.int64)
        depth, face, bary = torch.empty((H, W), device=dev), torch.empty((H, W), device=dev, dtype=torch.int32), torch.empty((H, W, 2), device=dev)
        facing = torch.empty((H, W), device=dev, dtype=torch.int32)
        invalid = torch.empty(1, device=dev, dtype=torch.int64)
        px, pf = _p(xyz) if n_vertices else None, _p(faces) if n_faces else None
        N.check(N.lib().estd_mesh_raster(px, n_vertices, pf, n_faces, 0, n_faces, m, H, W, z_near, MESH_RASTER_CLEAR | (MESH_RASTER_PRELOAD if preload else 0), _p(keys),
                                         _p(invalid),
                                         _stream()), "estd_mesh_raster")
        N.check(N.lib().estd_mesh_raster_resolve(px, n_vertices, pf, n_faces, m, H, W, _p(keys), _p(depth), _p(face), _p(bary), _p(facing),
                                                 _stream()), "estd_mesh_raster_resolve")
    return depth, face, bary, facing, invalid


# ---------------------------------------------------------------------------------- cross-view consistency (csrc/depth_consistency.hip)
CONSISTENCY_MAX_SOURCES = N.CONSISTENCY_MAX_SOURCES


def depth_consistency(target, sources, mats, px_max, rel_max, z_near):
    """Check the depth map ``target`` [H,W] against the 1..8 ``sources`` (device tensors of the same size) with the host matrices ``mats``
    (CPU float32 [S,2,12]: F_s and B_s of camera.consistency_matrices) -> (views, visible, depth, rel_err), each [H,W] on the target's device:
    the number of sources that agree with a pixel within ``px_max`` pixels of reprojection and ``rel_max`` of relative depth, the number that
    see it, the average of the target's depth and the agreeing sources' and their mean relative difference.  The contract is spelled out in
    include/estd_hip.h (estd_depth_consistency)."""
    sources = list(sources)
    px_max, rel_max, z_near = float(px_max), float(rel_max), float(z_near)
    if _use_torch():
        return tuple(T().depth_consistency(target, sources, mats, px_max, rel_max, z_near))
    op = "depth_consistency"
    H, W = _map(target, (-1, -1), op, "target")
    _map_size(H, W, op, "maps", least=2)
    S = len(sources)
    _need(1 <= S <= CONSISTENCY_MAX_SOURCES, "depth_consistency: 1..%d sources per call, got %d" % (CONSISTENCY_MAX_SOURCES, S))
    flat = _host_values(mats, S * 24, op, "mats", "[S,2,12]", finite=True)
    _positive(px_max, op, "px_max")
    _positive(rel_max, op, "rel_max")
    _not_negative(z_near, op, "z_near")
    dev = target.device
    for i, t in enumerate(sources):
        _map(t, (H, W), op, "source %d" % i, dev)
    with torch.cuda.device(dev):
        views, visible, depth, rel_err = (torch.empty((H, W), device=dev) for _ in range(4))
        d = N.DepthConsistencyDesc()
        d.H, d.W, d.S = H, W, S
        d.px_max, d.rel_max, d.z_near = px_max, rel_max, z_near
        d.target = target.data_ptr()
        d.views, d.visible, d.depth, d.rel_err = views.data_ptr(), visible.data_ptr(), depth.data_ptr(), rel_err.data_ptr()
        for s in range(S):
            d.source[s] = sources[s].data_ptr()
            d.mats[s][0][:], d.mats[s][1][:] = flat[s * 24:s * 24 + 12], flat[s * 24 + 12:s * 24 + 24]
        N.check(N.lib().estd_depth_consistency(ctypes.byref(d), _stream()), "estd_depth_consistency")
    return views, visible, depth, rel_err


# ---------------------------------------------------------------------------------- point clouds (csrc/cloud_nn.hip)
CLOUD_KEY_MAX_DIM = 1 << 20     # ESTD_CLOUD_KEY_MAX_DIM (include/estd_hip.h)
CLOUD_MAX_DIM = 1024            # ESTD_CLOUD_MAX_DIM
CLOUD_MAX_CELLS = 1 << 24       # ESTD_CLOUD_MAX_CELLS
CLOUD_MAX_ATTRS = 6             # ESTD_CLOUD_MAX_ATTRS


def _cloud(t, op, name, cols=3):
    _chk(t, name)
    _need(t.dim() == 2 and t.shape[1] == cols and t.shape[0] <= 0x7fffffff, "%s: %s must be [n,%d] with n < 2^31, got %s" % (op, name, cols, tuple(t.shape)))


def _cloud_grid(lo, cell, dims, op, max_dim):
    lo3 = _host_values(lo, 3, op, "lo", "[3]", finite=True)
    _positive(cell, op, "cell")
    c = ctypes.c_float(cell).value
    _need(math.isfinite(c) and math.isfinite(ctypes.c_float(1.0 / c).value), "%s: cell must be finite in fp32 (and its reciprocal too), got %r" % (op, cell))
    dims = tuple(int(v) for v in dims)
    _need(len(dims) == 3 and all(1 <= v <= max_dim for v in dims), "%s: dims must be three sizes in 1..%d, got %r" % (op, max_dim, dims))
    return lo3, dims


def cloud_cell_keys(points, lo, cell, dims):
    """Grid keys of ``points`` [n,3] -> int64 [n] on the points' device: ``lo`` CPU float32 [3], ``cell`` the cell edge, ``dims`` the cells
    along x, y, z; a point outside the grid gets the clamped cell (include/estd_hip.h, estd_cloud_cell_keys)."""
    cell, dims = float(cell), [int(v) for v in dims]
    if _use_torch():
        return T().cloud_cell_keys(points, lo, cell, dims)
    _cloud(points, "cloud_cell_keys", "points")
    lo3, dims = _cloud_grid(lo, cell, dims, "cloud_cell_keys", CLOUD_KEY_MAX_DIM)
    n = points.shape[0]
    with torch.cuda.device(points.device):
        keys = torch.empty(n, device=points.device, dtype=torch.int64)
        if n:
            N.check(N.lib().estd_cloud_cell_keys(_p(points), n, (ctypes.c_float * 3)(*lo3), cell, (ctypes.c_int * 3)(*dims),
                                                 ctypes.c_void_p(keys.data_ptr()), _stream()), "estd_cloud_cell_keys")
    return keys


def cloud_nearest(query, order, records, cell_start, lo, cell, dims, max_dist, stats=False):
    """Nearest target of every row of ``query`` [M,3] -> (dist [M] float32, index [M] int64[, stats [M] int32]) on the query's device.
    ``records`` [N,4] / ``cell_start`` int32 [cells + 1]: the key-sorted targets and the cell table (cloud_metrics.PointGrid builds them),
    ``order`` int64 [M]: the order the queries are taken in (a permutation, sorted by the queries' keys).  Not found within ``max_dist``:
    dist = max_dist, index = -1.  The contract is spelled out in include/estd_hip.h (estd_cloud_nearest)."""
    cell, max_dist, dims = float(cell), float(max_dist), [int(v) for v in dims]
    if _use_torch():
        dist, index, st = T().cloud_nearest(query, order, records, cell_start, lo, cell, dims, max_dist, bool(stats))
        return (dist, index, st) if stats else (dist, index)
    op = "cloud_nearest"
    _cloud(query, op, "query")
    _cloud(records, op, "records", cols=4)
    M, n, dev = query.shape[0], records.shape[0], query.device
    _ivec(order, op, "order", dev, M)
    _need(records.device == dev, "cloud_nearest: records are on %s but the query on %s" % (records.device, dev))
    _positive_square(max_dist, op, "max_dist")
    lo3, dims = _cloud_grid(lo, cell, dims, op, CLOUD_MAX_DIM)
    cells = dims[0] * dims[1] * dims[2]
    _need(cells <= CLOUD_MAX_CELLS, "cloud_nearest: %d cells, at most %d" % (cells, CLOUD_MAX_CELLS))
    _ivec(cell_start, op, "cell_start (cells + 1)", dev, cells + 1, torch.int32)
    with torch.cuda.device(dev):
        dist, index = torch.empty(M, device=dev), torch.empty(M, device=dev, dtype=torch.int64)
        st = torch.empty(M, device=dev, dtype=torch.int32) if stats else None
        if M:
            d = N.CloudNearestDesc()
            d.M, d.N = M, n
            d.query, d.order, d.records, d.cell_start = query.data_ptr(), order.data_ptr(), records.data_ptr(), cell_start.data_ptr()
            d.dist, d.index = dist.data_ptr(), index.data_ptr()
            d.stats = st.data_ptr() if stats else None
            d.cell, d.max_dist = cell, max_dist
            d.lo[:], d.dims[:] = lo3, dims
            N.check(N.lib().estd_cloud_nearest(ctypes.byref(d), _stream()), "estd_cloud_nearest")
    return (dist, index, st) if stats else (dist, index)


def cloud_cell_centroids(points, attrs, order, segments):
    """Means of the cells of a key-sorted cloud: ``points`` [n,3], ``attrs`` [n,C] (C <= 6) or None, ``order`` int64 [n] (sorted position ->
    original index), ``segments`` int64 [K + 1] -> (points [K,3], attrs [K,C] or None), summed in float64 in the sorted order
    (include/estd_hip.h, estd_cloud_cell_centroids)."""
    if _use_torch():
        _need(isinstance(points, torch.Tensor), "points must be a tensor")
        pts, att = T().cloud_cell_centroids(points, attrs if attrs is not None else points.new_empty((0, 0)), order, segments)      # C = 0: no attributes
        return pts, (att if attrs is not None else None)
    op = "cloud_cell_centroids"
    _cloud(points, op, "points")
    n, dev = points.shape[0], points.device
    C = 0
    if attrs is not None:
        _chk(attrs, "attrs")
        _need(attrs.dim() == 2 and attrs.shape[0] == n and attrs.shape[1] <= CLOUD_MAX_ATTRS and attrs.device == dev,
              "cloud_cell_centroids: attrs must be [n,C] with C <= %d on the points' device, got %s" % (CLOUD_MAX_ATTRS, tuple(attrs.shape)))
        C = attrs.shape[1]
    _ivec(order, op, "order", dev, n)
    _ivec(segments, op, "segments", dev)
    _need(1 <= segments.shape[0] <= n + 1, "cloud_cell_centroids: segments must be [K + 1] with K <= n, got %d for n = %d" % (segments.shape[0], n))
    K = segments.shape[0] - 1
    with torch.cuda.device(dev):
        out = torch.empty((K, 3), device=dev)
        out_attrs = torch.empty((K, C), device=dev) if attrs is not None else None
        if K:
            N.check(N.lib().estd_cloud_cell_centroids(_p(points), _p(attrs) if C else None, C, n, ctypes.c_void_p(order.data_ptr()),
                                                      ctypes.c_void_p(segments.data_ptr()), K, _p(out), _p(out_attrs) if C else None, _stream()),
                    "estd_cloud_cell_centroids")
    return out, out_attrs


# ---------------------------------------------------------------------------------- k nearest neighbours, normals (csrc/cloud/cloud_knn.hip)
CLOUD_KNN_MAX = 32              # ESTD_CLOUD_KNN_MAX (include/estd_hip.h)


def cloud_knn(query, order, records, cell_start, lo, cell, dims, max_dist, k, stats=False):
    """The ``k`` nearest targets of every row of ``query`` [M,3] -> (dist [M,k] float32, index [M,k] int32, count [M] int32[, stats [M]
    int32]) on the query's device, ascending by (d2, index); the slots from ``count`` on hold max_dist and -1.  ``records`` /
    ``cell_start`` / ``order``: as for cloud_nearest.  The contract is spelled out in include/estd_hip.h (estd_cloud_knn)."""
    cell, max_dist, dims, k = float(cell), float(max_dist), [int(v) for v in dims], int(k)
    if _use_torch():
        dist, index, count, st = T().cloud_knn(query, order, records, cell_start, lo, cell, dims, max_dist, k, bool(stats))
        return (dist, index, count, st) if stats else (dist, index, count)
    op = "cloud_knn"
    _cloud(query, op, "query")
    _cloud(records, op, "records", cols=4)
    M, n, dev = query.shape[0], records.shape[0], query.device
    _ivec(order, op, "order", dev, M)
    _need(records.device == dev, "cloud_knn: records are on %s but the query on %s" % (records.device, dev))
    _positive_square(max_dist, op, "max_dist")
    _count(k, 1, CLOUD_KNN_MAX, op, "k")
    lo3, dims = _cloud_grid(lo, cell, dims, op, CLOUD_MAX_DIM)
    cells = dims[0] * dims[1] * dims[2]
    _need(cells <= CLOUD_MAX_CELLS, "cloud_knn: %d cells, at most %d" % (cells, CLOUD_MAX_CELLS))
    _ivec(cell_start, op, "cell_start (cells + 1)", dev, cells + 1, torch.int32)
    with torch.cuda.device(dev):
        dist, index = torch.empty((M, k), device=dev), torch.empty((M, k), device=dev, dtype=torch.int32)
        count = torch.empty(M, device=dev, dtype=torch.int32)
        st = torch.empty(M, device=dev, dtype=torch.int32) if stats else None
        if M:
            d = N.CloudKnnDesc()
            d.M, d.N, d.k = M, n, k
            d.query, d.order, d.records, d.cell_start = query.data_ptr(), order.data_ptr(), records.data_ptr(), cell_start.data_ptr()
            d.dist, d.index, d.count = dist.data_ptr(), index.data_ptr(), count.data_ptr()
            d.stats = st.data_ptr() if stats else None
            d.cell, d.max_dist = cell, max_dist
            d.lo[:], d.dims[:] = lo3, dims
            N.check(N.lib().estd_cloud_knn(ctypes.byref(d), _stream()), "estd_cloud_knn")
    return (dist, index, count, st) if stats else (dist, index, count)


# ---------------------------------------------------------------------------------- clustering (csrc/cloud/cloud_cluster.hip)
def cloud_count_within(query, order, records, cell_start, lo, cell, dims, radius):
    """The number of targets within ``radius`` of every row of ``query`` [M,3] (d2 <= radius^2, inclusive, no cap) -> int32 [M] on the
    query's device.  ``records`` / ``cell_start`` / ``order``: as for cloud_nearest.  include/estd_hip.h, estd_cloud_count_within."""
    cell, radius, dims = float(cell), float(radius), [int(v) for v in dims]
    if _use_torch():
        return T().cloud_count_within(query, order, records, cell_start, lo, cell, dims, radius)
    op = "cloud_count_within"
    _cloud(query, op, "query")
    _cloud(records, op, "records", cols=4)
    M, n, dev = query.shape[0], records.shape[0], query.device
    _ivec(order, op, "order", dev, M)
    _need(records.device == dev, "cloud_count_within: records are on %s but the query on %s" % (records.device, dev))
    _positive_square(radius, op, "radius")
    lo3, dims = _cloud_grid(lo, cell, dims, op, CLOUD_MAX_DIM)
    cells = dims[0] * dims[1] * dims[2]
    _need(cells <= CLOUD_MAX_CELLS, "cloud_count_within: %d cells, at most %d" % (cells, CLOUD_MAX_CELLS))
    _ivec(cell_start, op, "cell_start (cells + 1)", dev, cells + 1, torch.int32)
    with torch.cuda.device(dev):
        count = torch.empty(M, device=dev, dtype=torch.int32)
        if M:
            d = N.CloudCountWithinDesc()
            d.M, d.N = M, n
            d.query, d.order, d.records, d.cell_start = query.data_ptr(), order.data_ptr(), records.data_ptr(), cell_start.data_ptr()
            d.count = count.data_ptr()
            d.cell, d.radius = cell, radius
            d.lo[:], d.dims[:] = lo3, dims
            N.check(N.lib().estd_cloud_count_within(ctypes.byref(d), _stream()), "estd_cloud_count_within")
    return count


def cloud_dbscan(records, cell_start, lo, cell, dims, eps, min_points):
    """DBSCAN of the cloud the key-sorted ``records`` [N,4] hold -> (label int32 [N], count int32 [N], size int32 [N], noise int32 [1]),
    all by ORIGINAL index: the smallest core index of the point's cluster or -1, the neighbours within ``eps`` (the point itself among
    them), the points per label, the points labelled -1.  The contract is spelled out in include/estd_hip.h (estd_cloud_dbscan)."""
    cell, eps, dims, min_points = float(cell), float(eps), [int(v) for v in dims], int(min_points)
    if _use_torch():
        return tuple(T().cloud_dbscan(records, cell_start, lo, cell, dims, eps, min_points))
    op = "cloud_dbscan"
    _cloud(records, op, "records", cols=4)
    n, dev = records.shape[0], records.device
    _positive_square(eps, op, "eps")
    _count(min_points, 1, 0x7fffffff, op, "min_points")
    lo3, dims = _cloud_grid(lo, cell, dims, op, CLOUD_MAX_DIM)
    cells = dims[0] * dims[1] * dims[2]
    _need(cells <= CLOUD_MAX_CELLS, "cloud_dbscan: %d cells, at most %d" % (cells, CLOUD_MAX_CELLS))
    _ivec(cell_start, op, "cell_start (cells + 1)", dev, cells + 1, torch.int32)
    with torch.cuda.device(dev):
        label, count, size, parent = (torch.empty(n, device=dev, dtype=torch.int32) for _ in range(4))
        noise = torch.empty(1, device=dev, dtype=torch.int32) if n else torch.zeros(1, device=dev, dtype=torch.int32)
        if n:
            d = N.CloudDbscanDesc()
            d.N, d.min_points = n, min_points
            d.records, d.cell_start = records.data_ptr(), cell_start.data_ptr()
            d.count, d.parent, d.label, d.size, d.noise = count.data_ptr(), parent.data_ptr(), label.data_ptr(), size.data_ptr(), noise.data_ptr()
            d.cell, d.eps = cell, eps
            d.lo[:], d.dims[:] = lo3, dims
            N.check(N.lib().estd_cloud_dbscan(ctypes.byref(d), _stream()), "estd_cloud_dbscan")
    return label, count, size, noise


def cloud_normals(points, query, index, count, toward=None, cov=False):
    """Normals by a plane fit over the neighbours ``index`` [M,k] int32 / ``count`` [M] int32 (cloud_knn's) of ``query`` [M,3] in the
    cloud ``points`` [N,3] -> (normal [M,3], eig [M,3] ascending, valid [M] uint8, invalid int64 [1], cov float64 [M,6] or None).
    ``toward``: None, or a device tensor [3] or [M,3] the normals are turned to.  The contract: include/estd_hip.h (estd_cloud_normals)."""
    if _use_torch():
        normal, eig, valid, invalid, c = T().cloud_normals(points, query, index, count, toward, bool(cov))
        return normal, eig, valid, invalid, (c if cov else None)
    op = "cloud_normals"
    _cloud(points, op, "points")
    _cloud(query, op, "query")
    n, M, dev = points.shape[0], query.shape[0], points.device
    _need(query.device == dev, "cloud_normals: query is on %s but the points on %s" % (query.device, dev))
    _need(isinstance(index, torch.Tensor) and index.dim() == 2 and index.dtype == torch.int32 and index.is_contiguous() and index.device == dev
          and index.shape[0] == M and 1 <= index.shape[1] <= CLOUD_KNN_MAX,
          "cloud_normals: index must be a contiguous int32 [%d,k] with 1 <= k <= %d on the operator's device" % (M, CLOUD_KNN_MAX))
    _ivec(count, op, "count", dev, M, torch.int32)
    per_query = 0
    if toward is not None:
        _chk(toward, "toward", op=op, dev=dev)
        _need(tuple(toward.shape) in ((3,), (M, 3)), "cloud_normals: toward must be [3] or [%d,3], got %s" % (M, list(toward.shape)))
        per_query = int(toward.dim() == 2)
    with torch.cuda.device(dev):
        normal, eig = torch.empty((M, 3), device=dev), torch.empty((M, 3), device=dev)
        valid, invalid = torch.empty(M, device=dev, dtype=torch.uint8), torch.zeros(1, device=dev, dtype=torch.int64)
        c = torch.empty((M, 6), device=dev, dtype=torch.float64) if cov else None
        if M:
            N.check(N.lib().estd_cloud_normals(_p(points), n, _p(query), M, ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(count.data_ptr()),
                                               int(index.shape[1]), _p(toward), per_query, _p(normal), _p(eig), ctypes.c_void_p(valid.data_ptr()),
                                               ctypes.c_void_p(invalid.data_ptr()), _p(c), _stream()), "estd_cloud_normals")
    return normal, eig, valid, invalid, c


# ---------------------------------------------------------------------------------- global registration (csrc/register/global_register.hip)
FPFH_BINS = 33                  # ESTD_FPFH_BINS (include/estd_hip.h)


def _table(t, op, name, dev, rows, cols, dtype, type_name):
    """a contiguous [rows, cols] (cols == 0: [rows]) tensor of ``dtype`` on ``dev``; rows None: any number below 2^31.  csrc/torch_ops.cpp:
    check_table()."""
    _need(isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and t.device == dev and t.dim() == (2 if cols else 1)
          and (t.shape[0] <= 0x7fffffff if rows is None else t.shape[0] == rows) and (not cols or t.shape[1] == cols),
          "%s: %s must be a contiguous %s [%s%s] on the operator's device" % (op, name, type_name, "n" if rows is None else rows, ",%d" % cols if cols else ""))


def _knn_lists(points, normal, index, count, op):
    """the cloud, its normals and cloud_knn's lists over it, as the two descriptor operators take them -> (n, k)"""
    _cloud(points, op, "points")
    n, dev = points.shape[0], points.device
    _table(normal, op, "normal", dev, n, 3, torch.float32, "float32")
    _need(isinstance(index, torch.Tensor) and index.dim() == 2 and index.dtype == torch.int32 and index.is_contiguous() and index.device == dev
          and index.shape[0] == n and 1 <= index.shape[1] <= CLOUD_KNN_MAX,
          "%s: index must be a contiguous int32 [%d,k] with 1 <= k <= %d on the operator's device" % (op, n, CLOUD_KNN_MAX))
    _table(count, op, "count", dev, n, 0, torch.int32, "int32")
    return n, int(index.shape[1])


def cloud_spfh(points, normal, index, count, oriented=True):
    """Simplified point feature histograms of the cloud ``points`` [n,3] with normals ``normal`` [n,3] (a zero row: none) over the lists
    ``index`` [n,k] int32 / ``count`` [n] int32 that cloud_knn found for the cloud against itself -> (hist int32 [n,33], pairs int32 [n]).
    ``oriented=False`` folds the features so that the sign of a normal does not matter.  The contract: include/estd_hip.h (estd_cloud_spfh)."""
    if _use_torch():
        return tuple(T().cloud_spfh(points, normal, index, count, bool(oriented)))
    op = "cloud_spfh"
    n, k = _knn_lists(points, normal, index, count, op)
    dev = points.device
    with torch.cuda.device(dev):
        hist, pairs = torch.empty((n, FPFH_BINS), device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
        if n:
            N.check(N.lib().estd_cloud_spfh(_p(points), _p(normal), n, _p(index), _p(count), k, int(bool(oriented)), _p(hist), _p(pairs), _stream()),
                    "estd_cloud_spfh")
    return hist, pairs


def cloud_fpfh(points, normal, index, count, hist, pairs):
    """Fast point feature histograms from cloud_spfh's ``hist`` / ``pairs`` over the same cloud and lists -> (desc [n,33] float32, valid
    uint8 [n], invalid int64 [1]).  The contract: include/estd_hip.h (estd_cloud_fpfh)."""
    if _use_torch():
        return tuple(T().cloud_fpfh(points, normal, index, count, hist, pairs))
    op = "cloud_fpfh"
    n, k = _knn_lists(points, normal, index, count, op)
    dev = points.device
    _table(hist, op, "hist", dev, n, FPFH_BINS, torch.int32, "int32")
    _table(pairs, op, "pairs", dev, n, 0, torch.int32, "int32")
    with torch.cuda.device(dev):
        desc, valid = torch.empty((n, FPFH_BINS), device=dev), torch.empty(n, device=dev, dtype=torch.uint8)
        invalid = torch.zeros(1, device=dev, dtype=torch.int64)
        if n:
            N.check(N.lib().estd_cloud_fpfh(_p(points), _p(normal), n, _p(index), _p(count), k, _p(hist), _p(pairs), _p(desc), _p(valid), _p(invalid),
                                            _stream()), "estd_cloud_fpfh")
    return desc, valid, invalid


def feature_match(a, b, a_valid=None, b_valid=None):
    """Per row of ``a`` [m,33] the nearest and second-nearest row of ``b`` [n,33] (float32; ``a_valid`` / ``b_valid``: uint8 masks or None)
    by brute force -> (index int32 [m], d2 [m], d2_second [m]); -1 / inf where there is none.  The contract: include/estd_hip.h
    (estd_feature_match)."""
    if _use_torch():
        return tuple(T().feature_match(a, b, a_valid, b_valid))
    op = "feature_match"
    _chk(a, "a", op=op)
    dev = a.device
    _table(a, op, "a", dev, None, FPFH_BINS, torch.float32, "float32")
    _table(b, op, "b", dev, None, FPFH_BINS, torch.float32, "float32")
    m, n = a.shape[0], b.shape[0]
    if a_valid is not None:
        _table(a_valid, op, "a_valid", dev, m, 0, torch.uint8, "uint8")
    if b_valid is not None:
        _table(b_valid, op, "b_valid", dev, n, 0, torch.uint8, "uint8")
    with torch.cuda.device(dev):
        index, d2, second = torch.empty(m, device=dev, dtype=torch.int32), torch.empty(m, device=dev), torch.empty(m, device=dev)
        if m:
            N.check(N.lib().estd_feature_match(_p(a), m, _p(b), n, _p(a_valid), _p(b_valid), _p(index), _p(d2), _p(second), _stream()),
                    "estd_feature_match")
    return index, d2, second


def ransac_pairs(P, Q, hypotheses, seed, dist_max, edge_ratio):
    """Three-point hypotheses over the correspondences ``P`` [c,3] -> ``Q`` [c,3] -> (count int32 [H], status uint8 [H], ssq float64 [H],
    T float64 [H,12], best int64 [1]: (count << 32) | (0xffffffff - h) of the winner, 0 when nothing was scored).  The contract:
    include/estd_hip.h (estd_ransac_pairs)."""
    for name, v in (("hypotheses", hypotheses), ("seed", seed)):              # no silent truncation of 4.7, no True
        _need(isinstance(v, numbers.Integral) and not isinstance(v, bool), "ransac_pairs: %s must be an integer, got %r" % (name, v))
    H, seed, dist_max, edge_ratio = int(hypotheses), int(seed) & 0xffffffffffffffff, float(dist_max), float(edge_ratio)
    if _use_torch():
        return tuple(T().ransac_pairs(P, Q, H, seed - (1 << 64) if seed >> 63 else seed, dist_max, edge_ratio))
    op = "ransac_pairs"
    _cloud(P, op, "P")
    c, dev = P.shape[0], P.device
    _table(Q, op, "Q", dev, c, 3, torch.float32, "float32")
    _count(H, 0, 0x7fffffff, op, "hypotheses")
    _need(math.isfinite(dist_max) and dist_max >= 0, "%s: dist_max must be finite and not negative, got %r" % (op, dist_max))
    _need(0 <= edge_ratio <= 1, "%s: edge_ratio must lie in 0 .. 1, got %r" % (op, edge_ratio))
    with torch.cuda.device(dev):
        count, status = torch.empty(H, device=dev, dtype=torch.int32), torch.empty(H, device=dev, dtype=torch.uint8)
        ssq, Tm = torch.empty(H, device=dev, dtype=torch.float64), torch.empty((H, 12), device=dev, dtype=torch.float64)
        best = torch.zeros(1, device=dev, dtype=torch.int64)
        if H:
            N.check(N.lib().estd_ransac_pairs(_p(P), _p(Q), c, H, seed, dist_max, edge_ratio, _p(count), _p(status), _p(ssq), _p(Tm), _p(best),
                                              _stream()), "estd_ransac_pairs")
    return count, status, ssq, Tm, best


# ---------------------------------------------------------------------------------- mesh simplification (csrc/mesh/mesh_simplify.hip)
MESH_MAX_FACES = 0x7fffffff // 3      # 3 F stays within int32


def _clusters(cluster, n_clusters, dev, op):
    """the clusters of a mesh's vertices: int32 [V] on ``dev``, ``n_clusters`` of them, none without a vertex -> V"""
    _ivec(cluster, op, "cluster", dev, dtype=torch.int32)
    n_vertices = cluster.shape[0]
    _count(n_vertices, 0, 0x7fffffff, op, "the number of vertices")
    _count(n_clusters, 1 if n_vertices else 0, n_vertices, op, "n_clusters")
    return n_vertices


def mesh_cluster_faces(faces, cluster, n_clusters):
    """The triangles ``faces`` [F,3] int32 carried over to the clusters ``cluster`` [V] int32 (values 0..n_clusters-1) of their vertices ->
    (corner [3F] int32: the cluster of corner j of face f at 3 f + j, n_clusters for a face with an index outside [0, V); triple [F,3]
    int32: the three clusters rotated so that the smallest comes first, the winding kept, or (-1, -1, -1) for such a face and for one
    that collapses because two of its clusters are equal; counts [2] int64 on the device: the invalid and the collapsed faces).
    The glue after it (fusion3d.simplify_mesh): keep the triples that are not (-1, -1, -1); among equal triples keep the one with the
    smallest input face index; emit them in ascending input face index; the same clusters in the opposite winding are another face and
    stay; stable sorts column by column, no packed key.  include/estd_hip.h, estd_mesh_cluster_faces."""
    n_clusters = int(n_clusters)
    if _use_torch():
        return tuple(T().mesh_cluster_faces(faces, cluster, n_clusters))
    op = "mesh_cluster_faces"
    n_faces = _faces(faces, op, "faces")
    dev = faces.device
    n_vertices = _clusters(cluster, n_clusters, dev, op)
    _need(n_faces <= MESH_MAX_FACES, "%s: at most %d faces, got %d" % (op, MESH_MAX_FACES, n_faces))
    with torch.cuda.device(dev):
        corner = torch.empty(3 * n_faces, device=dev, dtype=torch.int32)
        triple = torch.empty((n_faces, 3), device=dev, dtype=torch.int32)
        counts = torch.empty(2, device=dev, dtype=torch.int64)
        pp = (lambda t: _p(t)) if n_faces else (lambda t: None)
        N.check(N.lib().estd_mesh_cluster_faces(pp(faces), n_faces, n_vertices, _p(cluster) if n_vertices else None, n_clusters, pp(corner),
                                                pp(triple), _p(counts), _stream()), "estd_mesh_cluster_faces")
        if n_faces and not n_clusters:                       # without vertices every face is invalid; the entry point launched nothing
            corner.zero_()
            triple.fill_(-1)
            counts[0] = n_faces
    return corner, triple, counts


def mesh_cluster_quadrics(xyz, faces, order, segments, cell_key, mean, lo, cell, dims, reg):
    """The representative vertex of every cluster of the mesh ``xyz`` [V,3] float32 / ``faces`` [F,3] int32: ``order`` int64 [3F] (the
    corner records of mesh_cluster_faces sorted by cluster, stable: sorted position -> record), ``segments`` int64 [K + 1], ``cell_key``
    int64 [K] (the clusters' grid keys, ascending), ``mean`` [K,3] (cloud_cell_centroids' means), the grid ``lo`` CPU float32 [3] /
    ``cell`` / ``dims`` of cloud_cell_keys, ``reg`` the regularisation as a double -> (xyz [K,3]: the minimiser of the summed plane
    quadrics where it is well defined and inside its cell, else the mean's bits; normal [K,3]: the area-weighted normal of the cluster's
    faces; placed [K] bool).  Defined to the bit: include/estd_hip.h, estd_mesh_cluster_quadrics."""
    cell, dims, reg = float(cell), [int(v) for v in dims], float(reg)
    if _use_torch():
        return tuple(T().mesh_cluster_quadrics(xyz, faces, order, segments, cell_key, mean, lo, cell, dims, reg))
    op = "mesh_cluster_quadrics"
    n_vertices, n_faces = _mesh(xyz, faces, op)
    dev = faces.device
    _need(n_faces <= MESH_MAX_FACES, "%s: at most %d faces, got %d" % (op, MESH_MAX_FACES, n_faces))
    _ivec(order, op, "order", dev, 3 * n_faces)
    _ivec(segments, op, "segments", dev)
    _need(1 <= segments.shape[0] <= n_vertices + 1, "%s: segments must be [K + 1] with K <= %d vertices" % (op, n_vertices))
    K = segments.shape[0] - 1
    _ivec(cell_key, op, "cell_key", dev, K)
    _cloud(mean, op, "mean")
    _need(mean.shape[0] == K and mean.device == dev, "%s: mean must be [%d,3] on the faces' device" % (op, K))
    lo3, dims = _cloud_grid(lo, cell, dims, op, CLOUD_KEY_MAX_DIM)
    _need(math.isfinite(reg) and reg >= 0, "%s: reg must be finite and not negative, got %r" % (op, reg))
    with torch.cuda.device(dev):
        out, normal = torch.empty((K, 3), device=dev), torch.empty((K, 3), device=dev)
        placed = torch.empty(K, device=dev, dtype=torch.bool)
        pk = (lambda t: _p(t)) if K else (lambda t: None)
        N.check(N.lib().estd_mesh_cluster_quadrics(_p(xyz) if n_vertices else None, n_vertices, _p(faces) if n_faces else None, n_faces,
                                                   _p(order) if n_faces else None, _p(segments), pk(cell_key), K, pk(mean),
                                                   (ctypes.c_float * 3)(*lo3), cell, (ctypes.c_int * 3)(*dims), reg, pk(out), pk(normal),
                                                   pk(placed), _stream()), "estd_mesh_cluster_quadrics")
        if K and not n_faces:                                # without faces: the means, zero normals, nothing placed; nothing was launched
            out.copy_(mean)
            normal.zero_()
            placed.zero_()
    return out, normal, placed


# ---------------------------------------------------------------------------------- point-to-mesh distance (csrc/mesh/mesh_distance.hip)
MESH_DISTANCE_MAX_PAIRS = 1 << 23      # ESTD_MESH_DISTANCE_MAX_PAIRS (include/estd_hip.h)
MESH_DISTANCE_BIG_CELLS = 64           # ESTD_MESH_DISTANCE_BIG_CELLS


def _tri_grid(lo, cell, dims, big_cells, op):
    """the grid of the three operators: the rules of _cloud_grid, at most CLOUD_MAX_CELLS cells, big_cells not negative -> (lo3, dims, cells)"""
    lo3, dims = _cloud_grid(lo, cell, dims, op, CLOUD_MAX_DIM)
    cells = dims[0] * dims[1] * dims[2]
    _need(cells <= CLOUD_MAX_CELLS, "%s: %d cells, at most %d" % (op, cells, CLOUD_MAX_CELLS))
    _count(big_cells, 0, 0x7fffffff, op, "big_cells")
    return lo3, dims, cells


def mesh_tri_bins(xyz, faces, lo, cell, dims, big_cells=MESH_DISTANCE_BIG_CELLS):
    """Per triangle of the mesh ``xyz`` [V,3] float32 / ``faces`` [F,3] int32 the cells of the grid (``lo`` CPU float32 [3], ``cell``,
    ``dims``) its bounding box covers -> (count [F] int32: the (cell, face) pairs it owns, flag [F] int32: 0 invalid, 1 grid, 2 big list
    (more than ``big_cells`` cells), invalid [1] int64 on the device).  include/estd_hip.h, estd_mesh_tri_bins."""
    cell, dims, big_cells = float(cell), [int(v) for v in dims], int(big_cells)
    if _use_torch():
        return tuple(T().mesh_tri_bins(xyz, faces, lo, cell, dims, big_cells))
    op = "mesh_tri_bins"
    n_vertices, n_faces = _mesh(xyz, faces, op)
    lo3, dims, _ = _tri_grid(lo, cell, dims, big_cells, op)
    dev = faces.device
    with torch.cuda.device(dev):
        count, flag = torch.empty(n_faces, device=dev, dtype=torch.int32), torch.empty(n_faces, device=dev, dtype=torch.int32)
        invalid = torch.empty(1, device=dev, dtype=torch.int64)
        pp = (lambda t: _p(t)) if n_faces else (lambda t: None)
        N.check(N.lib().estd_mesh_tri_bins(_p(xyz) if n_vertices else None, n_vertices, pp(faces), n_faces, (ctypes.c_float * 3)(*lo3), cell,
                                           (ctypes.c_int * 3)(*dims), big_cells, pp(count), pp(flag), _p(invalid), _stream()),
                "estd_mesh_tri_bins")
    return count, flag, invalid


def mesh_tri_fill(xyz, faces, lo, cell, dims, big_cells, offset, n_pairs):
    """The (cell key, face) pairs of the grid triangles, each triangle's at ``offset`` [F] int64 (the exclusive prefix sum of
    mesh_tri_bins' count) -> (keys [n_pairs] int64, pair_face [n_pairs] int32).  include/estd_hip.h, estd_mesh_tri_fill."""
    cell, dims, big_cells, n_pairs = float(cell), [int(v) for v in dims], int(big_cells), int(n_pairs)
    if _use_torch():
        return tuple(T().mesh_tri_fill(xyz, faces, lo, cell, dims, big_cells, offset, n_pairs))
    op = "mesh_tri_fill"
    n_vertices, n_faces = _mesh(xyz, faces, op)
    lo3, dims, _ = _tri_grid(lo, cell, dims, big_cells, op)
    dev = faces.device
    _ivec(offset, op, "offset", dev, n_faces)
    _count(n_pairs, 0, MESH_DISTANCE_MAX_PAIRS, op, "n_pairs")
    with torch.cuda.device(dev):
        keys, pair_face = torch.empty(n_pairs, device=dev, dtype=torch.int64), torch.empty(n_pairs, device=dev, dtype=torch.int32)
        if n_pairs and n_faces:
            N.check(N.lib().estd_mesh_tri_fill(_p(xyz), n_vertices, _p(faces), n_faces, (ctypes.c_float * 3)(*lo3), cell, (ctypes.c_int * 3)(*dims),
                                               big_cells, _p(offset), n_pairs, _p(keys), _p(pair_face), _stream()), "estd_mesh_tri_fill")
    return keys, pair_face


def mesh_nearest(query, order, big_records, records, cell_start, lo, cell, dims, max_dist, bary=False, closest=False):
    """The nearest triangle of every row of ``query`` [M,3] -> (dist [M] float32, face [M] int32, bary [M,2] or None, closest [M,3] or
    None) on the query's device.  ``big_records`` [B,12] / ``records`` [P,12] with ``cell_start`` int32 [cells + 1]: the 48-byte records
    of the big list and of the (cell, face) pairs in cell order (cloud_metrics.TriangleGrid builds them), ``order`` int64 [M]: the order the
    queries are taken in.  Not found within ``max_dist``: dist = max_dist, face = -1, zeros.  The contract is spelled out in
    include/estd_hip.h (estd_mesh_nearest)."""
    cell, max_dist, dims = float(cell), float(max_dist), [int(v) for v in dims]
    if _use_torch():
        dist, face, b, c = T().mesh_nearest(query, order, big_records, records, cell_start, lo, cell, dims, max_dist, bool(bary), bool(closest))
        return dist, face, (b if bary else None), (c if closest else None)
    op = "mesh_nearest"
    _cloud(query, op, "query")
    _cloud(big_records, op, "big_records", cols=12)
    _cloud(records, op, "records", cols=12)
    M, B, P, dev = query.shape[0], big_records.shape[0], records.shape[0], query.device
    _need(big_records.device == dev and records.device == dev, "%s: the records are not on the query's device" % op)
    _count(B, 0, MESH_DISTANCE_MAX_PAIRS, op, "big records")
    _count(P, 0, MESH_DISTANCE_MAX_PAIRS, op, "records")
    _ivec(order, op, "order", dev, M)
    _positive_square(max_dist, op, "max_dist")
    lo3, dims, cells = _tri_grid(lo, cell, dims, 0, op)
    _ivec(cell_start, op, "cell_start (cells + 1)", dev, cells + 1, torch.int32)
    with torch.cuda.device(dev):
        dist, face = torch.empty(M, device=dev), torch.empty(M, device=dev, dtype=torch.int32)
        b = torch.empty((M, 2), device=dev) if bary else None
        c = torch.empty((M, 3), device=dev) if closest else None
        if M:
            d = N.MeshNearestDesc()
            d.M, d.B, d.P = M, B, P
            d.query, d.order, d.cell_start = query.data_ptr(), order.data_ptr(), cell_start.data_ptr()
            d.big_records = big_records.data_ptr() if B else None
            d.records = records.data_ptr() if P else None
            d.dist, d.face = dist.data_ptr(), face.data_ptr()
            d.bary, d.closest = (b.data_ptr() if bary else None), (c.data_ptr() if closest else None)
            d.cell, d.max_dist = cell, max_dist
            d.lo[:], d.dims[:] = lo3, dims
            N.check(N.lib().estd_mesh_nearest(ctypes.byref(d), _stream()), "estd_mesh_nearest")
    return dist, face, b, c


# ---------------------------------------------------------------------------------- frame-to-model alignment (csrc/track/frame_align.hip)
FRAME_ALIGN_SUMS = 29           # ESTD_FRAME_ALIGN_SUMS (include/estd_hip.h)


def frame_align(depth, conf, m_depth, m_normal, mats, dist_max, z_near, conf_min=0.0):
    """The Gauss-Newton system of the live ``depth`` [H,W] (``conf`` [H,W] or None: pixels below ``conf_min`` are skipped) against the model
    maps ``m_depth`` [Hm,Wm] / ``m_normal`` [Hm,Wm,3] with the host matrices ``mats`` (CPU float32 [3,12]: L, Fm, Bm of
    camera.frame_align_matrices) -> (residual [H,W], match int32 [H,W], sums float64 [29]) on the depth's device: the point-to-plane
    residual and the model pixel of every matched pixel (0 / -1 elsewhere), the 21 upper entries of sum J J^T, the 6 of sum J r, sum r^2
    and the match count.  The contract is spelled out in include/estd_hip.h (estd_frame_align)."""
    dist_max, z_near, conf_min = float(dist_max), float(z_near), float(conf_min)
    if _use_torch():
        return tuple(T().frame_align(depth, conf, m_depth, m_normal, mats, dist_max, z_near, conf_min))
    op = "frame_align"
    H, W = _map(depth, (-1, -1), op, "depth")
    _map_size(H, W, op, "depth")
    dev = depth.device
    if conf is not None:
        _map(conf, (H, W), op, "conf", dev)
    Hm, Wm = _map(m_depth, (-1, -1), op, "m_depth", dev)
    _map_size(Hm, Wm, op, "m_depth")
    _map(m_normal, (Hm, Wm, 3), op, "m_normal", dev)
    flat = _host_values(mats, 36, op, "mats", "[3,12] (L, Fm, Bm)", finite=True)
    _positive_square(dist_max, op, "dist_max", square_positive=True)
    _not_negative(z_near, op, "z_near")
    _not_nan(conf_min, op, "conf_min")
    with torch.cuda.device(dev):
        residual, match = torch.empty((H, W), device=dev), torch.empty((H, W), device=dev, dtype=torch.int32)
        sums = torch.empty((FRAME_ALIGN_SUMS,), device=dev, dtype=torch.float64)
        partials = torch.empty((N.lib().estd_frame_align_partials(H, W) // 8,), device=dev, dtype=torch.float64)
        d = N.FrameAlignDesc()
        d.H, d.W, d.Hm, d.Wm = H, W, Hm, Wm
        d.dist_max, d.z_near, d.conf_min = dist_max, z_near, conf_min
        d.depth, d.conf = depth.data_ptr(), conf.data_ptr() if conf is not None else None
        d.m_depth, d.m_normal = m_depth.data_ptr(), m_normal.data_ptr()
        d.residual, d.match, d.sums, d.partials = residual.data_ptr(), match.data_ptr(), sums.data_ptr(), partials.data_ptr()
        d.L[:], d.Fm[:], d.Bm[:] = flat[:12], flat[12:24], flat[24:]
        N.check(N.lib().estd_frame_align(ctypes.byref(d), _stream()), "estd_frame_align")
    return residual, match, sums


# ---------------------------------------------------------------------------------- rigid registration (csrc/track/rigid_align.hip)
RIGID_SYSTEM_SUMS = 29          # ESTD_RIGID_SYSTEM_SUMS (include/estd_hip.h)
RIGID_METRICS = {"plane": 0, "point": 1}      # ESTD_RIGID_PLANE, ESTD_RIGID_POINT


def rigid_apply(src, src_normal, T12):
    """``src`` [n,3] (and ``src_normal`` [n,3] or None) moved by the host matrix ``T12`` (CPU float32 [3,4], row-major) ->
    (moved [n,3], moved_normal [n,3] or None) on the points' device: T p per point and R n per normal, every coordinate a chain of
    fused multiply-adds (include/estd_hip.h, estd_rigid_apply)."""
    if _use_torch():
        moved, mn = T().rigid_apply(src, src_normal, T12)
        return moved, (mn if src_normal is not None else None)
    op = "rigid_apply"
    _cloud(src, op, "src")
    n, dev = src.shape[0], src.device
    if src_normal is not None:
        _cloud(src_normal, op, "src_normal")
        _need(src_normal.shape[0] == n and src_normal.device == dev, "%s: src_normal must be [%d,3] on the points' device" % (op, n))
    flat = _host_values(T12, 12, op, "T", "[3,4]", finite=True)
    with torch.cuda.device(dev):
        moved = torch.empty((n, 3), device=dev)
        mn = torch.empty((n, 3), device=dev) if src_normal is not None else None
        if n:
            N.check(N.lib().estd_rigid_apply(_p(src), _p(src_normal), n, (ctypes.c_float * 12)(*flat), _p(moved), _p(mn), _stream()), "estd_rigid_apply")
    return moved, mn


def rigid_system(moved, moved_normal, index, target, normal, by_index=True, metric="plane", dist_max=0.1, cos_min=None, two_sided=False):
    """The Gauss-Newton system of the moved cloud ``moved`` [N,3] against its partners: ``index`` int64 [N] names the partner of every
    point (-1 or any value out of range: none), ``target`` [Nt,3] is read at index[i] (``by_index``) or at i (the ``closest`` array of
    mesh_nearest), ``normal`` [Nn,3] at index[i] (target normals or face normals; None: the point metric without a cosine gate).
    ``metric``: "plane" or "point"; partners farther than ``dist_max`` are left out, and with ``moved_normal`` [N,3] and ``cos_min`` those
    whose normals' cosine is below it (``two_sided``: whose absolute cosine is).  -> (residual [N], match int64 [N], sums float64 [29]) on the
    points' device.  The contract is spelled out in include/estd_hip.h (estd_rigid_system)."""
    _need(metric in RIGID_METRICS, "rigid_system: metric must be one of %s, got %r" % (sorted(RIGID_METRICS), metric))
    dist_max, cos_min = float(dist_max), (float("-inf") if cos_min is None else float(cos_min))
    m, by_index, two_sided = RIGID_METRICS[metric], bool(by_index), bool(two_sided)
    if _use_torch():
        return tuple(T().rigid_system(moved, moved_normal, index, target, normal, by_index, m, dist_max, cos_min, two_sided))
    op = "rigid_system"
    _cloud(moved, op, "moved")
    n, dev = moved.shape[0], moved.device
    if moved_normal is not None:
        _cloud(moved_normal, op, "moved_normal")
        _need(moved_normal.shape[0] == n and moved_normal.device == dev, "%s: moved_normal must be [%d,3] on the points' device" % (op, n))
    _ivec(index, op, "index", dev, n)
    _cloud(target, op, "target")
    n_target = target.shape[0]
    _need(target.device == dev and (by_index or n_target >= n),
          "%s: target must be on the points' device, and [n,3] with n >= %d when it is not read by index" % (op, n))
    n_normal = n_target
    if normal is not None:
        _cloud(normal, op, "normal")
        _need(normal.device == dev, "%s: normal must be on the points' device" % op)
        n_normal = normal.shape[0]
    _positive_square(dist_max, op, "dist_max", square_positive=True)
    if moved_normal is not None:
        _not_nan(cos_min, op, "cos_min")
    _need(normal is not None or not (m == 0 or (moved_normal is not None and math.isfinite(cos_min))),
          "%s: the plane metric and the cosine gate need the target's normals" % op)
    with torch.cuda.device(dev):
        residual, match = torch.empty(n, device=dev), torch.empty(n, device=dev, dtype=torch.int64)
        sums = torch.empty((RIGID_SYSTEM_SUMS,), device=dev, dtype=torch.float64)
        partials = torch.empty((N.lib().estd_rigid_system_partials(n) // 8,), device=dev, dtype=torch.float64)
        d = N.RigidSystemDesc()
        d.N, d.Nt, d.Nn = n, n_target, n_normal
        d.metric, d.by_index, d.two_sided = m, int(by_index), int(two_sided)
        d.dist_max, d.cos_min = dist_max, cos_min
        d.moved, d.index, d.target = moved.data_ptr(), index.data_ptr(), target.data_ptr()
        d.moved_normal = moved_normal.data_ptr() if moved_normal is not None else None
        d.normal = normal.data_ptr() if normal is not None else None
        d.residual, d.match, d.sums = residual.data_ptr(), match.data_ptr(), sums.data_ptr()
        d.partials = partials.data_ptr() if n else None
        N.check(N.lib().estd_rigid_system(ctypes.byref(d), _stream()), "estd_rigid_system")
    return residual, match, sums
