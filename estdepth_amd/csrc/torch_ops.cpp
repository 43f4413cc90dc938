// torch_ops.cpp -- PyTorch-ROCm custom-operator registration of the ESTDepth hot path (namespace `estdepth_hip`).
//
// Thin, allocation-and-validation-only wrappers over the torch-free C ABI of libestd_hip.so (include/estd_hip.h):
//   * device / dtype / contiguity / shapes / buffer sizes are checked by one helper per kind of rule ("argument checks" below; the
//     ctypes front ends of estdepth_amd/ops.py call the same set in the same order)  -> Python RuntimeError naming the operator and
//     the argument, the way ATen shape errors surface from the reference today (SURVEY §8b "Errors"); value rules the C ABI
//     enforces itself (strides, channel multiples, 32-bit limits) come back as its status;
//   * outputs allocated with at::empty on the input device (caching allocator), never retained;
//   * every kernel is enqueued on at::hip::getCurrentHIPStream() -- asynchronous, graph-capturable;
//   * a negative estd_status becomes TORCH_CHECK(false, estd_status_string(status)).
// The operators replace these reference call sites: utils/homo_utils.py:458 (homo_warping), :240 (warp_volume),
// hybrid_models/model_hybrid.py:62-102 (get_costvolume front), networks/layers_op.py:16-39 (convbn*_3d),
// hybrid_models/hybrid_depth_decoder.py:33 (depthlayer), :229-260 (temporal fusion),
// transformer/epipolar_transformer.py:31-83 (attention + ConvGRU).
// Built by estdepth_amd/build.py into estdepth_amd/lib/libestd_torch_ops.so; loaded with torch.ops.load_library().
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "estd_hip.h"

namespace {

using at::Tensor;
using OptTensor = std::optional<Tensor>;

inline estd_stream_t cur_stream() { return static_cast<estd_stream_t>(c10::hip::getCurrentHIPStream().stream()); }

// Every operator opens an OpScope on its first tensor argument: a device guard (the kernels are enqueued on the current stream
// of THAT tensor's device, not of whatever device happens to be current), and every further tensor checked through fptr() must
// live on the same device.
struct OpScope {
    static inline thread_local const c10::Device* cur = nullptr;
    c10::OptionalDeviceGuard guard;
    c10::Device dev;
    const c10::Device* prev;
    explicit OpScope(const Tensor& t) : guard(at::device_of(t)), dev(t.defined() ? t.device() : c10::Device(c10::kCPU)), prev(cur) { cur = &dev; }
    ~OpScope() { cur = prev; }
    OpScope(const OpScope&) = delete;
    OpScope& operator=(const OpScope&) = delete;
};

inline void check_status(int st, const char* what)
{
    TORCH_CHECK(st == ESTD_OK, what, " failed: ", estd_status_string(st), " (estd_status ", st, ")");
}

// `op`: the operator's name, put in front of the message (the helpers of the argument checks pass it)
inline const float* fptr(const Tensor& t, const char* name, bool need_contiguous = true, const char* op = nullptr)
{
    const char* sep = op ? ": " : "";
    if (!op) op = "";
    TORCH_CHECK(t.defined(), op, sep, name, " must be a tensor");
    TORCH_CHECK(t.is_cuda(), op, sep, name, " must live on a ROCm device (estdepth_hip has no CPU path); got ", t.device());
    if (OpScope::cur) TORCH_CHECK(t.device() == *OpScope::cur, op, sep, name, " is on ", t.device(), " but the operator runs on ", *OpScope::cur);
    TORCH_CHECK(t.scalar_type() == at::kFloat, op, sep, name, " must be float32, got ", t.scalar_type());
    if (need_contiguous) TORCH_CHECK(t.is_contiguous(), op, sep, name, " must be contiguous");
    return t.data_ptr<float>();
}
inline float* fptr_mut(const Tensor& t, const char* name, bool need_contiguous = true) { return const_cast<float*>(fptr(t, name, need_contiguous)); }
inline const float* opt_fptr(const OptTensor& t, const char* name, bool need_contiguous = true)
{
    return (t.has_value() && t->defined()) ? fptr(*t, name, need_contiguous) : nullptr;
}
inline float* mut(const float* p) { return const_cast<float*>(p); }      // an argument the operator writes
inline Tensor new_f32(at::IntArrayRef shape, const Tensor& like) { return at::empty(shape, like.options().dtype(at::kFloat)); }

// ------------------------------------------------------------------------------------------------ argument checks
// One helper per kind of check for every operator of this file but the convolution plans' (estdepth_amd/ops.py has the same set for the
// ctypes binding, and each operator calls them in the same order there); each takes the operator's and the argument's name for its message.

// the volume argument: two float32 planes (0 = D, 1 = Wt), contiguous, on the operator's device, X % 4 == 0
struct VolumeArg { int64_t Z, Y, X; float* tsdf; float* weight; };
static VolumeArg check_volume(const Tensor& volume, const char* op, bool any_x = false)      // any_x: the mesh kernels take any X
{
    TORCH_CHECK(volume.dim() == 4 && volume.size(0) == 2, op, ": volume must be [2,Z,Y,X] (D plane, weight plane)");
    float* vol = mut(fptr(volume, "volume", true, op));
    const int64_t Z = volume.size(1), Y = volume.size(2), X = volume.size(3);
    TORCH_CHECK(any_x || X % 4 == 0, op, ": X must be a multiple of 4, got ", X);
    return {Z, Y, X, vol, vol + Z * Y * X};
}

static float* check_color_planes(const Tensor& color, const Tensor& volume, const char* op)
{
    TORCH_CHECK(color.dim() == 4 && color.size(0) == 3 && color.size(1) == volume.size(1) && color.size(2) == volume.size(2) &&
                color.size(3) == volume.size(3), op, ": color must be [3,Z,Y,X] with the volume's Z, Y, X");
    TORCH_CHECK(color.device() == volume.device(), op, ": color and the volume are on different devices");
    return mut(fptr(color, "color", true, op));
}

// host values of the launch arguments: exactly n of them (finite: none NaN or infinite)
static const float* host_values(const Tensor& t, int64_t n, const char* op, const char* name, const char* shape, bool finite = false)
{
    TORCH_CHECK(t.defined() && t.device().is_cpu() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == n,
                op, ": ", name, " must be a contiguous CPU float32 tensor ", shape);
    const float* v = t.data_ptr<float>();
    for (int64_t i = 0; finite && i < n; ++i) TORCH_CHECK(std::isfinite(v[i]), op, ": ", name, " holds a value that is not finite");
    return v;
}

// a float32 map on the operator's device whose last sizes are `tail` (-1: any size), leading 1s allowed; its sizes: t.size(-k)
static const float* map_ptr(const Tensor& t, at::IntArrayRef tail, const char* op, const char* name)
{
    const float* p = fptr(t, name, true, op);
    const int64_t k = (int64_t)tail.size();
    bool ok = t.dim() >= k;
    int64_t n = 1;
    for (int64_t i = 0; ok && i < k; ++i) {
        const int64_t s = t.size(t.dim() - k + i);
        ok = tail[i] < 0 || tail[i] == s;
        n *= s;
    }
    TORCH_CHECK(ok && t.numel() == n, op, ": ", name, " must end in the sizes ", tail, " (-1: any; leading 1s allowed), got ", t.sizes());
    return p;
}

static void check_map_size(int64_t H, int64_t W, const char* op, const char* name, int64_t least = 1)
{
    TORCH_CHECK(H >= least && W >= least && H * W <= 0x7fffffffLL, op, ": ", name, " must be at least ", least, " x ", least,
                " (and H * W < 2^31), got ", H, " x ", W);
}

// a float32 tensor on the operator's device that holds exactly (at_least: at least) n floats, whatever its shape; strided: the base of
// wider records, which need not be contiguous
static const float* floats_ptr(const Tensor& t, int64_t n, const char* op, const char* name, bool at_least = false, bool strided = false)
{
    const float* p = fptr(t, name, !strided, op);
    TORCH_CHECK(at_least ? t.numel() >= n : t.numel() == n, op, ": ", name, " must hold ", at_least ? "at least " : "exactly ", n,
                " floats, got ", t.numel());
    return p;
}

// a float32 tensor of whole 32-float records (voxels) and nothing else -> their number
static int64_t records(const Tensor& t, const char* op, const char* name)
{
    const int64_t n_vox = t.defined() ? t.numel() / 32 : 0;
    floats_ptr(t, n_vox * 32, op, name);
    return n_vox;
}

// an optional vector (a per-channel scale, shift or bias; a second pose): nothing, or exactly n floats
static const float* opt_floats_ptr(const OptTensor& t, int64_t n, const char* op, const char* name)
{
    return (t.has_value() && t->defined()) ? floats_ptr(*t, n, op, name) : nullptr;
}

// a list of float32 tensors on the operator's device, each of `first`'s shape
static std::vector<const float*> like_ptrs(at::TensorList ts, const Tensor& first, const char* op, const char* name)
{
    std::vector<const float*> ptrs(ts.size());
    for (size_t i = 0; i < ts.size(); ++i) {
        const std::string item = std::string(name) + "[" + std::to_string(i) + "]";
        ptrs[i] = fptr(ts[i], item.c_str(), true, op);
        TORCH_CHECK(ts[i].sizes() == first.sizes(), op, ": ", item, " has another shape than the first tensor: ", ts[i].sizes(), " for ", first.sizes());
    }
    return ptrs;
}

// bn_act_nhwc_'s tensors: float32 [N,C,H,W] in channels_last memory on the operator's device (like: and of that tensor's shape)
static float* channels_last_ptr(const Tensor& t, const char* op, const char* name, const Tensor* like = nullptr)
{
    const float* p = fptr(t, name, false, op);
    TORCH_CHECK(t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast), op, ": ", name, " must be [N,C,H,W] in channels_last memory, got ",
                t.sizes(), " with the strides ", t.strides());
    TORCH_CHECK(!like || t.sizes() == like->sizes(), op, ": ", name, " must have the shape ", like ? like->sizes() : t.sizes(), ", got ", t.sizes());
    return mut(p);
}

// a count (tensors of a list, a window, a stride the front end divides by) within lo..hi
static void check_count(int64_t v, int64_t lo, int64_t hi, const char* op, const char* name)
{
    TORCH_CHECK(v >= lo && v <= hi, op, ": ", name, ": at least ", lo, " and at most ", hi, " expected, got ", v);
}

// a contiguous integer vector (int64 unless I says otherwise) on `like`'s device, of `size` elements (< 0: any number)
template <class I = int64_t>
static const I* lptr(const Tensor& t, const char* op, const char* name, const Tensor& like, int64_t size)
{
    TORCH_CHECK(t.defined() && t.dim() == 1 && t.scalar_type() == c10::CppTypeToScalarType<I>::value && t.is_contiguous() &&
                t.device() == like.device() && (size < 0 || t.size(0) == size), op, ": ", name, " must be a contiguous ",
                c10::CppTypeToScalarType<I>::value, " vector of the right length on the operator's device");
    return t.data_ptr<I>();
}

// the four rules for a scalar that a kernel takes as fp32 -> the fp32 value
static float positive_f32(double v, const char* op, const char* name)
{
    TORCH_CHECK(std::isfinite(v) && (float)v > 0.f, op, ": ", name, " must be positive and finite, got ", v);
    return (float)v;
}
static float not_negative_f32(double v, const char* op, const char* name)
{
    TORCH_CHECK(std::isfinite(v) && v >= 0, op, ": ", name, " must be finite and not negative, got ", v);
    return (float)v;
}
static float not_nan_f32(double v, const char* op, const char* name)
{
    TORCH_CHECK(v == v, op, ": ", name, " must not be NaN");
    return (float)v;
}
// positive and finite, and its square finite in fp32 (square_positive: and not rounded to 0)
static float positive_square_f32(double v, const char* op, const char* name, bool square_positive = false)
{
    const float f = (float)v, sq = f * f;
    TORCH_CHECK(std::isfinite(v) && f > 0.f && std::isfinite(sq) && (sq > 0.f || !square_positive),
                op, ": ", name, " (and its square in fp32) must be positive and finite, got ", v);
    return f;
}

// Every entry point takes the stream last: one launch on the current stream of the operator's device, its status translated.
#define ESTD_LAUNCH(entry, ...) check_status(entry(__VA_ARGS__, cur_stream()), #entry)

// ------------------------------------------------------------------------------------------------ camera algebra
Tensor cam_pair_proj(const Tensor& src_proj, const Tensor& ref_proj)
{
    const char* op = "cam_pair_proj";
    const OpScope scope(src_proj);
    const float *sp = floats_ptr(src_proj, 16, op, "src_proj"), *rp = floats_ptr(ref_proj, 16, op, "ref_proj");
    Tensor out = new_f32({12}, src_proj);
    ESTD_LAUNCH(estd_cam_pair_proj, sp, rp, out.data_ptr<float>());
    return out;
}

Tensor cam_sweep_proj(const Tensor& ref_pose, const Tensor& src_pose, const Tensor& intr)
{
    const char* op = "cam_sweep_proj";
    const OpScope scope(ref_pose);
    const float *rp = floats_ptr(ref_pose, 16, op, "ref_pose"), *sp = floats_ptr(src_pose, 16, op, "src_pose");
    const float* k = floats_ptr(intr, 9, op, "intr");
    Tensor out = new_f32({12}, ref_pose);
    ESTD_LAUNCH(estd_cam_sweep_proj, rp, sp, k, out.data_ptr<float>());
    return out;
}

void cam_volume_mats(const Tensor& pose_j, const OptTensor& pose_i, const Tensor& intr, Tensor out)
{
    const char* op = "cam_volume_mats";
    const OpScope scope(pose_j);
    const float *pj = floats_ptr(pose_j, 16, op, "pose_j"), *pi = opt_floats_ptr(pose_i, 16, op, "pose_i");
    const float* k = floats_ptr(intr, 9, op, "intr");
    ESTD_LAUNCH(estd_cam_volume_mats, pj, pi, k, mut(floats_ptr(out, 30, op, "out")));
}

// ------------------------------------------------------------------------------------------------ plane sweep
// The body of homo_warping (depth: at least D plane depths) and homo_warping_px (per_pixel: depth is [D,H,W], which gives D).
template <class Launch>
static Tensor homo_warp(const char* op, Launch launch, const char* what, const Tensor& src_chw, const Tensor& proj12, const Tensor& depth, bool per_pixel, int64_t D)
{
    const OpScope scope(src_chw);
    const float* src = map_ptr(src_chw, {-1, -1, -1}, op, "src_chw");
    const int64_t C = src_chw.size(-3), H = src_chw.size(-2), W = src_chw.size(-1);
    const float* P = floats_ptr(proj12, 12, op, "proj12");
    const float* dv = per_pixel ? map_ptr(depth, {-1, H, W}, op, "depth_dhw") : floats_ptr(depth, D, op, "depth_values", true);
    if (per_pixel) D = depth.size(-3);
    Tensor out = new_f32({C, D, H, W}, src_chw);
    check_status(launch(src, P, dv, out.data_ptr<float>(), (int)C, (int)D, (int)H, (int)W, cur_stream()), what);
    return out;
}

Tensor homo_warping(const Tensor& src_chw, const Tensor& proj12, const Tensor& depth_values, int64_t D)
{
    return homo_warp("homo_warping", estd_homo_warping, "estd_homo_warping", src_chw, proj12, depth_values, false, D);
}

Tensor homo_warping_px(const Tensor& src_chw, const Tensor& proj12, const Tensor& depth_dhw)
{
    return homo_warp("homo_warping_px", estd_homo_warping_px, "estd_homo_warping_px", src_chw, proj12, depth_dhw, true, 0);
}

Tensor mix1x1(const Tensor& in_chw, const Tensor& w, const OptTensor& bias)
{
    const char* op = "mix1x1";
    const OpScope scope(in_chw);
    const float* in = map_ptr(in_chw, {-1, -1, -1}, op, "in_chw");
    const int64_t Cin = in_chw.size(-3), H = in_chw.size(-2), W = in_chw.size(-1);
    const float* wp = map_ptr(w, {-1, Cin}, op, "w");
    const int64_t Cout = w.size(-2);
    const float* b = opt_floats_ptr(bias, Cout, op, "bias");
    Tensor out = new_f32({H, W, Cout}, in_chw);
    ESTD_LAUNCH(estd_mix1x1_chw_to_hwc, in, wp, b, out.data_ptr<float>(), (int)Cin, (int)Cout, (int)(H * W));
    return out;
}

void homo_warp_costvol(const Tensor& src_mix, const Tensor& ref_mix, const Tensor& proj12, const Tensor& depth_values,
                       int64_t D, Tensor out)
{
    const char* op = "homo_warp_costvol";
    const OpScope scope(src_mix);
    const float* src = map_ptr(src_mix, {-1, -1, 32}, op, "src_mix");
    const int64_t H = src_mix.size(-3), W = src_mix.size(-2);
    const float* ref = map_ptr(ref_mix, {H, W, 32}, op, "ref_mix");
    const float* P = floats_ptr(proj12, 12, op, "proj12");
    const float* dv = floats_ptr(depth_values, D, op, "depth_values", true);
    ESTD_LAUNCH(estd_homo_warp_costvol, src, ref, P, dv, mut(floats_ptr(out, D * H * W * 32, op, "out")), (int)D, (int)H, (int)W);
}

// ------------------------------------------------------------------------------------------------ conv3d / conv2d
// Volumes are addressed as base pointers + strides (views into wider channels-last records are allowed), so only device
// and dtype are checked for them; the C ABI validates the stride / channel combinations.
void conv3d_k3(const Tensor& x, const OptTensor& x_extra, const OptTensor& w_main, const OptTensor& w_extra, const OptTensor& w_xout,
               const OptTensor& w_alt, const Tensor& scale, const Tensor& shift, at::IntArrayRef dims, int64_t cin_main,
               int64_t in_stride, int64_t n_tiles, int64_t act_a, int64_t act_b, int64_t act_split, const OptTensor& out,
               int64_t out_stride, int64_t out_channels, const OptTensor& residual, const OptTensor& residual2, double out_scale,
               bool accumulate, const OptTensor& out_extra, const OptTensor& head_w, const OptTensor& head_b, const OptTensor& out_head,
               const OptTensor& stats_partials, int64_t variant, const OptTensor& gate_r, const OptTensor& gate_stats,
               const OptTensor& gate_gamma, const OptTensor& gate_beta)
{
    const OpScope scope(x);
    TORCH_CHECK(dims.size() == 4, "conv3d_k3: dims = (N, D, H, W)");
    estd_conv3d_desc d{};
    d.N = (int)dims[0]; d.D = (int)dims[1]; d.H = (int)dims[2]; d.W = (int)dims[3];
    d.cin_main = (int)cin_main; d.in_stride = (int)in_stride; d.n_tiles = (int)n_tiles;
    const int64_t vox = dims[0] * dims[1] * dims[2] * dims[3];
    d.in_main = fptr(x, "conv3d input", false);
    d.in_extra = opt_fptr(x_extra, "conv3d extra input channel");
    if (d.in_extra) TORCH_CHECK(x_extra->numel() >= vox, "conv3d_k3: extra input channel smaller than N*D*H*W");
    d.w_main = opt_fptr(w_main, "packed weights");      // the direct kernel reads it (variant 0); the Winograd variants read w_alt
    TORCH_CHECK(variant != 0 || d.w_main, "conv3d_k3: the direct kernel (variant 0) needs w_main");
    d.w_extra = opt_fptr(w_extra, "packed extra-channel weights");
    d.w_xout = opt_fptr(w_xout, "packed 33rd-output weights");
    TORCH_CHECK((d.in_extra == nullptr) == (d.w_extra == nullptr), "conv3d plan/extra-channel mismatch");
    d.scale = fptr(scale, "scale"); d.shift = fptr(shift, "shift");
    d.act_a = (int)act_a; d.act_b = (int)act_b; d.act_split = (int)act_split;
    d.out_main = const_cast<float*>(opt_fptr(out, "conv3d output", false));
    d.out_stride = (int)out_stride; d.out_channels = (int)out_channels;
    d.residual = opt_fptr(residual, "residual", false);
    d.residual2 = opt_fptr(residual2, "residual2", false);
    d.out_scale = (float)out_scale; d.accumulate = accumulate ? 1 : 0;
    d.out_extra = const_cast<float*>(opt_fptr(out_extra, "33rd output channel"));
    d.head_w = opt_fptr(head_w, "head weight"); d.head_b = opt_fptr(head_b, "head bias");
    d.out_head = const_cast<float*>(opt_fptr(out_head, "head output"));
    if (!d.out_head) { d.head_w = nullptr; d.head_b = nullptr; }
    if (d.out_head) TORCH_CHECK(out_head->numel() >= vox, "conv3d_k3: head output smaller than N*D*H*W");
    d.stats_partials = nullptr;
    if (stats_partials.has_value() && stats_partials->defined()) {
        TORCH_CHECK(stats_partials->is_cuda() && stats_partials->scalar_type() == at::kDouble && stats_partials->is_contiguous(),
                    "conv3d_k3: stats_partials must be a contiguous float64 ROCm tensor");
        const int blocks = estd_conv3d_k3_grid(d.N, d.D, d.H, d.W);
        TORCH_CHECK(blocks > 0 && stats_partials->numel() >= (int64_t)blocks * 4, "conv3d_k3: stats_partials needs 4 doubles per tile");
        d.stats_partials = stats_partials->data_ptr<double>();
    }
    // reset gate folded into the loads of the 32 -> 16 two-axis Winograd instance (all four tensors or none)
    d.gate_r = opt_fptr(gate_r, "gate r volume", false);
    d.gate_stats = opt_fptr(gate_stats, "gate statistics");
    d.gate_gamma = opt_fptr(gate_gamma, "gate gamma");
    d.gate_beta = opt_fptr(gate_beta, "gate beta");
    if (d.gate_r) {
        TORCH_CHECK(d.gate_stats && d.gate_gamma && d.gate_beta, "conv3d_k3: the reset gate needs r, statistics, gamma and beta");
        TORCH_CHECK(gate_r->numel() >= vox * 32 && gate_stats->numel() >= 2 && gate_gamma->numel() >= 16 && gate_beta->numel() >= 16,
                    "conv3d_k3: reset-gate tensors too small");
        TORCH_CHECK(variant == 3, "conv3d_k3: the reset gate exists in the two-axis Winograd kernel's 32 -> 16 instance only");
    }
    // variant: 0 = direct fp32 MFMA; 1 = exact 3 x bf16 operand split (w_alt = split weights); 2 = fp32 MFMA with the depth
    // axis in Winograd F(2,3) form (w_alt = transformed filters); 3 = depth and row axis in Winograd form (w_extra / w_xout in that kernel's packing)
    if (variant != 0) TORCH_CHECK(w_alt.has_value() && w_alt->defined() && w_alt->is_cuda(), "conv3d_k3: this variant needs its packed weights");
    if (variant == 1 || variant == 2) {
#ifdef ESTD_BUILD_AB
        if (variant == 1) {
            d.w_split = w_alt->data_ptr();
            check_status(estd_conv3d_k3_split(&d, cur_stream()), "estd_conv3d_k3_split");
        } else {
            d.w_wino = fptr(*w_alt, "Winograd-packed weights");
            check_status(estd_conv3d_k3_wino(&d, cur_stream()), "estd_conv3d_k3_wino");
        }
#else
        TORCH_CHECK(false, "conv3d_k3: variant ", variant, " (bf16 operand split / depth-only Winograd) needs a library built with ESTD_BUILD_AB=1");
#endif
    } else if (variant == 3) {
        d.w_wino2 = fptr(*w_alt, "2-axis Winograd-packed weights");
        check_status(estd_conv3d_k3_wino2(&d, cur_stream()), "estd_conv3d_k3_wino2");
    } else if (variant == 4) {          // the 32 -> 32 instance on the operand-reuse kernel (w_alt = packing.pack_conv3d_wino2x)
#ifdef ESTD_BUILD_AB
        d.w_wino2 = fptr(*w_alt, "2-axis Winograd-packed weights (reuse form)");
        check_status(estd_conv3d_k3_wino2x(&d, cur_stream()), "estd_conv3d_k3_wino2x");
#else
        TORCH_CHECK(false, "conv3d_k3: variant 4 (operand-reuse two-axis Winograd kernel) needs a library built with ESTD_BUILD_AB=1");
#endif
    } else if (variant == 5) {          // the 32 -> 32 instance with all three axes in Winograd form (w_alt = packing.pack_conv3d_wino3)
        d.w_wino2 = fptr(*w_alt, "3-axis Winograd-packed weights");
        check_status(estd_conv3d_k3_wino3(&d, cur_stream()), "estd_conv3d_k3_wino3");
    } else if (variant == 6) {          // output channel 32 of the 33 -> 33 instance alone (w_alt = packing.pack_conv3d_xout_taps)
        d.w_xout = fptr(*w_alt, "tap-major weights of output channel 32");
        // the kernel reads scale[32] / shift[32] and writes N*D*H*W floats of out_extra
        TORCH_CHECK(scale.numel() >= 33 && shift.numel() >= 33, "conv3d_k3: output channel 32 needs scale and shift with 33 entries");
        TORCH_CHECK(d.out_extra && out_extra->numel() >= vox, "conv3d_k3: 33rd output channel smaller than N*D*H*W");
        check_status(estd_conv3d_k3_xout(&d, cur_stream()), "estd_conv3d_k3_xout");
    } else {
        TORCH_CHECK(variant == 0, "conv3d_k3: unknown variant ", variant);
        check_status(estd_conv3d_k3(&d, cur_stream()), "estd_conv3d_k3");
    }
}

Tensor conv2d_k3(const Tensor& x_nhwc, const OptTensor& w, const OptTensor& w_alt, const Tensor& scale, const Tensor& shift,
                 int64_t cout, int64_t dilation, int64_t group_tiles, bool relu_before_residual, bool relu_after_residual,
                 const OptTensor& residual, int64_t variant)
{
    const OpScope scope(x_nhwc);
    TORCH_CHECK(x_nhwc.dim() == 4, "conv2d_k3: input must be [N,H,W,Cin] (NHWC, contiguous)");
    estd_conv2d_desc d{};
    d.N = (int)x_nhwc.size(0); d.H = (int)x_nhwc.size(1); d.W = (int)x_nhwc.size(2); d.cin = (int)x_nhwc.size(3);
    d.cout = (int)cout; d.dilation = (int)dilation; d.group_tiles = (int)group_tiles;
    d.in = fptr(x_nhwc, "conv2d input");
    d.w = opt_fptr(w, "packed conv2d weights");         // the direct kernel reads it (variant 0); the other variants read w_alt
    TORCH_CHECK(variant != 0 || d.w, "conv2d_k3: the direct kernel (variant 0) needs w");
    d.scale = fptr(scale, "scale"); d.shift = fptr(shift, "shift");
    TORCH_CHECK(scale.numel() == cout && shift.numel() == cout, "conv2d_k3: scale/shift must have Cout entries");
    d.relu_before_residual = relu_before_residual; d.relu_after_residual = relu_after_residual;
    Tensor out = new_f32({x_nhwc.size(0), x_nhwc.size(1), x_nhwc.size(2), cout}, x_nhwc);
    d.residual = opt_fptr(residual, "conv2d residual");
    if (d.residual) TORCH_CHECK(residual->sizes() == out.sizes(), "conv2d_k3: residual must be contiguous NHWC of the output shape");
    d.out = out.data_ptr<float>();
    // variant: 0 = direct fp32 MFMA; 1 = exact 3 x bf16 operand split; 2 = fp32 MFMA with the row axis in Winograd F(2,3) form
    if (variant != 0) TORCH_CHECK(w_alt.has_value() && w_alt->defined() && w_alt->is_cuda(), "conv2d_k3: this variant needs its packed weights");
    if (variant == 1 || variant == 2) {
#ifdef ESTD_BUILD_AB
        if (variant == 1) {
            d.w_split = w_alt->data_ptr();
            check_status(estd_conv2d_k3_split(&d, cur_stream()), "estd_conv2d_k3_split");
        } else {
            d.w_wino = fptr(*w_alt, "Winograd-packed weights");
            check_status(estd_conv2d_k3_wino(&d, cur_stream()), "estd_conv2d_k3_wino");
        }
#else
        TORCH_CHECK(false, "conv2d_k3: variant ", variant, " (bf16 operand split / row-only Winograd) needs a library built with ESTD_BUILD_AB=1");
#endif
    } else if (variant == 3) {          // both image axes in Winograd form (w_alt = packing.pack_conv2d_wino2)
        d.w_wino = fptr(*w_alt, "2-axis Winograd-packed weights");
        check_status(estd_conv2d_k3_wino2(&d, cur_stream()), "estd_conv2d_k3_wino2");
    } else {
        TORCH_CHECK(variant == 0, "conv2d_k3: unknown variant ", variant);
        check_status(estd_conv2d_k3(&d, cur_stream()), "estd_conv2d_k3");
    }
    return out;
}

Tensor groupnorm_finalize(const Tensor& partials, int64_t n_blocks, double count, double eps)
{
    const OpScope scope(partials);
    TORCH_CHECK(partials.defined() && partials.is_cuda() && partials.scalar_type() == at::kDouble && partials.is_contiguous() &&
                partials.numel() >= n_blocks * 4,
                "groupnorm_finalize: partials must be a contiguous float64 ROCm tensor with 4 doubles per block");
    Tensor out = new_f32({4}, partials);
    ESTD_LAUNCH(estd_groupnorm_finalize, partials.data_ptr<double>(), (int)n_blocks, count, (float)eps, out.data_ptr<float>());
    return out;
}

// ------------------------------------------------------------------------------------------------ soft-argmin
std::tuple<Tensor, Tensor> softargmin_up(const Tensor& logits, const Tensor& depth_values, int64_t scale)
{
    const char* op = "softargmin_up";
    const OpScope scope(logits);
    const float* lg = map_ptr(logits, {-1, -1, -1, -1}, op, "logits");
    const int64_t N = logits.size(-4), D = logits.size(-3), H = logits.size(-2), W = logits.size(-1);
    const float* dv = floats_ptr(depth_values, D, op, "depth_values", true);
    Tensor depth = new_f32({N, 1, H * scale, W * scale}, logits);
    Tensor prob = at::empty_like(depth);
    ESTD_LAUNCH(estd_softargmin_up, lg, dv, depth.data_ptr<float>(), prob.data_ptr<float>(), (int)N, (int)D, (int)H, (int)W, (int)scale);
    return {depth, prob};
}

// ------------------------------------------------------------------------------------------------ EST fusion
// The body of warp_volume and warp_volume_ex: `launch` takes the checked pointers and sizes and passes the operator's own scalars on.
template <class Launch>
static Tensor warp_vol(const char* op, const char* what, const Tensor& vol, const Tensor& mats30, const Tensor& depth, bool depth_per_voxel,
                       Launch launch)
{
    const OpScope scope(vol);
    const float* v = map_ptr(vol, {-1, -1, -1, -1}, op, "vol");
    const int64_t C = vol.size(-4), D = vol.size(-3), H = vol.size(-2), W = vol.size(-1);
    const float* m = floats_ptr(mats30, 30, op, "mats30");
    const float* dv = floats_ptr(depth, depth_per_voxel ? D * H * W : D, op, "depth", true);
    Tensor out = at::empty_like(vol);
    check_status(launch(v, m, dv, out.data_ptr<float>(), (int)C, (int)D, (int)H, (int)W), what);
    return out;
}

Tensor warp_volume(const Tensor& vol, const Tensor& mats30, const Tensor& depth_values, double depth_min, double depth_interval)
{
    return warp_vol("warp_volume", "estd_warp_volume", vol, mats30, depth_values, false,
                    [&](const float* v, const float* m, const float* dv, float* out, int C, int D, int H, int W) {
                        return estd_warp_volume(v, m, dv, (float)depth_min, (float)depth_interval, out, C, D, H, W, cur_stream());
                    });
}

Tensor warp_volume_ex(const Tensor& vol, const Tensor& mats30, const Tensor& depth, bool depth_per_voxel, double depth_min,
                      double depth_interval, bool use_disp, double disp_min, double disp_interval, bool border, double padding_value)
{
    estd_warp_volume_opts o{};
    o.depth_per_voxel = depth_per_voxel; o.use_disp = use_disp; o.border = border;
    o.depth_min = (float)depth_min; o.depth_interval = (float)depth_interval;
    o.disp_min = (float)disp_min; o.disp_interval = (float)disp_interval; o.padding_value = (float)padding_value;
    return warp_vol("warp_volume_ex", "estd_warp_volume_ex", vol, mats30, depth, depth_per_voxel,
                    [&](const float* v, const float* m, const float* dv, float* out, int C, int D, int H, int W) {
                        return estd_warp_volume_ex(v, m, dv, &o, out, C, D, H, W, cur_stream());
                    });
}

// ------------------------------------------------------------------------------------------------ TSDF fusion (csrc/tsdf.hip)
// The body of tsdf_integrate_ and tsdf_integrate_color_.  Desc is the plain or the colour descriptor (the colour one begins with the plain
// one's fields) and `launch` the C entry point that takes it; `color` and `images` are read for the colour descriptor only.
template <class Desc>
static Tensor integrate(const char* op, int (*launch)(const Desc*, estd_stream_t), const char* what, Tensor volume, const Tensor& color,
                        at::TensorList depths, at::TensorList confs, at::TensorList images, const Tensor& mats, double trunc, double z_near,
                        double conf_min, bool weighted, double w_max, bool no_skip)
{
    const OpScope scope(volume);
    const VolumeArg v = check_volume(volume, op);
    const int64_t T = (int64_t)depths.size();
    TORCH_CHECK(T >= 1 && T <= ESTD_TSDF_MAX_FRAMES, op, ": 1..", ESTD_TSDF_MAX_FRAMES, " frames per call, got ", T);
    TORCH_CHECK(confs.empty() || (int64_t)confs.size() == T, op, ": one confidence map per depth map (or none)");
    TORCH_CHECK(!weighted || !confs.empty(), op, ": weighted fusion needs confidence maps");
    const float* m = host_values(mats, T * 12, op, "mats", "[T,12]");
    map_ptr(depths[0], {-1, -1}, op, "depth map");
    const int64_t H = depths[0].size(-2), W = depths[0].size(-1);
    Desc d{};
    d.Z = (int)v.Z; d.Y = (int)v.Y; d.X = (int)v.X; d.T = (int)T; d.H = (int)H; d.W = (int)W;
    d.weighted = weighted; d.no_skip = no_skip;
    d.trunc = (float)trunc; d.z_near = (float)z_near; d.conf_min = (float)conf_min; d.w_max = (float)w_max;
    d.tsdf = v.tsdf; d.weight = v.weight;
    for (int64_t t = 0; t < T; ++t) {
        d.depth[t] = map_ptr(depths[t], {H, W}, op, "depth map");
        if (!confs.empty()) d.conf[t] = map_ptr(confs[t], {H, W}, op, "confidence map");
        for (int i = 0; i < 12; ++i) d.mats[t][i] = m[t * 12 + i];
    }
    if constexpr (std::is_same_v<Desc, estd_tsdf_integrate_color_desc>) {
        d.color = check_color_planes(color, volume, op);
        TORCH_CHECK((int64_t)images.size() == T, op, ": one image per depth map, got ", images.size(), " for ", T);
        for (int64_t t = 0; t < T; ++t) d.image[t] = map_ptr(images[t], {3, H, W}, op, "image");
    }
    check_status(launch(&d, cur_stream()), what);
    return volume;
}

// volume [2,Z,Y,X]: plane 0 = D, plane 1 = Wt; in place.  mats: CPU float32 [T,12] (host values of the launch arguments).
Tensor tsdf_integrate_(Tensor volume, at::TensorList depths, at::TensorList confs, const Tensor& mats, double trunc, double z_near,
                       double conf_min, bool weighted, double w_max, bool no_skip)
{
    return integrate("tsdf_integrate_", estd_tsdf_integrate, "estd_tsdf_integrate", volume, Tensor(), depths, confs, {}, mats, trunc, z_near,
                     conf_min, weighted, w_max, no_skip);
}

// tsdf_integrate_ with colour: color [3,Z,Y,X] in place beside the volume; images: one [3,H,W] per depth map.
Tensor tsdf_integrate_color_(Tensor volume, Tensor color, at::TensorList depths, at::TensorList confs, at::TensorList images, const Tensor& mats,
                             double trunc, double z_near, double conf_min, bool weighted, double w_max, bool no_skip)
{
    return integrate("tsdf_integrate_color_", estd_tsdf_integrate_color, "estd_tsdf_integrate_color", volume, color, depths, confs, images, mats,
                     trunc, z_near, conf_min, weighted, w_max, no_skip);
}

// -> (count [1] int64 on the device = TOTAL crossings, xyz [capacity,3], normal [capacity,3], weight [capacity], edge [capacity] int64);
// capacity 0 counts only.  origin: CPU float32 [3].
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> tsdf_extract_points(const Tensor& volume, double voxel_size, const Tensor& origin,
                                                                       double w_min, int64_t capacity)
{
    const OpScope scope(volume);
    const VolumeArg v = check_volume(volume, "tsdf_extract_points");
    TORCH_CHECK(capacity >= 0, "tsdf_extract_points: capacity must not be negative");
    const float* org = host_values(origin, 3, "tsdf_extract_points", "origin", "[3]");
    Tensor count = at::zeros({1}, volume.options().dtype(at::kLong));
    Tensor xyz = new_f32({capacity, 3}, volume), normal = new_f32({capacity, 3}, volume), weight = new_f32({capacity}, volume);
    Tensor edge = at::empty({capacity}, volume.options().dtype(at::kLong));
    check_status(estd_tsdf_extract_points(v.tsdf, v.weight, (int)v.Z, (int)v.Y, (int)v.X, (float)voxel_size, org, (float)w_min,
                                          reinterpret_cast<unsigned long long*>(count.data_ptr<int64_t>()), (long long)capacity,
                                          capacity ? xyz.data_ptr<float>() : nullptr, capacity ? normal.data_ptr<float>() : nullptr,
                                          capacity ? weight.data_ptr<float>() : nullptr,
                                          capacity ? reinterpret_cast<long long*>(edge.data_ptr<int64_t>()) : nullptr, cur_stream()),
                 "estd_tsdf_extract_points");
    return {count, xyz, normal, weight, edge};
}

// The body of tsdf_raycast and tsdf_raycast_color, over the plain or the colour descriptor as in integrate() -> (depth, normal, weight and
// a fourth map: the colour of the colour call, the stats of the plain one).  n_steps is in 1..2^24, dt must be positive and finite as
// fp32, t_min finite and not negative, w_min not NaN.
template <class Desc>
static std::tuple<Tensor, Tensor, Tensor, Tensor> raycast(const char* op, int (*launch)(const Desc*, estd_stream_t), const char* what,
                                                          const Tensor& volume, const Tensor& color, const Tensor& mat, int64_t H, int64_t W,
                                                          double t_min, double dt, int64_t n_steps, double w_min, bool stats)
{
    const OpScope scope(volume);
    const VolumeArg v = check_volume(volume, op);
    const float* m = host_values(mat, 12, op, "mat", "[12] (3x4 row-major)");
    check_map_size(H, W, op, "the image");
    TORCH_CHECK(n_steps > 0 && n_steps <= (1 << 24), op, ": n_steps must be in 1..2^24, got ", n_steps);
    Desc d{};
    d.Z = (int)v.Z; d.Y = (int)v.Y; d.X = (int)v.X; d.H = (int)H; d.W = (int)W; d.n_steps = (int)n_steps;
    d.dt = positive_f32(dt, op, "dt"); d.t_min = not_negative_f32(t_min, op, "t_min"); d.w_min = not_nan_f32(w_min, op, "w_min");
    d.tsdf = v.tsdf; d.weight = v.weight;
    for (int i = 0; i < 12; ++i) d.mat[i] = m[i];
    Tensor fourth;
    if constexpr (std::is_same_v<Desc, estd_tsdf_raycast_color_desc>) {
        d.color = check_color_planes(color, volume, op);
        fourth = new_f32({H, W, 3}, volume);
        d.out_color = fourth.data_ptr<float>();
    } else {
        fourth = at::empty({stats ? H : 0, stats ? W : 0, stats ? 2 : 0}, volume.options().dtype(at::kInt));
        d.stats = stats ? reinterpret_cast<unsigned int*>(fourth.data_ptr<int32_t>()) : nullptr;
    }
    Tensor depth = new_f32({H, W}, volume), normal = new_f32({H, W, 3}, volume), weight = new_f32({H, W}, volume);
    d.depth = depth.data_ptr<float>(); d.normal = normal.data_ptr<float>(); d.out_weight = weight.data_ptr<float>();
    check_status(launch(&d, cur_stream()), what);
    return {depth, normal, weight, fourth};
}

// csrc/tsdf_raycast.hip: volume [2,Z,Y,X], mat: CPU float32 [12] (host values of the launch arguments) -> (depth [H,W], normal [H,W,3],
// weight [H,W], stats: int32 [H,W,2] when asked for (measurement only), else [0])
std::tuple<Tensor, Tensor, Tensor, Tensor> tsdf_raycast(const Tensor& volume, const Tensor& mat, int64_t H, int64_t W, double t_min, double dt,
                                                        int64_t n_steps, double w_min, bool stats)
{
    return raycast("tsdf_raycast", estd_tsdf_raycast, "estd_tsdf_raycast", volume, Tensor(), mat, H, W, t_min, dt, n_steps, w_min, stats);
}

// tsdf_raycast with a colour map -> (depth [H,W], normal [H,W,3], weight [H,W], color [H,W,3])
std::tuple<Tensor, Tensor, Tensor, Tensor> tsdf_raycast_color(const Tensor& volume, const Tensor& color, const Tensor& mat, int64_t H, int64_t W,
                                                              double t_min, double dt, int64_t n_steps, double w_min)
{
    return raycast("tsdf_raycast_color", estd_tsdf_raycast_color, "estd_tsdf_raycast_color", volume, color, mat, H, W, t_min, dt, n_steps, w_min,
                   false);
}

// edge: int64 [N] (the ids of tsdf_extract_points) -> colour at the crossings [N,3]
Tensor tsdf_edge_colors(const Tensor& volume, const Tensor& color, const Tensor& edge)
{
    const OpScope scope(volume);
    const VolumeArg v = check_volume(volume, "tsdf_edge_colors");
    const float* col = check_color_planes(color, volume, "tsdf_edge_colors");
    const int64_t* ids = lptr(edge, "tsdf_edge_colors", "edge", volume, -1);
    const int64_t n = edge.size(0);
    Tensor out = new_f32({n, 3}, volume);
    if (n)
        check_status(estd_tsdf_edge_colors(v.tsdf, col, (int)v.Z, (int)v.Y, (int)v.X, reinterpret_cast<const long long*>(ids), (long long)n,
                                           out.data_ptr<float>(), cur_stream()), "estd_tsdf_edge_colors");
    return out;
}

// ------------------------------------------------------------------------------------------------ surface nets
// csrc/mesh/tsdf_mesh.hip -> (count [1] int64 on the device = TOTAL vertices, cell [capacity] int64, xyz [capacity,3], normal [capacity,3],
// weight [capacity], colour [capacity,3] with colour planes, else [0,3]); capacity 0 counts only.  origin: CPU float32 [3].
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> tsdf_mesh_vertices(const Tensor& volume, const OptTensor& color, double voxel_size,
                                                                              const Tensor& origin, double w_min, int64_t capacity)
{
    const char* op = "tsdf_mesh_vertices";
    const OpScope scope(volume);
    const VolumeArg v = check_volume(volume, op, true);
    const bool has_color = color.has_value() && color->defined();
    const float* col = has_color ? check_color_planes(*color, volume, op) : nullptr;
    TORCH_CHECK(capacity >= 0, op, ": capacity must not be negative");
    const float voxel = positive_f32(voxel_size, op, "voxel_size"), wm = not_nan_f32(w_min, op, "w_min");
    const float* org = host_values(origin, 3, op, "origin", "[3]", true);
    Tensor count = at::zeros({1}, volume.options().dtype(at::kLong));
    Tensor cell = at::empty({capacity}, volume.options().dtype(at::kLong));
    Tensor xyz = new_f32({capacity, 3}, volume), normal = new_f32({capacity, 3}, volume), weight = new_f32({capacity}, volume);
    Tensor rgb = new_f32({has_color ? capacity : 0, 3}, volume);
    check_status(estd_tsdf_mesh_vertices(v.tsdf, v.weight, col, (int)v.Z, (int)v.Y, (int)v.X, voxel, org, wm,
                                         reinterpret_cast<unsigned long long*>(count.data_ptr<int64_t>()), (long long)capacity,
                                         capacity ? reinterpret_cast<long long*>(cell.data_ptr<int64_t>()) : nullptr,
                                         capacity ? xyz.data_ptr<float>() : nullptr, capacity ? normal.data_ptr<float>() : nullptr,
                                         capacity ? weight.data_ptr<float>() : nullptr,
                                         capacity && has_color ? rgb.data_ptr<float>() : nullptr, cur_stream()),
                 "estd_tsdf_mesh_vertices");
    return {count, cell, xyz, normal, weight, rgb};
}

// -> (count [1] int64 on the device = TOTAL quads, edge [capacity] int64, quad [capacity,4] int32: cell ids in winding order)
std::tuple<Tensor, Tensor, Tensor> tsdf_mesh_faces(const Tensor& volume, double w_min, int64_t capacity)
{
    const char* op = "tsdf_mesh_faces";
    const OpScope scope(volume);
    const VolumeArg v = check_volume(volume, op, true);
    TORCH_CHECK(capacity >= 0, op, ": capacity must not be negative");
    const float wm = not_nan_f32(w_min, op, "w_min");
    Tensor count = at::zeros({1}, volume.options().dtype(at::kLong));
    Tensor edge = at::empty({capacity}, volume.options().dtype(at::kLong));
    Tensor quad = at::empty({capacity, 4}, volume.options().dtype(at::kInt));
    check_status(estd_tsdf_mesh_faces(v.tsdf, v.weight, (int)v.Z, (int)v.Y, (int)v.X, wm,
                                      reinterpret_cast<unsigned long long*>(count.data_ptr<int64_t>()), (long long)capacity,
                                      capacity ? reinterpret_cast<long long*>(edge.data_ptr<int64_t>()) : nullptr,
                                      capacity ? quad.data_ptr<int32_t>() : nullptr, cur_stream()), "estd_tsdf_mesh_faces");
    return {count, edge, quad};
}

// ------------------------------------------------------------------------------------------------ mesh components
// a triangle list: int32 [F,3], contiguous, on a device
static const int32_t* faces_ptr(const Tensor& t, const char* op, const char* name)
{
    TORCH_CHECK(t.defined() && t.is_cuda() && t.scalar_type() == at::kInt && t.dim() == 2 && t.size(1) == 3 && t.is_contiguous(),
                op, ": ", name, " must be a contiguous int32 tensor [F,3] on a ROCm device");
    return t.data_ptr<int32_t>();
}

// csrc/mesh/mesh_components.hip -> (label [V] int32, triangles [V] int32, invalid [1] int64 on the device)
std::tuple<Tensor, Tensor, Tensor> mesh_components(const Tensor& faces, int64_t n_vertices)
{
    const char* op = "mesh_components";
    const int32_t* f = faces_ptr(faces, op, "faces");
    const OpScope scope(faces);
    check_count(n_vertices, 0, 0x7fffffffLL, op, "n_vertices");
    const int64_t n_faces = faces.size(0);
    Tensor label = at::empty({n_vertices}, faces.options()), triangles = at::empty({n_vertices}, faces.options());
    Tensor invalid = at::empty({1}, faces.options().dtype(at::kLong));
    check_status(estd_mesh_components(n_faces ? f : nullptr, (long long)n_faces, (long long)n_vertices,
                                      n_vertices ? label.data_ptr<int32_t>() : nullptr, n_vertices ? triangles.data_ptr<int32_t>() : nullptr,
                                      reinterpret_cast<long long*>(invalid.data_ptr<int64_t>()), cur_stream()), "estd_mesh_components");
    return {label, triangles, invalid};
}

// ------------------------------------------------------------------------------------------------ mesh sampling (csrc/mesh/mesh_sample.hip)
// the vertices float32 [V,3] and the triangles int32 [F,3] of one mesh on one device
static const float* check_cloud(const Tensor& t, const char* op, const char* name, int64_t cols);      // with the point clouds below
struct MeshArg { const float* xyz; const int32_t* faces; int64_t V, F; };
static MeshArg check_mesh(const Tensor& xyz, const Tensor& faces, const char* op)
{
    MeshArg m{};
    m.faces = faces_ptr(faces, op, "faces");
    m.xyz = check_cloud(xyz, op, "xyz", 3);
    TORCH_CHECK(xyz.device() == faces.device(), op, ": xyz is on ", xyz.device(), " but faces on ", faces.device());
    m.V = xyz.size(0); m.F = faces.size(0);
    return m;
}

static std::tuple<Tensor, Tensor, Tensor> face_area(const MeshArg& m, const Tensor& faces)
{
    Tensor area = at::empty({m.F}, faces.options().dtype(at::kDouble)), normal = at::empty({m.F, 3}, faces.options().dtype(at::kFloat));
    Tensor invalid = at::empty({1}, faces.options().dtype(at::kLong));
    check_status(estd_mesh_face_area(m.V ? m.xyz : nullptr, (long long)m.V, m.F ? m.faces : nullptr, (long long)m.F,
                                     m.F ? area.data_ptr<double>() : nullptr, m.F ? normal.data_ptr<float>() : nullptr,
                                     reinterpret_cast<long long*>(invalid.data_ptr<int64_t>()), cur_stream()), "estd_mesh_face_area");
    return {area, normal, invalid};
}

// -> (area [F] float64, face_normal [F,3], invalid [1] int64 on the device)
std::tuple<Tensor, Tensor, Tensor> mesh_face_area(const Tensor& xyz, const Tensor& faces)
{
    const OpScope scope(faces);
    return face_area(check_mesh(xyz, faces, "mesh_face_area"), faces);
}

// -> (xyz [N,3], face [N] int32, bary [N,2], normal [N,3], attrs [N,C] (C = 0 without), area [F] float64, invalid [1] int64); the glue
// between the two launches is the one of include/estd_hip.h, as in estdepth_amd/ops.py
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> mesh_sample(const Tensor& xyz, const Tensor& faces, const OptTensor& attrs,
                                                                               int64_t n_samples, int64_t seed)
{
    const char* op = "mesh_sample";
    const OpScope scope(faces);
    const MeshArg m = check_mesh(xyz, faces, op);
    int64_t C = 0;
    const float* att = nullptr;
    if (attrs.has_value() && attrs->defined()) {
        att = fptr(*attrs, "attrs", true, op);
        TORCH_CHECK(attrs->dim() == 2 && attrs->size(0) == m.V && attrs->size(1) >= 1 && attrs->size(1) <= ESTD_CLOUD_MAX_ATTRS,
                    op, ": attrs must be [", m.V, ",C] with 1 <= C <= ", ESTD_CLOUD_MAX_ATTRS);
        C = attrs->size(1);
    }
    check_count(n_samples, 0, 0x7fffffffLL, op, "n_samples");
    auto [area, face_normal, invalid] = face_area(m, faces);
    const int64_t n = m.F ? n_samples : 0;
    int64_t w = 0;
    Tensor cum;
    if (n) {
        const double amax = area.max().item<double>();
        TORCH_CHECK(std::isfinite(amax) && amax >= 0, "mesh_sample: xyz holds a coordinate that is not finite (the largest area is ", amax, ")");
        int e = 0, k = 0;
        if (amax > 0) {
            (void)std::frexp(amax, &k);
            int b = 0;
            while (((int64_t)1 << b) < m.F) ++b;
            e = std::min(1000, 62 - b - k);
        }
        cum = at::cumsum(at::floor(area * std::ldexp(1.0, e)).to(at::kLong), 0);
        const int64_t total = cum[m.F - 1].item<int64_t>();
        TORCH_CHECK(total > 0, "mesh_sample: the mesh has no area to put n_samples = ", n, " samples on");
        w = total / n;
        TORCH_CHECK(w >= ESTD_MESH_SAMPLE_MIN_STRATUM, "mesh_sample: n_samples = ", n, " leaves strata of ", w, " units of area, fewer than ",
                    ESTD_MESH_SAMPLE_MIN_STRATUM, ": too many samples for this mesh");
    }
    Tensor out_xyz = new_f32({n, 3}, xyz), face = at::empty({n}, faces.options()), bary = new_f32({n, 2}, xyz), normal = new_f32({n, 3}, xyz);
    Tensor out_attrs = new_f32({n, C}, xyz);
    if (n)
        check_status(estd_mesh_sample(m.xyz, (long long)m.V, m.faces, (long long)m.F, C ? att : nullptr, (int)C,
                                      reinterpret_cast<const long long*>(cum.data_ptr<int64_t>()), face_normal.data_ptr<float>(), (long long)n, 0LL,
                                      (long long)w, (unsigned long long)seed, out_xyz.data_ptr<float>(), face.data_ptr<int32_t>(),
                                      bary.data_ptr<float>(), normal.data_ptr<float>(), C ? out_attrs.data_ptr<float>() : nullptr, cur_stream()),
                     "estd_mesh_sample");
    return {out_xyz, face, bary, normal, out_attrs, area, invalid};
}

// ------------------------------------------------------------------------------------------------ mesh rasteriser (csrc/mesh/mesh_raster.hip)
// host values a kernel takes as float64: exactly n of them, all finite
static const double* host_doubles(const Tensor& t, int64_t n, const char* op, const char* name, const char* shape)
{
    TORCH_CHECK(t.defined() && t.device().is_cpu() && t.scalar_type() == at::kDouble && t.is_contiguous() && t.numel() == n,
                op, ": ", name, " must be a contiguous CPU float64 tensor ", shape);
    const double* v = t.data_ptr<double>();
    for (int64_t i = 0; i < n; ++i) TORCH_CHECK(std::isfinite(v[i]), op, ": ", name, " holds a value that is not finite");
    return v;
}

// mat: CPU float64 [12] -> (depth [H,W], face [H,W] int32, bary [H,W,2], facing [H,W] int32, invalid [1] int64 on the device); the key
// buffer lives here and is cleared by the first entry point with a memset on the stream
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> mesh_raster(const Tensor& xyz, const Tensor& faces, const Tensor& mat, int64_t H, int64_t W,
                                                               double z_near, bool preload)
{
    const char* op = "mesh_raster";
    const OpScope scope(faces);
    const MeshArg m = check_mesh(xyz, faces, op);
    const double* M = host_doubles(mat, 12, op, "mat", "[12] (3x4 row-major)");
    check_map_size(H, W, op, "the image");
    const float zn = not_negative_f32(z_near, op, "z_near");
    Tensor keys = at::empty({H, W}, faces.options().dtype(at::kLong));
    Tensor depth = new_f32({H, W}, xyz), face = at::empty({H, W}, faces.options()), bary = new_f32({H, W, 2}, xyz);
    Tensor facing = at::empty({H, W}, faces.options()), invalid = at::empty({1}, faces.options().dtype(at::kLong));
    const float* px = m.V ? m.xyz : nullptr;
    const int32_t* pf = m.F ? m.faces : nullptr;
    auto* k = reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>());
    check_status(estd_mesh_raster(px, (long long)m.V, pf, (long long)m.F, 0LL, (long long)m.F, M, (int)H, (int)W, zn,
                                  ESTD_MESH_RASTER_CLEAR | (preload ? ESTD_MESH_RASTER_PRELOAD : 0), k,
                                  reinterpret_cast<long long*>(invalid.data_ptr<int64_t>()), cur_stream()), "estd_mesh_raster");
    check_status(estd_mesh_raster_resolve(px, (long long)m.V, pf, (long long)m.F, M, (int)H, (int)W, k, depth.data_ptr<float>(),
                                          face.data_ptr<int32_t>(), bary.data_ptr<float>(), facing.data_ptr<int32_t>(), cur_stream()),
                 "estd_mesh_raster_resolve");
    return {depth, face, bary, facing, invalid};
}

// ------------------------------------------------------------------------------------------------ cross-view consistency
// csrc/depth_consistency.hip: target [H,W] and 1..8 sources of the same size, mats: CPU float32 [S,2,12] (F_s, B_s: host values of the
// launch arguments) -> (views, visible, depth, rel_err), each [H,W]
std::tuple<Tensor, Tensor, Tensor, Tensor> depth_consistency(const Tensor& target, at::TensorList sources, const Tensor& mats, double px_max,
                                                             double rel_max, double z_near)
{
    const char* op = "depth_consistency";
    const OpScope scope(target);
    estd_depth_consistency_desc d{};
    d.target = map_ptr(target, {-1, -1}, op, "target");
    const int64_t H = target.size(-2), W = target.size(-1);
    check_map_size(H, W, op, "maps", 2);
    const int64_t S = (int64_t)sources.size();
    TORCH_CHECK(S >= 1 && S <= ESTD_CONSISTENCY_MAX_SOURCES, "depth_consistency: 1..", ESTD_CONSISTENCY_MAX_SOURCES, " sources per call, got ", S);
    const float* m = host_values(mats, S * 24, op, "mats", "[S,2,12]", true);
    d.H = (int)H; d.W = (int)W; d.S = (int)S;
    d.px_max = positive_f32(px_max, op, "px_max"); d.rel_max = positive_f32(rel_max, op, "rel_max"); d.z_near = not_negative_f32(z_near, op, "z_near");
    for (int64_t s = 0; s < S; ++s) {
        d.source[s] = map_ptr(sources[s], {H, W}, op, "source");
        for (int i = 0; i < 24; ++i) d.mats[s][i / 12][i % 12] = m[s * 24 + i];
    }
    Tensor views = new_f32({H, W}, target), visible = new_f32({H, W}, target), depth = new_f32({H, W}, target), rel_err = new_f32({H, W}, target);
    d.views = views.data_ptr<float>(); d.visible = visible.data_ptr<float>(); d.depth = depth.data_ptr<float>(); d.rel_err = rel_err.data_ptr<float>();
    check_status(estd_depth_consistency(&d, cur_stream()), "estd_depth_consistency");
    return {views, visible, depth, rel_err};
}

// ------------------------------------------------------------------------------------------------ point clouds (csrc/cloud_nn.hip)
static const float* check_cloud(const Tensor& t, const char* op, const char* name, int64_t cols)
{
    const float* p = fptr(t, name);
    TORCH_CHECK(t.dim() == 2 && t.size(1) == cols && t.size(0) <= 0x7fffffffLL, op, ": ", name, " must be [n,", cols, "] with n < 2^31");
    return p;
}

static void check_cloud_grid(const Tensor& lo, double cell, at::IntArrayRef dims, const char* op, int64_t max_dim)
{
    host_values(lo, 3, op, "lo", "[3]", true);
    const float c = positive_f32(cell, op, "cell");
    TORCH_CHECK(std::isfinite(c) && std::isfinite(1.0f / c), op, ": cell must be finite in fp32 (and its reciprocal too), got ", cell);
    TORCH_CHECK(dims.size() == 3, op, ": dims must be three sizes");
    for (int j = 0; j < 3; ++j) TORCH_CHECK(dims[j] >= 1 && dims[j] <= max_dim, op, ": dims must be three sizes in 1..", max_dim, ", got ", dims[j]);
}

// points [n,3], lo: CPU float32 [3], dims: cells along x, y, z -> keys int64 [n]
Tensor cloud_cell_keys(const Tensor& points, const Tensor& lo, double cell, at::IntArrayRef dims)
{
    const OpScope scope(points);
    const float* pts = check_cloud(points, "cloud_cell_keys", "points", 3);
    check_cloud_grid(lo, cell, dims, "cloud_cell_keys", ESTD_CLOUD_KEY_MAX_DIM);
    const int64_t n = points.size(0);
    Tensor keys = at::empty({n}, points.options().dtype(at::kLong));
    const int d3[3] = {(int)dims[0], (int)dims[1], (int)dims[2]};
    if (n)
        check_status(estd_cloud_cell_keys(pts, (long long)n, lo.data_ptr<float>(), (float)cell, d3, reinterpret_cast<long long*>(keys.data_ptr<int64_t>()),
                                          cur_stream()), "estd_cloud_cell_keys");
    return keys;
}

// query [M,3], order int64 [M], records [N,4], cell_start int32 [cells + 1] -> (dist [M], index int64 [M], stats int32 [M] when asked
// for (measurement only), else [0])
std::tuple<Tensor, Tensor, Tensor> cloud_nearest(const Tensor& query, const Tensor& order, const Tensor& records, const Tensor& cell_start,
                                                 const Tensor& lo, double cell, at::IntArrayRef dims, double max_dist, bool stats)
{
    const char* op = "cloud_nearest";
    const OpScope scope(query);
    estd_cloud_nearest_desc d{};
    d.query = check_cloud(query, op, "query", 3);
    d.records = check_cloud(records, op, "records", 4);
    const int64_t M = query.size(0), N = records.size(0);
    d.order = reinterpret_cast<const long long*>(lptr(order, op, "order", query, M));
    d.max_dist = positive_square_f32(max_dist, op, "max_dist");
    check_cloud_grid(lo, cell, dims, op, ESTD_CLOUD_MAX_DIM);
    const int64_t cells = dims[0] * dims[1] * dims[2];
    TORCH_CHECK(cells <= ESTD_CLOUD_MAX_CELLS, "cloud_nearest: ", cells, " cells, at most ", ESTD_CLOUD_MAX_CELLS);
    d.cell_start = lptr<int32_t>(cell_start, op, "cell_start (cells + 1)", query, cells + 1);
    Tensor dist = new_f32({M}, query), index = at::empty({M}, query.options().dtype(at::kLong));
    Tensor st = at::empty({stats ? M : 0}, query.options().dtype(at::kInt));
    if (M) {
        d.M = (long long)M; d.N = (long long)N;
        d.dist = dist.data_ptr<float>(); d.index = reinterpret_cast<long long*>(index.data_ptr<int64_t>());
        d.stats = stats ? reinterpret_cast<unsigned int*>(st.data_ptr<int32_t>()) : nullptr;
        d.cell = (float)cell;
        for (int j = 0; j < 3; ++j) { d.lo[j] = lo.data_ptr<float>()[j]; d.dims[j] = (int)dims[j]; }
        check_status(estd_cloud_nearest(&d, cur_stream()), "estd_cloud_nearest");
    }
    return {dist, index, st};
}

// ------------------------------------------------------------------------------------------------ k nearest neighbours, normals (csrc/cloud/cloud_knn.hip)
// query [M,3], order int64 [M], records [N,4], cell_start int32 [cells + 1] -> (dist [M,k], index int32 [M,k], count int32 [M], stats
// int32 [M] when asked for (measurement only), else [0])
std::tuple<Tensor, Tensor, Tensor, Tensor> cloud_knn(const Tensor& query, const Tensor& order, const Tensor& records, const Tensor& cell_start,
                                                     const Tensor& lo, double cell, at::IntArrayRef dims, double max_dist, int64_t k, bool stats)
{
    const char* op = "cloud_knn";
    const OpScope scope(query);
    estd_cloud_knn_desc d{};
    d.query = check_cloud(query, op, "query", 3);
    d.records = check_cloud(records, op, "records", 4);
    const int64_t M = query.size(0), N = records.size(0);
    d.order = reinterpret_cast<const long long*>(lptr(order, op, "order", query, M));
    d.max_dist = positive_square_f32(max_dist, op, "max_dist");
    check_count(k, 1, ESTD_CLOUD_KNN_MAX, op, "k");
    check_cloud_grid(lo, cell, dims, op, ESTD_CLOUD_MAX_DIM);
    const int64_t cells = dims[0] * dims[1] * dims[2];
    TORCH_CHECK(cells <= ESTD_CLOUD_MAX_CELLS, "cloud_knn: ", cells, " cells, at most ", ESTD_CLOUD_MAX_CELLS);
    d.cell_start = lptr<int32_t>(cell_start, op, "cell_start (cells + 1)", query, cells + 1);
    Tensor dist = new_f32({M, k}, query), index = at::empty({M, k}, query.options().dtype(at::kInt));
    Tensor count = at::empty({M}, query.options().dtype(at::kInt));
    Tensor st = at::empty({stats ? M : 0}, query.options().dtype(at::kInt));
    if (M) {
        d.M = (long long)M; d.N = (long long)N; d.k = (int)k;
        d.dist = dist.data_ptr<float>(); d.index = index.data_ptr<int32_t>(); d.count = count.data_ptr<int32_t>();
        d.stats = stats ? reinterpret_cast<unsigned int*>(st.data_ptr<int32_t>()) : nullptr;
        d.cell = (float)cell;
        for (int j = 0; j < 3; ++j) { d.lo[j] = lo.data_ptr<float>()[j]; d.dims[j] = (int)dims[j]; }
        check_status(estd_cloud_knn(&d, cur_stream()), "estd_cloud_knn");
    }
    return {dist, index, count, st};
}

// ------------------------------------------------------------------------------------------------ clustering (csrc/cloud/cloud_cluster.hip)
// query [M,3], order int64 [M], records [N,4], cell_start int32 [cells + 1] -> count int32 [M]: the targets within `radius`
Tensor cloud_count_within(const Tensor& query, const Tensor& order, const Tensor& records, const Tensor& cell_start, const Tensor& lo, double cell,
                          at::IntArrayRef dims, double radius)
{
    const char* op = "cloud_count_within";
    const OpScope scope(query);
    estd_cloud_count_within_desc d{};
    d.query = check_cloud(query, op, "query", 3);
    d.records = check_cloud(records, op, "records", 4);
    const int64_t M = query.size(0), N = records.size(0);
    d.order = reinterpret_cast<const long long*>(lptr(order, op, "order", query, M));
    d.radius = positive_square_f32(radius, op, "radius");
    check_cloud_grid(lo, cell, dims, op, ESTD_CLOUD_MAX_DIM);
    const int64_t cells = dims[0] * dims[1] * dims[2];
    TORCH_CHECK(cells <= ESTD_CLOUD_MAX_CELLS, "cloud_count_within: ", cells, " cells, at most ", ESTD_CLOUD_MAX_CELLS);
    d.cell_start = lptr<int32_t>(cell_start, op, "cell_start (cells + 1)", query, cells + 1);
    Tensor count = at::empty({M}, query.options().dtype(at::kInt));
    if (M) {
        d.M = (long long)M; d.N = (long long)N;
        d.count = count.data_ptr<int32_t>();
        d.cell = (float)cell;
        for (int j = 0; j < 3; ++j) { d.lo[j] = lo.data_ptr<float>()[j]; d.dims[j] = (int)dims[j]; }
        check_status(estd_cloud_count_within(&d, cur_stream()), "estd_cloud_count_within");
    }
    return count;
}

// records [N,4], cell_start int32 [cells + 1] -> (label int32 [N], count int32 [N], size int32 [N], noise int32 [1])
std::tuple<Tensor, Tensor, Tensor, Tensor> cloud_dbscan(const Tensor& records, const Tensor& cell_start, const Tensor& lo, double cell,
                                                        at::IntArrayRef dims, double eps, int64_t min_points)
{
    const char* op = "cloud_dbscan";
    const OpScope scope(records);
    estd_cloud_dbscan_desc d{};
    d.records = check_cloud(records, op, "records", 4);
    const int64_t N = records.size(0);
    d.eps = positive_square_f32(eps, op, "eps");
    check_count(min_points, 1, 0x7fffffffLL, op, "min_points");
    check_cloud_grid(lo, cell, dims, op, ESTD_CLOUD_MAX_DIM);
    const int64_t cells = dims[0] * dims[1] * dims[2];
    TORCH_CHECK(cells <= ESTD_CLOUD_MAX_CELLS, "cloud_dbscan: ", cells, " cells, at most ", ESTD_CLOUD_MAX_CELLS);
    d.cell_start = lptr<int32_t>(cell_start, op, "cell_start (cells + 1)", records, cells + 1);
    const auto i32 = records.options().dtype(at::kInt);
    Tensor label = at::empty({N}, i32), count = at::empty({N}, i32), size = at::empty({N}, i32), parent = at::empty({N}, i32);
    Tensor noise = N ? at::empty({1}, i32) : at::zeros({1}, i32);
    if (N) {
        d.N = (long long)N; d.min_points = (int)min_points;
        d.count = count.data_ptr<int32_t>(); d.parent = parent.data_ptr<int32_t>(); d.label = label.data_ptr<int32_t>();
        d.size = size.data_ptr<int32_t>(); d.noise = noise.data_ptr<int32_t>();
        d.cell = (float)cell;
        for (int j = 0; j < 3; ++j) { d.lo[j] = lo.data_ptr<float>()[j]; d.dims[j] = (int)dims[j]; }
        check_status(estd_cloud_dbscan(&d, cur_stream()), "estd_cloud_dbscan");
    }
    return {label, count, size, noise};
}

// points [N,3], query [M,3], index int32 [M,k], count int32 [M], toward: nothing, [3] or [M,3] -> (normal [M,3], eig [M,3], valid uint8
// [M], invalid int64 [1], cov float64 [M,6] when asked for, else [0,6])
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> cloud_normals(const Tensor& points, const Tensor& query, const Tensor& index, const Tensor& count,
                                                                 const OptTensor& toward, bool cov)
{
    const char* op = "cloud_normals";
    const OpScope scope(points);
    const float* pts = check_cloud(points, op, "points", 3);
    const float* qs = check_cloud(query, op, "query", 3);
    const int64_t n = points.size(0), M = query.size(0);
    TORCH_CHECK(index.defined() && index.dim() == 2 && index.scalar_type() == at::kInt && index.is_contiguous() && index.device() == points.device() &&
                index.size(0) == M && index.size(1) >= 1 && index.size(1) <= ESTD_CLOUD_KNN_MAX,
                "cloud_normals: index must be a contiguous int32 [", M, ",k] with 1 <= k <= ", ESTD_CLOUD_KNN_MAX, " on the operator's device");
    const int32_t* cnt = lptr<int32_t>(count, op, "count", points, M);
    const float* tw = nullptr;
    int per_query = 0;
    if (toward.has_value() && toward->defined()) {
        tw = fptr(*toward, "toward", true, op);
        TORCH_CHECK((toward->dim() == 1 && toward->size(0) == 3) || (toward->dim() == 2 && toward->size(0) == M && toward->size(1) == 3),
                    "cloud_normals: toward must be [3] or [", M, ",3], got ", toward->sizes());
        per_query = toward->dim() == 2;
    }
    Tensor normal = new_f32({M, 3}, points), eig = new_f32({M, 3}, points);
    Tensor valid = at::empty({M}, points.options().dtype(at::kByte)), invalid = at::zeros({1}, points.options().dtype(at::kLong));
    Tensor c = at::empty({cov ? M : 0, 6}, points.options().dtype(at::kDouble));
    if (M)
        check_status(estd_cloud_normals(pts, (long long)n, qs, (long long)M, index.data_ptr<int32_t>(), cnt, (int)index.size(1), tw, per_query,
                                        normal.data_ptr<float>(), eig.data_ptr<float>(), valid.data_ptr<uint8_t>(),
                                        reinterpret_cast<long long*>(invalid.data_ptr<int64_t>()), cov ? c.data_ptr<double>() : nullptr, cur_stream()),
                     "estd_cloud_normals");
    return {normal, eig, valid, invalid, c};
}

// ------------------------------------------------------------------------------------------------ global registration (csrc/register/global_register.hip)
// a contiguous [rows, cols] (cols == 0: [rows]) tensor of type S on `like`'s device; rows < 0: any number below 2^31
template <class S>
static const S* check_table(const Tensor& t, const char* op, const char* name, const Tensor& like, int64_t rows, int64_t cols, const char* type)
{
    TORCH_CHECK(t.defined() && t.scalar_type() == c10::CppTypeToScalarType<S>::value && t.is_contiguous() && t.device() == like.device() &&
                t.dim() == (cols ? 2 : 1) && (rows < 0 ? t.size(0) <= 0x7fffffffLL : t.size(0) == rows) && (!cols || t.size(1) == cols),
                op, ": ", name, " must be a contiguous ", type, " [", rows < 0 ? "n" : std::to_string(rows).c_str(), cols ? "," : "",
                cols ? std::to_string(cols).c_str() : "", "] on the operator's device");
    return t.data_ptr<S>();
}

struct KnnLists { const float* points; const float* normal; const int32_t* index; const int32_t* count; int64_t n, k; };
// the cloud, its normals and estd_cloud_knn's lists over it, as the two descriptor operators take them
static KnnLists check_knn_lists(const Tensor& points, const Tensor& normal, const Tensor& index, const Tensor& count, const char* op)
{
    KnnLists a{};
    a.points = check_cloud(points, op, "points", 3);
    a.n = points.size(0);
    a.normal = check_table<float>(normal, op, "normal", points, a.n, 3, "float32");
    TORCH_CHECK(index.defined() && index.dim() == 2 && index.scalar_type() == at::kInt && index.is_contiguous() && index.device() == points.device() &&
                index.size(0) == a.n && index.size(1) >= 1 && index.size(1) <= ESTD_CLOUD_KNN_MAX,
                op, ": index must be a contiguous int32 [", a.n, ",k] with 1 <= k <= ", ESTD_CLOUD_KNN_MAX, " on the operator's device");
    a.index = index.data_ptr<int32_t>();
    a.k = index.size(1);
    a.count = check_table<int32_t>(count, op, "count", points, a.n, 0, "int32");
    return a;
}

// points [n,3], normal [n,3], index int32 [n,k], count int32 [n] -> (hist int32 [n,33], pairs int32 [n])
std::tuple<Tensor, Tensor> cloud_spfh(const Tensor& points, const Tensor& normal, const Tensor& index, const Tensor& count, bool oriented)
{
    const char* op = "cloud_spfh";
    const OpScope scope(points);
    const KnnLists a = check_knn_lists(points, normal, index, count, op);
    Tensor hist = at::empty({a.n, ESTD_FPFH_BINS}, points.options().dtype(at::kInt)), pairs = at::empty({a.n}, points.options().dtype(at::kInt));
    if (a.n)
        check_status(estd_cloud_spfh(a.points, a.normal, (long long)a.n, a.index, a.count, (int)a.k, oriented ? 1 : 0, hist.data_ptr<int32_t>(),
                                     pairs.data_ptr<int32_t>(), cur_stream()), "estd_cloud_spfh");
    return {hist, pairs};
}

// ... and hist, pairs -> (desc [n,33], valid uint8 [n], invalid int64 [1])
std::tuple<Tensor, Tensor, Tensor> cloud_fpfh(const Tensor& points, const Tensor& normal, const Tensor& index, const Tensor& count, const Tensor& hist,
                                              const Tensor& pairs)
{
    const char* op = "cloud_fpfh";
    const OpScope scope(points);
    const KnnLists a = check_knn_lists(points, normal, index, count, op);
    const int32_t* h = check_table<int32_t>(hist, op, "hist", points, a.n, ESTD_FPFH_BINS, "int32");
    const int32_t* pr = check_table<int32_t>(pairs, op, "pairs", points, a.n, 0, "int32");
    Tensor desc = new_f32({a.n, ESTD_FPFH_BINS}, points), valid = at::empty({a.n}, points.options().dtype(at::kByte));
    Tensor invalid = at::zeros({1}, points.options().dtype(at::kLong));
    if (a.n)
        check_status(estd_cloud_fpfh(a.points, a.normal, (long long)a.n, a.index, a.count, (int)a.k, h, pr, desc.data_ptr<float>(),
                                     valid.data_ptr<uint8_t>(), reinterpret_cast<long long*>(invalid.data_ptr<int64_t>()), cur_stream()),
                     "estd_cloud_fpfh");
    return {desc, valid, invalid};
}

// a [m,33], b [n,33], masks uint8 [m] / [n] or nothing -> (index int32 [m], d2 [m], d2_second [m])
std::tuple<Tensor, Tensor, Tensor> feature_match(const Tensor& a, const Tensor& b, const OptTensor& a_valid, const OptTensor& b_valid)
{
    const char* op = "feature_match";
    const OpScope scope(a);
    fptr(a, "a", true, op);
    const float* pa = check_table<float>(a, op, "a", a, -1, ESTD_FPFH_BINS, "float32");
    const float* pb = check_table<float>(b, op, "b", a, -1, ESTD_FPFH_BINS, "float32");
    const int64_t m = a.size(0), n = b.size(0);
    const uint8_t* va = (a_valid.has_value() && a_valid->defined()) ? check_table<uint8_t>(*a_valid, op, "a_valid", a, m, 0, "uint8") : nullptr;
    const uint8_t* vb = (b_valid.has_value() && b_valid->defined()) ? check_table<uint8_t>(*b_valid, op, "b_valid", a, n, 0, "uint8") : nullptr;
    Tensor index = at::empty({m}, a.options().dtype(at::kInt)), d2 = new_f32({m}, a), second = new_f32({m}, a);
    if (m)
        check_status(estd_feature_match(pa, (long long)m, pb, (long long)n, va, vb, index.data_ptr<int32_t>(), d2.data_ptr<float>(),
                                        second.data_ptr<float>(), cur_stream()), "estd_feature_match");
    return {index, d2, second};
}

// P [c,3], Q [c,3] -> (count int32 [H], status uint8 [H], ssq float64 [H], T float64 [H,12], best int64 [1]: the key of the header)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> ransac_pairs(const Tensor& P, const Tensor& Q, int64_t hypotheses, int64_t seed, double dist_max,
                                                                double edge_ratio)
{
    const char* op = "ransac_pairs";
    const OpScope scope(P);
    const float* p = check_cloud(P, op, "P", 3);
    const int64_t c = P.size(0);
    const float* q = check_table<float>(Q, op, "Q", P, c, 3, "float32");
    check_count(hypotheses, 0, 0x7fffffffLL, op, "hypotheses");
    TORCH_CHECK(std::isfinite(dist_max) && dist_max >= 0, op, ": dist_max must be finite and not negative, got ", dist_max);
    TORCH_CHECK(edge_ratio >= 0 && edge_ratio <= 1, op, ": edge_ratio must lie in 0 .. 1, got ", edge_ratio);
    const int64_t H = hypotheses;
    Tensor count = at::empty({H}, P.options().dtype(at::kInt)), status = at::empty({H}, P.options().dtype(at::kByte));
    Tensor ssq = at::empty({H}, P.options().dtype(at::kDouble)), T = at::empty({H, 12}, P.options().dtype(at::kDouble));
    Tensor best = at::zeros({1}, P.options().dtype(at::kLong));
    if (H)
        check_status(estd_ransac_pairs(p, q, (long long)c, (long long)H, (unsigned long long)seed, dist_max, edge_ratio, count.data_ptr<int32_t>(),
                                       status.data_ptr<uint8_t>(), ssq.data_ptr<double>(), T.data_ptr<double>(),
                                       reinterpret_cast<unsigned long long*>(best.data_ptr<int64_t>()), cur_stream()), "estd_ransac_pairs");
    return {count, status, ssq, T, best};
}

// ------------------------------------------------------------------------------------------------ point-to-mesh distance (csrc/mesh/mesh_distance.hip)
// the grid of the three operators: the rules of check_cloud_grid, at most ESTD_CLOUD_MAX_CELLS cells, big_cells not negative
static int64_t check_tri_grid(const Tensor& lo, double cell, at::IntArrayRef dims, int64_t big_cells, const char* op)
{
    check_cloud_grid(lo, cell, dims, op, ESTD_CLOUD_MAX_DIM);
    const int64_t cells = dims[0] * dims[1] * dims[2];
    TORCH_CHECK(cells <= ESTD_CLOUD_MAX_CELLS, op, ": ", cells, " cells, at most ", ESTD_CLOUD_MAX_CELLS);
    check_count(big_cells, 0, 0x7fffffffLL, op, "big_cells");
    return cells;
}

// -> (count [F] int32, flag [F] int32, invalid [1] int64 on the device)
std::tuple<Tensor, Tensor, Tensor> mesh_tri_bins(const Tensor& xyz, const Tensor& faces, const Tensor& lo, double cell, at::IntArrayRef dims,
                                                 int64_t big_cells)
{
    const char* op = "mesh_tri_bins";
    const OpScope scope(faces);
    const MeshArg m = check_mesh(xyz, faces, op);
    check_tri_grid(lo, cell, dims, big_cells, op);
    Tensor count = at::empty({m.F}, faces.options()), flag = at::empty({m.F}, faces.options());
    Tensor invalid = at::empty({1}, faces.options().dtype(at::kLong));
    const int d3[3] = {(int)dims[0], (int)dims[1], (int)dims[2]};
    check_status(estd_mesh_tri_bins(m.V ? m.xyz : nullptr, (long long)m.V, m.F ? m.faces : nullptr, (long long)m.F, lo.data_ptr<float>(), (float)cell,
                                    d3, (int)big_cells, m.F ? count.data_ptr<int32_t>() : nullptr, m.F ? flag.data_ptr<int32_t>() : nullptr,
                                    reinterpret_cast<long long*>(invalid.data_ptr<int64_t>()), cur_stream()), "estd_mesh_tri_bins");
    return {count, flag, invalid};
}

// offset int64 [F] (the exclusive prefix sum of count) -> (keys int64 [n_pairs], pair_face int32 [n_pairs])
std::tuple<Tensor, Tensor> mesh_tri_fill(const Tensor& xyz, const Tensor& faces, const Tensor& lo, double cell, at::IntArrayRef dims,
                                         int64_t big_cells, const Tensor& offset, int64_t n_pairs)
{
    const char* op = "mesh_tri_fill";
    const OpScope scope(faces);
    const MeshArg m = check_mesh(xyz, faces, op);
    check_tri_grid(lo, cell, dims, big_cells, op);
    const auto* off = reinterpret_cast<const long long*>(lptr(offset, op, "offset", faces, m.F));
    check_count(n_pairs, 0, ESTD_MESH_DISTANCE_MAX_PAIRS, op, "n_pairs");
    Tensor keys = at::empty({n_pairs}, faces.options().dtype(at::kLong)), pair_face = at::empty({n_pairs}, faces.options());
    const int d3[3] = {(int)dims[0], (int)dims[1], (int)dims[2]};
    if (n_pairs && m.F)
        check_status(estd_mesh_tri_fill(m.xyz, (long long)m.V, m.faces, (long long)m.F, lo.data_ptr<float>(), (float)cell, d3, (int)big_cells, off,
                                        (long long)n_pairs, reinterpret_cast<long long*>(keys.data_ptr<int64_t>()), pair_face.data_ptr<int32_t>(),
                                        cur_stream()), "estd_mesh_tri_fill");
    return {keys, pair_face};
}

// query [M,3], order int64 [M], big_records [B,12], records [P,12], cell_start int32 [cells + 1] -> (dist [M], face int32 [M],
// bary [M,2] and closest [M,3] when asked for, else [0,2] and [0,3])
std::tuple<Tensor, Tensor, Tensor, Tensor> mesh_nearest(const Tensor& query, const Tensor& order, const Tensor& big_records, const Tensor& records,
                                                        const Tensor& cell_start, const Tensor& lo, double cell, at::IntArrayRef dims,
                                                        double max_dist, bool bary, bool closest)
{
    const char* op = "mesh_nearest";
    const OpScope scope(query);
    estd_mesh_nearest_desc d{};
    d.query = check_cloud(query, op, "query", 3);
    d.big_records = check_cloud(big_records, op, "big_records", 12);
    d.records = check_cloud(records, op, "records", 12);
    const int64_t M = query.size(0), B = big_records.size(0), P = records.size(0);
    TORCH_CHECK(big_records.device() == query.device() && records.device() == query.device(), op, ": the records are not on the query's device");
    check_count(B, 0, ESTD_MESH_DISTANCE_MAX_PAIRS, op, "big records");
    check_count(P, 0, ESTD_MESH_DISTANCE_MAX_PAIRS, op, "records");
    d.order = reinterpret_cast<const long long*>(lptr(order, op, "order", query, M));
    d.max_dist = positive_square_f32(max_dist, op, "max_dist");
    const int64_t cells = check_tri_grid(lo, cell, dims, 0, op);
    d.cell_start = lptr<int32_t>(cell_start, op, "cell_start (cells + 1)", query, cells + 1);
    Tensor dist = new_f32({M}, query), face = at::empty({M}, query.options().dtype(at::kInt));
    Tensor bar = new_f32({bary ? M : 0, 2}, query), clo = new_f32({closest ? M : 0, 3}, query);
    if (M) {
        d.M = (long long)M; d.B = (long long)B; d.P = (long long)P;
        d.dist = dist.data_ptr<float>(); d.face = face.data_ptr<int32_t>();
        d.bary = bary ? bar.data_ptr<float>() : nullptr; d.closest = closest ? clo.data_ptr<float>() : nullptr;
        d.cell = (float)cell;
        for (int j = 0; j < 3; ++j) { d.lo[j] = lo.data_ptr<float>()[j]; d.dims[j] = (int)dims[j]; }
        check_status(estd_mesh_nearest(&d, cur_stream()), "estd_mesh_nearest");
    }
    return {dist, face, bar, clo};
}

// points [n,3], attrs [n,C] (C = 0: none), order int64 [n], segments int64 [K + 1] -> (points [K,3], attrs [K,C])
std::tuple<Tensor, Tensor> cloud_cell_centroids(const Tensor& points, const Tensor& attrs, const Tensor& order, const Tensor& segments)
{
    const char* op = "cloud_cell_centroids";
    const OpScope scope(points);
    const float* pts = check_cloud(points, op, "points", 3);
    const int64_t n = points.size(0);
    TORCH_CHECK(attrs.defined() && attrs.dim() == 2, "cloud_cell_centroids: attrs must be [n,C]");
    const int64_t C = attrs.size(1);
    const float* att = nullptr;
    if (C) {
        att = fptr(attrs, "attrs");
        TORCH_CHECK(attrs.size(0) == n && C <= ESTD_CLOUD_MAX_ATTRS, "cloud_cell_centroids: attrs must be [n,C] with C <= ", ESTD_CLOUD_MAX_ATTRS);
    }
    const int64_t* ord = lptr(order, op, "order", points, n);
    const int64_t* seg = lptr(segments, op, "segments", points, -1);
    TORCH_CHECK(segments.size(0) >= 1 && segments.size(0) <= n + 1, "cloud_cell_centroids: segments must be [K + 1] with K <= n");
    const int64_t K = segments.size(0) - 1;
    Tensor out = new_f32({K, 3}, points), out_attrs = new_f32({K, C}, points);
    if (K)
        check_status(estd_cloud_cell_centroids(pts, att, (int)C, (long long)n, reinterpret_cast<const long long*>(ord),
                                               reinterpret_cast<const long long*>(seg), (long long)K, out.data_ptr<float>(),
                                               C ? out_attrs.data_ptr<float>() : nullptr, cur_stream()), "estd_cloud_cell_centroids");
    return {out, out_attrs};
}

// ------------------------------------------------------------------------------------------------ mesh simplification (csrc/mesh/mesh_simplify.hip)
// the clusters of a mesh's vertices: int32 [V] on the faces' device, K of them, none without a vertex -> (V, K)
static const int32_t* check_clusters(const Tensor& cluster, int64_t n_clusters, const Tensor& faces, const char* op)
{
    const int32_t* c = lptr<int32_t>(cluster, op, "cluster", faces, -1);
    check_count(cluster.size(0), 0, 0x7fffffffLL, op, "the number of vertices");
    check_count(n_clusters, cluster.size(0) ? 1 : 0, cluster.size(0), op, "n_clusters");
    return c;
}

// faces [F,3] int32, cluster [V] int32 -> (corner [3F] int32, triple [F,3] int32, counts [2] int64 on the device: invalid, collapsed)
std::tuple<Tensor, Tensor, Tensor> mesh_cluster_faces(const Tensor& faces, const Tensor& cluster, int64_t n_clusters)
{
    const char* op = "mesh_cluster_faces";
    const int32_t* f = faces_ptr(faces, op, "faces");
    const OpScope scope(faces);
    const int32_t* c = check_clusters(cluster, n_clusters, faces, op);
    const int64_t F = faces.size(0), V = cluster.size(0);
    TORCH_CHECK(F <= 0x7fffffffLL / 3, op, ": at most ", 0x7fffffffLL / 3, " faces, got ", F);
    Tensor corner = at::empty({3 * F}, faces.options()), triple = at::empty({F, 3}, faces.options());
    Tensor counts = at::empty({2}, faces.options().dtype(at::kLong));
    check_status(estd_mesh_cluster_faces(F ? f : nullptr, (long long)F, (long long)V, V ? c : nullptr, (long long)n_clusters,
                                         F ? corner.data_ptr<int32_t>() : nullptr, F ? triple.data_ptr<int32_t>() : nullptr,
                                         reinterpret_cast<long long*>(counts.data_ptr<int64_t>()), cur_stream()), "estd_mesh_cluster_faces");
    if (F && !n_clusters) {                                   // without vertices every face is invalid; the entry point launched nothing
        corner.zero_();
        triple.fill_(-1);
        counts.select(0, 0).fill_(F);
    }
    return {corner, triple, counts};
}

// xyz [V,3], faces [F,3] int32, order int64 [3F], segments int64 [K + 1], cell_key int64 [K], mean [K,3], lo: CPU float32 [3] ->
// (xyz [K,3], normal [K,3], placed [K] bool)
std::tuple<Tensor, Tensor, Tensor> mesh_cluster_quadrics(const Tensor& xyz, const Tensor& faces, const Tensor& order, const Tensor& segments,
                                                         const Tensor& cell_key, const Tensor& mean, const Tensor& lo, double cell,
                                                         at::IntArrayRef dims, double reg)
{
    const char* op = "mesh_cluster_quadrics";
    const OpScope scope(faces);
    const MeshArg m = check_mesh(xyz, faces, op);
    TORCH_CHECK(m.F <= 0x7fffffffLL / 3, op, ": at most ", 0x7fffffffLL / 3, " faces, got ", m.F);
    const int64_t* ord = lptr(order, op, "order", faces, 3 * m.F);
    const int64_t* seg = lptr(segments, op, "segments", faces, -1);
    TORCH_CHECK(segments.size(0) >= 1 && segments.size(0) <= m.V + 1, op, ": segments must be [K + 1] with K <= ", m.V, " vertices");
    const int64_t K = segments.size(0) - 1;
    const int64_t* key = lptr(cell_key, op, "cell_key", faces, K);
    const float* mu = check_cloud(mean, op, "mean", 3);
    TORCH_CHECK(mean.size(0) == K && mean.device() == faces.device(), op, ": mean must be [", K, ",3] on the faces' device");
    check_cloud_grid(lo, cell, dims, op, ESTD_CLOUD_KEY_MAX_DIM);
    TORCH_CHECK(std::isfinite(reg) && reg >= 0, op, ": reg must be finite and not negative, got ", reg);
    Tensor out = new_f32({K, 3}, xyz), normal = new_f32({K, 3}, xyz), placed = at::empty({K}, faces.options().dtype(at::kBool));
    const int d3[3] = {(int)dims[0], (int)dims[1], (int)dims[2]};
    check_status(estd_mesh_cluster_quadrics(m.V ? m.xyz : nullptr, (long long)m.V, m.F ? m.faces : nullptr, (long long)m.F,
                                            m.F ? reinterpret_cast<const long long*>(ord) : nullptr, reinterpret_cast<const long long*>(seg),
                                            K ? reinterpret_cast<const long long*>(key) : nullptr, (long long)K, K ? mu : nullptr,
                                            lo.data_ptr<float>(), (float)cell, d3, reg, K ? out.data_ptr<float>() : nullptr,
                                            K ? normal.data_ptr<float>() : nullptr,
                                            K ? reinterpret_cast<unsigned char*>(placed.data_ptr<bool>()) : nullptr, cur_stream()),
                 "estd_mesh_cluster_quadrics");
    if (K && !m.F) {                                          // without faces: the means, zero normals, nothing placed; nothing was launched
        out.copy_(mean);
        normal.zero_();
        placed.zero_();
    }
    return {out, normal, placed};
}

// ------------------------------------------------------------------------------------------------ EST fusion: attention, ConvGRU glue
Tensor warp_attention(const Tensor& kv_target, at::TensorList kv_sources, const Tensor& mats, const Tensor& depth_values,
                      double depth_min, double depth_interval)
{
    const char* op = "warp_attention";
    const OpScope scope(kv_target);
    const float* kv = map_ptr(kv_target, {-1, -1, -1, 32}, op, "kv_target");
    const int64_t D = kv_target.size(-4), H = kv_target.size(-3), W = kv_target.size(-2), n = (int64_t)kv_sources.size();
    check_count(n, 1, ESTD_MAX_ATTENTION_SOURCES, op, "kv_sources");
    const std::vector<const float*> srcs = like_ptrs(kv_sources, kv_target, op, "kv_sources");
    const float* m = floats_ptr(mats, n * 30, op, "mats");
    const float* dv = floats_ptr(depth_values, D, op, "depth_values", true);
    Tensor xh = at::empty_like(kv_target);
    ESTD_LAUNCH(estd_warp_attention, kv, srcs.data(), m, (int)n, dv, (float)depth_min, (float)depth_interval, xh.data_ptr<float>(), (int)D, (int)H,
                (int)W);
    return xh;
}

Tensor attention_prewarped(const Tensor& kv_target, at::TensorList kv_sources)
{
    const char* op = "attention_prewarped";
    const OpScope scope(kv_target);
    const int64_t n_vox = records(kv_target, op, "kv_target"), n = (int64_t)kv_sources.size();
    check_count(n, 1, ESTD_MAX_ATTENTION_SOURCES, op, "kv_sources");
    const std::vector<const float*> srcs = like_ptrs(kv_sources, kv_target, op, "kv_sources");
    Tensor xh = at::empty_like(kv_target);
    ESTD_LAUNCH(estd_attention_prewarped, kv_target.data_ptr<float>(), srcs.data(), (int)n, xh.data_ptr<float>(), n_vox);
    return xh;
}

Tensor gru_reset_apply(const Tensor& xh, const Tensor& ru, const Tensor& stats4, const Tensor& gamma_r, const Tensor& beta_r)
{
    const char* op = "gru_reset_apply";
    const OpScope scope(xh);
    const int64_t n_vox = records(xh, op, "xh");
    const float *x = xh.data_ptr<float>(), *r = floats_ptr(ru, n_vox * 32, op, "ru");
    const float *st = floats_ptr(stats4, 4, op, "stats4"), *ga = floats_ptr(gamma_r, 16, op, "gamma_r"), *be = floats_ptr(beta_r, 16, op, "beta_r");
    Tensor xrh = at::empty_like(xh);
    ESTD_LAUNCH(estd_gru_reset_apply, x, r, st, ga, be, xrh.data_ptr<float>(), n_vox);
    return xrh;
}

void gru_blend(const Tensor& xh, const Tensor& ru, const Tensor& o_raw, const Tensor& stats_ru, const Tensor& stats_o,
               const Tensor& gamma_u, const Tensor& beta_u, const Tensor& gamma_o, const Tensor& beta_o, Tensor out_value, int64_t out_stride)
{
    const char* op = "gru_blend";
    const OpScope scope(xh);
    const int64_t n_vox = records(xh, op, "xh");
    const float *x = xh.data_ptr<float>(), *r = floats_ptr(ru, n_vox * 32, op, "ru"), *o = floats_ptr(o_raw, n_vox * 16, op, "o_raw");
    const float *sr = floats_ptr(stats_ru, 4, op, "stats_ru"), *so = floats_ptr(stats_o, 4, op, "stats_o");
    const float *gu = floats_ptr(gamma_u, 16, op, "gamma_u"), *bu = floats_ptr(beta_u, 16, op, "beta_u");
    const float *go = floats_ptr(gamma_o, 16, op, "gamma_o"), *bo = floats_ptr(beta_o, 16, op, "beta_o");
    const float* out = floats_ptr(out_value, (n_vox - 1) * out_stride + 16, op, "out_value", true, true);
    ESTD_LAUNCH(estd_gru_blend, x, r, o, sr, so, gu, bu, go, bo, mut(out), (int)out_stride, n_vox);
}

// ------------------------------------------------------------------------------------------------ 2D backbone epilogues, layouts
Tensor bn_act_nhwc_(Tensor x, const Tensor& scale, const Tensor& shift, bool relu, const OptTensor& residual)
{
    const char* op = "bn_act_nhwc_";
    const OpScope scope(x);
    float* xp = channels_last_ptr(x, op, "x");
    const int64_t n = x.size(0), c = x.size(1), h = x.size(2), w = x.size(3);
    const float *sc = floats_ptr(scale, c, op, "scale"), *sh = floats_ptr(shift, c, op, "shift");
    const float* res = (residual.has_value() && residual->defined()) ? channels_last_ptr(*residual, op, "residual", &x) : nullptr;
    ESTD_LAUNCH(estd_bn_act_nhwc, xp, sc, sh, res, relu ? 1 : 0, n * h * w, (int)c);
    return x;
}

Tensor spp_upsample_cat(const Tensor& raw, const Tensor& skip, at::TensorList branches)
{
    const char* op = "spp_upsample_cat";
    const OpScope scope(raw);
    const float* rp = map_ptr(raw, {-1, -1, -1, -1}, op, "raw");
    const int64_t n = raw.size(-4), h = raw.size(-3), w = raw.size(-2), cr = raw.size(-1), nb = (int64_t)branches.size();
    const float* sp = map_ptr(skip, {n, h, w, -1}, op, "skip");
    const int64_t cs = skip.size(-1);
    check_count(nb, 1, 4, op, "branches");
    std::vector<const float*> ptrs(nb);
    std::vector<int> bh(nb), bw(nb);
    int64_t cb = -1;                                           // the first branch's channel count is every branch's
    for (int64_t k = 0; k < nb; ++k) {
        const std::string item = "branches[" + std::to_string(k) + "]";
        ptrs[k] = map_ptr(branches[k], {n, -1, -1, cb}, op, item.c_str());
        bh[k] = (int)branches[k].size(-3); bw[k] = (int)branches[k].size(-2); cb = branches[k].size(-1);
    }
    Tensor out = new_f32({n, h, w, cr + cs + nb * cb}, raw);
    ESTD_LAUNCH(estd_spp_upsample_cat, rp, (int)cr, sp, (int)cs, ptrs.data(), bh.data(), bw.data(), (int)nb, (int)cb, out.data_ptr<float>(), (int)n,
                (int)h, (int)w);
    return out;
}

// The body of conv1x1_nhwc and conv2d_taps_nhwc: `d` arrives with the operator's own fields (stride; ksize, pad) set, `w_tail` are the
// weight's sizes around cout ([cout,cin] / [k*k,cout,cin]: cout is w.size(-2)), ho x wo the output map.
template <class Desc>
static Tensor desc_conv(const char* op, int (*launch)(const Desc*, estd_stream_t), const char* what, Desc d, const Tensor& x, const Tensor& w,
                        at::IntArrayRef w_tail, int64_t ho, int64_t wo, const OptTensor& scale, const OptTensor& shift, bool relu,
                        const OptTensor& residual)
{
    d.w = map_ptr(w, w_tail, op, "w");
    const int64_t n = x.size(-4), cout = w.size(-2);
    d.N = (int)n; d.H = (int)x.size(-3); d.W = (int)x.size(-2); d.cin = (int)x.size(-1); d.cout = (int)cout; d.relu = relu ? 1 : 0;
    d.in = x.data_ptr<float>();
    d.scale = opt_floats_ptr(scale, cout, op, "scale"); d.shift = opt_floats_ptr(shift, cout, op, "shift");
    if (residual.has_value() && residual->defined()) d.residual = map_ptr(*residual, {n, ho, wo, cout}, op, "residual");
    Tensor out = new_f32({n, ho, wo, cout}, x);
    d.out = out.data_ptr<float>();
    check_status(launch(&d, cur_stream()), what);
    return out;
}

Tensor conv1x1_nhwc(const Tensor& x, const Tensor& w2, const OptTensor& scale, const OptTensor& shift, int64_t stride, bool relu,
                    const OptTensor& residual)
{
    const char* op = "conv1x1_nhwc";
    const OpScope scope(x);
    map_ptr(x, {-1, -1, -1, -1}, op, "x");
    check_count(stride, 1, 2, op, "stride");
    estd_conv1x1_desc d{};
    d.stride = (int)stride;
    return desc_conv(op, estd_conv1x1_nhwc, "estd_conv1x1_nhwc", d, x, w2, {-1, x.size(-1)}, (x.size(-3) - 1) / stride + 1,
                     (x.size(-2) - 1) / stride + 1, scale, shift, relu, residual);
}

Tensor conv2d_taps_nhwc(const Tensor& x, const Tensor& w_taps, const OptTensor& scale, const OptTensor& shift, int64_t ksize, int64_t stride,
                        int64_t pad, bool relu, const OptTensor& residual)
{
    const char* op = "conv2d_taps_nhwc";
    const OpScope scope(x);
    map_ptr(x, {-1, -1, -1, -1}, op, "x");
    check_count(stride, 1, 2, op, "stride");
    estd_conv2d_taps_desc d{};
    d.ksize = (int)ksize; d.stride = (int)stride; d.pad = (int)pad;
    return desc_conv(op, estd_conv2d_taps_nhwc, "estd_conv2d_taps_nhwc", d, x, w_taps, {ksize * ksize, -1, x.size(-1)},
                     (x.size(-3) + 2 * pad - ksize) / stride + 1, (x.size(-2) + 2 * pad - ksize) / stride + 1, scale, shift, relu, residual);
}

// The body of the four "NHWC in, packed weights, scale / shift [cout], NHWC out" convolutions: x and the weights `w` have been checked,
// `launch` takes the five pointers and passes the operator's own sizes on.
template <class Launch>
static Tensor packed_conv(const char* op, const char* what, const Tensor& x, const float* w, const Tensor& scale, const Tensor& shift,
                          at::IntArrayRef out_shape, Launch launch)
{
    const float *sc = floats_ptr(scale, out_shape[3], op, "scale"), *sh = floats_ptr(shift, out_shape[3], op, "shift");
    Tensor out = new_f32(out_shape, x);
    check_status(launch(x.data_ptr<float>(), w, sc, sh, out.data_ptr<float>()), what);
    return out;
}

Tensor stem7x7s2_nhwc(const Tensor& x, const Tensor& w_packed, const Tensor& scale, const Tensor& shift)
{
    const char* op = "stem7x7s2_nhwc";
    const OpScope scope(x);
    map_ptr(x, {-1, -1, -1, 3}, op, "x");
    const int n = (int)x.size(-4), h = (int)x.size(-3), w = (int)x.size(-2);
    return packed_conv(op, "estd_stem7x7s2_nhwc", x, floats_ptr(w_packed, 7 * 6 * 4 * 64, op, "w_packed"), scale, shift,
                       {n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, 64},
                       [&](auto... p) { return estd_stem7x7s2_nhwc(p..., n, h, w, cur_stream()); });
}

Tensor stem3x3s2_nhwc(const Tensor& x, const Tensor& weight, const Tensor& scale, const Tensor& shift)
{
    const char* op = "stem3x3s2_nhwc";
    const OpScope scope(x);
    map_ptr(x, {-1, -1, -1, 3}, op, "x");
    const int n = (int)x.size(-4), h = (int)x.size(-3), w = (int)x.size(-2);
    return packed_conv(op, "estd_stem3x3s2_nhwc", x, map_ptr(weight, {32, 3, 3, 3}, op, "weight"), scale, shift,
                       {n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, 32},
                       [&](auto... p) { return estd_stem3x3s2_nhwc(p..., n, h, w, cur_stream()); });
}

Tensor conv2d_small_nhwc(const Tensor& x, const Tensor& w_packed, const Tensor& scale, const Tensor& shift, int64_t cout, int64_t ksize,
                         int64_t stride, bool relu)
{
    const char* op = "conv2d_small_nhwc";
    const OpScope scope(x);
    map_ptr(x, {-1, -1, -1, -1}, op, "x");
    const int64_t n = x.size(-4), h = x.size(-3), w = x.size(-2), cin = x.size(-1);
    // (the weight count below divides by these)
    TORCH_CHECK((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2) && cout > 0 && cout % 16 == 0 && cin % 16 == 0,
                "conv2d_small_nhwc: ksize 1|3, stride 1|2, the channel counts of x and cout multiples of 16");
    const float* wp = floats_ptr(w_packed, cout / 16 * ksize * ksize * (cin / 16) * 256, op, "w_packed");
    const int64_t pad = ksize / 2;
    return packed_conv(op, "estd_conv2d_small_nhwc", x, wp, scale, shift, {n, (h + 2 * pad - ksize) / stride + 1, (w + 2 * pad - ksize) / stride + 1, cout},
                       [&](auto... p) {
                           return estd_conv2d_small_nhwc(p..., (int)n, (int)h, (int)w, (int)cin, (int)cout, (int)ksize, (int)stride, relu ? 1 : 0,
                                                         cur_stream());
                       });
}

Tensor conv2d_k3_to16_nhwc(const Tensor& x, const Tensor& w_packed, const Tensor& scale, const Tensor& shift, bool upsample)
{
    const char* op = "conv2d_k3_to16_nhwc";
    const OpScope scope(x);
    map_ptr(x, {-1, -1, -1, -1}, op, "x");
    const int64_t n = x.size(-4), c = x.size(-1), h = (upsample ? 2 : 1) * x.size(-3), w = (upsample ? 2 : 1) * x.size(-2);
    TORCH_CHECK(c == 16 || c == 32, "conv2d_k3_to16_nhwc: x must have 16 or 32 channels, got ", c);      // (the weight count depends on it)
    const float* wp = floats_ptr(w_packed, 9 * (c / 16) * 256, op, "w_packed");
    return packed_conv(op, "estd_conv2d_k3_to16_nhwc", x, wp, scale, shift, {n, h, w, 16}, [&](auto... p) {
        return estd_conv2d_k3_to16_nhwc(p..., (int)n, (int)h, (int)w, (int)c, upsample ? 1 : 0, cur_stream());
    });
}

Tensor maxpool3x3s2_nhwc(const Tensor& x)
{
    const OpScope scope(x);
    const float* xp = map_ptr(x, {-1, -1, -1, -1}, "maxpool3x3s2_nhwc", "x");
    const int64_t n = x.size(-4), h = x.size(-3), w = x.size(-2), c = x.size(-1);
    Tensor out = new_f32({n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, c}, x);
    ESTD_LAUNCH(estd_maxpool3x3s2_nhwc, xp, out.data_ptr<float>(), (int)n, (int)h, (int)w, (int)c);
    return out;
}

Tensor avgpool_nhwc(const Tensor& x, int64_t k)
{
    const OpScope scope(x);
    const float* xp = map_ptr(x, {-1, -1, -1, -1}, "avgpool_nhwc", "x");
    const int64_t n = x.size(-4), h = x.size(-3), w = x.size(-2), c = x.size(-1);
    check_count(k, 1, std::min(h, w), "avgpool_nhwc", "k");                      // (the output size divides by it)
    Tensor out = new_f32({n, h / k, w / k, c}, x);
    ESTD_LAUNCH(estd_avgpool_nhwc, xp, out.data_ptr<float>(), (int)n, (int)h, (int)w, (int)c, (int)k);
    return out;
}

Tensor normalise_nhwc(const Tensor& imgs)
{
    const OpScope scope(imgs);
    const float* in = map_ptr(imgs, {-1, 3, -1, -1}, "normalise_nhwc", "imgs");
    const int64_t n = imgs.size(-4), h = imgs.size(-2), w = imgs.size(-1);
    Tensor out = new_f32({n, h, w, 3}, imgs);
    ESTD_LAUNCH(estd_normalise_nhwc, in, out.data_ptr<float>(), (int)n, h * w);
    return out;
}

Tensor nhwc_to_planes(const Tensor& x)
{
    const OpScope scope(x);
    const float* xp = map_ptr(x, {-1, -1, -1, -1}, "nhwc_to_planes", "x");
    const int64_t n = x.size(-4), h = x.size(-3), w = x.size(-2), c = x.size(-1);
    Tensor out = new_f32({n, c, h, w}, x);
    ESTD_LAUNCH(estd_nhwc_to_planes, xp, (int)c, out.data_ptr<float>(), (int)n, h * w);
    return out;
}

Tensor planes_cat_nhwc(const Tensor& a, const Tensor& b, bool relu_b)
{
    const char* op = "planes_cat_nhwc";
    const OpScope scope(a);
    const float* ap = map_ptr(a, {-1, -1, -1, -1}, op, "a");
    const int64_t n = a.size(-4), ca = a.size(-3), h = a.size(-2), w = a.size(-1);
    const float* bp = map_ptr(b, {n, -1, h, w}, op, "b");
    const int64_t cb = b.size(-3);
    Tensor out = new_f32({n, h, w, ca + cb}, a);
    ESTD_LAUNCH(estd_planes_cat_nhwc, ap, (int)ca, bp, (int)cb, relu_b ? 1 : 0, out.data_ptr<float>(), (int)n, h * w);
    return out;
}

Tensor upsample2_cat_nhwc(const Tensor& x, const Tensor& skip)
{
    const char* op = "upsample2_cat_nhwc";
    const OpScope scope(x);
    const float* xp = map_ptr(x, {-1, -1, -1, -1}, op, "x");
    const int64_t n = x.size(-4), h = 2 * x.size(-3), w = 2 * x.size(-2), cx = x.size(-1);
    const float* sp = map_ptr(skip, {n, h, w, -1}, op, "skip");
    const int64_t cs = skip.size(-1);
    Tensor out = new_f32({n, h, w, cx + cs}, x);
    ESTD_LAUNCH(estd_upsample2_cat_nhwc, xp, (int)cx, sp, (int)cs, out.data_ptr<float>(), (int)n, (int)h, (int)w);
    return out;
}

Tensor disp_head_nhwc(const Tensor& x, const Tensor& weight, const Tensor& bias, double depth_max, int64_t upscale)
{
    const char* op = "disp_head_nhwc";
    const OpScope scope(x);
    const float* xp = map_ptr(x, {-1, -1, -1, -1}, op, "x");
    const int64_t n = x.size(-4), h = x.size(-3), w = x.size(-2), c = x.size(-1);
    const float *wp = map_ptr(weight, {1, c, 3, 3}, op, "weight"), *bp = floats_ptr(bias, 1, op, "bias");
    Tensor out = new_f32({n, 1, upscale * h, upscale * w}, x);
    ESTD_LAUNCH(estd_disp_head_nhwc, xp, wp, bp, (float)depth_max, out.data_ptr<float>(), (int)n, (int)h, (int)w, (int)c, (int)upscale);
    return out;
}

// ------------------------------------------------------------------------------------------------ layout converters
void cdhw_to_vol(const Tensor& src, Tensor dst, int64_t dst_stride, int64_t dst_off)
{
    const char* op = "cdhw_to_vol";
    const OpScope scope(src);
    const float* sp = fptr(src, "src", true, op);
    TORCH_CHECK(src.dim() >= 2 && src.size(0) >= 1, op, ": src must be [C, ...] with C >= 1, got ", src.sizes());
    const int64_t C = src.size(0), S = src.numel() / C;
    check_count(dst_off, 0, dst_stride, op, "dst_off");                      // (estd_cdhw_to_vol checks its upper end only)
    const float* dp = floats_ptr(dst, S * dst_stride, op, "dst", true, true);
    ESTD_LAUNCH(estd_cdhw_to_vol, sp, mut(dp), (int)C, S, (int)dst_stride, (int)dst_off);
}

Tensor vol_to_cdhw(const Tensor& src, int64_t C, at::IntArrayRef dims, int64_t src_stride, int64_t src_off)
{
    const char* op = "vol_to_cdhw";
    const OpScope scope(src);
    check_count((int64_t)dims.size(), 3, 3, op, "dims");
    const int64_t S = dims[0] * dims[1] * dims[2];
    check_count(src_off, 0, src_stride, op, "src_off");                      // (estd_vol_to_cdhw checks its upper end only)
    const float* sp = floats_ptr(src, S * src_stride, op, "src", true, true);
    Tensor out = new_f32({C, dims[0], dims[1], dims[2]}, src);
    ESTD_LAUNCH(estd_vol_to_cdhw, sp, out.data_ptr<float>(), (int)C, S, (int)src_stride, (int)src_off);
    return out;
}

// ------------------------------------------------------------------------------------------------ camera algebra on the HOST
// The reference composes its camera matrices with torch.inverse / torch.matmul on [B,4,4] CPU tensors (model_hybrid.py:74-88,
// homo_utils.py:469-471, hybrid_depth_decoder.py:235, homo_utils.py:51,:258).  These matrices decide which samples fall across
// the discontinuous |norm| > 1 masks, so the product evaluates them with the SAME ATen CPU kernels, shapes and association
// order -- bit-identical matrices (estdepth_amd/camera.py is the line-by-line Python statement of this function; a CPU test
// asserts equality).  One call per forward from C++ instead of ~40 Python-dispatched ATen calls (0.4 ms -> 0.06 ms of host
// time during which the GPU would idle behind the D2H copy of the poses).
std::tuple<Tensor, Tensor> camera_matrices_host(const Tensor& cam_poses, const Tensor& cam_intr_q, at::TensorList pre_poses, bool with_volume)
{
    TORCH_CHECK(cam_poses.device().is_cpu() && cam_intr_q.device().is_cpu(), "camera_matrices_host: CPU tensors expected (copy the poses once)");
    TORCH_CHECK(cam_poses.dim() == 4 && cam_poses.size(0) == 1 && cam_poses.size(2) == 4 && cam_poses.size(3) == 4 && cam_poses.size(1) >= 3,
                "camera_matrices_host: cam_poses must be [1,V,4,4] with V >= 3");
    TORCH_CHECK(cam_intr_q.sizes() == at::IntArrayRef({1, 3, 3}), "camera_matrices_host: cam_intr must be [1,3,3]");
    using namespace at::indexing;
    const Tensor poses = cam_poses.to(at::kFloat), K = cam_intr_q.to(at::kFloat);
    const int64_t V = poses.size(1), T = V - 2;
    auto view_proj = [&](int64_t v) {
        Tensor extrinsic = at::inverse(poses.index({Slice(), v, Slice(), Slice()}));                   // model_hybrid.py:74,:83
        Tensor proj = extrinsic.clone();
        proj.index_put_({Slice(), Slice(None, 3), Slice(None, 4)},
                        at::matmul(K, extrinsic.index({Slice(), Slice(None, 3), Slice(None, 4)})));    // :87-88
        return proj;
    };
    Tensor sweep = at::empty({T, 2, 12}, poses.options());
    for (int64_t t = 0; t < T; ++t) {
        const Tensor ref_inv = at::inverse(view_proj(t + 1));
        const int64_t srcs[2] = {t, t + 2};
        for (int k = 0; k < 2; ++k) {
            const Tensor pr = at::matmul(view_proj(srcs[k]), ref_inv);                                 // homo_utils.py:469
            sweep.index_put_({t, k, Slice(None, 9)}, pr.index({0, Slice(None, 3), Slice(None, 3)}).reshape({9}));   // :470
            sweep.index_put_({t, k, Slice(9, None)}, pr.index({0, Slice(None, 3), 3}));                              // :471
        }
    }
    Tensor vol;
    if (with_volume) {
        std::vector<Tensor> P;
        for (int64_t t = 0; t < T; ++t) P.push_back(poses.index({Slice(), t + 1}).reshape({1, 4, 4}));
        for (const Tensor& p : pre_poses) {
            TORCH_CHECK(p.device().is_cpu() && p.numel() == 16, "camera_matrices_host: memory poses must be CPU [1,4,4] tensors");
            P.push_back(p.to(at::kFloat).reshape({1, 4, 4}));
        }
        const int64_t n = (int64_t)P.size();
        TORCH_CHECK(n >= 2, "camera_matrices_host: the EST fusion needs at least one other view");
        const Tensor kinv = at::inverse(K);                                                            // homo_utils.py:51
        vol = at::empty({T, n - 1, 30}, poses.options());
        for (int64_t i = 0; i < T; ++i) {
            const Tensor inv_i = at::inverse(P[i]);
            int64_t r = 0;
            for (int64_t j = 0; j < n; ++j) {
                if (j == i) continue;
                const Tensor rel = at::matmul(P[j], inv_i);                                            // hybrid_depth_decoder.py:235 (Q8)
                const Tensor m = at::inverse(rel);                                                     // homo_utils.py:258
                vol.index_put_({i, r, Slice(None, 9)}, kinv[0].reshape({9}));
                vol.index_put_({i, r, Slice(9, 21)}, m.index({0, Slice(None, 3), Slice()}).reshape({12}));
                vol.index_put_({i, r, Slice(21, None)}, K[0].reshape({9}));
                ++r;
            }
        }
    } else {
        vol = at::empty({0}, poses.options());
    }
    return {sweep, vol};
}

int64_t set_reserved_cus(int64_t n) { return estd_set_reserved_cus((int)n); }
// ------------------------------------------------------------------------------------------------ frame-to-model alignment
// csrc/track/frame_align.hip: live depth [H,W] (+ optional conf) against the model maps m_depth [Hm,Wm] / m_normal [Hm,Wm,3]; mats: CPU
// float32 [3,12] (L, Fm, Bm: host values of the launch arguments) -> (residual [H,W], match int32 [H,W], sums float64 [29])
std::tuple<Tensor, Tensor, Tensor> frame_align(const Tensor& depth, const OptTensor& conf, const Tensor& m_depth, const Tensor& m_normal,
                                               const Tensor& mats, double dist_max, double z_near, double conf_min)
{
    const char* op = "frame_align";
    const OpScope scope(depth);
    estd_frame_align_desc d{};
    d.depth = map_ptr(depth, {-1, -1}, op, "depth");
    const int64_t H = depth.size(-2), W = depth.size(-1);
    check_map_size(H, W, op, "depth");
    d.conf = opt_fptr(conf, "conf");
    if (d.conf) map_ptr(*conf, {H, W}, op, "conf");
    d.m_depth = map_ptr(m_depth, {-1, -1}, op, "m_depth");
    const int64_t Hm = m_depth.size(-2), Wm = m_depth.size(-1);
    check_map_size(Hm, Wm, op, "m_depth");
    d.m_normal = map_ptr(m_normal, {Hm, Wm, 3}, op, "m_normal");
    const float* m = host_values(mats, 36, op, "mats", "[3,12] (L, Fm, Bm)", true);
    d.H = (int)H; d.W = (int)W; d.Hm = (int)Hm; d.Wm = (int)Wm;
    d.dist_max = positive_square_f32(dist_max, op, "dist_max", true); d.z_near = not_negative_f32(z_near, op, "z_near");
    d.conf_min = not_nan_f32(conf_min, op, "conf_min");
    for (int i = 0; i < 12; ++i) { d.L[i] = m[i]; d.Fm[i] = m[12 + i]; d.Bm[i] = m[24 + i]; }
    Tensor residual = new_f32({H, W}, depth), match = at::empty({H, W}, depth.options().dtype(at::kInt));
    Tensor sums = at::empty({ESTD_FRAME_ALIGN_SUMS}, depth.options().dtype(at::kDouble));
    Tensor partials = at::empty({estd_frame_align_partials((int)H, (int)W) / 8}, depth.options().dtype(at::kDouble));
    d.residual = residual.data_ptr<float>(); d.match = match.data_ptr<int>();
    d.sums = sums.data_ptr<double>(); d.partials = partials.data_ptr<double>();
    check_status(estd_frame_align(&d, cur_stream()), "estd_frame_align");
    return {residual, match, sums};
}

// ------------------------------------------------------------------------------------------------ rigid registration
// csrc/track/rigid_align.hip: src [n,3] (+ optional normals [n,3]) moved by T, a CPU float32 [3,4] (host values of the launch arguments)
// -> (moved [n,3], moved_normal [n,3], or [0,3] without normals)
std::tuple<Tensor, Tensor> rigid_apply(const Tensor& src, const OptTensor& src_normal, const Tensor& T)
{
    const char* op = "rigid_apply";
    const OpScope scope(src);
    const float* sp = check_cloud(src, op, "src", 3);
    const int64_t n = src.size(0);
    const bool normals = src_normal.has_value() && src_normal->defined();
    const float* np = nullptr;
    if (normals) {
        np = check_cloud(*src_normal, op, "src_normal", 3);
        TORCH_CHECK(src_normal->size(0) == n && src_normal->device() == src.device(), op, ": src_normal must be [", n, ",3] on the points' device");
    }
    const float* t = host_values(T, 12, op, "T", "[3,4]", true);
    Tensor moved = new_f32({n, 3}, src), moved_normal = new_f32({normals ? n : 0, 3}, src);
    if (n)
        check_status(estd_rigid_apply(sp, np, (long long)n, t, moved.data_ptr<float>(), normals ? moved_normal.data_ptr<float>() : nullptr, cur_stream()),
                     "estd_rigid_apply");
    return {moved, moved_normal};
}

// moved [N,3] (+ moved_normal [N,3]), index int64 [N], target [Nt,3], normal [Nn,3] or none -> (residual [N], match int64 [N], sums float64 [29])
std::tuple<Tensor, Tensor, Tensor> rigid_system(const Tensor& moved, const OptTensor& moved_normal, const Tensor& index, const Tensor& target,
                                                const OptTensor& normal, bool by_index, int64_t metric, double dist_max, double cos_min, bool two_sided)
{
    const char* op = "rigid_system";
    const OpScope scope(moved);
    estd_rigid_system_desc d{};
    d.moved = check_cloud(moved, op, "moved", 3);
    const int64_t N = moved.size(0);
    if (moved_normal.has_value() && moved_normal->defined()) {
        d.moved_normal = check_cloud(*moved_normal, op, "moved_normal", 3);
        TORCH_CHECK(moved_normal->size(0) == N && moved_normal->device() == moved.device(), op, ": moved_normal must be [", N, ",3] on the points' device");
    }
    d.index = reinterpret_cast<const long long*>(lptr(index, op, "index", moved, N));
    d.target = check_cloud(target, op, "target", 3);
    const int64_t Nt = target.size(0);
    TORCH_CHECK(target.device() == moved.device() && (by_index || Nt >= N), op, ": target must be on the points' device, and [n,3] with n >= ", N,
                " when it is not read by index");
    int64_t Nn = Nt;
    if (normal.has_value() && normal->defined()) {
        d.normal = check_cloud(*normal, op, "normal", 3);
        TORCH_CHECK(normal->device() == moved.device(), op, ": normal must be on the points' device");
        Nn = normal->size(0);
    }
    check_count(metric, ESTD_RIGID_PLANE, ESTD_RIGID_POINT, op, "metric");
    d.dist_max = positive_square_f32(dist_max, op, "dist_max", true);
    d.cos_min = d.moved_normal ? not_nan_f32(cos_min, op, "cos_min") : (float)cos_min;
    TORCH_CHECK(d.normal || !(metric == ESTD_RIGID_PLANE || (d.moved_normal && std::isfinite(d.cos_min))), op,
                ": the plane metric and the cosine gate need the target's normals");
    d.N = (long long)N; d.Nt = (long long)Nt; d.Nn = (long long)Nn;
    d.metric = (int)metric; d.by_index = by_index; d.two_sided = two_sided;
    Tensor residual = new_f32({N}, moved), match = at::empty({N}, moved.options().dtype(at::kLong));
    Tensor sums = at::empty({ESTD_RIGID_SYSTEM_SUMS}, moved.options().dtype(at::kDouble));
    Tensor partials = at::empty({estd_rigid_system_partials((long long)N) / 8}, moved.options().dtype(at::kDouble));
    d.residual = residual.data_ptr<float>(); d.match = reinterpret_cast<long long*>(match.data_ptr<int64_t>());
    d.sums = sums.data_ptr<double>(); d.partials = N ? partials.data_ptr<double>() : nullptr;
    check_status(estd_rigid_system(&d, cur_stream()), "estd_rigid_system");
    return {residual, match, sums};
}

void profile_mark(int64_t id) { check_status(estd_profile_mark((int)id, cur_stream()), "estd_profile_mark"); }
int64_t conv3d_grid(int64_t N, int64_t D, int64_t H, int64_t W)
{
    const int g = estd_conv3d_k3_grid((int)N, (int)D, (int)H, (int)W);
    check_status(g < 0 ? g : ESTD_OK, "estd_conv3d_k3_grid");
    return g;
}

}  // namespace

TORCH_LIBRARY(estdepth_hip, m)
{
    m.def("cam_pair_proj(Tensor src_proj, Tensor ref_proj) -> Tensor");
    m.def("cam_sweep_proj(Tensor ref_pose, Tensor src_pose, Tensor intr) -> Tensor");
    m.def("cam_volume_mats(Tensor pose_j, Tensor? pose_i, Tensor intr, Tensor(a!) out) -> ()");
    m.def("homo_warping(Tensor src_chw, Tensor proj12, Tensor depth_values, int D) -> Tensor");
    m.def("homo_warping_px(Tensor src_chw, Tensor proj12, Tensor depth_dhw) -> Tensor");
    m.def("mix1x1(Tensor in_chw, Tensor w, Tensor? bias) -> Tensor");
    m.def("homo_warp_costvol(Tensor src_mix, Tensor ref_mix, Tensor proj12, Tensor depth_values, int D, Tensor(a!) out) -> ()");
    m.def("conv3d_k3(Tensor x, Tensor? x_extra, Tensor? w_main, Tensor? w_extra, Tensor? w_xout, Tensor? w_alt, Tensor scale, Tensor shift, "
          "int[] dims, int cin_main, int in_stride, int n_tiles, int act_a, int act_b, int act_split, Tensor(a!)? out, int out_stride, "
          "int out_channels, Tensor? residual, Tensor? residual2, float out_scale, bool accumulate, Tensor(b!)? out_extra, Tensor? head_w, "
          "Tensor? head_b, Tensor(c!)? out_head, Tensor(d!)? stats_partials, int variant, Tensor? gate_r=None, Tensor? gate_stats=None, "
          "Tensor? gate_gamma=None, Tensor? gate_beta=None) -> ()");
    m.def("conv2d_k3(Tensor x_nhwc, Tensor? w, Tensor? w_alt, Tensor scale, Tensor shift, int cout, int dilation, int group_tiles, "
          "bool relu_before_residual, bool relu_after_residual, Tensor? residual, int variant) -> Tensor");
    m.def("groupnorm_finalize(Tensor partials, int n_blocks, float count, float eps) -> Tensor");
    m.def("softargmin_up(Tensor logits, Tensor depth_values, int scale) -> (Tensor, Tensor)");
    m.def("warp_volume(Tensor vol, Tensor mats30, Tensor depth, float depth_min, float depth_interval) -> Tensor");
    m.def("warp_volume_ex(Tensor vol, Tensor mats30, Tensor depth, bool depth_per_voxel, float depth_min, float depth_interval, "
          "bool use_disp, float disp_min, float disp_interval, bool border, float padding_value) -> Tensor");
    m.def("warp_attention(Tensor kv_target, Tensor[] kv_sources, Tensor mats, Tensor depth_values, float depth_min, float depth_interval) -> Tensor");
    m.def("attention_prewarped(Tensor kv_target, Tensor[] kv_sources) -> Tensor");
    m.def("gru_reset_apply(Tensor xh, Tensor ru, Tensor stats4, Tensor gamma_r, Tensor beta_r) -> Tensor");
    m.def("gru_blend(Tensor xh, Tensor ru, Tensor o_raw, Tensor stats_ru, Tensor stats_o, Tensor gamma_u, Tensor beta_u, Tensor gamma_o, "
          "Tensor beta_o, Tensor(a!) out_value, int out_stride) -> ()");
    m.def("bn_act_nhwc_(Tensor(a!) x, Tensor scale, Tensor shift, bool relu, Tensor? residual) -> Tensor(a!)");
    m.def("spp_upsample_cat(Tensor raw, Tensor skip, Tensor[] branches) -> Tensor");
    m.def("conv1x1_nhwc(Tensor x, Tensor w, Tensor? scale, Tensor? shift, int stride, bool relu, Tensor? residual) -> Tensor");
    m.def("conv2d_taps_nhwc(Tensor x, Tensor w, Tensor? scale, Tensor? shift, int ksize, int stride, int pad, bool relu, Tensor? residual) -> Tensor");
    m.def("stem7x7s2_nhwc(Tensor x, Tensor w_packed, Tensor scale, Tensor shift) -> Tensor");
    m.def("maxpool3x3s2_nhwc(Tensor x) -> Tensor");
    m.def("avgpool_nhwc(Tensor x, int k) -> Tensor");
    m.def("conv2d_small_nhwc(Tensor x, Tensor w_packed, Tensor scale, Tensor shift, int cout, int ksize, int stride, bool relu) -> Tensor");
    m.def("conv2d_k3_to16_nhwc(Tensor x, Tensor w_packed, Tensor scale, Tensor shift, bool upsample) -> Tensor");
    m.def("normalise_nhwc(Tensor imgs) -> Tensor");
    m.def("stem3x3s2_nhwc(Tensor x, Tensor weight, Tensor scale, Tensor shift) -> Tensor");
    m.def("nhwc_to_planes(Tensor x) -> Tensor");
    m.def("planes_cat_nhwc(Tensor a, Tensor b, bool relu_b) -> Tensor");
    m.def("upsample2_cat_nhwc(Tensor x, Tensor skip) -> Tensor");
    m.def("disp_head_nhwc(Tensor x, Tensor weight, Tensor bias, float depth_max, int upscale) -> Tensor");
    m.def("cdhw_to_vol(Tensor src, Tensor(a!) dst, int dst_stride, int dst_off) -> ()");
    m.def("vol_to_cdhw(Tensor src, int C, int[] dims, int src_stride, int src_off) -> Tensor");
    m.def("camera_matrices_host(Tensor cam_poses, Tensor cam_intr, Tensor[] pre_poses, bool with_volume) -> (Tensor, Tensor)");
    m.def("tsdf_integrate_(Tensor(a!) volume, Tensor[] depths, Tensor[] confs, Tensor mats, float trunc, float z_near, float conf_min, "
          "bool weighted, float w_max, bool no_skip) -> Tensor(a!)");
    m.def("tsdf_extract_points(Tensor volume, float voxel_size, Tensor origin, float w_min, int capacity) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("tsdf_raycast(Tensor volume, Tensor mat, int H, int W, float t_min, float dt, int n_steps, float w_min, bool stats) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("tsdf_integrate_color_(Tensor(a!) volume, Tensor(b!) color, Tensor[] depths, Tensor[] confs, Tensor[] images, Tensor mats, float trunc, "
          "float z_near, float conf_min, bool weighted, float w_max, bool no_skip) -> Tensor(a!)");
    m.def("tsdf_edge_colors(Tensor volume, Tensor color, Tensor edge) -> Tensor");
    m.def("tsdf_mesh_vertices(Tensor volume, Tensor? color, float voxel_size, Tensor origin, float w_min, int capacity) -> "
          "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("tsdf_mesh_faces(Tensor volume, float w_min, int capacity) -> (Tensor, Tensor, Tensor)");
    m.def("mesh_components(Tensor faces, int n_vertices) -> (Tensor, Tensor, Tensor)");
    m.def("mesh_face_area(Tensor xyz, Tensor faces) -> (Tensor, Tensor, Tensor)");
    m.def("mesh_sample(Tensor xyz, Tensor faces, Tensor? attrs, int n_samples, int seed) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("mesh_raster(Tensor xyz, Tensor faces, Tensor mat, int H, int W, float z_near, bool preload) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("tsdf_raycast_color(Tensor volume, Tensor color, Tensor mat, int H, int W, float t_min, float dt, int n_steps, float w_min) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("depth_consistency(Tensor target, Tensor[] sources, Tensor mats, float px_max, float rel_max, float z_near) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("cloud_cell_keys(Tensor points, Tensor lo, float cell, int[] dims) -> Tensor");
    m.def("cloud_nearest(Tensor query, Tensor order, Tensor records, Tensor cell_start, Tensor lo, float cell, int[] dims, float max_dist, "
          "bool stats) -> (Tensor, Tensor, Tensor)");
    m.def("cloud_cell_centroids(Tensor points, Tensor attrs, Tensor order, Tensor segments) -> (Tensor, Tensor)");
    m.def("cloud_knn(Tensor query, Tensor order, Tensor records, Tensor cell_start, Tensor lo, float cell, int[] dims, float max_dist, "
          "int k, bool stats) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("cloud_count_within(Tensor query, Tensor order, Tensor records, Tensor cell_start, Tensor lo, float cell, int[] dims, float radius) -> Tensor");
    m.def("cloud_dbscan(Tensor records, Tensor cell_start, Tensor lo, float cell, int[] dims, float eps, int min_points) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("cloud_normals(Tensor points, Tensor query, Tensor index, Tensor count, Tensor? toward, bool cov) -> "
          "(Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("cloud_spfh(Tensor points, Tensor normal, Tensor index, Tensor count, bool oriented) -> (Tensor, Tensor)");
    m.def("cloud_fpfh(Tensor points, Tensor normal, Tensor index, Tensor count, Tensor hist, Tensor pairs) -> (Tensor, Tensor, Tensor)");
    m.def("feature_match(Tensor a, Tensor b, Tensor? a_valid, Tensor? b_valid) -> (Tensor, Tensor, Tensor)");
    m.def("ransac_pairs(Tensor P, Tensor Q, int hypotheses, int seed, float dist_max, float edge_ratio) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("mesh_tri_bins(Tensor xyz, Tensor faces, Tensor lo, float cell, int[] dims, int big_cells) -> (Tensor, Tensor, Tensor)");
    m.def("mesh_tri_fill(Tensor xyz, Tensor faces, Tensor lo, float cell, int[] dims, int big_cells, Tensor offset, int n_pairs) -> "
          "(Tensor, Tensor)");
    m.def("mesh_cluster_faces(Tensor faces, Tensor cluster, int n_clusters) -> (Tensor, Tensor, Tensor)");
    m.def("mesh_cluster_quadrics(Tensor xyz, Tensor faces, Tensor order, Tensor segments, Tensor cell_key, Tensor mean, Tensor lo, float cell, "
          "int[] dims, float reg) -> (Tensor, Tensor, Tensor)");
    m.def("mesh_nearest(Tensor query, Tensor order, Tensor big_records, Tensor records, Tensor cell_start, Tensor lo, float cell, int[] dims, "
          "float max_dist, bool bary, bool closest) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("frame_align(Tensor depth, Tensor? conf, Tensor m_depth, Tensor m_normal, Tensor mats, float dist_max, float z_near, float conf_min) -> "
          "(Tensor, Tensor, Tensor)");
    m.def("rigid_apply(Tensor src, Tensor? src_normal, Tensor T) -> (Tensor, Tensor)");
    m.def("rigid_system(Tensor moved, Tensor? moved_normal, Tensor index, Tensor target, Tensor? normal, bool by_index, int metric, float dist_max, "
          "float cos_min, bool two_sided) -> (Tensor, Tensor, Tensor)");
    m.def("profile_mark(int id) -> ()");
    m.def("set_reserved_cus(int n) -> int");
    m.def("conv3d_grid(int N, int D, int H, int W) -> int");
}

// Every operator is ROCm-only: registered for the CUDA dispatch key (= HIP in PyTorch-ROCm).  CPU tensors find no kernel and
// raise the dispatcher's NotImplementedError -- there is no CPU fallback by design.  The two argument-free helpers are
// registered as CompositeExplicitAutograd (no tensor to dispatch on).
TORCH_LIBRARY_IMPL(estdepth_hip, CUDA, m)
{
    m.impl("cam_pair_proj", cam_pair_proj);
    m.impl("cam_sweep_proj", cam_sweep_proj);
    m.impl("cam_volume_mats", cam_volume_mats);
    m.impl("homo_warping", homo_warping);
    m.impl("homo_warping_px", homo_warping_px);
    m.impl("mix1x1", mix1x1);
    m.impl("homo_warp_costvol", homo_warp_costvol);
    m.impl("conv3d_k3", conv3d_k3);
    m.impl("conv2d_k3", conv2d_k3);
    m.impl("groupnorm_finalize", groupnorm_finalize);
    m.impl("softargmin_up", softargmin_up);
    m.impl("warp_volume", warp_volume);
    m.impl("warp_volume_ex", warp_volume_ex);
    m.impl("warp_attention", warp_attention);
    m.impl("attention_prewarped", attention_prewarped);
    m.impl("gru_reset_apply", gru_reset_apply);
    m.impl("gru_blend", gru_blend);
    m.impl("bn_act_nhwc_", bn_act_nhwc_);
    m.impl("spp_upsample_cat", spp_upsample_cat);
    m.impl("conv1x1_nhwc", conv1x1_nhwc);
    m.impl("conv2d_taps_nhwc", conv2d_taps_nhwc);
    m.impl("stem7x7s2_nhwc", stem7x7s2_nhwc);
    m.impl("maxpool3x3s2_nhwc", maxpool3x3s2_nhwc);
    m.impl("avgpool_nhwc", avgpool_nhwc);
    m.impl("conv2d_small_nhwc", conv2d_small_nhwc);
    m.impl("conv2d_k3_to16_nhwc", conv2d_k3_to16_nhwc);
    m.impl("normalise_nhwc", normalise_nhwc);
    m.impl("stem3x3s2_nhwc", stem3x3s2_nhwc);
    m.impl("nhwc_to_planes", nhwc_to_planes);
    m.impl("planes_cat_nhwc", planes_cat_nhwc);
    m.impl("upsample2_cat_nhwc", upsample2_cat_nhwc);
    m.impl("disp_head_nhwc", disp_head_nhwc);
    m.impl("cdhw_to_vol", cdhw_to_vol);
    m.impl("vol_to_cdhw", vol_to_cdhw);
    m.impl("tsdf_integrate_", tsdf_integrate_);
    m.impl("tsdf_extract_points", tsdf_extract_points);
    m.impl("tsdf_raycast", tsdf_raycast);
    m.impl("tsdf_integrate_color_", tsdf_integrate_color_);
    m.impl("tsdf_edge_colors", tsdf_edge_colors);
    m.impl("tsdf_mesh_vertices", tsdf_mesh_vertices);
    m.impl("tsdf_mesh_faces", tsdf_mesh_faces);
    m.impl("mesh_components", mesh_components);
    m.impl("mesh_face_area", mesh_face_area);
    m.impl("mesh_sample", mesh_sample);
    m.impl("mesh_raster", mesh_raster);
    m.impl("tsdf_raycast_color", tsdf_raycast_color);
    m.impl("depth_consistency", depth_consistency);
    m.impl("cloud_cell_keys", cloud_cell_keys);
    m.impl("cloud_nearest", cloud_nearest);
    m.impl("cloud_cell_centroids", cloud_cell_centroids);
    m.impl("cloud_knn", cloud_knn);
    m.impl("cloud_count_within", cloud_count_within);
    m.impl("cloud_dbscan", cloud_dbscan);
    m.impl("cloud_normals", cloud_normals);
    m.impl("cloud_spfh", cloud_spfh);
    m.impl("cloud_fpfh", cloud_fpfh);
    m.impl("feature_match", feature_match);
    m.impl("ransac_pairs", ransac_pairs);
    m.impl("mesh_tri_bins", mesh_tri_bins);
    m.impl("mesh_tri_fill", mesh_tri_fill);
    m.impl("mesh_nearest", mesh_nearest);
    m.impl("mesh_cluster_faces", mesh_cluster_faces);
    m.impl("mesh_cluster_quadrics", mesh_cluster_quadrics);
    m.impl("frame_align", frame_align);
    m.impl("rigid_apply", rigid_apply);
    m.impl("rigid_system", rigid_system);
}

TORCH_LIBRARY_IMPL(estdepth_hip, CPU, m)
{
    m.impl("camera_matrices_host", camera_matrices_host);      // host-side algebra on CPU tensors (not a compute fallback)
}

TORCH_LIBRARY_IMPL(estdepth_hip, CompositeExplicitAutograd, m)
{
    m.impl("profile_mark", profile_mark);
    m.impl("set_reserved_cus", set_reserved_cus);
    m.impl("conv3d_grid", conv3d_grid);
}
