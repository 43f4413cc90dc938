/*
 * estd_hip.h -- C ABI of libestd_hip.so: the MI355X (gfx950) kernels of ESTDepth's
 * plane-sweep + EST-transformer hot path.
 *
 * The reference (xxlong0/ESTDepth) has no native layer at all: every op below replaces a
 * composition of ATen calls inside the Python functions cited per entry point.  The ABI is
 * therefore ours: plain device pointers + sizes + a hipStream_t, int status return (0 = OK,
 * negative = estd_status), no exceptions, no torch types.  All pointers are DEVICE pointers to
 * fp32 unless stated; every call only enqueues work on `stream` (no hidden synchronisation).
 *
 * Internal volume layouts (private to the library + its host wrapper):
 *   vol32  : [N][D][H][W][32]  channels-last cost / feature volumes
 *   kv     : [D][H][W][32]     value = channels 0..15, key = channels 16..31
 *   scalar : [N][D][H][W]      1-channel volumes (semantic plane scores, logits, 33rd channel)
 */
#ifndef ESTD_HIP_H
#define ESTD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* estd_stream_t; /* hipStream_t */

enum estd_status {
    ESTD_OK = 0,
    ESTD_ERR_ARG = -1,      /* null pointer / non-positive size / unsupported channel count */
    ESTD_ERR_LAUNCH = -2,   /* hipLaunch / hipGetLastError failure */
    ESTD_ERR_UNSUPPORTED = -3
};

enum estd_act { ESTD_ACT_NONE = 0, ESTD_ACT_RELU = 1, ESTD_ACT_TANH = 2 };

/* upper bound on the views + memory volumes one target attends to in estd_warp_attention (the reference loops over
 * any number, hybrid_depth_decoder.py:229-246; 16 covers Joint mode up to seq_len 17 / 15 targets + 2 memories) */
#define ESTD_MAX_ATTENTION_SOURCES 16

int estd_version(void);
/* launches the empty kernel `estd_mark_kernel` so a rocprofv3 kernel trace can be cut to a timed region */
int estd_profile_mark(int id, estd_stream_t stream);
const char* estd_status_string(int status);
/* Compute units the persistent convolution grids leave free (0..128, rounded up to a multiple of 8 = one per XCD; default 0, or
 * the environment variable ESTD_RESERVED_CUS read at load time).  The convolution kernels launch one or two resident
 * workgroups per CU with STATIC tile ranges: a concurrent kernel that holds even a few CUs (an RCCL collective overlapped
 * with the step) would push the workgroups that no longer fit behind all the others and double the launch's duration.
 * Multi-GPU hosts reserve 8 (bench.py does for N > 1).  Process-wide; takes effect for launches (and graph captures) made
 * afterwards.  Returns the value in effect. */
int estd_set_reserved_cus(int n);
int estd_get_reserved_cus(void);

/* ---- camera algebra on device (tiny fp64 kernels; keeps the forward free of host syncs) ------
 * Replaces the torch.inverse / matmul calls at hybrid_models/model_hybrid.py:74-88,
 * utils/homo_utils.py:469-471, hybrid_models/hybrid_depth_decoder.py:235 and
 * utils/homo_utils.py:51,:258.  */

/* proj12 = rows 0..2 of (src_proj @ inverse(ref_proj)) as rot[9] | trans[3]  (homo_utils.py:469-471) */
int estd_cam_pair_proj(const float* src_proj16, const float* ref_proj16, float* proj12, estd_stream_t stream);

/* Same, starting from camera-to-world poses and the 1/4-scale intrinsics, i.e. including
 * model_hybrid.py:74-88 (extrinsic = inverse(pose); proj[:3,:4] = K @ extrinsic[:3,:4]). */
int estd_cam_sweep_proj(const float* ref_pose16, const float* src_pose16, const float* intr9,
                        float* proj12, estd_stream_t stream);

/* mats30 = inverse(K)[9] | inverse(pose_j @ inverse(pose_i))[rows 0..2 = 12] | K[9]
 * (hybrid_depth_decoder.py:235 then homo_utils.py:51,:258).  If pose_i == NULL, pose_j is taken
 * as the already-formed relative pose (the level-1 warp_volume() call). */
int estd_cam_volume_mats(const float* pose_j16, const float* pose_i16, const float* intr9,
                         float* mats30, estd_stream_t stream);

/* ---- plane sweep ----------------------------------------------------------------------------- */

/* Level-1 operator utils/homo_utils.py:458-504 homo_warping(): src [C][H][W] -> out [C][D][H][W]. */
int estd_homo_warping(const float* src_chw, const float* proj12, const float* depth_values,
                      float* out_cdhw, int C, int D, int H, int W, estd_stream_t stream);

/* Same operator with PER-PIXEL depth hypotheses depth_dhw [D][H][W] (the reference's second accepted shape of depth_values,
 * utils/homo_utils.py:462 "[B, Ndepth] o [B, Ndepth, H, W]", :480-481). */
int estd_homo_warping_px(const float* src_chw, const float* proj12, const float* depth_dhw,
                         float* out_cdhw, int C, int D, int H, int W, estd_stream_t stream);

/* 1x1 channel mix of a 2D feature map, NCHW in -> HWC out: out[p][o] = sum_c w[o][c]*in[c][p] + b[o].
 * Used to push pre0 (model_hybrid.py:58,:93-94: 1x1x1 conv 64->32 + BN over cat[ref, warped]) in
 * front of the warp: pre0(cat[ref,warp(src)]) = mix_ref(ref)+shift + warp(mix_src(src)). Cin,Cout<=64 */
int estd_mix1x1_chw_to_hwc(const float* in_chw, const float* w, const float* bias, float* out_hwc,
                           int Cin, int Cout, int HW, estd_stream_t stream);

/* Fused homo_warping + pre0: out[d][y][x][:] = ref_mix[y][x][:] + bilinear(src_mix)(d,y,x)  (32 ch). */
int estd_homo_warp_costvol(const float* src_mix_hwc, const float* ref_mix_hwc, const float* proj12,
                           const float* depth_values, float* out_vol32, int D, int H, int W,
                           estd_stream_t stream);

/* ---- 3x3x3 convolution, implicit GEMM on fp32 MFMA (v_mfma_f32_16x16x4_f32) -------------------
 * Replaces networks/layers_op.py:16-39 (Conv3d bias=False + BatchNorm3d eval + ReLU/Tanh) as used at
 * model_hybrid.py:59-60,:95 and hybrid_depth_decoder.py:84-112,:190-200,:256,:377, and the two biased
 * Conv3d of transformer/epipolar_transformer.py:21,:26.  Weights are pre-packed by the host wrapper
 * (estdepth_amd/packing.py documents the fragment order). */
typedef struct estd_conv3d_desc {
    int N, D, H, W;
    int cin_main;             /* 16 or 32 channels read from in_main */
    int in_stride;            /* floats between consecutive voxels of in_main (>= cin_main) */
    int n_tiles;              /* output 16-channel tiles: 1 or 2; 3 = 32 channels on MFMA + a 33rd channel on the VALU */
    const float* in_main;     /* [N][D][H][W][in_stride] */
    const float* in_extra;    /* [N][D][H][W] scalar input channel, or NULL */
    const float* w_main;      /* packed, see packing.py */
    const float* w_extra;     /* packed extra-channel taps, or NULL */
    const float* w_xout;      /* n_tiles == 3 only: output channel 32's weights in the packing of the entry point called (packing.py:
                               * pack_xout / pack_conv3d_wino_xout / pack_conv3d_wino2_xout), else NULL */
    const float* scale;       /* [n_out] folded BN scale per output channel (n_out = 16, 32 or 33) */
    const float* shift;       /* [n_out] folded BN shift / conv bias */
    int act_a, act_b, act_split;  /* channels < act_split use act_a, others act_b (output channel 32 too); even, or >= 32 */
    /* main output (channels-last, out_stride floats per voxel, may alias a sub-range of a wider tensor) */
    float* out_main;          /* NULL when only the head output is wanted */
    int out_stride;
    int out_channels;         /* 16 or 32 real channels written to out_main */
    const float* residual;    /* vol with the layout of out_main added after the activation, or NULL */
    const float* residual2;   /* a second such volume (sum over two source views before the linear pre2), or NULL */
    float out_scale;          /* applied after the residual add (1.0 = none) */
    int accumulate;           /* 1: out_main += result (running sum over source views) */
    float* out_extra;         /* scalar volume receiving output channel 32 (n_tiles == 3), or NULL */
    /* fused 1x1x1 head (stereo_head*.1, hybrid_depth_decoder.py:106,:111): logit = sum_c head_w[c]*y[c] + head_b */
    const float* head_w;      /* [16] or NULL (requires n_tiles == 1) */
    const float* head_b;      /* device pointer to 1 float */
    float* out_head;          /* scalar volume [N][D][H][W] */
    /* GroupNorm(1 group) statistics of the raw outputs, per 16-channel group: partial sums per block,
     * double[grid][2 groups][2] = {sum, sumsq}; finalised by estd_groupnorm_finalize. */
    double* stats_partials;   /* or NULL */
    /* estd_conv3d_k3_split only: the 32->32 weights split into three bf16 pieces,
     * uint16 [27 taps][3 pieces][2 n-tiles][64 lanes][8] (packing.py::pack_conv3d_split), else NULL */
    const void* w_split;
    /* estd_conv3d_k3_wino only: the 32->32 filters in depth-Winograd F(2,3) form, float32
     * [37 taps (4 x 9 + 1 pad)][2 channel halves][2 quads][64 lanes][4] (packing.py::pack_conv3d_wino), else NULL */
    const float* w_wino;
    /* estd_conv3d_k3_wino2 only: the 32->32 filters with depth AND row axis in Winograd F(2,3) form, float32
     * [48 taps = (3 sd + kw) * 4 + sh][2 channel halves][2 quads][64 lanes][4] (packing.py::pack_conv3d_wino2), else NULL */
    const float* w_wino2;
    /* estd_conv3d_k3_wino2, 32 -> 16 instance only (the ConvGRU's output convolution, transformer/epipolar_transformer.py:51-52): the reset
     * gate applied in the convolution's plane loads instead of in a pass of its own (estd_gru_reset_apply): input channels 16..31 (h) are
     * multiplied by sigmoid(GroupNorm(r)) with r = channels 0..15 of gate_r [N][D][H][W][32] (the gate convolution's raw output),
     * gate_stats = {mean_r, rstd_r, ..} as estd_groupnorm_finalize writes them, gate_gamma / gate_beta [16] the affine of
     * reset_gate_norm (:44,:46).  All four NULL = no gate. */
    const float* gate_r;
    const float* gate_stats;
    const float* gate_gamma;
    const float* gate_beta;
} estd_conv3d_desc;

int estd_conv3d_k3(const estd_conv3d_desc* desc, estd_stream_t stream);
#ifdef ESTD_BUILD_AB   /* superseded A/B kernel: built and exported only with ESTD_BUILD_AB=1 (estdepth_amd/build.py) */
/* Same operator for the plain 32->32 case (cin_main = 32, n_tiles = 2, no extra channel / head / 33rd output), with
 * every fp32 product evaluated as six bf16 MFMA products of exactly split operands (a = a1+a2+a3, b = b1+b2+b3,
 * fp32 accumulation; dropped terms <= 2^-26 |ab|): fp32-level error at 96 instead of 256 matrix-pipe cycles per
 * 16x16x32 block.  Reads w_split instead of w_main.  ESTD_ERR_UNSUPPORTED for any other shape. */
int estd_conv3d_k3_split(const estd_conv3d_desc* desc, estd_stream_t stream);
#endif
#ifdef ESTD_BUILD_AB   /* superseded A/B kernel: built and exported only with ESTD_BUILD_AB=1 (estdepth_amd/build.py) */
/* Same operator for the plain 32->32 instance (cin_main = 32, n_tiles = 2, no extra channel / head / 33rd output; BN, ReLU,
 * residuals, scale, accumulation and GroupNorm partials as estd_conv3d_k3) with the depth axis in Winograd F(2,3) form:
 * two output planes from four transformed input planes, 36 instead of 54 tap products, every product an fp32 MFMA with
 * fp32 accumulation (csrc/conv3d_wino.hip).  Reads w_wino instead of w_main.  ESTD_ERR_UNSUPPORTED for any other shape. */
int estd_conv3d_k3_wino(const estd_conv3d_desc* desc, estd_stream_t stream);
#endif
/* Same operator with the depth AND the image-row axis in Winograd form, F(2x2, 3x3): 2 x 2 outputs (two planes, two rows) from a
 * 4 x 4 transformed input patch, 48 tap products per 4 outputs = 0.444 of the direct kernel's MFMA work (csrc/conv3d_wino2.hip).
 * Instances: cin_main = 32 with n_tiles = 2 (32 -> 32; with in_extra + w_extra the 33 -> 32 key|value form; every epilogue feature of
 * estd_conv3d_k3_wino -- GroupNorm partials not together with in_extra) and n_tiles = 1 (32 -> 16, the ConvGRU output convolution;
 * no in_extra), and cin_main = 16 with n_tiles = 1, head_w / head_b / out_head set and out_main = NULL (16 -> 16 + the fused 1x1x1
 * head, only the logit volume is written: stereo_head0 / stereo_head1, hybrid_depth_decoder.py:96-112; csrc/conv3d_wino2_c16.hip,
 * weights float32 [48 taps][64 lanes][4], packing.py::pack_conv3d_wino2_c16; no residuals / statistics / tanh).
 * n_tiles = 3 with in_extra, w_extra, out_extra and w_xout (packing.py::pack_conv3d_wino2_xout): the 33 -> 33 instance (dres2,
 * hybrid_depth_decoder.py:106) -- output channel 32 on the VALU from the fragments the MFMAs consume; no read-back streams, no statistics.
 * Reads w_wino2 (packing.py::pack_conv3d_wino2).  ESTD_ERR_UNSUPPORTED for any other shape. */
int estd_conv3d_k3_wino2(const estd_conv3d_desc* desc, estd_stream_t stream);
#ifdef ESTD_BUILD_AB   /* superseded A/B kernel: built and exported only with ESTD_BUILD_AB=1 (estdepth_amd/build.py) */
/* The 32 -> 32 instance of estd_conv3d_k3_wino2 (cin_main = 32, n_tiles = 2, no in_extra / out_extra / head; BN, ReLU, residuals, scale,
 * running sum, GroupNorm partials -- the latter without read-back streams; no tanh) on the operand-reuse kernel csrc/conv3d_wino2x.hip:
 * same F(2x2, 3x3) arithmetic, one 512-register wave per SIMD on v_mfma_f32_32x32x2_f32, both transforms in front of the LDS, wave-private
 * operand blocks.  Reads desc->w_wino2, which must then hold the packing of packing.py::pack_conv3d_wino2x: float32
 * [4 sd][3 kw][2 chunks][2 q][4 sh][64 lanes][4].  ESTD_ERR_UNSUPPORTED for any other shape (callers fall back to estd_conv3d_k3_wino2). */
int estd_conv3d_k3_wino2x(const estd_conv3d_desc* desc, estd_stream_t stream);
#endif
/* The 32-output-channel instances of estd_conv3d_k3_wino2 (cin_main = 32, n_tiles = 2, no out_extra / head / gate) with ALL THREE axes in
 * Winograd F(2,3) form -- F(2x2x2, 3x3x3), 8/27 of the direct products (csrc/conv3d_wino3.hip; the default for these launches).  Instances:
 *   * 32 -> 32: BN, activation (ReLU / tanh / split), residuals, scale, running sum (the read-back epilogues);
 *   * 32 -> 32 + stats_partials (GroupNorm partial sums; the ConvGRU gate convolution) -- WITHOUT read-back streams;
 *   * 33 -> 32: in_extra + w_extra, the latter in packing.py::pack_conv3d_wino3_extra form (the key || value convolution,
 *     hybrid_depth_decoder.py:198-199) -- without read-back streams and without stats_partials.
 * Reads desc->w_wino2, which must then hold the packing of packing.py::pack_conv3d_wino3: float32
 * [64 blocks ((4 sd + sh) * 2 + cc) * 2 + hh][2 halves][2 tap pairs][64 lanes][4].  ESTD_ERR_UNSUPPORTED for any other shape (callers fall back to
 * estd_conv3d_k3_wino2). */
int estd_conv3d_k3_wino3(const estd_conv3d_desc* desc, estd_stream_t stream);
/* Output channel 32 ALONE of the 33 -> 33 instance (n_tiles = 3: dres2, hybrid_depth_decoder.py:93-95,:196): out_extra = act(conv(in_main[32] | in_extra
 * -> 1 channel) * scale[32] + shift[32]) -- the pass that lets the 32 main output channels of that layer run on estd_conv3d_k3_wino3's 33 -> 32
 * instance (csrc/conv3d_xout.hip: the 27 taps as the matrix core's rows, a shifted sum of scalars behind it).  Reads desc->w_xout in the packing of
 * packing.py::pack_conv3d_xout_taps (float32 [2][2][64][4] + [2][64]); cin_main = 32, in_extra, scale / shift with 33 entries and out_extra required;
 * out_main and every other output field are ignored.  ESTD_ERR_UNSUPPORTED for any other shape and when channel 32's activation
 * (act_a if act_split > 32, else act_b) is neither NONE nor RELU. */
int estd_conv3d_k3_xout(const estd_conv3d_desc* desc, estd_stream_t stream);
/* number of thread blocks estd_conv3d_k3 launches for a volume (size of stats_partials / 4 doubles) */
int estd_conv3d_k3_grid(int N, int D, int H, int W);

/* ---- 3x3 2D convolution on NHWC maps (PSMNet matching features) ------------------------------
 * Replaces Conv2d(3x3, stride 1, dilation 1|2, bias=False) + BatchNorm2d(eval) [+ReLU] [+residual add] of
 * networks/layers_op.py:10-27 as used by networks/psm_submodule.py:14-37,43-60,112-114.  Cin, Cout multiples of 32.
 * Weights packed by estdepth_amd/packing.py::pack_conv2d in groups of 16*group_tiles output channels. */
typedef struct estd_conv2d_desc {
    int N, H, W;
    int cin, cout;
    int dilation;             /* 1 or 2 (padding = dilation) */
    int group_tiles;          /* 2 or 4: output channels per work item = 16*group_tiles */
    const float* in;          /* [N][H][W][cin] */
    const float* w;           /* packed [cout/(16*group_tiles)][cin/32][10 taps (9 + 1 pad)][2*group_tiles][64][4] */
    const float* scale;       /* [cout] folded BN scale */
    const float* shift;       /* [cout] folded BN shift */
    int relu_before_residual; /* conv-bn-relu */
    int relu_after_residual;  /* relu(conv-bn + residual) */
    const float* residual;    /* [N][H][W][cout] or NULL */
    float* out;               /* [N][H][W][cout] */
    /* estd_conv2d_k3_split only: int16 [cout/32][cin/32][9 taps][4096] bf16 split weights (packing.py::pack_conv2d_split) */
    const void* w_split;
    /* estd_conv2d_k3_wino only: the filters with the ROW taps in Winograd F(2,3) form, float32
     * [cout/(16*group_tiles)][cin/32][13 taps (4 x 3 + 1 pad)][2*group_tiles][64][4] (packing.py::pack_conv2d_wino) */
    const float* w_wino;
} estd_conv2d_desc;

int estd_conv2d_k3(const estd_conv2d_desc* desc, estd_stream_t stream);
#ifdef ESTD_BUILD_AB   /* superseded A/B kernel: built and exported only with ESTD_BUILD_AB=1 (estdepth_amd/build.py) */
/* Same operator with the row axis in Winograd F(2,3) form: two output rows from four transformed input rows, 12 instead of
 * 18 tap products, every product an fp32 MFMA with fp32 accumulation (csrc/conv2d_wino.hip).  Reads w_wino instead of w. */
int estd_conv2d_k3_wino(const estd_conv2d_desc* desc, estd_stream_t stream);
#endif
/* Same operator (dilation 1 | 2; group_tiles ignored: 32 output channels per work item) with BOTH image axes in Winograd form,
 * F(2x2, 3x3): 2 x 2 output pixels from a 4 x 4 transformed input patch, 16 instead of 36 tap products = 0.444 of the direct kernel's
 * MFMA work (csrc/conv2d_wino2.hip).  Reads desc->w_wino, which must then hold the F(2x2, 3x3) packing: float32
 * [cout/32][cin/32][8 steps][4][2][64][4] (packing.py::pack_conv2d_wino2). */
int estd_conv2d_k3_wino2(const estd_conv2d_desc* desc, estd_stream_t stream);
#ifdef ESTD_BUILD_AB   /* superseded A/B kernel: built and exported only with ESTD_BUILD_AB=1 (estdepth_amd/build.py) */
/* Same operator (group_tiles ignored: 32 output channels per work item) with every fp32 product as six
 * bf16 MFMA products of exactly 3-way split operands, fp32 accumulation (see estd_conv3d_k3_split). */
int estd_conv2d_k3_split(const estd_conv2d_desc* desc, estd_stream_t stream);
#endif

/* mean/rstd from the partials: stats_out = {mean_g0, rstd_g0, mean_g1, rstd_g1}; count = 16*D*H*W per group
 * (transformer/epipolar_transformer.py:22-23,:27 GroupNorm(1, 16, eps=1e-5)). */
int estd_groupnorm_finalize(const double* partials, int n_blocks, double count, float eps, float* stats_out4,
                            estd_stream_t stream);

/* ---- soft-argmin ------------------------------------------------------------------------------
 * hybrid_depth_decoder.py:33-38 depthlayer() applied to F.interpolate(logits, scale_factor=s) (nearest;
 * :202-204,:259-260,:359-361,:379-381), computed at low resolution and replicated s x s.
 * logits [N][D][H][W] -> depth, prob [N][s*H][s*W]. */
int estd_softargmin_up(const float* logits, const float* depth_values, float* depth, float* prob,
                       int N, int D, int H, int W, int s, estd_stream_t stream);

/* ---- EST transformer --------------------------------------------------------------------------*/

/* Level-1 operator utils/homo_utils.py:240-279 warp_volume() (zeros padding, trilinear):
 * vol [C][D][H][W] -> out [C][D][H][W]; depth_values [D] are the plane depths (the reference passes
 * depth_values.repeat(H,W), hybrid_depth_decoder.py:237). */
int estd_warp_volume(const float* vol_cdhw, const float* mats30, const float* depth_values,
                     float depth_min, float depth_interval, float* out_cdhw,
                     int C, int D, int H, int W, estd_stream_t stream);

/* Every branch of the reference's warp_volume() signature (utils/homo_utils.py:240-279): depth per plane [D] or per VOXEL
 * [D][H*W] (:246,:253), depth or disparity planes for the z normalisation (:187-190), padding_mode 'zeros' or 'border' -- the
 * latter samples the volume whose outermost voxel layer is replaced by padding_value (:271-274, _set_vol_border :305-319). */
typedef struct estd_warp_volume_opts {
    int depth_per_voxel;      /* 0: depth[D], 1: depth[D][H*W] */
    int use_disp;             /* 0: depth planes (depth_min, depth_interval), 1: disparity planes (disp_min, disp_interval) */
    int border;               /* 0: padding_mode='zeros', 1: padding_mode='border' with padding_value */
    float depth_min, depth_interval;
    float disp_min, disp_interval;
    float padding_value;
} estd_warp_volume_opts;
int estd_warp_volume_ex(const float* vol_cdhw, const float* mats30, const float* depth, const estd_warp_volume_opts* opts,
                        float* out_cdhw, int C, int D, int H, int W, estd_stream_t stream);

/* Fused warp_volume(K_j), warp_volume(V_j) for all sources j + epipolar attention
 * (hybrid_depth_decoder.py:233-246 + transformer/epipolar_transformer.py:62-73):
 *   xh[vox][0:16] = V_t ; xh[vox][16:32] = h = mean_j( softmax_j(K_t . warp(K_j)) * warp(V_j) ).
 * kv_src: HOST array of n_src device pointers to kv volumes (copied into the launch arguments);
 * mats_dev: device [n_src][30] from estd_cam_volume_mats.  n_src in 1..ESTD_MAX_ATTENTION_SOURCES
 * (more: ESTD_ERR_UNSUPPORTED).  Global gather of the eight corner records per source (LDS staging of the source boxes
 * was measured slower and dropped, csrc/est_fusion.hip), 2x4x8 target bricks in XCD-contiguous order, 4 lanes per target
 * voxel; instances specialised for 1..4 sources and generic ones for up to 8 / 16 (per-source correlation held in registers,
 * max-subtracted softmax as the reference's). */
int estd_warp_attention(const float* kv_target, const float* const* kv_src, const float* mats_dev,
                        int n_src, const float* depth_values, float depth_min, float depth_interval,
                        float* xh_out, int D, int H, int W, estd_stream_t stream);

/* Attention over already-warped kv volumes (the level-1 EpipolarTransformer.forward signature,
 * transformer/epipolar_transformer.py:56-73): same output as estd_warp_attention without the gather; n_src in
 * 1..ESTD_MAX_ATTENTION_SOURCES like it (more: ESTD_ERR_UNSUPPORTED). */
int estd_attention_prewarped(const float* kv_target, const float* const* kv_src, int n_src,
                             float* xh_out, int64_t n_vox, estd_stream_t stream);

/* xrh[vox] = [ x , sigmoid(GN(r_raw)) * h ]  (epipolar_transformer.py:44,:46,:51):
 * xh = [x,h]; ru = raw gate conv output [r(0..15), u(16..31)];
 * stats4 from estd_groupnorm_finalize; gamma/beta = reset_gate_norm affine [16]. */
int estd_gru_reset_apply(const float* xh, const float* ru, const float* stats4, const float* gamma_r,
                         const float* beta_r, float* xrh, int64_t n_vox, estd_stream_t stream);

/* out_value[vox][0:16] (stride out_stride) = u*h + (1-u)*tanh(GN(o_raw)),  u = sigmoid(GN(u_raw))
 * (epipolar_transformer.py:45,:47,:53,:82-83). */
int estd_gru_blend(const float* xh, const float* ru, const float* o_raw, const float* stats_ru4,
                   const float* stats_o4, const float* gamma_u, const float* beta_u, const float* gamma_o,
                   const float* beta_o, float* out_value, int out_stride, int64_t n_vox, estd_stream_t stream);

/* ---- layout conversion at the API edge (reference tensors are NCDHW) -------------------------- */
/* [C][S] (channel planes, S = D*H*W) -> [S][dst_stride] at channel offset dst_off */
int estd_cdhw_to_vol(const float* src_cdhw, float* dst, int C, int64_t S, int dst_stride, int dst_off,
                     estd_stream_t stream);
int estd_vol_to_cdhw(const float* src, float* dst_cdhw, int C, int64_t S, int src_stride, int src_off,
                     estd_stream_t stream);

/* ---- fused inference BatchNorm2d (+ residual add) (+ ReLU) on NHWC maps, in place --------------------------------
 * x[p][c] = act(x[p][c] * scale[c] + shift[c] + residual[p][c]); replaces the BatchNorm2d -> (add) -> ReLU launches that
 * follow the library convolutions of the 2D backbones (resnet_encoder.py:43-49, psm_submodule.py:14-37,
 * hybrid_depth_decoder.py:17-30).  C multiple of 4; residual may be NULL.
 * The ReLU is fmaxf(v, 0): a NaN becomes 0, where torch's ReLU propagates it (without relu a NaN passes through). */
int estd_bn_act_nhwc(float* x, const float* scale, const float* shift, const float* residual, int relu,
                     int64_t n_pix, int C, estd_stream_t stream);

/* ---- PSMNet SPP tail (networks/psm_submodule.py:100-116): out[n][y][x] = cat(raw, skip, up(b[0]), .. up(b[nb-1])) ----------
 * raw [N][H][W][c_raw], skip [N][H][W][c_skip], b[k] [N][bh[k]][bw[k]][c_b] (NHWC), up = bilinear resize to HxW with
 * align_corners = False (F.upsample in the reference's torch version = F.interpolate(..., align_corners=False)).
 * One pass instead of nb upsample kernels + a 123 MB concatenation.  Channel counts multiples of 4, nb <= 4. */
int estd_spp_upsample_cat(const float* raw, int c_raw, const float* skip, int c_skip, const float* const* branches,
                          const int* bh, const int* bw, int nb, int c_b, float* out, int N, int H, int W,
                          estd_stream_t stream);

/* ---- 2D refinement tail of the decoder (hybrid_models/hybrid_depth_decoder.py:267-290 / :392-415), glue around its convolutions --
 * estd_planes_cat_nhwc:    torch.cat([a, relu?(b)], 1) of two NCHW stacks a [N][Ca][HW], b [N][Cb][HW] (:268
 *                          cat([semantic_vs, relu(all_fused_logits)])) written as the NHWC map [N][HW][Ca+Cb]; Ca+Cb <= 496.
 *                          The ReLU is v > 0 ? v : 0: a NaN in b becomes 0, where torch's ReLU propagates it (relu_b = 0 copies it).
 * estd_upsample2_cat_nhwc: torch.cat([upsample(x), skip], 1) (:269-272, :280-281): x [N][H/2][W/2][Cx] nearest x2 beside
 *                          skip [N][H][W][Cs] -> out [N][H][W][Cx+Cs] (NHWC; channel counts multiples of 4, H and W even).
 * estd_disp_head_nhwc:     depth_max * sigmoid(Conv2d(C, 1, 3, stride 1, padding 1, bias)(in)) (:274 dispconv_1, :279 dispconv_0):
 *                          in [N][H][W][C] NHWC, w [1][C][3][3], bias [1] (device), C = 16 | 32; out [N][1][upscale*H][upscale*W],
 *                          upscale = 1, or 2 = the F.interpolate(scale_factor=2) (nearest) of :274 fused in. */
/* 3x3 / stride 1 / padding 1 convolution to 16 channels + folded BatchNorm2d + ReLU on NHWC maps, the full-resolution ConvBlocks
 * of the decoder (hybrid_models/hybrid_depth_decoder.py:17-30 ConvBlock; :276 upconv_0_0, :277-278 upconv_0_1(upsample(x))):
 * in [N][Hin][Win][cin], cin = 16 | 32; upsample = 1: the convolution reads the nearest-x2 upsampled map (Hin = H/2, Win = W/2,
 * :11-14) without materialising it; out [N][H][W][16].  w_packed: packing.pack_conv2d_to16 ([9 taps][cin/16][64 lanes][4]). */
/* The small convolutions of the PSM extractor outside the tiled 3x3 / stride-1 kernels (networks/psm_submodule.py): 3x3 stride 2
 * (:52 layer2[0].conv1), 1x1 stride 1 | 2 (:78-83 downsample, :100-110 SPP branches, :72-74 lastconv's 1x1) + folded BatchNorm2d
 * (scale 1 / shift 0 where the reference has none) [+ ReLU] on NHWC maps: in [N][Hin][Win][cin] -> out [N][Ho][Wo][cout], padding
 * ksize / 2.  Instances: (cin, ksize, stride) = (32,3,2), (32,1,2), (32,1,1), (64,1,1), (128,1,1); cout a multiple of 16;
 * w_packed: packing.pack_conv2d_small ([cout/16][ksize^2 taps][cin/16][64 lanes][4]).  Other shapes: ESTD_ERR_UNSUPPORTED. */
int estd_conv2d_small_nhwc(const float* in, const float* w_packed, const float* scale, const float* shift, float* out, int N, int Hin,
                           int Win, int cin, int cout, int ksize, int stride, int relu, estd_stream_t stream);
/* 1x1 convolution (stride 1 | 2, no padding) of an NHWC map + folded BatchNorm2d(eval) [+ residual] [+ ReLU] in ONE launch: the
 * bottleneck convolutions of the semantic branch's ResNet (hybrid_models/resnet_encoder.py:40-51 over torchvision's Bottleneck:
 * conv1 + bn1 + relu, conv3 + bn3 + shortcut + relu, downsample[0] + downsample[1]).  out = max(in . w^T * scale + shift
 * (+ residual), relu ? 0 : -inf).  cin a multiple of 16, cout a multiple of 32; other shapes: ESTD_ERR_UNSUPPORTED
 * (csrc/conv1x1.hip). */
typedef struct estd_conv1x1_desc {
    int N, H, W;              /* input map */
    int cin, cout;
    int stride;               /* 1 or 2: output pixel (y, x) reads input pixel (stride*y, stride*x); Ho = (H-1)/stride+1 */
    int relu;                 /* 1: ReLU after the (residual) add */
    const float* in;          /* [N][H][W][cin] */
    const float* w;           /* [cout][cin]: the Conv2d weight [cout, cin, 1, 1] as it lies in memory */
    const float* scale;       /* [cout] folded BN scale, or NULL (= 1) */
    const float* shift;       /* [cout] folded BN shift / bias, or NULL (= 0) */
    const float* residual;    /* [N][Ho][Wo][cout] added before the ReLU, or NULL */
    float* out;               /* [N][Ho][Wo][cout] */
} estd_conv1x1_desc;
int estd_conv1x1_nhwc(const estd_conv1x1_desc* desc, estd_stream_t stream);
/* k x k convolution (k = 1 | 3 | 5, stride 1 | 2, zero padding pad) of an NHWC map + folded BatchNorm2d(eval) [+ residual]
 * [+ ReLU] in ONE launch: the stride-2 3x3 convolutions of the semantic ResNet's layer2..4 (hybrid_models/resnet_encoder.py:40-51
 * over torchvision's Bottleneck.conv2 / BasicBlock.conv1 + bn + relu) and the 3x3 convolutions on maps too small for the tiled
 * Winograd kernels (hybrid_models/hybrid_depth_decoder.py:17-30 ConvBlock on the 1/32 map).  cin a multiple of 16, cout a multiple
 * of 32; Ho = (H + 2 pad - ksize) / stride + 1.  w: packing.pack_conv2d_taps = [ksize*ksize taps][cout][cin].  Other shapes:
 * ESTD_ERR_UNSUPPORTED (csrc/conv2d_taps.hip). */
typedef struct estd_conv2d_taps_desc {
    int N, H, W;              /* input map */
    int cin, cout;
    int ksize, stride, pad;
    int relu;                 /* 1: ReLU after the (residual) add */
    const float* in;          /* [N][H][W][cin] */
    const float* w;           /* [ksize*ksize][cout][cin] */
    const float* scale;       /* [cout] folded BN scale, or NULL (= 1) */
    const float* shift;       /* [cout] folded BN shift / bias, or NULL (= 0) */
    const float* residual;    /* [N][Ho][Wo][cout] added before the ReLU, or NULL */
    float* out;               /* [N][Ho][Wo][cout] */
} estd_conv2d_taps_desc;
int estd_conv2d_taps_nhwc(const estd_conv2d_taps_desc* desc, estd_stream_t stream);
/* first layer of the semantic ResNet (torchvision conv1 = Conv2d(3, 64, 7, stride 2, padding 3) + bn1 + relu,
 * hybrid_models/resnet_encoder.py:42-44): in [N][H][W][3] NHWC -> out [N][Ho][Wo][64] NHWC, Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1.
 * w_packed: packing.pack_stem7x7 ([7 rows][6 k-steps][4 channel tiles][64 lanes]); scale / shift [64] = folded BatchNorm2d. */
int estd_stem7x7s2_nhwc(const float* in, const float* w_packed, const float* scale, const float* shift, float* out, int N, int H,
                        int W, estd_stream_t stream);
/* MaxPool2d(3, stride 2, padding 1) of an NHWC map (torchvision ResNet.maxpool, resnet_encoder.py:45): in [N][H][W][C] ->
 * out [N][(H-1)/2+1][(W-1)/2+1][C]; C a multiple of 4; a NaN in a window is the window's result (ATen). */
int estd_maxpool3x3s2_nhwc(const float* in, float* out, int N, int H, int W, int C, estd_stream_t stream);
/* AvgPool2d(k, k) of an NHWC map (networks/psm_submodule.py:56-70, the SPP branches): in [N][H][W][C] -> out [N][H/k][W/k][C];
 * C a multiple of 4; window sum in row-major order, then one division by k*k (ATen's order). */
int estd_avgpool_nhwc(const float* in, float* out, int N, int H, int W, int C, int k, estd_stream_t stream);
int estd_conv2d_k3_to16_nhwc(const float* in, const float* w_packed, const float* scale, const float* shift, float* out, int N,
                             int H, int W, int cin, int upsample, estd_stream_t stream);
/* image normalisation of DepthNetHybrid.forward (hybrid_models/model_hybrid.py:119: imgs = 2 * (imgs / 255.) - 1.):
 * in [N][3][HW] planes (0..255) -> out [N][HW][3] NHWC records; the same three fp32 roundings as the reference's three ops. */
int estd_normalise_nhwc(const float* in, float* out, int N, int64_t HW, estd_stream_t stream);
/* first layer of the PSM matching-feature extractor (networks/psm_submodule.py:47 convbn(3, 32, 3, 2, 1, 1) + ReLU, :14-22):
 * in [N][H][W][3] NHWC, w [32][3][3][3] (Conv2d layout), scale/shift [32] = folded BatchNorm2d -> out [N][Ho][Wo][32] NHWC,
 * Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1 (kernel 3, stride 2, zero padding 1). */
int estd_stem3x3s2_nhwc(const float* in, const float* w, const float* scale, const float* shift, float* out, int N, int H, int W,
                        estd_stream_t stream);
int estd_planes_cat_nhwc(const float* a, int Ca, const float* b, int Cb, int relu_b, float* out, int N, int64_t HW,
                         estd_stream_t stream);
/* [N][HW][C] NHWC records -> [N][C][HW] planes: the 2D decoder's plane scores (hybrid_depth_decoder.py:162-184, the last ConvBlock's
 * D-channel NHWC map) as the scalar volumes [T][D][H][W] the 3D path reads (dres2's 33rd input channel, :268's concatenation). */
int estd_nhwc_to_planes(const float* in, int C, float* out, int N, int64_t HW, estd_stream_t stream);
int estd_upsample2_cat_nhwc(const float* x, int Cx, const float* skip, int Cs, float* out, int N, int H, int W,
                            estd_stream_t stream);
int estd_disp_head_nhwc(const float* in, const float* w, const float* bias, float depth_max, float* out, int N, int H, int W,
                        int C, int upscale, estd_stream_t stream);

/* ---- TSDF fusion of posed depth maps (csrc/tsdf.hip) --------------------------------------------
 * The reference stops at per-frame .npy depth maps (eval_hybrid_seq.py:215-230); these entry points accumulate the depth /
 * confidence maps the model returns into a scene on the device (KinectFusion's truncated signed distance update) and read the
 * surface back as an oriented point cloud.
 *
 * Volume: two fp32 planes of [Z][Y][X] voxels, x fastest: `tsdf` (D in [-1, 1]) and `weight` (Wt >= 0); all zeros = empty.  X must be
 * a multiple of 4 (a lane moves four voxels = 16 bytes per access), else ESTD_ERR_ARG.  Offsets are 64-bit; Z <= 65535,
 * Y <= 262140, X <= 2^20 (launch grids), beyond that ESTD_ERR_UNSUPPORTED.
 *
 * The integrate call fuses T frames (1..ESTD_TSDF_MAX_FRAMES) in ONE pass over the voxels.  mats[t] is the HOST 3x4 row-major matrix
 * A = K [R|t]_world->camera V in fp32 (V: voxel index -> voxel centre origin + (idx + 0.5) voxel_size; estdepth_amd/camera.py
 * tsdf_matrices forms it in float64).  Per voxel (ix, iy, iz), for each frame in order:
 *   1. a = fma(A0, ix, fma(A1, iy, fma(A2, iz, A3))), b and c likewise from rows 1 and 2; skip if c <= z_near;
 *   2. ui = floor(a / c + 0.5), vi = floor(b / c + 0.5) (pixel centres on integers); skip if outside [0, W) x [0, H);
 *   3. d = depth[t][vi * W + ui]; skip unless finite and > 0;
 *   4. with confidence maps: skip if conf < conf_min; w = conf (weighted; skip unless finite and > 0) else w = 1;
 *   5. sdf = d - c; skip if sdf < -trunc; tsdf = min(1, sdf / trunc);
 *   6. D = fma(D, Wt, tsdf * w) / (Wt + w); Wt = min(Wt + w, w_max).
 * IEEE divisions throughout.  A 16-byte group of four voxels that no frame updates is neither read nor written. */
#define ESTD_TSDF_MAX_FRAMES 8
typedef struct estd_tsdf_integrate_desc {
    int Z, Y, X;                                  /* volume dimensions */
    int T;                                        /* frames in this call */
    int H, W;                                     /* size of every depth / confidence map */
    int weighted;                                 /* 1: w = conf (needs conf), 0: w = 1 */
    int no_skip;                                  /* 1: measurement only -- every voxel is loaded and stored (tools/tsdf_bench.py) */
    float trunc, z_near, conf_min, w_max;
    float* tsdf;                                  /* [Z][Y][X] */
    float* weight;                                /* [Z][Y][X] */
    const float* depth[ESTD_TSDF_MAX_FRAMES];     /* [H][W] each */
    const float* conf[ESTD_TSDF_MAX_FRAMES];      /* [H][W] each: all T set, or all NULL */
    float mats[ESTD_TSDF_MAX_FRAMES][12];         /* host values, copied into the launch arguments */
} estd_tsdf_integrate_desc;
int estd_tsdf_integrate(const estd_tsdf_integrate_desc* desc, estd_stream_t stream);

/* The same fusion with colour.  The colour volume is one more fp32 tensor [3][Z][Y][X] (planar, x fastest, zeros = empty) that SHARES the
 * weight plane: colour is updated in exactly the voxels, frames and order in which D is, with the same w.  image[t] is the frame the
 * depth map t belongs to, [3][H][W] planar at the depth maps' size.  Steps 1-6 above apply verbatim -- D and Wt come out bit-identical to
 * the call without colour on the same inputs -- and, with Wt the weight BEFORE step 6, for channel k = 0, 1, 2:
 *   7. col_k = image[t][k * H * W + vi * W + ui] (the pixel the depth was read at);  C_k = fma(C_k, Wt, col_k * w) / (Wt + w).
 * Colour values are used as they are: finite values are the caller's duty (a NaN or an infinity stays in the voxel); negative values
 * (normalised images) are fine -- the average is affine, so a caller can undo the normalisation at export.  A 16-byte group that no
 * frame updates is neither read nor written in any of the five planes.  One T = 3 call equals three T = 1 calls bit for bit.
 * Argument errors as for the call without colour; in addition ESTD_ERR_ARG for a null `color` or a null image[t], t < T. */
typedef struct estd_tsdf_integrate_color_desc {
    int Z, Y, X;
    int T;
    int H, W;                                     /* size of every depth / confidence map and of every image plane */
    int weighted;
    int no_skip;                                  /* 1: measurement only (tools/tsdf_bench.py) */
    float trunc, z_near, conf_min, w_max;
    float* tsdf;                                  /* [Z][Y][X] */
    float* weight;                                /* [Z][Y][X] */
    const float* depth[ESTD_TSDF_MAX_FRAMES];     /* [H][W] each */
    const float* conf[ESTD_TSDF_MAX_FRAMES];      /* [H][W] each: all T set, or all NULL */
    float mats[ESTD_TSDF_MAX_FRAMES][12];
    float* color;                                 /* [3][Z][Y][X] */
    const float* image[ESTD_TSDF_MAX_FRAMES];     /* [3][H][W] each */
} estd_tsdf_integrate_color_desc;
int estd_tsdf_integrate_color(const estd_tsdf_integrate_color_desc* desc, estd_stream_t stream);

/* Zero crossings of the volume as points.  For every voxel with Wt >= w_min and each of its +x, +y, +z neighbours with Wt >= w_min:
 * a point when D0 < 0 <= D1 or D1 < 0 <= D0, at s = D0 / (D0 - D1) along the edge:
 *   xyz    = origin + (idx + 0.5 + s e_axis) voxel_size                      (fma(cell, voxel_size, origin) per coordinate)
 *   normal = g / |g|, g = fma(s, g1 - g0, g0): g0, g1 the gradients of D at the two end voxels (per axis the central difference
 *            0.5 (D+ - D-) where both neighbours exist with Wt >= w_min, the one-sided difference where one does, 0 where
 *            neither); the zero vector when g = 0.  Points towards increasing D = the free space the cameras saw.
 *   weight = fma(s, Wt1 - Wt0, Wt0);      edge = 3 * linear voxel index + axis (0 = x, 1 = y, 2 = z), exact.
 * origin3 is a HOST pointer to three floats.  `counter` (device, zeroed by the caller) ends at the TOTAL number of crossings -- one
 * increment per wave (lane ballots + population counts); records whose slot is >= capacity are dropped.  capacity == 0 counts only
 * (the output pointers may then be NULL).  xyz, normal [capacity][3]; point_weight, edge [capacity].  Order unspecified. */
int estd_tsdf_extract_points(const float* tsdf, const float* weight, int Z, int Y, int X, float voxel_size, const float* origin3,
                             float w_min, unsigned long long* counter, long long capacity, float* xyz, float* normal,
                             float* point_weight, long long* edge, estd_stream_t stream);

/* The colour at crossings: for each of the n ids edge[i] = 3 * linear voxel index + axis (as the extraction emits them), with D0, C0 at
 * that voxel and D1, C1 at its neighbour along the axis:  s = D0 / (D0 - D1) from the stored values (the extraction's expression);
 *   out[i][k] = fma(s, C1_k - C0_k, C0_k).
 * An id that is negative or >= 3 Z Y X, or whose neighbour along the axis lies outside the volume, writes (0, 0, 0).  The weights are not
 * read: ids of unobserved voxels blend whatever the planes hold.  edge, out: device, [n] and [n][3]; n == 0 launches nothing. */
int estd_tsdf_edge_colors(const float* tsdf, const float* color, int Z, int Y, int X, const long long* edge, long long n, float* out,
                          estd_stream_t stream);

/* Depth, normal and weight maps of the volume as a pinhole camera sees it (csrc/tsdf_raycast.hip; KinectFusion's surface prediction).
 * Depth is the z-depth along the optical axis with pixel centres on integers: the convention of the model's depth maps and of
 * estd_tsdf_integrate's c, so a rendered map can be scored against ground truth or fused again as it is.
 *
 * mat is the HOST 3x4 row-major matrix M = [ R K^-1 / voxel_size | (c - origin) / voxel_size - 0.5 ] in fp32 (R, c from the
 * camera-to-world pose; rows = x, y, z in voxel-index coordinates, where voxel i's centre is at i; estdepth_amd/camera.py
 * tsdf_ray_matrix forms it in float64).  Per pixel (u, v):
 *   1. r_j = fma(M[j][0], u, fma(M[j][1], v, M[j][2])); sample k = 0 .. n_steps - 1 at t_k = fma(k, dt, t_min) (never an accumulated
 *      sum), position p_j = fma(t_k, r_j, M[j][3]);
 *   2. cell i_j = floor(p_j), f_j = p_j - i_j; the sample is OBSERVED iff 0 <= i_j <= dim_j - 2 on all three axes and all eight corner
 *      weights are >= w_min.  With lerp(a, b, f) = fma(f, b - a, a) and D_xyz the corner values (x, y, z offsets 0 / 1):
 *        c_yz = lerp(D_0yz, D_1yz, f_x);  c_z = lerp(c_0z, c_1z, f_y);  F = lerp(c_0, c_1, f_z);  Wb = the same blend of the weights;
 *        G_x = lerp(lerp(D_100 - D_000, D_110 - D_010, f_y), lerp(D_101 - D_001, D_111 - D_011, f_y), f_z),
 *        G_y = lerp(c_10 - c_00, c_11 - c_01, f_z),  G_z = c_1 - c_0           (the gradient of the trilinear interpolant, per voxel);
 *   3. hit = the first k >= 1 with samples k - 1 and k both observed and F_{k-1} > 0 >= F_k (front faces only: a ray that starts behind
 *      a surface does not hit until it finds such a pair).  s = F_{k-1} / (F_{k-1} - F_k);
 *        depth  = fma(dt, s, t_{k-1});
 *        normal = g / |g|, g_j = fma(s, G_k,j - G_{k-1},j, G_{k-1},j), |g| = sqrt(fma(g_z, g_z, fma(g_y, g_y, g_x g_x))): world axes,
 *                 towards increasing D = the free space the cameras saw (as estd_tsdf_extract_points); the zero vector when |g| = 0;
 *        weight = fma(s, Wb_k - Wb_{k-1}, Wb_{k-1});
 *   4. no hit: depth = weight = 0, normal = (0, 0, 0).  Every output pixel is written by every call.
 * IEEE divisions and square root, no atomics: two calls give the same bits.  The kernel may skip samples it can prove unobserved (a
 * ray / box slab test with a conservative margin, a weight probe in front of the D gathers); the result does not depend on it.
 * ESTD_ERR_ARG: null pointers (stats excepted), H, W or n_steps <= 0, dt not finite or <= 0, t_min negative or not finite, w_min or an
 * element of mat not finite / NaN, X % 4, a dimension <= 0.  ESTD_ERR_UNSUPPORTED: the volume limits above, H * W >= 2^31,
 * n_steps > 2^24 (k is exact in fp32 up to there). */
typedef struct estd_tsdf_raycast_desc {
    int Z, Y, X;                                  /* volume dimensions */
    int H, W;                                     /* size of the output maps */
    int n_steps;                                  /* samples per ray */
    float t_min, dt;                              /* z-depth of sample 0 and the step, in the units of voxel_size */
    float w_min;                                  /* a corner counts as observed from this weight */
    const float* tsdf;                            /* [Z][Y][X] */
    const float* weight;                          /* [Z][Y][X] */
    float* depth;                                 /* [H][W] */
    float* normal;                                /* [H][W][3] */
    float* out_weight;                            /* [H][W] */
    unsigned int* stats;                          /* NULL, or measurement only (tools/tsdf_bench.py) [H][W][2]: samples whose weights
                                                     were read, samples whose D values were read */
    float mat[12];                                /* host values, copied into the launch arguments */
} estd_tsdf_raycast_desc;
int estd_tsdf_raycast(const estd_tsdf_raycast_desc* desc, estd_stream_t stream);

/* The same render with a colour map.  Depth, normal and weight come out bit-identical to the call without colour.  At the hit between
 * samples k - 1 and k, per channel: Cb = the trilinear blend of the eight corner colours of a sample's cell with the nesting of Wb;
 *   out_color = fma(s, Cb_k - Cb_{k-1}, Cb_{k-1}).
 * Both cells are observed, so every corner has been fused at least once.  No hit: (0, 0, 0).  The 2 x 8 x 3 colour values are read once
 * per pixel, at the hit.  Errors as above; in addition ESTD_ERR_ARG for a null `color` or `out_color`. */
typedef struct estd_tsdf_raycast_color_desc {
    int Z, Y, X;
    int H, W;
    int n_steps;
    float t_min, dt;
    float w_min;
    const float* tsdf;                            /* [Z][Y][X] */
    const float* weight;                          /* [Z][Y][X] */
    float* depth;                                 /* [H][W] */
    float* normal;                                /* [H][W][3] */
    float* out_weight;                            /* [H][W] */
    unsigned int* stats;                          /* NULL, or measurement only [H][W][2] */
    float mat[12];
    const float* color;                           /* [3][Z][Y][X] */
    float* out_color;                             /* [H][W][3] */
} estd_tsdf_raycast_color_desc;
int estd_tsdf_raycast_color(const estd_tsdf_raycast_color_desc* desc, estd_stream_t stream);

/* ---- cross-view consistency of depth maps (csrc/depth_consistency.hip) ---------------------------
 * The step multi-view pipelines put between "depth per frame" and fusion (MVSNet's / COLMAP's geometric filter; the reference has none):
 * ONE target depth map is checked against S = 1..ESTD_CONSISTENCY_MAX_SOURCES source maps.  All maps are fp32 [H][W] of one size, pixel
 * centres on integers, z-depth along the optical axis: the conventions of estd_tsdf_integrate and estd_tsdf_raycast.
 *
 * mats[s][0] = F_s = [ K_s R_st K_t^-1 | K_s t_st ] takes (target pixel) x depth to source s, mats[s][1] = B_s is the same the other
 * way; R_st, t_st from inv(P_s) P_t with camera-to-world poses P.  HOST 3x4 row-major matrices in fp32 (estdepth_amd/camera.py
 * consistency_matrices forms them in float64).  With row(M, j; x, y, z) = fma(z, fma(M[j][0], x, fma(M[j][1], y, M[j][2])), M[j][3])
 * and lerp(a, b, f) = fma(f, b - a, a), per target pixel (u, v):
 *   1. d = target[v][u]; the pixel is INVALID unless d is finite and d > z_near: all four outputs are 0.  For each source, in order:
 *   2. a, b, c = row(F, 0 / 1 / 2; u, v, d); skip the source unless c > z_near; us = a / c, vs = b / c;
 *   3. skip unless 0 <= us <= W - 1 and 0 <= vs <= H - 1 (false for a NaN); x0 = min(floor(us), W - 2), y0 = min(floor(vs), H - 2);
 *      the taps t00 = source[y0][x0], t10 = [y0][x0 + 1], t01 = [y0 + 1][x0], t11 = [y0 + 1][x0 + 1]; skip unless all four are finite
 *      and > z_near;
 *   4. fx = us - x0, fy = vs - y0; ds = lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy);
 *   5. a', b', c' = row(B, 0 / 1 / 2; us, vs, ds); skip unless c' > z_near; u' = a' / c', v' = b' / c'.  The source is now VISIBLE;
 *   6. e2 = fma(u' - u, u' - u, (v' - v) (v' - v)), rel = |c' - d| / d; the source is CONSISTENT iff e2 < px_max^2 and rel < rel_max
 *      (px_max^2 = px_max * px_max, formed once on the host in fp32).
 * Outputs, fp32 [H][W], every pixel written by every call:
 *   views   = the number of consistent sources;          visible = the number of visible sources;
 *   depth   = (d + c'_1 + c'_2 + ...) / (1 + views), the c' of the consistent sources added to d in source order: the target's own depth
 *             where nothing agrees, so the map can be fused as it is (gate it with `views`);
 *   rel_err = (rel_1 + rel_2 + ...) / views over the consistent sources in source order; 0 where views = 0.
 * IEEE divisions, no atomics: two calls give the same bits.
 * ESTD_ERR_ARG (before any launch, no device needed): a null descriptor, a null map pointer (source[s] for s < S), S outside
 * 1..ESTD_CONSISTENCY_MAX_SOURCES, H < 2 or W < 2, px_max or rel_max not finite or <= 0 (or px_max^2 not a positive finite fp32),
 * z_near negative or not finite, a matrix element of a source s < S not finite.  ESTD_ERR_UNSUPPORTED: H * W >= 2^31. */
#define ESTD_CONSISTENCY_MAX_SOURCES 8
typedef struct estd_depth_consistency_desc {
    int H, W;                                                 /* size of every map */
    int S;                                                    /* sources in this call */
    float px_max, rel_max, z_near;
    const float* target;                                      /* [H][W] */
    const float* source[ESTD_CONSISTENCY_MAX_SOURCES];        /* [H][W] each */
    float* views;                                             /* [H][W] */
    float* visible;                                           /* [H][W] */
    float* depth;                                             /* [H][W] */
    float* rel_err;                                           /* [H][W] */
    float mats[ESTD_CONSISTENCY_MAX_SOURCES][2][12];          /* F_s, B_s: host values, copied into the launch arguments */
} estd_depth_consistency_desc;
int estd_depth_consistency(const estd_depth_consistency_desc* desc, estd_stream_t stream);

/* ---- nearest neighbours between point clouds and voxel-grid down-sampling (csrc/cloud_nn.hip) ----
 * What the 3D scores of a reconstruction are made of (estdepth_amd/cloud_metrics.py: accuracy, completeness, precision / recall /
 * F-score, chamfer distance).  Clouds are fp32 [n][3], every coordinate finite (the caller's duty; cloud_metrics.py checks it).
 *
 * The grid: cell_j(p) = (int)min(max(floor((p_j - lo_j) * inv_cell), 0), dims_j - 1) with inv_cell = 1.0f / cell formed once by the
 * entry point in fp32, and key(p) = (cell_2 dims[1] + cell_1) dims[0] + cell_0; dims[j] counts the cells along coordinate j.
 * lo3 and dims3 are HOST pointers to three values.  estd_cloud_cell_keys writes key(points[i]) to keys[i], i < n (a point outside
 * the grid gets the clamped cell).  ESTD_ERR_ARG: n < 0, a null pointer (points / keys: with n > 0), lo not finite, cell or
 * 1.0f / cell not positive and finite, a dims_j outside 1..ESTD_CLOUD_KEY_MAX_DIM.  ESTD_ERR_UNSUPPORTED: n >= 2^31.  n == 0 launches
 * nothing. */
#define ESTD_CLOUD_KEY_MAX_DIM (1 << 20)
#define ESTD_CLOUD_MAX_DIM 1024
#define ESTD_CLOUD_MAX_CELLS (1 << 24)
#define ESTD_CLOUD_MAX_ATTRS 6
int estd_cloud_cell_keys(const float* points, long long n, const float* lo3, float cell, const int* dims3, long long* keys,
                         estd_stream_t stream);

/* Nearest target per query.  THE CONTRACT, defined to the bit and independent of the grid: for query q and EVERY target p, in fp32,
 *   dx = qx - px, dy = qy - py, dz = qz - pz;   d2 = fma(dx, dx, fma(dy, dy, dz * dz));
 *   d2min = the smallest d2 over all targets;   index = the SMALLEST original target index attaining d2min;
 *   found iff d2min <= r2, r2 = max_dist * max_dist (formed once by the entry point in fp32);
 *   dist[q] = the IEEE correctly rounded square root of d2min, or max_dist when not found;   index[q] = index, or -1 when not found.
 * Every element of dist [M] and index [M] is written by every call, with plain vector stores and no atomics: two calls give the same
 * bits.  N == 0: nothing is found (records, cell_start and the grid are not read).  M == 0: no launch.
 *
 * The targets arrive sorted by key (stable) as 16-byte records: records[j] = (x, y, z, the bits of the int32 original index), 16-byte
 * aligned, and cell_start [cells + 1] (int32): cell_start[k] = the number of targets whose key is < k.  The kernel walks the cells in
 * rings around the query's (clamped) cell and stops in front of ring r >= 2 once (1 - 2^-5) ((r - 1) cell)^2 exceeds the smallest d2
 * so far (at most r2): with dims_j <= ESTD_CLOUD_MAX_DIM the cell coordinates are off by less than 2^-12 cells, so no target that could
 * win or tie is skipped, and `cell` never changes a bit of the output.  `order` [M] (or NULL = identity) is the order the queries are
 * taken in -- a permutation of 0..M-1, sorted by the queries' own keys so that the lanes of a wave share cells; results are written
 * at the query's own position; an entry outside 0..M-1 is ignored.  `stats` (or NULL; measurement only, tools/cloud_bench.py): [M]
 * uint32, the candidates whose distance was evaluated.
 * ESTD_ERR_ARG (before any launch, no device needed): a null descriptor, M or N negative, max_dist not finite or <= 0 or with a square
 * that leaves fp32; with N > 0: null or misaligned records, null cell_start, a grid estd_cloud_cell_keys would reject, a dims_j above
 * ESTD_CLOUD_MAX_DIM, more than ESTD_CLOUD_MAX_CELLS cells; with M > 0: null query, dist or index.  ESTD_ERR_UNSUPPORTED: M or
 * N >= 2^31. */
typedef struct estd_cloud_nearest_desc {
    long long M, N;                               /* queries, targets */
    const float* query;                           /* [M][3] */
    const long long* order;                       /* [M] or NULL */
    const float* records;                         /* [N][4], sorted by key */
    const int* cell_start;                        /* [dims[0] dims[1] dims[2] + 1] */
    float* dist;                                  /* [M] */
    long long* index;                             /* [M] */
    unsigned int* stats;                          /* NULL, or [M] */
    float lo[3];                                  /* host values, copied into the launch arguments */
    float cell;
    float max_dist;
    int dims[3];
} estd_cloud_nearest_desc;
int estd_cloud_nearest(const estd_cloud_nearest_desc* desc, estd_stream_t stream);

/* Voxel-grid down-sampling: one output point per occupied cell, the mean of the cell's points.  The host sorts the points by key
 * (stable, so a cell's points keep their original order) and passes `order` [n] (sorted position -> original index) and `segments`
 * [K + 1] (cell k owns the sorted positions segments[k] .. segments[k + 1] - 1).  Per cell and column the values are added in float64
 * in that order, divided by the count in float64 and rounded to fp32 once: out_points [K][3], and out_attrs [K][C] from the optional
 * attribute columns attrs [n][C], C <= ESTD_CLOUD_MAX_ATTRS (normals, colour).  Cells come out in the order of `segments` (ascending
 * key): the result does not depend on the launch shape.  Entries of `order` outside 0..n-1 are left out, segment bounds are clamped
 * to 0..n.  ESTD_ERR_ARG: n or K negative, K > n, C outside 0..ESTD_CLOUD_MAX_ATTRS, a null pointer with K > 0 (attrs / out_attrs:
 * with C > 0).  ESTD_ERR_UNSUPPORTED: n >= 2^31.  K == 0 launches nothing. */
int estd_cloud_cell_centroids(const float* points, const float* attrs, int C, long long n, const long long* order,
                              const long long* segments, long long K, float* out_points, float* out_attrs, estd_stream_t stream);

/* ---- k nearest neighbours and PCA normals of a point cloud (csrc/cloud/cloud_knn.hip; numpy form: tests/cloud_knn_ref.py) ----
 * The k nearest targets per query.  THE CONTRACT, defined to the bit and independent of the grid: for query q and EVERY target p, in
 * fp32, d2 exactly as estd_cloud_nearest forms it:
 *   dx = qx - px, dy = qy - py, dz = qz - pz;   d2 = fma(dx, dx, fma(dy, dy, dz * dz)).
 *   A candidate's key is the pair (d2, original index), ordered lexicographically.  The result is the k smallest keys among the
 *   candidates with d2 <= r2, r2 = max_dist * max_dist (formed once by the entry point in fp32), in ascending order;
 *   count[q] = how many there are (<= k);   dist[q][j] = the IEEE correctly rounded square root of the j-th d2, index[q][j] its index;
 *   the slots j >= count[q] hold max_dist and -1.
 * 1 <= k <= ESTD_CLOUD_KNN_MAX.  Column 0 is, bit for bit, what estd_cloud_nearest returns.  Every element of dist [M][k], index [M][k]
 * (int32) and count [M] (int32) is written by every call with plain stores and no atomics: two calls give the same bits, and the grid,
 * the cell edge and `order` change none.  N == 0: nothing is found.  M == 0: no launch.
 *
 * records, cell_start, the grid and `order` are estd_cloud_nearest's (an `order` entry outside 0..M-1 is ignored).  The kernel walks
 * the same rings and stops in front of ring r >= 2 once (1 - 2^-5) ((r - 1) cell)^2 exceeds the d2 of the current k-th key (r2 while
 * fewer than k candidates have been found); a candidate that ties the k-th d2 is still examined, so the index decides.  `stats` (or
 * NULL; measurement only): [M] uint32, the candidates whose distance was evaluated.
 * ESTD_ERR_ARG (before any launch, no device needed): what estd_cloud_nearest refuses, k outside 1..ESTD_CLOUD_KNN_MAX, with M > 0 a
 * null count.  ESTD_ERR_UNSUPPORTED: M or N >= 2^31. */
#define ESTD_CLOUD_KNN_MAX 32
typedef struct estd_cloud_knn_desc {
    long long M, N;                               /* queries, targets */
    const float* query;                           /* [M][3] */
    const long long* order;                       /* [M] or NULL */
    const float* records;                         /* [N][4], sorted by key */
    const int* cell_start;                        /* [dims[0] dims[1] dims[2] + 1] */
    float* dist;                                  /* [M][k] */
    int* index;                                   /* [M][k] */
    int* count;                                   /* [M] */
    unsigned int* stats;                          /* NULL, or [M] */
    float lo[3];                                  /* host values, copied into the launch arguments */
    float cell;
    float max_dist;
    int dims[3];
    int k;
} estd_cloud_knn_desc;
int estd_cloud_knn(const estd_cloud_knn_desc* desc, estd_stream_t stream);

/* Normals by a plane fit over the neighbours estd_cloud_knn found: points [n][3] is the cloud that index [m][k] (int32) names, query
 * [m][3] the points the lists belong to (read for the sign only), count [m] (int32, clamped to 0..k) how many entries of a row are used,
 * in list order.  With c = count[q] and p_i the used neighbours, everything in float64 and uncontracted (numpy reproduces the bits):
 *   mean_j = (sum_i (double)p_i[j]) / c;   x_i = (double)p_i - mean;   C_ab = sum_i (x_ia * x_ib), each product rounded, then added,
 *   ab = xx, xy, xz, yy, yz, zz -> cov [m][6] (or NULL; for tests and measurement).  c == 0 or a refused row: zeros.
 * The eigenproblem of C is solved in float64 inside the kernel by the cyclic Jacobi method (eight sweeps).  eig [m][3]: the eigenvalues
 * ascending, clamped at 0 from below, rounded to fp32 once.  normal [m][3]: the unit eigenvector of the smallest, rounded to fp32 once.
 *   valid[q] = 1 iff c >= 3, every used index lies in [0, n), l2 > 0 and (l1 - l0) > 2^-16 l2; otherwise 0, and the normal is zero.
 *   An index out of range is never an address: the row is invalid, and its eig and cov are zero.  invalid[0] (int64) = the invalid rows,
 *   one integer atomic per wave (set to 0 by the entry point first).
 * Sign.  toward (or NULL): 3 floats (toward_per_query == 0) or [m][3] (toward_per_query != 0) on the device; the fp32 normal is flipped
 *   so that sum_j n_j ((double)toward_j - (double)query_j) >= 0, evaluated in float64 left to right.  Without toward, or when that sum
 *   is exactly 0, the component of largest magnitude is positive, the lowest axis winning among equal magnitudes.
 * ESTD_ERR_ARG (before any launch): n or m negative, k outside 1..ESTD_CLOUD_KNN_MAX, with m > 0 a null query, index, count, normal,
 * eig, valid or invalid, with m > 0 and n > 0 null points.  ESTD_ERR_UNSUPPORTED: n or m >= 2^31.  m == 0: no launch, nothing written. */
int estd_cloud_normals(const float* points, long long n, const float* query, long long m, const int* index, const int* count, int k,
                       const float* toward, int toward_per_query, float* normal, float* eig, unsigned char* valid, long long* invalid,
                       double* cov, estd_stream_t stream);

/* ---- density-based clustering of a point cloud, DBSCAN (csrc/cloud/cloud_cluster.hip; numpy form: tests/cloud_cluster_ref.py) ----
 * Neighbours within a radius.  For query q and EVERY target p, in fp32, d2 exactly as estd_cloud_nearest forms it:
 *   dx = qx - px, dy = qy - py, dz = qz - pz;   d2 = fma(dx, dx, fma(dy, dy, dz * dz));
 *   count[q] = the number of targets with d2 <= r2, r2 = radius * radius (formed once by the entry point in fp32).  The test is
 *   INCLUSIVE: a target at d2 == r2 counts.  There is no cap on the count.
 * count [M] (int32) is written by every call with plain stores; records, cell_start, the grid and `order` are estd_cloud_nearest's (an
 * `order` entry outside 0..M-1 is ignored), and the cell edge changes no value: the kernel walks the rings up to the constant bound r2.
 * N == 0: every count is 0.  M == 0: no launch.
 * ESTD_ERR_ARG (before any launch, no device needed): what estd_cloud_nearest refuses (radius in the place of max_dist), with M > 0 a
 * null query or count.  ESTD_ERR_UNSUPPORTED: M or N >= 2^31. */
typedef struct estd_cloud_count_within_desc {
    long long M, N;                               /* queries, targets */
    const float* query;                           /* [M][3] */
    const long long* order;                       /* [M] or NULL */
    const float* records;                         /* [N][4], sorted by key */
    const int* cell_start;                        /* [dims[0] dims[1] dims[2] + 1] */
    int* count;                                   /* [M] */
    float lo[3];                                  /* host values, copied into the launch arguments */
    float cell;
    float radius;
    int dims[3];
} estd_cloud_count_within_desc;
int estd_cloud_count_within(const estd_cloud_count_within_desc* desc, estd_stream_t stream);

/* DBSCAN of the cloud the records hold (N points, original indices 0..N-1).  THE CONTRACT, defined to the integer and independent of
 * the grid, the launch shape and the scheduling:
 *   d2(i, j) is the expression above between points i and j.  It is exactly symmetric: negating dx, dy and dz changes no bit.
 *   r2 = eps * eps, formed once by the entry point in fp32.  j is a NEIGHBOUR of i iff d2(i, j) <= r2 (inclusive); i is its own.
 *   count[i] = the number of neighbours of i.  i is a CORE point iff count[i] >= min_points.
 *   Clusters are the connected components of the graph on the CORE POINTS ONLY, with an edge where two core points are neighbours; a
 *   point that is not core never links two clusters.
 *   label[i], i core     = the smallest original index among the core points of i's component.
 *   label[i], i not core = label[b], b the core neighbour of i with the smallest key (d2(i, b), b), ordered lexicographically: the
 *                          nearest core neighbour, the smaller index among equals; -1 (noise) when i has no core neighbour.
 *   size[r]  = the number of points i, core or not, with label[i] == r; 0 at every index that is no label.
 *   noise[0] = the number of points with label -1.
 * count, label, size [N] and noise [1] (all int32) are written completely by every call; parent [N] (int32) is work space whose content
 * afterwards is unspecified.  The only atomics are integer ones (compare-and-swap and min on parent, add on size and noise); all of
 * them commute, so two calls give the same values.  A permutation of the points permutes the partition with it.  A record whose index
 * lies outside 0..N-1 is skipped and never an address.  N == 0 launches nothing and writes nothing.
 * ESTD_ERR_ARG (before any launch, no device needed): a null descriptor, N negative, min_points < 1, eps not finite or <= 0 or with a
 * square that leaves fp32; with N > 0: null or misaligned records, null cell_start, a grid estd_cloud_nearest would refuse, a null
 * count, parent, label, size or noise.  ESTD_ERR_UNSUPPORTED: N >= 2^31. */
typedef struct estd_cloud_dbscan_desc {
    long long N;                                  /* points */
    const float* records;                         /* [N][4], sorted by key */
    const int* cell_start;                        /* [dims[0] dims[1] dims[2] + 1] */
    int* count;                                   /* [N] */
    int* parent;                                  /* [N], work space */
    int* label;                                   /* [N] */
    int* size;                                    /* [N] */
    int* noise;                                   /* [1] */
    float lo[3];                                  /* host values, copied into the launch arguments */
    float cell;
    float eps;
    int dims[3];
    int min_points;
} estd_cloud_dbscan_desc;
int estd_cloud_dbscan(const estd_cloud_dbscan_desc* desc, estd_stream_t stream);

/* ---- global registration: FPFH descriptors, feature matching, three-point hypotheses (csrc/register/global_register.hip; numpy form:
 * tests/global_reg_ref.py) ----
 * Every decision below is taken in float64 operations (or integers) written in a fixed order and NOT contracted: a * b + c is a rounded
 * product and a rounded sum.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2;  cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0);
 * norm(a) = sqrt(dot(a, a)) with the IEEE square root; a / s divides each component.  No float atomics anywhere: two calls, either
 * binding and any launch shape give the same bits.
 *
 * SPFH (simplified point feature histograms).  points [n][3], normal [n][3] (a row of three zeros: no normal), index [n][k] (int32) and
 * count [n] (int32, clamped to 0..k) as estd_cloud_knn writes them for the cloud against itself, 1 <= k <= ESTD_CLOUD_KNN_MAX.  For point
 * s and each used list entry t, in list order, everything widened to float64:
 *   d = p_t - p_s;  len = norm(d);  dn = d / len;  u = n_s;  phi = dot(u, dn);  v = cross(dn, u);  vl = norm(v);  v = v / vl;
 *   w = cross(u, v);  alpha = dot(v, n_t);  y = dot(w, n_t);  x = dot(u, n_t).
 *   The pair is SKIPPED (not counted) when t == s, t lies outside [0, n) (never an address), n_s or n_t is zero, len == 0 or vl == 0.
 *   oriented != 0:  a = min(max(alpha, -1), 1), f = phi alike;  bin_alpha = min(10, (int)floor((a + 1) * 5.5)), bin_phi alike;
 *                   q = |x| + |y|;  bin_theta = 5 when q == 0, else with r = y / q and
 *                   pa = r (x >= 0), 2 - r (x < 0, y >= 0), -2 - r (otherwise):  min(10, (int)floor((pa + 2) * 2.75)).
 *   oriented == 0:  alpha, phi, y, x are replaced by their absolute values first, and the half ranges are cut into the same 11 bins:
 *                   bin_alpha = min(10, (int)floor(min(alpha, 1) * 11)), bin_phi alike;  bin_theta = 5 when q == 0, else
 *                   min(10, (int)floor((y / q) * 11)).  Changing the sign of any normal changes no bit of the result.
 *   The pseudo-angle pa is a monotone function of atan2(y, x) in [-2, 2]: no transcendental function is evaluated.  PCL bins atan2
 *   itself and swaps source and target by the angle to the connecting line; neither is done here.
 *   hist [n][33] (int32): the counts, alpha in 0..10, phi in 11..21, theta in 22..32;  pairs [n] (int32): the pairs counted.
 * ESTD_ERR_ARG: n negative, k outside 1..ESTD_CLOUD_KNN_MAX, with n > 0 a null pointer.  ESTD_ERR_UNSUPPORTED: n >= 2^31.  n == 0: no
 * launch. */
#define ESTD_FPFH_BINS 33
int estd_cloud_spfh(const float* points, const float* normal, long long n, const int* index, const int* count, int k, int oriented,
                    int* hist, int* pairs, estd_stream_t stream);

/* FPFH from the SPFH of a cloud: the same points, normal, index, count and k, hist and pairs as estd_cloud_spfh wrote them.  For point
 * i, acc_b = 0, m = 0, and for each used list entry j in list order that is not i, lies in [0, n), has pairs_j > 0 and
 * d2 = dot(p_j - p_i, p_j - p_i) > 0 (float64):  wj = 1.0 / ((double)pairs_j * d2);  acc_b = acc_b + (double)hist_j[b] * wj for
 * every b;  m = m + 1.  Then
 *   F_b = (pairs_i > 0 ? (double)hist_i[b] / (double)pairs_i : 0.0) + (m > 0 ? acc_b / (double)m : 0.0),
 * and per group of 11 bins g = (((F_0 + F_1) + F_2) + ... + F_10);  desc [n][33] (fp32) = (float)(F_b / g), or 0 for a group with
 * g == 0: rounded to fp32 once.  valid [n] (uint8) = 1 iff n_i is not zero and pairs_i >= 3;  invalid[0] (int64) = the rows with
 * valid == 0, one integer atomic per wave (set to 0 by the entry point first).
 * ESTD_ERR_ARG / ESTD_ERR_UNSUPPORTED: as for estd_cloud_spfh.  n == 0: no launch, nothing written. */
int estd_cloud_fpfh(const float* points, const float* normal, long long n, const int* index, const int* count, int k, const int* hist,
                    const int* pairs, float* desc, unsigned char* valid, long long* invalid, estd_stream_t stream);

/* Nearest and second-nearest descriptor by brute force.  a [m][33], b [n][33] (fp32); a_valid [m], b_valid [n] (uint8, or NULL: every
 * row).  For row i of a and every row j of b with b_valid[j] != 0, in fp32:
 *   e_c = a[i][c] - b[j][c];   d2 = e_0 * e_0;   d2 = fma(e_c, e_c, d2) for c = 1 .. 32 in this order.
 * index [m] (int32) = the j of the smallest key (d2, j), d2 [m] its d2, d2_second [m] the second smallest d2 of the row (equal to d2
 * when two rows tie).  Without a partner: -1, +inf;  with a single one: d2_second = +inf;  a row with a_valid[i] == 0 gets -1, +inf, +inf.
 * A d2 that is NaN never wins.  ESTD_ERR_ARG: m or n negative, with m > 0 a null a or output, with m > 0 and n > 0 a null b.
 * ESTD_ERR_UNSUPPORTED: m or n >= 2^31.  m == 0: no launch. */
int estd_feature_match(const float* a, long long m, const float* b, long long n, const unsigned char* a_valid, const unsigned char* b_valid,
                       int* index, float* d2, float* d2_second, estd_stream_t stream);

/* Three-point hypotheses over correspondences (RANSAC's hypothesise-and-verify, every hypothesis evaluated).  P [c][3], Q [c][3] (fp32):
 * row r pairs a source point with a target point.  Hypothesis h in 0 .. hypotheses - 1 draws c_j = h64(seed, h, j) mod c, j = 0, 1, 2
 * (the mixer of estd_mesh_sample: two rounds of SplitMix64's finaliser, see there), a, b, c = rows c_0, c_1, c_2, widened to float64.
 * status [hypotheses] (uint8), tested in this order:
 *   1  two of c_0, c_1, c_2 are equal;
 *   2  for one of the edges (a, b), (b, c), (c, a), with lp = norm of the edge in P and lq in Q:  lp < edge_ratio * lq or
 *      lq < edge_ratio * lp  (Open3D's edge-length checker);
 *   3  a degenerate frame: on either side norm(b - a) == 0 or norm(cross(e1, c - a)) == 0, or R or t below is not finite;
 *   0  scored.
 * The transform, closed form: on each side e1 = (b - a) / norm(b - a);  e3 = cross(e1, c - a) / its norm;  e2 = cross(e3, e1);
 *   R_ij = (e1q_i e1p_j + e2q_i e2p_j) + e3q_i e3p_j;   cen = ((a + b) + c) / 3.0;   t_i = cenq_i - ((R_i0 cenp_0 + R_i1 cenp_1) + R_i2 cenp_2).
 * The score over ALL rows r:  m_i = ((R_i0 p_0 + R_i1 p_1) + R_i2 p_2) + t_i;  e = m - q;  r2 = (e_0 e_0 + e_1 e_1) + e_2 e_2;  the row
 * is an inlier iff r2 <= dist_max * dist_max (the product formed once, in float64).
 *   count [hypotheses] (int32) = the inliers;  ssq [hypotheses] (float64) = the sum of their r2: lane l of 64 adds its rows l, l + 64, ...
 *   in ascending order, then the lanes are joined by an exclusive-or butterfly (lane distances 32 .. 1), as estd_rigid_system joins them;
 *   T [hypotheses][12] (float64) = the rows of [R | t].  A hypothesis with status != 0 gets count 0, ssq 0 and T zero.
 *   best[0] (uint64, set to 0 by the entry point first) = the largest key  (count << 32) | (0xffffffff - h)  over the scored hypotheses,
 *   by an integer atomic maximum: the largest count and among equals the smallest h, whatever the schedule; 0 = nothing was scored.
 * ESTD_ERR_ARG: c or hypotheses negative, dist_max not finite or negative, edge_ratio outside [0, 1], with hypotheses > 0 a null output,
 * with hypotheses > 0 and c > 0 a null P or Q.  ESTD_ERR_UNSUPPORTED: c or hypotheses >= 2^31.  hypotheses == 0: no launch, nothing
 * written.  c == 0: every status is 1. */
int estd_ransac_pairs(const float* P, const float* Q, long long c, long long hypotheses, unsigned long long seed, double dist_max,
                      double edge_ratio, int* count, unsigned char* status, double* ssq, double* T, unsigned long long* best,
                      estd_stream_t stream);

/* ---- frame-to-model alignment of a depth map (csrc/track/frame_align.hip) -------------------------
 * Projective point-to-plane alignment, KinectFusion's tracking step: ONE live depth map against ONE set of model maps, the depth and
 * normal maps estd_tsdf_raycast writes (normals in world axes towards the cameras, no hit = zeros).  One call forms the Gauss-Newton
 * system of the frame at the pose guess and the per-pixel picture "does this frame sit on the model".  All maps are fp32, pixel centres
 * on integers, z-depth along the optical axis: the conventions of estd_tsdf_integrate and estd_tsdf_raycast.
 *
 * Three HOST 3x4 row-major fp32 matrices (estdepth_amd/camera.py frame_align_matrices forms them in float64; poses are camera-to-world,
 * R_g, c_g of the guess, R_m, c_m of the model camera):
 *   L  = [ R_g K^-1 | c_g ]            (live pixel) x depth -> world;
 *   Fm = K_m [R|t]_world->model        world -> (model pixel) x depth;
 *   Bm = [ R_m K_m^-1 | c_m ]          (model pixel) x depth -> world.
 * With row(M, j; x, y, z) = fma(z, fma(M[j][0], x, fma(M[j][1], y, M[j][2])), M[j][3]), per live pixel (u, v):
 *   1. d = depth[v][u]; the pixel is SKIPPED unless d is finite, d > z_near and conf is NULL or conf[v][u] >= conf_min;
 *   2. p_j = row(L, j; u, v, d), j = x, y, z;
 *   3. a, b, c = fma(Fm[j][0], p_x, fma(Fm[j][1], p_y, fma(Fm[j][2], p_z, Fm[j][3]))), j = 0, 1, 2; skipped unless c > z_near;
 *   4. um = floor(a / c + 0.5), vm = floor(b / c + 0.5); skipped unless 0 <= um < Wm and 0 <= vm < Hm (false for a NaN);
 *   5. dm = m_depth[vm][um]; skipped unless dm > 0; n = m_normal[vm][um]; q_j = row(Bm, j; um, vm, dm);
 *   6. e = q - p; skipped unless fma(e_x, e_x, fma(e_y, e_y, e_z e_z)) <= dist_max^2 (dist_max * dist_max, formed once on the host in
 *      fp32; false for a NaN, so a model depth that is not finite skips the pixel);
 *   7. r = fma(n_x, e_x, fma(n_y, e_y, n_z e_z));  J = (n_x, n_y, n_z, w_x, w_y, w_z) with w = p x n:
 *        w_x = fma(p_y, n_z, -(p_z n_y)),  w_y = fma(p_z, n_x, -(p_x n_z)),  w_z = fma(p_x, n_y, -(p_y n_x)).
 *      r ~ n . (q - Exp(xi) p) linearised: the system belongs to the LEFT update P <- Exp(xi) P of the guess with xi = (t, omega) in world
 *      axes, and the Gauss-Newton step solves (sum J J^T) xi = sum J r.
 * Per-pixel outputs, every pixel written by every call with plain vector stores:
 *   residual [H][W] = r, or 0 where the pixel was skipped;   match [H][W] (int32) = vm Wm + um, or -1 where it was skipped.
 * sums: ESTD_FRAME_ALIGN_SUMS = 29 float64 values on the device,
 *   [0..20]  the upper triangle of sum J J^T, row by row: (0,0) (0,1) .. (0,5) (1,1) .. (1,5) (2,2) .. (5,5);
 *   [21..26] sum J_i r;   [27] sum r^2;   [28] the number of matched pixels.
 * Each per-pixel term is ONE fp32 value (J_i * J_j, J_i * r, r * r, 1: a product rounded once), widened and added in float64.  No
 * atomics; the order is fixed: the lanes of a wave (an exclusive-or butterfly over lane distances 32 .. 1), the four waves of a 16 x 16
 * pixel workgroup in wave order, then the workgroups: lane l of the reduction adds workgroups l, l + 64, ... in ascending order and the
 * same butterfly joins the lanes.  The 29 values are bit-identical across calls.
 * partials: device scratch of estd_frame_align_partials(H, W) BYTES (29 float64 per 16 x 16 tile of the live map), owned by the caller;
 * the function returns 0 for sizes the entry point refuses.
 * ESTD_ERR_ARG (before any launch, no device needed): a null descriptor or pointer (conf excepted), a size <= 0, dist_max or its square
 * not a positive finite fp32, z_near negative or not finite, conf_min NaN with a conf map, a matrix element not finite.
 * ESTD_ERR_UNSUPPORTED: H * W or Hm * Wm >= 2^31. */
#define ESTD_FRAME_ALIGN_SUMS 29
typedef struct estd_frame_align_desc {
    int H, W;                                     /* size of the live maps */
    int Hm, Wm;                                   /* size of the model maps */
    float dist_max, z_near, conf_min;
    const float* depth;                           /* [H][W] */
    const float* conf;                            /* [H][W] or NULL */
    const float* m_depth;                         /* [Hm][Wm] */
    const float* m_normal;                        /* [Hm][Wm][3] */
    float* residual;                              /* [H][W] */
    int* match;                                   /* [H][W] */
    double* sums;                                 /* [ESTD_FRAME_ALIGN_SUMS] */
    double* partials;                             /* estd_frame_align_partials(H, W) bytes */
    float L[12], Fm[12], Bm[12];                  /* host values, copied into the launch arguments */
} estd_frame_align_desc;
long long estd_frame_align_partials(int H, int W);
int estd_frame_align(const estd_frame_align_desc* desc, estd_stream_t stream);

/* The fused surface as a triangle mesh by naive surface nets (csrc/mesh/tsdf_mesh.hip; float64 form: tests/tsdf_mesh_ref.py): one vertex
 * per surface cell, one quad (two triangles) per sign-changing voxel edge -- the edges the point extraction ids as 3 * voxel + axis.
 * There is no case table: every topological decision compares stored fp32 values (D < 0, Wt >= w_min), so the vertex set and the face
 * list are defined to the integer; only the vertex attributes carry rounding.  The volume is [Z][Y][X] as above, ANY X >= 1 here.
 *
 * Cells.  Cell c = (cz, cy, cx), 0 <= c < dims - 1, has the eight voxels c + {0,1}^3 as corners (corner order: x fastest, then y, then
 *   z) and the linear voxel index of its lowest corner as id.  OBSERVED: all eight corner weights >= w_min (the ray caster's predicate).
 *   ACTIVE: observed, with a corner D < 0 and a corner that is not.
 * Crossings.  An edge with D0 at its lower-index end crosses when exactly one of D0 < 0, D1 < 0 holds; s = D0 / (D0 - D1) (IEEE division).
 * Vertex of an active cell.  Its twelve edges in a fixed order: the four x-edges, then the y-, then the z-edges; within an axis by the
 *   offsets (0/1) of the edge on the two other axes, the lower axis fastest: (0,0), (1,0), (0,1), (1,1).  Every crossing gives the
 *   cell-local point with s on the edge's axis and the edge's offsets on the other two; the points are added in that order, starting
 *   from 0, and divided by their number n:  xyz_k = fma((float)c_k + 0.5f + sum_k / n, voxel_size, origin_k)     (k = x, y, z)
 *   normal: g_k = the sum over the four k-edges, in the same order and from 0, of D1 - D0; normal = g / sqrt(fma(gz, gz, fma(gy, gy,
 *           gx gx))), the zero vector when that length is 0.  Points towards increasing D = the free space.
 *   weight: the eight corner weights added in corner order from 0, times 0.125.
 *   colour (color != NULL; [3][Z][Y][X]): per channel the sum over the crossings, same order, of fma(s, C1 - C0, C0), divided by n.
 * Faces.  For a voxel v and an axis a whose +a edge crosses, with (b, c) the next two axes cyclically (x: y z; y: z x; z: x y): the four
 *   cells round the edge are q0 = v - e_b - e_c, q1 = v - e_c, q2 = v, q3 = v - e_b.  All four must exist and be observed, else there
 *   is no face.  The record is {edge = 3 * index of v + a, quad}: quad = (q0, q1, q2, q3) when D0 < 0 (free space on the +a side), else
 *   (q3, q2, q1, q0); its triangles are (quad0, quad1, quad2), (quad0, quad2, quad3): counter-clockwise seen from the free side.  Every
 *   cell of a record is active, so it is among the vertices.
 * Known limit: a cell two separate sheets cross gets ONE vertex, the sheets pinch together there (marching cubes would keep them apart).
 *
 * Protocol of both calls (the point extraction's): `counter` (device, zeroed by the caller) ends at the TOTAL number of records -- one
 * integer increment per wave (ballot + population count; no float atomics); records whose slot is >= capacity are dropped;
 * capacity == 0 counts only (the output pointers may then be NULL).  Order unspecified: sort by cell / by edge.  origin3 is a HOST pointer.
 * cell [capacity] (int64), xyz, normal, vertex_color [capacity][3], vertex_weight [capacity]; edge [capacity] (int64), quad
 * [capacity][4] (int32, 16-byte aligned).  A dimension of 1 has no cells: ESTD_OK, nothing is launched or written.
 * ESTD_ERR_ARG (before any launch): a null tsdf, weight, origin3 or counter, an output pointer null with capacity > 0 (vertex_color:
 * only with color), capacity < 0, voxel_size not positive and finite, w_min NaN, a dimension <= 0.  ESTD_ERR_UNSUPPORTED: Z > 65535,
 * Y > 262140, X > 2^20, or more than 2^31 - 1 voxels (the ids in `quad` are 32-bit). */
int estd_tsdf_mesh_vertices(const float* tsdf, const float* weight, const float* color, int Z, int Y, int X, float voxel_size,
                            const float* origin3, float w_min, unsigned long long* counter, long long capacity, long long* cell,
                            float* xyz, float* normal, float* vertex_weight, float* vertex_color, estd_stream_t stream);
int estd_tsdf_mesh_faces(const float* tsdf, const float* weight, int Z, int Y, int X, float w_min, unsigned long long* counter,
                         long long capacity, long long* edge, int* quad, estd_stream_t stream);

/* The connected components of a triangle mesh (csrc/mesh/mesh_components.hip; numpy form: tests/mesh_components_ref.py): a lock-free
 * union-find over all workgroups, every output defined to the integer and independent of the order of the faces and of scheduling.
 *
 * Input.  faces [n_faces][3] int32, contiguous: vertex indices; n_vertices = V.  Two vertices are in one component when a chain of
 *   triangles links them; a triangle links its three vertices.  A triangle with repeated indices is a triangle like any other.
 *   A triangle with an index outside [0, V) is INVALID: it is ignored entirely -- its indices are never used as an address, it links
 *   nothing and is counted in `invalid` only.
 * Outputs (all device memory).
 *   label [V] int32: label[v] = the smallest vertex index of v's component; a vertex in no (valid) triangle has label[v] = v.  While the
 *     call runs the array is the parent forest of the union-find; no other scratch is needed.
 *   triangles [V] int32: at a root (label[r] == r) the number of valid triangles whose vertices carry label r, 0 everywhere else.
 *   invalid [1] int64: the number of invalid triangles.  Always written (the caller need not zero it).
 * Launches.  mesh_cc_init_kernel always (it defines label, triangles and invalid when there are no faces or no vertices); with V > 0
 *   and n_faces > 0 also mesh_cc_hook_kernel, mesh_cc_flatten_kernel and mesh_cc_count_kernel, in this order on `stream`.  The count
 *   uses integer atomics only, one per wave and distinct root.
 * ESTD_ERR_ARG (before any launch): n_faces < 0 or n_vertices < 0, a null `invalid`, a null `faces` with n_faces > 0, a null `label` or
 *   `triangles` with n_vertices > 0.  ESTD_ERR_UNSUPPORTED: n_vertices or 3 * n_faces beyond 2^31 - 1. */
int estd_mesh_components(const int* faces, long long n_faces, long long n_vertices, int* label, int* triangles, long long* invalid,
                         estd_stream_t stream);

/* An evenly spread point cloud on a triangle mesh (csrc/mesh/mesh_sample.hip; numpy form: tests/mesh_sample_ref.py): per-triangle areas,
 * then stratified sampling along the cumulative area.  Two entry points with integer glue between them, which the host layers
 * (estdepth_amd/ops.py, mesh_sample) own; a foreign host repeats it as written here.
 *
 * estd_mesh_face_area (mesh_face_area_kernel, one lane per triangle).  xyz [V][3] float32, faces [F][3] int32, both contiguous.
 *   A triangle with an index outside [0, V) is INVALID (estd_mesh_components' rule): its indices are never used as an address, its
 *   area is +0, its normal 0 0 0, and it is counted in invalid [1] int64, which the call zeroes first (a memset on `stream`) and
 *   raises with ONE integer atomic add per wave.  Otherwise, with a, b, c the vertices widened to float64 and every operation below
 *   one IEEE float64 operation in this order, never contracted into an fma:
 *     e1 = b - a;  e2 = c - a;
 *     nx = e1y * e2z - e1z * e2y;  ny = e1z * e2x - e1x * e2z;  nz = e1x * e2y - e1y * e2x;
 *     len = sqrt((nx * nx + ny * ny) + nz * nz);   area[f] = 0.5 * len;
 *     face_normal[f] = ((float)(nx / len), (float)(ny / len), (float)(nz / len)), or 0 0 0 when len == 0.
 *   area [F] float64 and face_normal [F][3] float32 are written with plain stores: two calls give the same bits.  F == 0: the memset
 *   alone.  ESTD_ERR_ARG: a negative size, a null `invalid`, a null xyz with V > 0, a null faces / area / face_normal with F > 0.
 *   ESTD_ERR_UNSUPPORTED: V or 3 F beyond 2^31 - 1.
 *
 * The glue.  scale = 2^e with e = 62 - ceil(log2 F) - k, where max(area) = m 2^k, 0.5 <= m < 1 (e = 0 without area, and at most
 *   1000); q_f = (int64) floor(area_f * scale), exact because scale is a power of two; cum = the running sum of q in int64, exact in
 *   any order; Q = cum[F - 1] < 2^62.  For N samples the stratum is w = Q / N (integer division); the host layers refuse Q == 0 and
 *   w < 2^20 (ESTD_MESH_SAMPLE_MIN_STRATUM: the Q mod N units no sample can reach are below 2^-20 of a stratum each).
 *
 * estd_mesh_sample (mesh_sample_kernel, one lane per sample).  Sample i = first + j, j < n_samples, all unsigned arithmetic mod 2^64:
 *     mix(z):  z ^= z >> 30;  z *= 0xbf58476d1ce4e5b9;  z ^= z >> 27;  z *= 0x94d049bb133111eb;  z ^= z >> 31;
 *     h64(seed, i, s) = mix(mix(seed + (i + 1) * 0x9e3779b97f4a7c15) + (s + 1) * 0xd1b54a32d192ed03);   h32 = h64 >> 32;
 *     t_i = i * w + (h64(seed, i, 0) mod w);   f_i = the first f with cum[f] > t_i (F - 1 should there be none);
 *     iu = h32(seed, i, 1) >> 8;  iv = h32(seed, i, 2) >> 8;  when iu + iv > 2^24:  iu = 2^24 - iu, iv = 2^24 - iv;
 *     u = iu * 2^-24,  v = iv * 2^-24 (exact in fp32: the fold to 1 - u, 1 - v when u + v > 1, with no rounding and no square root);
 *     with a, b, c the vertices of f_i, per coordinate in fp32:  p = fmaf(v, c - a, fmaf(u, b - a, a)).
 *   A triangle of q_f = 0 (no area, or invalid) is never chosen; triangle f holds, within +-2, N q_f / Q samples; the samples come
 *   in ascending i, hence in non-decreasing f.  Outputs, row j: out_xyz [n][3], out_face [n] int32 = f_i, out_bary [n][2] = (u, v),
 *   out_normal [n][3] = face_normal[f_i], out_attrs [n][C] = the expression of p on the rows of attrs [V][C] (0 <= C <=
 *   ESTD_CLOUD_MAX_ATTRS; C == 0: both attribute pointers are ignored), not renormalised.  Plain stores, no atomics: the result does
 *   not depend on the launch shape, and a call split at any `first` gives the same rows.  Should cum not belong to this mesh and f_i
 *   name a vertex outside [0, V), that row is face -1 and zeros: still never an address.
 *   n_samples == 0 launches nothing.  ESTD_ERR_ARG: a negative size or `first`, C outside 0..6, and with n_samples > 0: V == 0 or
 *   F == 0, w < 1 or (first + n_samples) * w > 2^62, a null pointer.  ESTD_ERR_UNSUPPORTED: V, 3 F or first + n_samples beyond 2^31 - 1. */
#define ESTD_MESH_SAMPLE_MIN_STRATUM (1 << 20)
int estd_mesh_face_area(const float* xyz, long long n_vertices, const int* faces, long long n_faces, double* area, float* face_normal,
                        long long* invalid, estd_stream_t stream);
int estd_mesh_sample(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const float* attrs, int C,
                     const long long* cum, const float* face_normal, long long n_samples, long long first, long long w,
                     unsigned long long seed, float* out_xyz, int* out_face, float* out_bary, float* out_normal, float* out_attrs,
                     estd_stream_t stream);

/* A z-buffer rasteriser for triangle lists (csrc/mesh/mesh_raster.hip; numpy form: tests/mesh_raster_ref.py): which triangle a camera
 * sees in every pixel, at which depth, where on the triangle and from which side.  Conventions of the TSDF ray-cast and integration:
 * pixel centres on integers, depth = the z-depth along the optical axis, poses camera-to-world.  Two entry points, rasterise and
 * resolve, with a key buffer between them that the caller owns.
 *
 * Inputs of both: xyz [V][3] float32, faces [F][3] int32, contiguous, on the device; mat: 12 DOUBLES ON THE HOST, 3 x 4 row-major,
 *   M = K [R^T | -R^T c] formed in float64 (estdepth_amd/camera.py, mesh_raster_matrix), so that the third component of M (x, 1) is the
 *   z-depth and pixel (u, v) is the ray direction (u, v, 1) of that space; H, W: the image.
 *
 * The arithmetic.  Every operation below is ONE IEEE float64 operation in the order written, never contracted into an fma.
 *   per vertex, widened to float64:   q_j = ((M_j0 * x + M_j1 * y) + M_j2 * z) + M_j3,   j = 0, 1, 2
 *   per triangle (q0, q1, q2):        n0 = q1 x q2,  n1 = q2 x q0,  n2 = q0 x q1,  each component a_y * b_z - a_z * b_y (two rounded
 *                                     products, one difference);   det = (n0x * q0x + n0y * q0y) + n0z * q0z
 *   per pixel (u, v), as doubles:     E_k = (n_kx * u + n_ky * v) + n_kz;   S = (E_0 + E_1) + E_2
 *     the triangle COVERS the pixel iff  E_0, E_1, E_2 >= 0 and S > 0,  or  E_0, E_1, E_2 <= 0 and S < 0  (both windings are drawn);
 *     c = det / S;  d = (float) c;  the triangle CONTRIBUTES iff d is finite and d > z_near.
 *   The cross product is exactly antisymmetric, so two triangles that share an edge see the same edge function with opposite sign
 *   and no pixel falls between them; a pixel on the edge belongs to both.  No clipping: the test is a ray-triangle test, a triangle
 *   that crosses the camera plane is drawn where its hit lies in front of z_near.  A comparison with a NaN is false: a triangle with
 *   a vertex that is not finite covers nothing, one of no area (S = 0 everywhere) neither.
 *   The winner of a pixel: key = ((uint64) bits(d) << 32) | f, the smallest key over all contributing triangles f -- d is a positive
 *   finite float32, whose bit pattern orders like its value, so the nearest surface wins and among equal depths the smallest face
 *   index.  A minimum does not depend on the order of arrival: the maps are bit-identical across calls, bindings, face ranges and
 *   launch shapes.
 *   The kernel may skip pixels it can prove uncovered (it sweeps the projections' bounding box with a one-pixel margin when all three
 *   q_z > z_near, the whole image otherwise) and triangles whose det is 0 or not finite (c is then 0, infinite or a NaN).
 *
 * estd_mesh_raster (mesh_raster_kernel, one wave per triangle): merges the triangles face_first .. face_first + face_count - 1 into
 *   keys [H][W] uint64 with 64-bit unsigned atomic minima at agent scope.  keys must be all ones before the first call: the flag
 *   ESTD_MESH_RASTER_CLEAR makes the call set it so first (a memset with 0xff on `stream`, no kernel); without the flag the call
 *   accumulates into the buffer as it is, and a mesh rendered in two face ranges gives the bits of one call.  A triangle with an index outside [0, V) is INVALID (estd_mesh_components' rule): never an address, covers
 *   nothing, and is counted in invalid [1] int64, which the call zeroes first (a memset on `stream`) and raises with one integer
 *   atomic add per wave: the count of THIS call's range.  flags: ESTD_MESH_RASTER_CLEAR, and ESTD_MESH_RASTER_PRELOAD -- with it a relaxed load stands
 *   in front of the atomic and skips it when key >= the value read (keys only decrease, so a value read is never smaller than the
 *   current one and the skip never loses a winner): faster where thousands of triangles want the same pixels, slower elsewhere
 *   (DESIGN 3.14).  The bits are the same.  face_count == 0 (F == 0
 *   included): the memsets alone.
 * estd_mesh_raster_resolve (mesh_resolve_kernel, one lane per pixel, a later launch on the same stream): unpacks keys and recomputes
 *   the winner's E_k and S (the same operations, the same bits).  Every pixel of every map is written by every call:
 *     depth [H][W] float32 = d, 0 = nothing;   face [H][W] int32 = f, -1 = nothing;
 *     bary [H][W][2] float32 = ((float)(E_1 / S), (float)(E_2 / S)): E_k / S is the 3D barycentric coordinate, so these are the
 *       perspective-correct weights of the second and third vertex and the point is a + b1 (b - a) + b2 (c - a);  0 0 = nothing;
 *     facing [H][W] int32 = +1 where S < 0, -1 where S > 0, 0 = nothing: +1 is a triangle whose vertices run counter-clockwise seen
 *       from the camera (in a right-handed world), i.e. the triangles of estd_tsdf_mesh_faces seen from the free side give +1.
 *   A key that names no face of this mesh (a foreign buffer) gives the empty pixel: still never an address.
 * ESTD_ERR_ARG, before any launch and with no device needed: a negative size, H or W <= 0, a null mat or one with an element that is
 *   not finite, a null xyz with V > 0 or faces with F > 0, a null keys / invalid / output map, z_near negative or not finite, an
 *   unknown flag, a face range outside [0, F].  ESTD_ERR_UNSUPPORTED: H * W, V or 3 F beyond 2^31 - 1. */
#define ESTD_MESH_RASTER_PRELOAD 1
#define ESTD_MESH_RASTER_CLEAR 2
int estd_mesh_raster(const float* xyz, long long n_vertices, const int* faces, long long n_faces, long long face_first, long long face_count,
                     const double* mat, int H, int W, float z_near, int flags, unsigned long long* keys, long long* invalid,
                     estd_stream_t stream);
int estd_mesh_raster_resolve(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const double* mat, int H, int W,
                             const unsigned long long* keys, float* depth, int* face, float* bary, int* facing, estd_stream_t stream);

/* Mesh simplification by vertex clustering with quadric placement (csrc/mesh/mesh_simplify.hip; numpy form: tests/mesh_simplify_ref.py):
 * every vertex that falls in one cell of a uniform grid becomes one vertex (Rossignac-Borrel), triangles that lose a corner disappear,
 * and the new vertex sits where the summed plane quadrics of the cell's triangles are smallest (Lindstrom 2000), which keeps the edges
 * and corners that the mean of the cell's vertices rounds off.  Two entry points with integer glue between them, which the host layer
 * (estdepth_amd/fusion3d.py, simplify_mesh) owns; a foreign host repeats it as written here.  Known limit: clustering does not preserve
 * topology -- two sheets closer than a cell weld, and edges shared by more than two triangles can appear; nothing repairs them.
 *
 * Grid and clusters (host glue).  The grid is the one of estd_cloud_cell_keys (lo3, cell, dims3, the same limits) and the key of a
 *   vertex is the key that entry point writes for it.  cell_key [K] int64 = the occupied keys in ascending order, cluster [V] int32 =
 *   the rank of the vertex's key among them (a stable sort of the keys, the distinct values, their ranks).  mean [K][3] float32 = the
 *   per-cluster mean of the vertices as estd_cloud_cell_centroids gives it for that sort.
 *
 * estd_mesh_cluster_faces (mesh_cluster_faces_kernel, one lane per input face).  faces [F][3] int32, cluster [V] int32.
 *   A face with an index outside [0, V) is INVALID (the rule of estd_mesh_components): never an address, its three corner records get
 *   cluster K, its triple is (-1, -1, -1), and it is counted in counts[0].  Otherwise corner[3 f + j] = cluster[faces[f][j]], taken
 *   as it is.  The face COLLAPSES when two of its three clusters are equal: counted in counts[1], triple (-1, -1, -1).  Otherwise
 *   triple[f] = the three clusters rotated so that the smallest comes first; the winding is kept.
 *   counts [2] int64 is zeroed by the call (a memset on `stream`) and raised with ONE integer atomic add per wave and counter.
 *   corner [3 F] int32 and triple [F][3] int32 are written with plain stores, every element by every call that launches.
 *   The glue after it: keep the faces whose triple is not (-1, -1, -1); among equal triples keep the one with the smallest input face
 *   index; emit the kept triples in ascending input face index.  The same three clusters in the opposite winding are a different
 *   triple and stay.  Stable sorts column by column: no packed key that could leave int64.
 *
 * estd_mesh_cluster_quadrics (mesh_cluster_quadric_kernel, eight neighbouring lanes per cluster).  The host sorts the 3 F corner records
 *   by cluster (stable, so a cluster's records ascend in r = 3 f + j) and passes order [3 F] int64 (sorted position -> r) and segments
 *   [K + 1] int64 (cluster k owns the sorted positions segments[k] .. segments[k + 1] - 1; the records of invalid faces, cluster K, lie
 *   behind segments[K]).  Every operation below is ONE IEEE float64 operation in the order written, never contracted into an fma.
 *     g = the cell of cell_key[k]:  gz = key / (dims0 dims1),  gy = (key - gz dims0 dims1) / dims0,  gx = the rest;
 *     centre_i = (double)lo_i + ((double)g_i + 0.5) * (double)cell.
 *   Per record r = 3 f + j of the segment, with a, b, c the vertices of face f in the face's own order, widened to float64:
 *     e1 = b - a;  e2 = c - a;
 *     mx = e1y * e2z - e1z * e2y;  my = e1z * e2x - e1x * e2z;  mz = e1x * e2y - e1y * e2x;      (the order of estd_mesh_face_area)
 *     p = a - centre;  delta = (mx * px + my * py) + mz * pz;
 *     the twelve terms  mx mx, mx my, mx mz, my my, my mz, mz mz (A),  delta mx, delta my, delta mz (b),  mx, my, mz (n).
 *   This weights a face's plane by its squared area: no square root and no division per face.  A face with two corners in the cluster
 *   has two records there and counts twice.  A record outside [0, 3 F) or of an invalid face is skipped: never an address.
 *   The order of the sum.  With the segment's records numbered i = 0, 1, ... in ascending r, chain l (l = 0..7) starts from 0.0 and
 *   adds the terms of records l, l + 8, l + 16, ... in that order; then per accumulator  x_l += x_(l xor 4),  x_l += x_(l xor 2),
 *   x_l += x_(l xor 1), i.e. ((c0 + c4) + (c2 + c6)) + ((c1 + c5) + (c3 + c7)).
 *   After the sum:
 *     t = (Axx + Ayy) + Azz;  lam = t * reg;  gbar_i = (double)mean[k][i] - centre_i;
 *     M = A + lam I (lam added to the three diagonal entries);  rhs_i = b_i + lam * gbar_i;
 *     d0 = M00;  l10 = M10 / d0;  l20 = M20 / d0;  d1 = M11 - l10 * M10;  u21 = M21 - l20 * M10;  l21 = u21 / d1;
 *     d2 = (M22 - l20 * M20) - l21 * u21;
 *     y0 = rhs0;  y1 = rhs1 - l10 * y0;  y2 = (rhs2 - l20 * y0) - l21 * y1;   z_i = y_i / d_i;
 *     s2 = z2;  s1 = z1 - l21 * s2;  s0 = (z0 - l10 * s1) - l20 * s2.
 *   The vertex is PLACED when t > 0, d0 > 0, d1 > 0, d2 > 0 and fabs(s_i) <= 0.5 * (double)cell for i = 0, 1, 2 (a NaN fails every
 *   test): out_xyz[k][i] = (float)(centre_i + s_i).  Otherwise out_xyz[k] = the bits of mean[k], unchanged.
 *     len = sqrt((nx * nx + ny * ny) + nz * nz);  out_normal[k] = ((float)(nx / len), (float)(ny / len), (float)(nz / len)), or 0 0 0 when
 *     len == 0: the area-weighted normal of the cluster's faces.  placed [K] bytes: 1 placed, 0 not.
 *   A cluster without records (a vertex no face uses) is not placed and has a zero normal.  out_xyz [K][3], out_normal [K][3] and
 *   placed [K] are written with plain vector stores, every element by every call that launches; no float atomics; the result is
 *   bit-identical across calls, bindings and launch shapes.
 *
 * Both: F == 0 or K == 0 returns ESTD_OK and launches no kernel (estd_mesh_cluster_faces still zeroes counts); the host layers fill in
 *   what the definition gives then -- without faces the means, zero normals and nothing placed; without vertices every face invalid.
 * ESTD_ERR_ARG, before any launch and with no device needed: a negative size, K > V, a null counts, a null pointer with work to do
 *   (faces / corner / triple / order with F > 0, cluster / xyz with V > 0, the per-cluster arrays with K > 0), a grid
 *   estd_cloud_cell_keys would refuse, reg negative or not finite.  ESTD_ERR_UNSUPPORTED: V or 3 F beyond 2^31 - 1. */
int estd_mesh_cluster_faces(const int* faces, long long n_faces, long long n_vertices, const int* cluster, long long n_clusters, int* corner,
                            int* triple, long long* counts, estd_stream_t stream);
int estd_mesh_cluster_quadrics(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const long long* order,
                               const long long* segments, const long long* cell_key, long long n_clusters, const float* mean,
                               const float* lo3, float cell, const int* dims3, double reg, float* out_xyz, float* out_normal,
                               unsigned char* placed, estd_stream_t stream);

/* The distance from a point to a triangle mesh (csrc/mesh/mesh_distance.hip; numpy form: tests/mesh_distance_ref.py): per query the
 * nearest point of the nearest triangle.  What compare_meshes(exact=True) of estdepth_amd/cloud_metrics.py scores with: the distance
 * to a surface, not to its nearest sample.
 *
 * Inputs.  q [M][3] float32, every coordinate finite (the host layers refuse others); the mesh xyz [V][3] float32, faces [F][3] int32,
 *   contiguous; max_dist, positive and finite with r2 = max_dist * max_dist (one fp32 product, formed once by the entry point) finite.
 *
 * Invalid faces.  Face f = (i0, i1, i2) with a = xyz[i0], b = xyz[i1], c = xyz[i2] is INVALID when an index is outside [0, V), when one
 *   of the nine coordinates is not finite, or when the fp32 normal is zero: with ab = b - a, ac = c - a (componentwise),
 *     nx = ab.y * ac.z - ab.z * ac.y;  ny = ab.z * ac.x - ab.x * ac.z;  nz = ab.x * ac.y - ab.y * ac.x;
 *     degenerate iff fmaf(nx, nx, fmaf(ny, ny, nz * nz)) == 0
 *   -- each component two ROUNDED products and their difference, not contracted: a face that names a vertex twice has ab == ac or a
 *   zero edge and gives exactly 0, which an fma (one product unrounded) would not.
 *   An invalid face is ignored, counted in `invalid`, and its indices are never used as an address (estd_mesh_components' rule; the
 *   coordinates are read only after the three indices were found in range).
 *
 * The pair.  tri_closest(q, a, b, c), every operation ONE fp32 operation as written, nothing contracted, dot(x, y) =
 *   fmaf(x0, y0, fmaf(x1, y1, x2 * y2)); the region tests of Ericson, Real-Time Collision Detection, 5.1.5, taken in this order:
 *     ab = b - a;  ac = c - a;  ap = q - a;  bp = q - b;  cp = q - c;
 *     d1 = dot(ab, ap);  d2 = dot(ac, ap);  d3 = dot(ab, bp);  d4 = dot(ac, bp);  d5 = dot(ab, cp);  d6 = dot(ac, cp);
 *     vc = fmaf(d1, d4, -(d3 * d2));  vb = fmaf(d5, d2, -(d1 * d6));  va = fmaf(d3, d6, -(d5 * d4));  e43 = d4 - d3;  e56 = d5 - d6;
 *     vertex A    if d1 <= 0 and d2 <= 0:                     v = 0, w = 0
 *     vertex B    else if d3 >= 0 and d4 <= d3:               v = 1, w = 0
 *     edge AB     else if vc <= 0 and d1 >= 0 and d3 <= 0:    v = d1 / (d1 - d3), w = 0
 *     vertex C    else if d6 >= 0 and d5 <= d6:               v = 0, w = 1
 *     edge AC     else if vb <= 0 and d2 >= 0 and d6 <= 0:    v = 0, w = d2 / (d2 - d6)
 *     edge BC     else if va <= 0 and e43 >= 0 and e56 >= 0:  w = e43 / (e43 + e56), v = 1 - w
 *     interior    else:                                       denom = 1 / ((va + vb) + vc);  v = vb * denom;  w = vc * denom
 *     p = fmaf(w, ac, fmaf(v, ab, a)) per component;   d = q - p;   d2(q, f) = fmaf(d.x, d.x, fmaf(d.y, d.y, d.z * d.z)).
 *   Divisions are IEEE correctly rounded.  A comparison with a NaN is false: a pair whose d2 is a NaN (coordinates whose products
 *   leave fp32) never wins.
 *
 * The result of a query, defined to the bit and independent of the grid, the cell edge, the launch shape and the binding:
 *     d2min = the smallest d2(q, f) over ALL valid faces f;   face = the SMALLEST f attaining it;   found iff d2min <= r2;
 *     dist[q] = the IEEE correctly rounded square root of d2min, or max_dist when not found;   face[q] = face, or -1;
 *     bary[q] = (v, w) and closest[q] = p of tri_closest(q, face) (optional outputs), zeros when not found.
 *   Every element of every output is written by every call with plain vector stores: two calls give the same bits.
 *
 * The structure (tuning only).  A grid as estd_cloud_cell_keys defines it (lo3, cell, dims3: host pointers / values, dims_j <=
 *   ESTD_CLOUD_MAX_DIM, at most ESTD_CLOUD_MAX_CELLS cells).  A valid face covers the cells c0_j .. c1_j per axis, c0 / c1 the cell
 *   coordinates of the componentwise minimum / maximum of its three vertices, n = the product of (c1_j - c0_j + 1) cells.  With
 *   n <= big_cells it is a GRID face and owns n (key, face) pairs, key = (z dims[1] + y) dims[0] + x, in ascending z, then y, then x;
 *   with n > big_cells it is a BIG face and owns none: every query tests it.  big_cells = 0 puts every valid face on the big list,
 *   big_cells >= the number of cells none.
 * estd_mesh_tri_bins (mesh_tri_bins_kernel, one lane per face): count [F] int32 = the pairs face f owns (0 for invalid and big
 *   faces), flag [F] int32 = 0 invalid, 1 grid, 2 big; invalid [1] int64 = the number of invalid faces, zeroed by the call (a memset
 *   on `stream`) and raised with ONE integer atomic add per wave.  F == 0: the memset alone.
 * estd_mesh_tri_fill (mesh_tri_fill_kernel, one lane per face): offset [F] int64 is the exclusive prefix sum of count (the host
 *   forms it); grid face f writes its pairs to keys [n_pairs] int64 / pair_face [n_pairs] int32 at offset[f] .. offset[f] + n - 1
 *   with plain stores, no atomics: the same bits for every launch.  A position outside [0, n_pairs) is dropped, never written.
 *   n_pairs == 0 or F == 0 launches nothing.
 * The host sorts the pairs by key (stable), forms cell_start [cells + 1] int32 (cell_start[k] = the pairs with a key < k) and
 *   gathers one 48-byte RECORD per pair in that order: twelve 32-bit words a.x a.y a.z b.x b.y b.z c.x c.y c.z, the bits of f, 0, 0;
 *   the big faces give records of the same form, in any order.  Both arrays are 16-byte aligned.
 * estd_mesh_nearest (mesh_nearest_kernel, one lane per query): tests every one of the B big records (the record's address is the
 *   same in every lane: scalar loads), then walks the cell table in rings around the query's (clamped) cell as estd_cloud_nearest
 *   does and stops in front of ring r >= 2 once (1 - 2^-5) ((r - 1) cell)^2 exceeds the smallest d2 so far (at most r2).  Every point
 *   of a triangle lies in the box of its vertices, hence in a cell the triangle is registered in, and cell coordinates are off by less
 *   than 2^-12 cells, so a triangle not met in rings 0 .. r - 1 is further than that bound: no face that could win or tie is skipped
 *   PROVIDED the vertices of all grid faces lie inside the grid's box [lo, lo + dims * cell) -- the caller's duty; the host layers
 *   take the box from the valid faces.  A face met in several cells is tested again; the minimum does not notice.  `order` as in
 *   estd_cloud_nearest.  Records are only read as coordinates and as the face index to report: nothing in them becomes an address.
 *   M == 0 launches nothing.  B == 0 and P == 0: nothing is found.
 * ESTD_ERR_ARG (before any launch, no device needed): a negative size or big_cells, a null `invalid`, a null pointer that the sizes
 *   make necessary (xyz with V > 0; faces, count, flag with F > 0; everything of estd_mesh_tri_fill with n_pairs > 0 and F > 0; query,
 *   dist, face with M > 0; big_records with B > 0; records and cell_start with P > 0), a misaligned record array, a grid
 *   estd_cloud_nearest would refuse (estd_mesh_nearest: only with P > 0), max_dist not finite or <= 0 or with a square that leaves
 *   fp32.  ESTD_ERR_UNSUPPORTED: V, 3 F or M beyond 2^31 - 1, n_pairs, B or P beyond ESTD_MESH_DISTANCE_MAX_PAIRS. */
#define ESTD_MESH_DISTANCE_MAX_PAIRS (1 << 23)
#define ESTD_MESH_DISTANCE_BIG_CELLS 64       /* the host layers' default for big_cells */
int estd_mesh_tri_bins(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const float* lo3, float cell,
                       const int* dims3, int big_cells, int* count, int* flag, long long* invalid, estd_stream_t stream);
int estd_mesh_tri_fill(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const float* lo3, float cell,
                       const int* dims3, int big_cells, const long long* offset, long long n_pairs, long long* keys, int* pair_face,
                       estd_stream_t stream);
typedef struct estd_mesh_nearest_desc {
    long long M, B, P;                            /* queries, big records, grid records */
    const float* query;                           /* [M][3] */
    const long long* order;                       /* [M] or NULL */
    const float* big_records;                     /* [B][12] */
    const float* records;                         /* [P][12], in cell order */
    const int* cell_start;                        /* [dims[0] dims[1] dims[2] + 1] */
    float* dist;                                  /* [M] */
    int* face;                                    /* [M] */
    float* bary;                                  /* NULL, or [M][2] */
    float* closest;                               /* NULL, or [M][3] */
    float lo[3];                                  /* host values, copied into the launch arguments */
    float cell;
    float max_dist;
    int dims[3];
} estd_mesh_nearest_desc;
int estd_mesh_nearest(const estd_mesh_nearest_desc* desc, estd_stream_t stream);

/* ---- rigid registration of a point cloud to a cloud or a mesh (csrc/track/rigid_align.hip; float64 form: tests/rigid_align_ref.py) ----
 * One iteration of ICP is: move the cloud, find a partner for every moved point (estd_cloud_nearest: the nearest target point;
 * estd_mesh_nearest with `closest`: the closest surface point and its face), form the 6 x 6 Gauss-Newton system.  The two entry points
 * below are the first and the last step; estdepth_amd/registration.py strings them together.
 *
 * estd_rigid_apply (rigid_apply_kernel, one lane per point).  src [n][3] float32, T12: 12 floats ON THE HOST, 3 x 4 row-major, copied
 *   into the launch arguments.  Per point p = (x, y, z) and row j:
 *     moved[i][j] = fma(T_j0, x, fma(T_j1, y, fma(T_j2, z, T_j3)));
 *   with src_normal [n][3] (both normal pointers or neither), for its rows (a, b, c):
 *     moved_normal[i][j] = fma(T_j0, a, fma(T_j1, b, T_j2 c)).
 *   Plain vector stores; every element is written by every call.  n == 0 launches nothing.
 *   ESTD_ERR_ARG (before any launch, no device needed): n < 0, a null T12 or an element of it that is not finite, with n > 0 a null src
 *   or moved or only one of the two normal pointers.  ESTD_ERR_UNSUPPORTED: n >= 2^31.
 *
 * estd_rigid_system (rigid_system_kernel, one lane per point, 256 points per workgroup; then rigid_reduce_kernel).  Inputs, all on the
 *   device: moved [N][3]; moved_normal [N][3] or NULL; index [N] int64; target [Nt][3], read at index[i] when by_index is set and at i
 *   otherwise (then Nt >= N: the `closest` array of estd_mesh_nearest as it is); normal [Nn][3], read at index[i] (target normals, or
 *   face normals).  Per point i, with k = index[i], m = moved[i]:
 *   1. SKIPPED unless 0 <= k < Nn, and k < Nt when by_index is set: an index outside is never turned into an address;
 *   2. q = target[by_index ? k : i];  e = q - m (per component);  e2 = fma(e_x, e_x, fma(e_y, e_y, e_z e_z));  skipped unless
 *      e2 <= dist_max^2 (dist_max * dist_max, formed once on the host in fp32; false for a NaN);
 *   3. with moved_normal and a cos_min that is finite (pass -infinity for no test): n = normal[k], s = moved_normal[i],
 *      c = fma(n_x, s_x, fma(n_y, s_y, n_z s_z));  skipped unless c >= cos_min, with two_sided unless fabsf(c) >= cos_min (a ground
 *      truth of either winding; false for a NaN).
 *   metric == ESTD_RIGID_PLANE (n = normal[k]):
 *      r = fma(n_x, e_x, fma(n_y, e_y, n_z e_z));  J = (n_x, n_y, n_z, w_x, w_y, w_z) with w = q x n:
 *        w_x = fma(q_y, n_z, -(q_z n_y)),  w_y = fma(q_z, n_x, -(q_x n_z)),  w_z = fma(q_x, n_y, -(q_y n_x));
 *      the 29 per-point terms are frame_align's: J_i J_j for the upper triangle row by row, J_i r, r r, 1.   residual[i] = r.
 *   metric == ESTD_RIGID_POINT: the residual is the vector e, linearised as e - (t + omega x q) = e - J xi with J = [I | -[q]x] (3 x 6).
 *      The 29 slots hold J^T J, J^T e, |e|^2 and 1, each entry ONE fp32 expression; upper triangle row by row:
 *        [0] 1   [1] 0   [2] 0   [3] 0      [4] q_z    [5] -q_y
 *                [6] 1   [7] 0   [8] -q_z   [9] 0      [10] q_x
 *                        [11] 1  [12] q_y   [13] -q_x  [14] 0
 *                                [15] fma(q_y, q_y, q_z q_z)   [16] -(q_x q_y)   [17] -(q_x q_z)
 *                                                   [18] fma(q_x, q_x, q_z q_z)   [19] -(q_y q_z)
 *                                                                      [20] fma(q_x, q_x, q_y q_y)
 *        [21..23] e_x, e_y, e_z;   [24] fma(q_y, e_z, -(q_z e_y))   [25] fma(q_z, e_x, -(q_x e_z))   [26] fma(q_x, e_y, -(q_y e_x));
 *        [27] e2 (the gated value);   [28] 1.                          residual[i] = the correctly rounded square root of e2.
 *   A skipped point contributes zeros to all 29 sums.  In both metrics r (e) ~ the partner minus the moved point, so the system belongs to
 *   the LEFT update T <- Exp(xi) T with xi = (t, omega) in the target's axes and the Gauss-Newton step solves (sum J^T J) xi = sum J^T r:
 *   sums[0..20] is the upper triangle of the matrix, sums[21..26] the right-hand side, sums[27] the sum of squares, sums[28] the count.
 * Per-point outputs, every element written by every call with plain vector stores:
 *   residual [N] float32 (0 where the point was skipped);   match [N] int64 = k, or -1 where it was skipped.
 * sums [ESTD_RIGID_SYSTEM_SUMS = 29] float64 on the device.  Each per-point term is widened and added in float64, no atomics, in
 *   frame_align's fixed order: the 64 lanes of a wave by an exclusive-or butterfly (lane distances 32 .. 1), the four waves of a
 *   workgroup in wave order through LDS, one partial per workgroup and term; in the reduce kernel lane l adds the partials of workgroups
 *   l, l + 64, ... in ascending order and the same butterfly joins the lanes.  Bit-identical across calls and bindings.
 * partials: device scratch of estd_rigid_system_partials(N) BYTES (29 float64 per 256 points), owned by the caller; the function
 *   returns 0 for sizes the entry point refuses, and for N == 0.  N == 0 runs the reduce kernel alone: the sums are +0.
 * ESTD_ERR_ARG (before any launch, no device needed): a null descriptor, a negative size, an unknown metric, dist_max or its square not
 *   a positive finite fp32, cos_min NaN with moved_normal, a null sums, with N > 0 a null moved / index / residual / match / partials,
 *   a null target with Nt > 0, a null normal with Nn > 0 where step 3 or the plane metric reads it, Nt < N without by_index.
 * ESTD_ERR_UNSUPPORTED: N, Nt or Nn >= 2^31. */
#define ESTD_RIGID_SYSTEM_SUMS 29
#define ESTD_RIGID_PLANE 0
#define ESTD_RIGID_POINT 1
typedef struct estd_rigid_system_desc {
    long long N, Nt, Nn;                          /* moved points, target rows, normal rows */
    int metric;                                   /* ESTD_RIGID_PLANE / ESTD_RIGID_POINT */
    int by_index;                                 /* target is read at index[i] (else at i) */
    int two_sided;
    float dist_max, cos_min;
    const float* moved;                           /* [N][3] */
    const float* moved_normal;                    /* [N][3] or NULL */
    const long long* index;                       /* [N] */
    const float* target;                          /* [Nt][3] */
    const float* normal;                          /* [Nn][3] */
    float* residual;                              /* [N] */
    long long* match;                             /* [N] */
    double* sums;                                 /* [ESTD_RIGID_SYSTEM_SUMS] */
    double* partials;                             /* estd_rigid_system_partials(N) bytes */
} estd_rigid_system_desc;
int estd_rigid_apply(const float* src, const float* src_normal, long long n, const float* T12, float* moved, float* moved_normal,
                     estd_stream_t stream);
long long estd_rigid_system_partials(long long N);
int estd_rigid_system(const estd_rigid_system_desc* desc, estd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ESTD_HIP_H */
