// est_fusion.hip -- epipolar spatio-temporal fusion: frustum-to-frustum volume warp + cross-view
// attention, GroupNorm(1 group) plumbing, ConvGRU elementwise stages, soft-argmin and the layout
// converters at the API edge.
//
// Reference semantics restated (file:line into the reference repo):
//   utils/homo_utils.py:240-279 warp_volume (+ :26-62, :107-134, :170-205)      trilinear, zeros,
//       align_corners=False, |norm|>1 -> 2, eps 1e-10
//   transformer/epipolar_transformer.py:56-83 EpipolarTransformer.forward       softmax over views,
//       MEAN of weighted values (Q10), GRU gates with GroupNorm(1,16)
//   hybrid_models/hybrid_depth_decoder.py:33-38 depthlayer on x4 nearest-upsampled logits
// All of these are HBM / gather-latency bound; the fused warp+attention kernel never materialises
// the 2N warped volumes the reference writes and re-reads.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "estd_hip.h"
#include <cstdlib>

#include "estd_common.h"
#include "estd_device.h"

namespace {

struct Tri {
    int off[8];         // voxel offsets ((z*H+y)*W+x), 0 when masked (volumes are < 2^31 voxels)
    float w[8];         // trilinear weights, 0 when the corner is out of bounds
};

// base corner (floor of the un-normalised sample position; -2 when the position is NaN) and the trilinear fractions
struct TriBase {
    int x0, y0, z0;
    float tx, ty, tz;
};

// homo_utils.py:51-54 (pixel2cam), :33-36 (cam2cam), :115-121 (cam2pixel_depth), :183-198 (normalise+mask),
// then ATen grid_sampler_3d un-normalisation for align_corners=False.  M = [kinv(9) | m(12) | k(9)].
__device__ __forceinline__ TriBase volume_coords_base(const float* __restrict__ M, float dep, int x, int y,
                                                      float depth_min, float depth_interval, int D, int H, int W)
{
    // Rounding sequence of the reference's torch-CPU composition, op for op, so that the |norm| > 1 masks (discontinuous!)
    // see bit-identical coordinates: the three matrix products are bmm/matmul calls (homo_utils.py:52-54, :35, :116) whose
    // GEMM kernels accumulate k = 0,1,2(,3) in order with fused multiply-adds -- acc = a0*b0; acc = fma(a1,b1,acc); ... (checked
    // against torch.matmul/bmm bit for bit, tests/test_oracle_ops_golden.py) -- everything else is an elementwise ATen op with
    // its own rounding.  Hence explicit fmaf() for the products and NO contraction anywhere else.
#pragma clang fp contract(off)
    const float fx = (float)x, fy = (float)y;
    const float c0 = (fmaf(M[1], fy, M[0] * fx) + M[2]) * dep;          // (K^-1 @ [x, y, 1]) * depth
    const float c1 = (fmaf(M[4], fy, M[3] * fx) + M[5]) * dep;
    const float c2 = (fmaf(M[7], fy, M[6] * fx) + M[8]) * dep;
    const float s0 = fmaf(M[11], c2, fmaf(M[10], c1, M[9] * c0)) + M[12];    // extrinsic @ [c, 1]
    const float s1 = fmaf(M[15], c2, fmaf(M[14], c1, M[13] * c0)) + M[16];
    const float s2 = fmaf(M[19], c2, fmaf(M[18], c1, M[17] * c0)) + M[20];
    const float q0 = fmaf(M[23], s2, fmaf(M[22], s1, M[21] * s0));           // K @ s
    const float q1 = fmaf(M[26], s2, fmaf(M[25], s1, M[24] * s0));
    const float q2 = fmaf(M[29], s2, fmaf(M[28], s1, M[27] * s0));
    const float den = q2 + 1e-10f;
    const float X = q0 / den, Y = q1 / den, Z = q2;
    float xn = 2.0f * X / (float)(W - 1) - 1.0f;
    float yn = 2.0f * Y / (float)(H - 1) - 1.0f;
    float zn = 2.0f * ((Z - depth_min) / depth_interval) / (float)(D - 1) - 1.0f;
    if (xn > 1.0f || xn < -1.0f) xn = 2.0f;
    if (yn > 1.0f || yn < -1.0f) yn = 2.0f;
    if (zn > 1.0f || zn < -1.0f) zn = 2.0f;
    const float ix = ((xn + 1.0f) * (float)W - 1.0f) * 0.5f;
    const float iy = ((yn + 1.0f) * (float)H - 1.0f) * 0.5f;
    const float iz = ((zn + 1.0f) * (float)D - 1.0f) * 0.5f;
    const float fx0 = floorf(ix), fy0 = floorf(iy), fz0 = floorf(iz);
    const bool finite = (ix == ix) && (iy == iy) && (iz == iz);
    TriBase b;
    b.tx = ix - fx0; b.ty = iy - fy0; b.tz = iz - fz0;
    b.x0 = finite ? (int)fx0 : -2; b.y0 = finite ? (int)fy0 : -2; b.z0 = finite ? (int)fz0 : -2;
    return b;
}

__device__ __forceinline__ Tri volume_coords(const float* __restrict__ M, float dep, int x, int y,
                                             float depth_min, float depth_interval, int D, int H, int W)
{
#pragma clang fp contract(off)
    const TriBase b = volume_coords_base(M, dep, x, y, depth_min, depth_interval, D, H, W);
    Tri t;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = (k >> 2) & 1;
        const int xx = b.x0 + dx, yy = b.y0 + dy, zz = b.z0 + dz;
        const bool ok = xx >= 0 && xx < W && yy >= 0 && yy < H && zz >= 0 && zz < D;
        const float wgt = (dx ? b.tx : 1.0f - b.tx) * (dy ? b.ty : 1.0f - b.ty) * (dz ? b.tz : 1.0f - b.tz);
        t.w[k] = ok ? wgt : 0.0f;
        t.off[k] = ok ? (zz * H + yy) * W + xx : 0;
    }
    return t;
}

// Level-1 operator (NCDHW in/out): one thread per target voxel, loop over channels.
__global__ __launch_bounds__(256) void warp_volume_kernel(const float* __restrict__ vol, const float* __restrict__ M,
                                                          const float* __restrict__ dvals, float depth_min, float depth_interval,
                                                          float* __restrict__ out, int C, int D, int H, int W)
{
    const long long HW = (long long)H * W, S = (long long)D * HW;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < S; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const int d = (int)(idx / HW);
        const Tri t = volume_coords(M, dvals[d], x, y, depth_min, depth_interval, D, H, W);
        for (int c = 0; c < C; ++c) {
            const float* s = vol + (long long)c * S;
            float v = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) v += s[(long long)t.off[k]] * t.w[k];
            out[(long long)c * S + idx] = v;
        }
    }
}

// Level-1 operator, every branch of the reference's signature (homo_utils.py:240-279): per-VOXEL depth (:246,:253), disparity
// planes (:187-190), padding_mode='border' on the volume whose outermost voxel layer holds padding_value (:271-274,:305-319).
// Same rounding sequence as volume_coords_base; the masks stay on in border mode (normalize_pixel_coords_volume is called with
// its own default padding_mode, :262-269).  Off the hot path: one thread per target voxel, loop over channels.
__global__ __launch_bounds__(256) void warp_volume_ex_kernel(const float* __restrict__ vol, const float* __restrict__ M,
                                                             const float* __restrict__ depth, estd_warp_volume_opts o,
                                                             float* __restrict__ out, int C, int D, int H, int W)
{
#pragma clang fp contract(off)
    const long long HW = (long long)H * W, S = (long long)D * HW;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < S; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const int d = (int)(idx / HW);
        const float dep = o.depth_per_voxel ? depth[idx] : depth[d];
        const float fx = (float)x, fy = (float)y;
        const float c0 = (fmaf(M[1], fy, M[0] * fx) + M[2]) * dep;
        const float c1 = (fmaf(M[4], fy, M[3] * fx) + M[5]) * dep;
        const float c2 = (fmaf(M[7], fy, M[6] * fx) + M[8]) * dep;
        const float s0 = fmaf(M[11], c2, fmaf(M[10], c1, M[9] * c0)) + M[12];
        const float s1 = fmaf(M[15], c2, fmaf(M[14], c1, M[13] * c0)) + M[16];
        const float s2 = fmaf(M[19], c2, fmaf(M[18], c1, M[17] * c0)) + M[20];
        const float q0 = fmaf(M[23], s2, fmaf(M[22], s1, M[21] * s0));
        const float q1 = fmaf(M[26], s2, fmaf(M[25], s1, M[24] * s0));
        const float q2 = fmaf(M[29], s2, fmaf(M[28], s1, M[27] * s0));
        const float den = q2 + 1e-10f;
        const float X = q0 / den, Y = q1 / den, Z = q2;
        float xn = 2.0f * X / (float)(W - 1) - 1.0f;
        float yn = 2.0f * Y / (float)(H - 1) - 1.0f;
        float zn = o.use_disp ? 2.0f * ((1.0f / (Z + 1e-10f) - o.disp_min) / o.disp_interval) / (float)(D - 1) - 1.0f
                              : 2.0f * ((Z - o.depth_min) / o.depth_interval) / (float)(D - 1) - 1.0f;
        if (xn > 1.0f || xn < -1.0f) xn = 2.0f;
        if (yn > 1.0f || yn < -1.0f) yn = 2.0f;
        if (zn > 1.0f || zn < -1.0f) zn = 2.0f;
        float ix = ((xn + 1.0f) * (float)W - 1.0f) * 0.5f;
        float iy = ((yn + 1.0f) * (float)H - 1.0f) * 0.5f;
        float iz = ((zn + 1.0f) * (float)D - 1.0f) * 0.5f;
        if (o.border) {                                     // ATen clip_coordinates: min(size - 1, max(i, 0))
            ix = fminf((float)(W - 1), fmaxf(ix, 0.0f));
            iy = fminf((float)(H - 1), fmaxf(iy, 0.0f));
            iz = fminf((float)(D - 1), fmaxf(iz, 0.0f));
        }
        const float fx0 = floorf(ix), fy0 = floorf(iy), fz0 = floorf(iz);
        const bool finite = (ix == ix) && (iy == iy) && (iz == iz);
        const float tx = ix - fx0, ty = iy - fy0, tz = iz - fz0;
        const int x0 = finite ? (int)fx0 : -2, y0 = finite ? (int)fy0 : -2, z0 = finite ? (int)fz0 : -2;
        float wgt[8];
        long long off[8];
        bool edge[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int dx = k & 1, dy = (k >> 1) & 1, dz = (k >> 2) & 1;
            const int xx = x0 + dx, yy = y0 + dy, zz = z0 + dz;
            const bool ok = xx >= 0 && xx < W && yy >= 0 && yy < H && zz >= 0 && zz < D;
            const float w = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty) * (dz ? tz : 1.0f - tz);
            wgt[k] = ok ? w : 0.0f;
            off[k] = ok ? ((long long)zz * H + yy) * W + xx : 0;
            edge[k] = o.border && (xx == 0 || xx == W - 1 || yy == 0 || yy == H - 1 || zz == 0 || zz == D - 1);
        }
        for (int c = 0; c < C; ++c) {
            const float* s = vol + (long long)c * S;
            float v = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) v += (edge[k] ? o.padding_value : s[off[k]]) * wgt[k];
            out[(long long)c * S + idx] = v;
        }
    }
}

// Fused warp(K_j), warp(V_j) + attention.  4 lanes per target voxel; lane c owns float4 chunk c of
// the 16 value channels and chunk c of the 16 key channels (kv record = [V(16) | K(16)] = 128 B).
#ifndef WA_SHARE
#define WA_SHARE 0   // 1: dx = 1 corner records from the x-neighbour's registers (DPP) instead of a second gather -- measured SLOWER (348 vs 255 us at N = 3, profiles/r3_warp_attention_share_pmc.csv): A/B switch only
#endif
#ifndef ESTD_WA_ABL
#define ESTD_WA_ABL 0   // timing ablations only (results are wrong for the consumers when != 0): what writing only h would buy (profiles/r6_warp_attention_honly.txt)
#endif
#ifndef WA_TD
#define WA_TD 2      // target brick of one 256-thread workgroup (64 voxels x 4 lanes): depth x rows x columns
#define WA_TY 4
#define WA_TX 8
#endif
static_assert(WA_TD * WA_TY * WA_TX == 64, "a workgroup owns 64 target voxels");

struct WarpAttnArgs {
    const float* kv_src[ESTD_MAX_ATTENTION_SOURCES];
};

// BUF: the corner records through buffer loads -- a source volume is one buffer descriptor (4 SGPRs) and a corner is ONE 32-bit byte offset for
// its value chunk and its key chunk (immediate +64) -- instead of two 64-bit flat addresses per corner: a third of the address arithmetic
// (PMC: 3 % fewer VALU instructions, CU-busy cycles -5.4 % at 3 sources; the texture-address unit's busy cycles do not move: -2 %).
// Volumes of 2 GiB and more take the pointer form.

template <int NS, bool BUF>
__global__ __launch_bounds__(256) void warp_attention_kernel(const float* __restrict__ kv_t, WarpAttnArgs srcs,
                                                             const float* __restrict__ mats, int n_src,
                                                             const float* __restrict__ dvals, float depth_min, float depth_interval,
                                                             float* __restrict__ xh, int D, int H, int W)
{
    // NS = compile-time source count (2..4), or 8 / 16 = generic loop bounded by n_src (1 and 5..8 / 9..16 sources): registers
    // follow the real count.  Measured alternatives that were SLOWER on MI355X (profiles/README.md, round 2): staging the
    // source box of a 2x8x16 brick in LDS (DMA or register-staged, 304-386 us vs 255 us at N = 3: the fill/blend phases
    // serialise and the larger bricks miss more in L2), sharing the sample positions inside the 4-lane group with DPP moves and
    // raising occupancy to 4-5 waves per SIMD (325 us: more bricks in flight than the 4 MB L2 of an XCD holds lines for).
    const long long HW = (long long)H * W;
    const int sub = threadIdx.x & 3;
    // A workgroup owns a compact 2 x 4 x 8 (d, y, x) brick of target voxels: the gathered source footprint of a brick is
    // ~135 records per source instead of ~260 for 64 voxels along x, and bricks are numbered x-fastest inside a contiguous
    // eighth of the volume per XCD, so neighbouring bricks (which gather the same source lines) share one private L2.
    // (rocprofv3 PMC, profiles/r2_hbm_kernels_pmc.csv: 1.24x the compulsory read bytes reach HBM; the linear mapping fetched 2.95x.)
    unsigned bid = blockIdx.x;
    if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
    const int tx_n = (W + WA_TX - 1) / WA_TX, ty_n = (H + WA_TY - 1) / WA_TY;
    const int bx = (int)(bid % tx_n), by = (int)((bid / tx_n) % ty_n), bd = (int)(bid / ((unsigned)tx_n * ty_n));
    const int v = threadIdx.x >> 2;                       // voxel inside the brick: x fastest
    const int x = bx * WA_TX + (v % WA_TX), y = by * WA_TY + ((v / WA_TX) % WA_TY), d = bd * WA_TD + v / (WA_TX * WA_TY);
    if (x >= W || y >= H || d >= D) return;               // whole 4-lane groups exit together
    const long long idx = (long long)d * HW + (long long)y * W + x;
    const float dep = dvals[d];

    const float4* t4 = reinterpret_cast<const float4*>(kv_t) + idx * 8;
#if ESTD_WA_ABL == 0
    const float4 vt = t4[sub];        // target value chunk
#endif
    const float4 kt = t4[4 + sub];    // target key chunk

    float corr[NS];
    float4 wv[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        corr[j] = -INFINITY;
        wv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (NS < 8 || j < n_src) {     // generic instances: slots past n_src keep corr = -inf (softmax weight 0)
            const Tri t = volume_coords(mats + j * 30, dep, x, y, depth_min, depth_interval, D, H, W);
            const float4* s4 = reinterpret_cast<const float4*>(srcs.kv_src[j]) + sub;
            float4 cv[8], ck[8];
            if (BUF) {
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(srcs.kv_src[j]), 0,
                                                                                    (int)((long long)D * HW * 128), 0x00020000);
#pragma unroll
                for (int k = 0; k < 8; ++k) {          // all 16 gathers of this source before any is used
                    const int vo = t.off[k] * 128 + sub * 16;
                    cv[k] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(rs, vo, 0, 0));
                    ck[k] = as_float4(__builtin_amdgcn_raw_buffer_load_b128(rs, vo + 64, 0, 0));
                }
            } else {
#if WA_SHARE
            // Corner sharing across x-neighbours: the texture-address path, not HBM, bounds this kernel (TA busy 90 % of the CU-busy
            // cycles, 31 TA cycles per 64-lane 16-byte gather, profiles/r2_warp_attention_ta_pmc.csv).  The voxel one step further
            // in x (the next 4-lane group of the wave) samples one record further in x for small relative motion: its dx = 0 corner
            // IS this voxel's dx = 1 corner.  Every group gathers its four dx = 0 corners; a dx = 1 corner is taken from the
            // neighbour's registers (ds_bpermute: the LDS crossbar, 4x the TA's bytes per clock) when the neighbour loaded that very
            // record, and gathered directly otherwise (row ends, large motion, volume border).  Same records, same arithmetic.
#pragma unroll
            for (int c = 0; c < 4; ++c) {          // the 8 gathers of the dx = 0 corners, issued before anything is used
                cv[2 * c] = s4[(long long)t.off[2 * c] * 8];
                ck[2 * c] = s4[(long long)t.off[2 * c] * 8 + 4];
            }
            // neighbour = the next 4-lane group of the same 16-lane DPP row (v_mov_b32_dpp row_shl:4: VALU, idle in this kernel; a
            // ds_bpermute through the LDS crossbar costs more than the gather it replaces: measured 362 vs 255 us)
            const bool has_nb = (v & 3) != 3 && x + 1 < W;
            auto shl4 = [](float f) {
                return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, f), 0x104, 0xf, 0xf, true));
            };
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int k0 = 2 * c, k1 = 2 * c + 1;
                const int nb_off = __builtin_amdgcn_update_dpp(-1, t.off[k0], 0x104, 0xf, 0xf, false);
                const bool need = t.w[k1] != 0.0f;                       // out-of-volume corners carry weight 0: their data is never used
                const bool share = has_nb && nb_off == t.off[k1];
                float4 nv, nk;
                nv.x = shl4(cv[k0].x); nv.y = shl4(cv[k0].y); nv.z = shl4(cv[k0].z); nv.w = shl4(cv[k0].w);
                nk.x = shl4(ck[k0].x); nk.y = shl4(ck[k0].y); nk.z = shl4(ck[k0].z); nk.w = shl4(ck[k0].w);
                cv[k1] = nv;
                ck[k1] = nk;
                if (need && !share) {
                    cv[k1] = s4[(long long)t.off[k1] * 8];
                    ck[k1] = s4[(long long)t.off[k1] * 8 + 4];
                }
            }
#else
#pragma unroll
            for (int k = 0; k < 8; ++k) {          // issue all 16 gathers of this source before using any
                cv[k] = s4[(long long)t.off[k] * 8];
                ck[k] = s4[(long long)t.off[k] * 8 + 4];
            }
#endif
            }
            float4 av = make_float4(0.f, 0.f, 0.f, 0.f), ak = av;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float w = t.w[k];
                av.x += cv[k].x * w; av.y += cv[k].y * w; av.z += cv[k].z * w; av.w += cv[k].w * w;
                ak.x += ck[k].x * w; ak.y += ck[k].y * w; ak.z += ck[k].z * w; ak.w += ck[k].w * w;
            }
            float c = kt.x * ak.x + kt.y * ak.y + kt.z * ak.z + kt.w * ak.w;   // epipolar_transformer.py:65
            c += __shfl_xor(c, 1);
            c += __shfl_xor(c, 2);
            corr[j] = c;
            wv[j] = av;
        }
    }
    // softmax over views (:69) and mean of the weighted values (:73); unused generic slots hold -inf -> weight 0
    float mx = corr[0];
#pragma unroll
    for (int j = 1; j < NS; ++j) mx = fmaxf(mx, corr[j]);
    float den = 0.0f;
#pragma unroll
    for (int j = 0; j < NS; ++j) { corr[j] = expf(corr[j] - mx); den += corr[j]; }
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const float a = corr[j] / den;
        h.x += wv[j].x * a; h.y += wv[j].y * a; h.z += wv[j].z * a; h.w += wv[j].w * a;
    }
    const float inv_n = 1.0f / (float)n_src;
    h.x *= inv_n; h.y *= inv_n; h.z *= inv_n; h.w *= inv_n;
#if ESTD_WA_ABL == 1        // timing ablation: only h, as a compact 16-channel volume (64 B per voxel, whole lines), no V_t load / copy
    reinterpret_cast<float4*>(xh)[idx * 4 + sub] = h;
#elif ESTD_WA_ABL == 2      // timing ablation: only h, into its half of the 32-channel record (64 of every 128 bytes), no V_t load / copy
    reinterpret_cast<float4*>(xh)[idx * 8 + 4 + sub] = h;
#else
    float4* o4 = reinterpret_cast<float4*>(xh) + idx * 8;
    o4[sub] = vt;
    o4[4 + sub] = h;
#endif
}

// Attention over ALREADY WARPED key/value volumes (the level-1 EpipolarTransformer.forward signature,
// transformer/epipolar_transformer.py:56-73).  Same lane mapping as the fused kernel, no gather.
__global__ __launch_bounds__(256) void attention_prewarped_kernel(const float* __restrict__ kv_t, WarpAttnArgs srcs, int n_src,
                                                                  float* __restrict__ xh, long long S)
{
    const int sub = threadIdx.x & 3;
    const long long idx = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);
    if (idx >= S) return;
    const float4* t4 = reinterpret_cast<const float4*>(kv_t) + idx * 8;
    const float4 vt = t4[sub];
    const float4 kt = t4[4 + sub];
    float corr[ESTD_MAX_ATTENTION_SOURCES];
    float4 wv[ESTD_MAX_ATTENTION_SOURCES];
#pragma unroll
    for (int j = 0; j < ESTD_MAX_ATTENTION_SOURCES; ++j) {
        if (j < n_src) {
            const float4* s4 = reinterpret_cast<const float4*>(srcs.kv_src[j]) + idx * 8;
            wv[j] = s4[sub];
            const float4 kk = s4[4 + sub];
            float c = kt.x * kk.x + kt.y * kk.y + kt.z * kk.z + kt.w * kk.w;
            c += __shfl_xor(c, 1);
            c += __shfl_xor(c, 2);
            corr[j] = c;
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < ESTD_MAX_ATTENTION_SOURCES; ++j) if (j < n_src) mx = fmaxf(mx, corr[j]);
    float den = 0.0f;
#pragma unroll
    for (int j = 0; j < ESTD_MAX_ATTENTION_SOURCES; ++j) if (j < n_src) { corr[j] = expf(corr[j] - mx); den += corr[j]; }
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < ESTD_MAX_ATTENTION_SOURCES; ++j) if (j < n_src) {
        const float a = corr[j] / den;
        h.x += wv[j].x * a; h.y += wv[j].y * a; h.z += wv[j].z * a; h.w += wv[j].w * a;
    }
    const float inv_n = 1.0f / (float)n_src;
    h.x *= inv_n; h.y *= inv_n; h.z *= inv_n; h.w *= inv_n;
    float4* o4 = reinterpret_cast<float4*>(xh) + idx * 8;
    o4[sub] = vt;
    o4[4 + sub] = h;
}

__global__ __launch_bounds__(1024) void groupnorm_finalize_kernel(const double* __restrict__ partials, int n_blocks, double count, float eps,
                                                                  float* __restrict__ out4)
{
    // ONE block of 1024 threads (it sits between two convolutions of the serial ConvGRU chain: its latency is what counts).  Thread t owns
    // the partials t, t + 1024, ...: the loads of a thread are independent (issued back to back, 32 bytes each), then a fixed-order tree
    // through LDS -> deterministic.  (256 threads with a dependent loop: 15 us; this: half.)
    __shared__ double red[1024 * 4];
    const double2* p2 = reinterpret_cast<const double2*>(partials);
    double a[4] = {0, 0, 0, 0};
    constexpr int U = 8;
    for (int b0 = threadIdx.x; b0 < n_blocks; b0 += 1024 * U) {
        double2 v0[U], v1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b = b0 + u * 1024;
            const bool ok = b < n_blocks;
            v0[u] = ok ? p2[(size_t)b * 2] : make_double2(0.0, 0.0);
            v1[u] = ok ? p2[(size_t)b * 2 + 1] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { a[0] += v0[u].x; a[1] += v0[u].y; a[2] += v1[u].x; a[3] += v1[u].y; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[threadIdx.x * 4 + k] = a[k];
    __syncthreads();
    for (int s = 512; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[threadIdx.x * 4 + k] += red[(threadIdx.x + s) * 4 + k];
        __syncthreads();
    }
    if (threadIdx.x < 2) {
        const int gidx = threadIdx.x;
        const double mean = red[gidx * 2] / count;
        double var = red[gidx * 2 + 1] / count - mean * mean;   // fp64 sums: cancellation-safe at these sizes
        if (var < 0.0) var = 0.0;
        out4[gidx * 2] = (float)mean;
        out4[gidx * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// A/B switch ESTD_GRU_FAST=1: sigmoid and tanh on the transcendental units (v_exp_f32 / v_rcp_f32, 1 ulp each; 4 and 5 instructions per value
// where expf + an IEEE division and the device library's tanhf take ~20 and ~30; absolute error <= 2e-7).  Measured NEUTRAL on MI355X
// (gru_blend 92.9 vs 94.8 us, gru_reset 79.0 vs 80.0 us stand-alone; Joint step 17.40-17.42 vs 17.40 ms, profiles/r4_graph_memory_ab.txt):
// both kernels are bound by their memory access pattern (64-byte halves of 128-byte records), not by the VALU -- so the default keeps
// the library functions the oracle uses.  sigmoid_fast and tanh_fast: csrc/estd_device.h.

// xrh = [x, sigmoid(GN(r_raw)) * h]; one lane per float4 of the 16-channel halves
template <bool FAST>
__global__ __launch_bounds__(256) void gru_reset_kernel(const float* __restrict__ xh, const float* __restrict__ ru,
                                                        const float* __restrict__ stats, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ xrh, long long n_vox)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one per (voxel, chunk of 4)
    if (t >= n_vox * 4) return;
    const long long vox = t >> 2;
    const int c = (int)(t & 3);
    const float mean = stats[0], rstd = stats[1];
    const float4 x = reinterpret_cast<const float4*>(xh)[vox * 8 + c];
    const float4 h = reinterpret_cast<const float4*>(xh)[vox * 8 + 4 + c];
    const float4 r = reinterpret_cast<const float4*>(ru)[vox * 8 + c];
    const float4 g = reinterpret_cast<const float4*>(gamma)[c];
    const float4 b = reinterpret_cast<const float4*>(beta)[c];
    float4 o;
    auto sg = [](float v) { return FAST ? sigmoid_fast(v) : sigmoidf_(v); };
    o.x = sg((r.x - mean) * rstd * g.x + b.x) * h.x;
    o.y = sg((r.y - mean) * rstd * g.y + b.y) * h.y;
    o.z = sg((r.z - mean) * rstd * g.z + b.z) * h.z;
    o.w = sg((r.w - mean) * rstd * g.w + b.w) * h.w;
    reinterpret_cast<float4*>(xrh)[vox * 8 + c] = x;
    reinterpret_cast<float4*>(xrh)[vox * 8 + 4 + c] = o;
}

// out = u * h + (1 - u) * tanh(GN(o)),  u = sigmoid(GN(u_raw))   (transformer/epipolar_transformer.py:47,:82-83)
template <bool FAST>
__global__ __launch_bounds__(256) void gru_blend_kernel(const float* __restrict__ xh, const float* __restrict__ ru,
                                                        const float* __restrict__ o_raw, const float* __restrict__ st_ru,
                                                        const float* __restrict__ st_o, const float* __restrict__ gamma_u,
                                                        const float* __restrict__ beta_u, const float* __restrict__ gamma_o,
                                                        const float* __restrict__ beta_o, float* __restrict__ out, int out_stride,
                                                        long long n_vox)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_vox * 4) return;
    const long long vox = t >> 2;
    const int c = (int)(t & 3);
    const float mu = st_ru[2], ru_ = st_ru[3];     // update gate = group 1 of the gate conv
    const float mo = st_o[0], ro = st_o[1];
    const float4 h = reinterpret_cast<const float4*>(xh)[vox * 8 + 4 + c];
    const float4 u = reinterpret_cast<const float4*>(ru)[vox * 8 + 4 + c];
    const float4 o = reinterpret_cast<const float4*>(o_raw)[vox * 4 + c];
    const float4 gu = reinterpret_cast<const float4*>(gamma_u)[c], bu = reinterpret_cast<const float4*>(beta_u)[c];
    const float4 go = reinterpret_cast<const float4*>(gamma_o)[c], bo = reinterpret_cast<const float4*>(beta_o)[c];
    auto one = [&](float hv, float uv, float ov, float guv, float buv, float gov, float bov) {
        const float ua = (uv - mu) * ru_ * guv + buv, oa = (ov - mo) * ro * gov + bov;
        const float uu = FAST ? sigmoid_fast(ua) : sigmoidf_(ua);
        const float yy = FAST ? tanh_fast(oa) : tanhf(oa);
        return uu * hv + (1.0f - uu) * yy;
    };
    float4 r;
    r.x = one(h.x, u.x, o.x, gu.x, bu.x, go.x, bo.x);
    r.y = one(h.y, u.y, o.y, gu.y, bu.y, go.y, bo.y);
    r.z = one(h.z, u.z, o.z, gu.z, bu.z, go.z, bo.z);
    r.w = one(h.w, u.w, o.w, gu.w, bu.w, go.w, bo.w);
    *reinterpret_cast<float4*>(out + vox * out_stride + c * 4) = r;
}

// soft-argmin at low resolution, replicated s x s (hybrid_depth_decoder.py:33-38 after F.interpolate(scale_factor=s)).
// A 256-thread workgroup owns 32 consecutive low-res pixels of one row; thread (px, g) reduces the depth planes
// d = g, g+8, g+16, ... of pixel px (every plane read is a coalesced 128-byte segment), the eight partial maxima / sums of
// a pixel meet in LDS, and the eight threads of a pixel then write its s x s replicas of (depth, max probability).
// (One thread per pixel looping over all D planes left 225 workgroups for a whole Joint step: pure latency.)
__global__ __launch_bounds__(256) void softargmin_up_kernel(const float* __restrict__ logits, const float* __restrict__ dvals,
                                                            float* __restrict__ depth, float* __restrict__ prob,
                                                            int N, int D, int H, int W, int s)
{
    __shared__ float red[3][8][32];
    const int px = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int wt = (W + 31) / 32;
    const int bw = blockIdx.x % wt, y = (blockIdx.x / wt) % H, n = blockIdx.x / (wt * H);
    const int x = bw * 32 + px;
    const bool ok = x < W;
    const long long HW = (long long)H * W;
    const float* l = logits + (long long)n * D * HW + (long long)y * W + (ok ? x : W - 1);
    float mx = -INFINITY;
    for (int d = g; d < D; d += 8) mx = fmaxf(mx, l[(long long)d * HW]);
    red[0][g][px] = mx;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) mx = fmaxf(mx, red[0][k][px]);
    float den = 0.0f, num = 0.0f;
    for (int d = g; d < D; d += 8) {
        const float e = expf(l[(long long)d * HW] - mx);      // second read of the same lines: L2 / L1 resident
        den += e;
        num += e * dvals[d];
    }
    red[1][g][px] = den;
    red[2][g][px] = num;
    __syncthreads();
    den = 0.0f; num = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) { den += red[1][k][px]; num += red[2][k][px]; }     // fixed order: deterministic
    if (!ok) return;
    const float dep = num / den;
    const float pm = 1.0f / den;        // max_d softmax = exp(0)/den
    const int Wo = W * s;
    const long long obase = (long long)n * HW * s * s + (long long)y * s * Wo + (long long)x * s;
    // s * 2 row segments (s rows of depth, s rows of prob) spread over the 8 threads of the pixel
    for (int q = g; q < 2 * s; q += 8) {
        const int r = q % s;
        float* dst = (q < s ? depth : prob) + obase + (long long)r * Wo;
        const float v = q < s ? dep : pm;
        if (s == 4) *reinterpret_cast<float4*>(dst) = make_float4(v, v, v, v);
        else for (int c = 0; c < s; ++c) dst[c] = v;
    }
}

// [C][S] planes <-> [S][stride] channels-last records, through an LDS tile so both sides coalesce
__global__ __launch_bounds__(256) void cdhw_to_vol_kernel(const float* __restrict__ src, float* __restrict__ dst, int C,
                                                          long long S, int dst_stride, int dst_off)
{
    __shared__ float tile[32][65];
    const long long s0 = (long long)blockIdx.x * 64;
    for (int e = threadIdx.x; e < C * 64; e += 256) {
        const int c = e / 64, k = e % 64;
        tile[c][k] = (s0 + k < S) ? src[(long long)c * S + s0 + k] : 0.0f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < C * 64; e += 256) {
        const int k = e / C, c = e % C;
        if (s0 + k < S) dst[(s0 + k) * dst_stride + dst_off + c] = tile[c][k];
    }
}

__global__ __launch_bounds__(256) void vol_to_cdhw_kernel(const float* __restrict__ src, float* __restrict__ dst, int C,
                                                          long long S, int src_stride, int src_off)
{
    __shared__ float tile[32][65];
    const long long s0 = (long long)blockIdx.x * 64;
    for (int e = threadIdx.x; e < C * 64; e += 256) {
        const int k = e / C, c = e % C;
        tile[c][k] = (s0 + k < S) ? src[(s0 + k) * src_stride + src_off + c] : 0.0f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < C * 64; e += 256) {
        const int c = e / 64, k = e % 64;
        if (s0 + k < S) dst[(long long)c * S + s0 + k] = tile[c][k];
    }
}

}  // namespace

extern "C" int estd_warp_volume(const float* vol, const float* mats30, const float* dvals, float depth_min,
                                float depth_interval, float* out, int C, int D, int H, int W, estd_stream_t s)
{
    if (!vol || !mats30 || !dvals || !out || C <= 0 || D <= 1 || H <= 1 || W <= 1) return ESTD_ERR_ARG;
    const long long S = (long long)D * H * W;
    const long long nb = (S + 255) / 256;
    hipLaunchKernelGGL(warp_volume_kernel, dim3((unsigned)(nb > 1048576 ? 1048576 : nb)), dim3(256), 0, estd_stream(s),
                       vol, mats30, dvals, depth_min, depth_interval, out, C, D, H, W);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_warp_volume_ex(const float* vol, const float* mats30, const float* depth, const estd_warp_volume_opts* opts,
                                   float* out, int C, int D, int H, int W, estd_stream_t s)
{
    if (!vol || !mats30 || !depth || !opts || !out || C <= 0 || D <= 1 || H <= 1 || W <= 1) return ESTD_ERR_ARG;
    if (opts->use_disp ? !(opts->disp_interval != 0.0f) : !(opts->depth_interval != 0.0f)) return ESTD_ERR_ARG;
    const long long S = (long long)D * H * W;
    const long long nb = (S + 255) / 256;
    hipLaunchKernelGGL(warp_volume_ex_kernel, dim3((unsigned)(nb > 1048576 ? 1048576 : nb)), dim3(256), 0, estd_stream(s),
                       vol, mats30, depth, *opts, out, C, D, H, W);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_warp_attention(const float* kv_target, const float* const* kv_src, const float* mats_dev,
                                   int n_src, const float* dvals, float depth_min, float depth_interval,
                                   float* xh_out, int D, int H, int W, estd_stream_t s)
{
    if (!kv_target || !kv_src || !mats_dev || !dvals || !xh_out) return ESTD_ERR_ARG;
    if (n_src < 1 || D <= 1 || H <= 1 || W <= 1) return ESTD_ERR_ARG;
    if (n_src > ESTD_MAX_ATTENTION_SOURCES) return ESTD_ERR_UNSUPPORTED;
    WarpAttnArgs a;
    for (int j = 0; j < n_src; ++j) if (!kv_src[j]) return ESTD_ERR_ARG;
    for (int j = 0; j < ESTD_MAX_ATTENTION_SOURCES; ++j) a.kv_src[j] = kv_src[j < n_src ? j : 0];
    const dim3 grid((unsigned)(((D + WA_TD - 1) / WA_TD) * ((H + WA_TY - 1) / WA_TY) * ((W + WA_TX - 1) / WA_TX)));   // one workgroup per brick
    // Buffer-load gathers (BUF) where they measured faster: 3 sources 236-243 -> 220-226 us (same 144 registers, same occupancy: the gain is the
    // address traffic); 2 sources are SLOWER with them (84 instead of 104 registers -> 6 waves per SIMD: 205 us; capped to the pointer form's 4
    // by an unused LDS allocation: 190 us; pointer form 182-187 us), 1 source equal, 4 sources need 224 instead of 184 registers (not measured).
    // ESTD_WA_BUF = 0 | 1 forces the form for every source count, ESTD_WA_OCC = n caps the resident workgroups per CU (sweep: profiles/r4_warp_attention_buf.txt).
    static const int buf_env = [] { const char* e = getenv("ESTD_WA_BUF"); return e ? atoi(e) : -1; }();             // A/B switches, read once
    static const int occ_env = [] { const char* e = getenv("ESTD_WA_OCC"); return e ? atoi(e) : 0; }();
    const bool buf = (buf_env >= 0 ? buf_env != 0 : n_src == 3) && (long long)D * H * W * 128 < 0x7fffffffLL;
    const int lds = occ_env > 0 ? ((160 * 1024 / occ_env) & ~255) : 0;
#define ESTD_WA_LAUNCH(NS)                                                                                                              \
    do {                                                                                                                                \
        if (buf) {                                                                                                                      \
            if (lds > 48 * 1024) estd_allow_dynamic_lds<warp_attention_kernel<NS, true>>(160 * 1024);                                   \
            hipLaunchKernelGGL((warp_attention_kernel<NS, true>), grid, dim3(256), lds, estd_stream(s), kv_target, a, mats_dev,         \
                               n_src, dvals, depth_min, depth_interval, xh_out, D, H, W);                                               \
        } else {                                                                                                                        \
            if (lds > 48 * 1024) estd_allow_dynamic_lds<warp_attention_kernel<NS, false>>(160 * 1024);                                  \
            hipLaunchKernelGGL((warp_attention_kernel<NS, false>), grid, dim3(256), lds, estd_stream(s), kv_target, a, mats_dev,        \
                               n_src, dvals, depth_min, depth_interval, xh_out, D, H, W);                                               \
        }                                                                                                                               \
    } while (0)
    switch (n_src) {
        case 2: ESTD_WA_LAUNCH(2); break;
        case 3: ESTD_WA_LAUNCH(3); break;
        case 4: ESTD_WA_LAUNCH(4); break;
        default:                              /* measured: for one source the generic body beats a 1-source specialisation */
            if (n_src <= 8) ESTD_WA_LAUNCH(8); else ESTD_WA_LAUNCH(16);
            break;
    }
#undef ESTD_WA_LAUNCH
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_attention_prewarped(const float* kv_target, const float* const* kv_src, int n_src,
                                        float* xh_out, int64_t n_vox, estd_stream_t s)
{
    if (!kv_target || !kv_src || !xh_out || n_src < 1 || n_vox <= 0) return ESTD_ERR_ARG;
    if (n_src > ESTD_MAX_ATTENTION_SOURCES) return ESTD_ERR_UNSUPPORTED;
    WarpAttnArgs a;
    for (int j = 0; j < n_src; ++j) if (!kv_src[j]) return ESTD_ERR_ARG;
    for (int j = 0; j < ESTD_MAX_ATTENTION_SOURCES; ++j) a.kv_src[j] = j < n_src ? kv_src[j] : kv_src[0];
    hipLaunchKernelGGL(attention_prewarped_kernel, dim3((unsigned)((n_vox + 63) / 64)), dim3(256), 0, estd_stream(s),
                       kv_target, a, n_src, xh_out, (long long)n_vox);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_groupnorm_finalize(const double* partials, int n_blocks, double count, float eps, float* out4,
                                       estd_stream_t s)
{
    if (!partials || !out4 || n_blocks <= 0 || count <= 0) return ESTD_ERR_ARG;
    hipLaunchKernelGGL(groupnorm_finalize_kernel, dim3(1), dim3(1024), 0, estd_stream(s), partials, n_blocks, count, eps, out4);
    return ESTD_LAUNCH_CHECK();
}

static bool gru_fast_math()       // A/B switch, read once (default off: measured neutral, see sigmoid_fast)
{
    static const bool fast = [] { const char* e = getenv("ESTD_GRU_FAST"); return e && atoi(e) == 1; }();
    return fast;
}

extern "C" int estd_gru_reset_apply(const float* xh, const float* ru, const float* stats4, const float* gamma_r,
                                    const float* beta_r, float* xrh, int64_t n_vox, estd_stream_t s)
{
    if (!xh || !ru || !stats4 || !gamma_r || !beta_r || !xrh || n_vox <= 0) return ESTD_ERR_ARG;
    const dim3 grid((unsigned)((n_vox * 4 + 255) / 256));
    if (gru_fast_math())
        hipLaunchKernelGGL(gru_reset_kernel<true>, grid, dim3(256), 0, estd_stream(s), xh, ru, stats4, gamma_r, beta_r, xrh, (long long)n_vox);
    else
        hipLaunchKernelGGL(gru_reset_kernel<false>, grid, dim3(256), 0, estd_stream(s), xh, ru, stats4, gamma_r, beta_r, xrh, (long long)n_vox);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_gru_blend(const float* xh, const float* ru, const float* o_raw, const float* stats_ru4,
                              const float* stats_o4, const float* gamma_u, const float* beta_u, const float* gamma_o,
                              const float* beta_o, float* out_value, int out_stride, int64_t n_vox, estd_stream_t s)
{
    if (!xh || !ru || !o_raw || !stats_ru4 || !stats_o4 || !gamma_u || !beta_u || !gamma_o || !beta_o || !out_value)
        return ESTD_ERR_ARG;
    if (n_vox <= 0 || out_stride < 16 || (out_stride & 3)) return ESTD_ERR_ARG;
    const dim3 grid((unsigned)((n_vox * 4 + 255) / 256));
    if (gru_fast_math())
        hipLaunchKernelGGL(gru_blend_kernel<true>, grid, dim3(256), 0, estd_stream(s), xh, ru, o_raw, stats_ru4, stats_o4, gamma_u, beta_u,
                           gamma_o, beta_o, out_value, out_stride, (long long)n_vox);
    else
        hipLaunchKernelGGL(gru_blend_kernel<false>, grid, dim3(256), 0, estd_stream(s), xh, ru, o_raw, stats_ru4, stats_o4, gamma_u, beta_u,
                           gamma_o, beta_o, out_value, out_stride, (long long)n_vox);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_softargmin_up(const float* logits, const float* dvals, float* depth, float* prob,
                                  int N, int D, int H, int W, int sc, estd_stream_t s)
{
    if (!logits || !dvals || !depth || !prob || N <= 0 || D <= 0 || H <= 0 || W <= 0 || sc <= 0) return ESTD_ERR_ARG;
    const long long blocks = (long long)N * H * ((W + 31) / 32);
    if (blocks > 0x7fffffffLL) return ESTD_ERR_ARG;
    hipLaunchKernelGGL(softargmin_up_kernel, dim3((unsigned)blocks), dim3(256), 0, estd_stream(s),
                       logits, dvals, depth, prob, N, D, H, W, sc);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_cdhw_to_vol(const float* src, float* dst, int C, int64_t S, int dst_stride, int dst_off, estd_stream_t s)
{
    if (!src || !dst || C <= 0 || C > 32 || S <= 0 || dst_stride < dst_off + C) return ESTD_ERR_ARG;
    hipLaunchKernelGGL(cdhw_to_vol_kernel, dim3((unsigned)((S + 63) / 64)), dim3(256), 0, estd_stream(s),
                       src, dst, C, (long long)S, dst_stride, dst_off);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_vol_to_cdhw(const float* src, float* dst, int C, int64_t S, int src_stride, int src_off, estd_stream_t s)
{
    if (!src || !dst || C <= 0 || C > 32 || S <= 0 || src_stride < src_off + C) return ESTD_ERR_ARG;
    hipLaunchKernelGGL(vol_to_cdhw_kernel, dim3((unsigned)((S + 63) / 64)), dim3(256), 0, estd_stream(s),
                       src, dst, C, (long long)S, src_stride, src_off);
    return ESTD_LAUNCH_CHECK();
}

__global__ void estd_mark_kernel(int id) { (void)id; }

extern "C" int estd_profile_mark(int id, estd_stream_t s)
{
    hipLaunchKernelGGL(estd_mark_kernel, dim3(1), dim3(1), 0, estd_stream(s), id);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_version(void) { return 100; }

namespace {
int clamp_reserved(int n) { n = n < 0 ? 0 : n > 128 ? 128 : n; return (n + 7) & ~7; }
std::atomic<int>& reserved_cus()
{
    static std::atomic<int> v{[] { const char* e = getenv("ESTD_RESERVED_CUS"); return clamp_reserved(e ? atoi(e) : 0); }()};
    return v;
}
}  // namespace
extern "C" int estd_set_reserved_cus(int n) { reserved_cus().store(clamp_reserved(n)); return reserved_cus().load(); }
extern "C" int estd_get_reserved_cus(void) { return reserved_cus().load(); }

extern "C" const char* estd_status_string(int st)
{
    switch (st) {
        case ESTD_OK: return "ok";
        case ESTD_ERR_ARG: return "invalid argument (null pointer, non-positive size or unsupported channel count)";
        case ESTD_ERR_LAUNCH: return "HIP kernel launch failed";
        case ESTD_ERR_UNSUPPORTED: return "unsupported configuration";
        default: return "unknown status";
    }
}

// ---------------------------------------------------------------------------------------------------------------
// fused BatchNorm2d(eval) (+ residual) (+ ReLU), NHWC, in place: one pass instead of BN -> add -> clamp
namespace {
__global__ __launch_bounds__(256) void bn_act_nhwc_kernel(float4* __restrict__ x, const float4* __restrict__ scale,
                                                          const float4* __restrict__ shift, const float4* __restrict__ residual,
                                                          int relu, long long n4, int c4)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += stride) {
        const int c = (int)(e % c4);
        float4 v = x[e];
        const float4 s = scale[c], t = shift[c];
        v.x = v.x * s.x + t.x; v.y = v.y * s.y + t.y; v.z = v.z * s.z + t.z; v.w = v.w * s.w + t.w;
        if (residual) { const float4 r = residual[e]; v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        x[e] = v;
    }
}
}  // namespace

extern "C" int estd_bn_act_nhwc(float* x, const float* scale, const float* shift, const float* residual, int relu,
                                int64_t n_pix, int C, estd_stream_t stream)
{
    if (!x || !scale || !shift || n_pix <= 0 || C <= 0 || (C & 3)) return ESTD_ERR_ARG;
    const long long n4 = (long long)n_pix * (C / 4);
    long long blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(bn_act_nhwc_kernel, dim3((unsigned)blocks), dim3(256), 0, estd_stream(stream),
                       reinterpret_cast<float4*>(x), reinterpret_cast<const float4*>(scale), reinterpret_cast<const float4*>(shift),
                       reinterpret_cast<const float4*>(residual), relu, n4, C / 4);
    return ESTD_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------
// PSM SPP tail: bilinear upsampling of the (tiny) pooled branch maps fused with the channel concatenation
namespace {
struct SppArgs { const float* b[4]; int bh[4], bw[4]; };

__global__ __launch_bounds__(256) void spp_upsample_cat_kernel(const float4* __restrict__ raw, int raw4, const float4* __restrict__ skip, int skip4,
                                                               SppArgs a, int nb, int cb4, float4* __restrict__ out, int N, int H, int W)
{
    const int out4 = raw4 + skip4 + nb * cb4;
    const long long total = (long long)N * H * W * out4;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int c = (int)(e % out4);
        const long long pix = e / out4;
        float4 v;
        if (c < raw4) v = raw[pix * raw4 + c];
        else if (c < raw4 + skip4) v = skip[pix * skip4 + (c - raw4)];
        else {
            const int k = (c - raw4 - skip4) / cb4, cc = (c - raw4 - skip4) - k * cb4;
            const int x = (int)(pix % W), y = (int)((pix / W) % H), n = (int)(pix / ((long long)W * H));
            const int bh = a.bh[k], bw = a.bw[k];
            // ATen area_pixel_compute_source_index, align_corners = False: src = scale * (dst + 0.5) - 0.5, clamped at 0
            const float sy = fmaxf(((float)bh / (float)H) * ((float)y + 0.5f) - 0.5f, 0.0f);
            const float sx = fmaxf(((float)bw / (float)W) * ((float)x + 0.5f) - 0.5f, 0.0f);
            const int y0 = (int)sy, x0 = (int)sx;
            const int y1 = y0 + (y0 < bh - 1 ? 1 : 0), x1 = x0 + (x0 < bw - 1 ? 1 : 0);
            const float ly = sy - (float)y0, lx = sx - (float)x0;
            const float hy = 1.0f - ly, hx = 1.0f - lx;
            const float4* src = reinterpret_cast<const float4*>(a.b[k]) + (long long)n * bh * bw * cb4 + cc;
            const float4 v00 = src[((long long)y0 * bw + x0) * cb4], v01 = src[((long long)y0 * bw + x1) * cb4];
            const float4 v10 = src[((long long)y1 * bw + x0) * cb4], v11 = src[((long long)y1 * bw + x1) * cb4];
            v.x = hy * (hx * v00.x + lx * v01.x) + ly * (hx * v10.x + lx * v11.x);
            v.y = hy * (hx * v00.y + lx * v01.y) + ly * (hx * v10.y + lx * v11.y);
            v.z = hy * (hx * v00.z + lx * v01.z) + ly * (hx * v10.z + lx * v11.z);
            v.w = hy * (hx * v00.w + lx * v01.w) + ly * (hx * v10.w + lx * v11.w);
        }
        out[e] = v;
    }
}
}  // namespace

extern "C" int estd_spp_upsample_cat(const float* raw, int c_raw, const float* skip, int c_skip, const float* const* branches,
                                     const int* bh, const int* bw, int nb, int c_b, float* out, int N, int H, int W, estd_stream_t stream)
{
    if (!raw || !skip || !branches || !bh || !bw || !out || nb < 1 || nb > 4 || N <= 0 || H <= 0 || W <= 0) return ESTD_ERR_ARG;
    if (c_raw <= 0 || c_skip <= 0 || c_b <= 0 || ((c_raw | c_skip | c_b) & 3)) return ESTD_ERR_ARG;
    SppArgs a;
    for (int k = 0; k < 4; ++k) {
        a.b[k] = branches[k < nb ? k : 0]; a.bh[k] = bh[k < nb ? k : 0]; a.bw[k] = bw[k < nb ? k : 0];
        if (k < nb && (!a.b[k] || a.bh[k] <= 0 || a.bw[k] <= 0)) return ESTD_ERR_ARG;
    }
    const long long total = (long long)N * H * W * ((c_raw + c_skip + nb * c_b) / 4);
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(spp_upsample_cat_kernel, dim3((unsigned)blocks), dim3(256), 0, estd_stream(stream),
                       reinterpret_cast<const float4*>(raw), c_raw / 4, reinterpret_cast<const float4*>(skip), c_skip / 4, a, nb, c_b / 4,
                       reinterpret_cast<float4*>(out), N, H, W);
    return ESTD_LAUNCH_CHECK();
}
