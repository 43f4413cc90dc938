// tsdf.hip -- volumetric fusion of posed depth maps into a truncated signed distance volume (KinectFusion's update rule) and the
// extraction of its zero crossings as an oriented point cloud.  Consumes what the model produces: ("depth", t, s) and ("fused_prob", t).
//
// Volume: two fp32 planes of [Z][Y][X] voxels, x fastest -- D in [-1, 1] and the weight Wt >= 0; all zeros = empty.  PLANAR storage: a lane
// owns four consecutive x voxels and moves them with one 16-byte access per plane (global_load_dwordx4 / global_store_dwordx4); the extraction
// reads D alone for most of its neighbours, which a planar volume serves at half the bytes of an interleaved one.
//
// estd_tsdf_integrate: ONE pass over the voxels for up to 8 frames.  Per voxel and frame, in frame order (the contract of include/estd_hip.h):
//     a = fma(A0, ix, fma(A1, iy, fma(A2, iz, A3)))          (b, c likewise; A = K [R|t] V rounded to fp32 on the host)
//     c > z_near;  ui = floor(a / c + 0.5), vi = floor(b / c + 0.5) inside the image;  d = depth[vi][ui] finite and > 0;
//     conf >= conf_min, w = conf (weighted, w > 0) or 1;  sdf = d - c >= -trunc;  tsdf = min(1, sdf / trunc);
//     D = fma(D, Wt, tsdf * w) / (Wt + w);  Wt = min(Wt + w, w_max).
// Every division is an IEEE division and every fused multiply-add is spelled out, so the pixel a voxel lands in and the bits of the result do
// not depend on how many frames share the launch (one T = 3 call == three T = 1 calls, bit for bit).
//
// Launch shape: a wave covers a 64 x 4 (x, y) brick -- 16 lanes x 16 bytes = 256 contiguous bytes per row -- and a workgroup of four waves a
// 64 x 16 brick that marches ZCHUNK planes along z (the (y, z) part of each dot product is shared by a lane's four voxels).  Phase 1
// projects a lane's four voxels into every frame and keeps (tsdf, w) in registers; only a lane that found an update loads its 2 x 16 bytes,
// applies the frames in order and stores them back.  A voxel more than a pixel outside an image is rejected by four compares before the
// divisions (the kernel is bound by the projection arithmetic, not by HBM, whenever the frusta fill little of the volume: profiles/tsdf_bench.txt).
// The predicate is per lane, so a wave whose brick lies outside every frustum issues no
// volume access at all (exec = 0 skips the block), and a 16-byte group no frame updates is neither read nor written.  The matrices, pointers
// and constants are kernel arguments (uniform values in SGPRs); the depth / confidence gathers go through the ordinary cached path.
// Offsets into the volume are 64-bit.
//
// estd_tsdf_integrate_color: the same kernel with COLOR set.  The colour volume is three more planes [3][Z][Y][X] that share the weight plane:
//     C_k = fma(C_k, Wt, image[t][k][vi][ui] * w) / (Wt + w)            (Wt before the update of D, the pixel the depth was read at)
// Phase 1 keeps the pixel index beside (tsdf, w) -- 32 registers, where 8 x 4 x 3 colours would take 96 -- and phase 2, where only updating
// lanes run, gathers the three channels.  estd_tsdf_edge_colors blends the colour planes along the edges the extraction emitted.
#include <type_traits>

#include "estd_common.h"

namespace {

constexpr int ZCHUNK = 8;          // planes a workgroup marches along z

struct IntegrateParams {
    int Z, Y, X, T, H, W, weighted;
    float trunc, z_near, conf_min, w_max;
    float* D;
    float* Wt;
    const float* depth[ESTD_TSDF_MAX_FRAMES];
    const float* conf[ESTD_TSDF_MAX_FRAMES];
    float A[ESTD_TSDF_MAX_FRAMES][12];
};

// the colour instances' arguments: the same fields first, then the three colour planes [3][Z][Y][X] and one [3][H][W] image per frame
struct IntegrateColorParams : IntegrateParams {
    float* C;
    const float* image[ESTD_TSDF_MAX_FRAMES];
};

// SKIP = false (the tool's ablation): every lane inside the volume loads and stores its voxels whether a frame updates them or not.
// COLOR (estd_tsdf_integrate_color): phase 1 also keeps the pixel it chose, phase 2 gathers that pixel's three channels -- only in lanes
// that update, once per (frame, voxel) update -- and blends them with the weight the D update starts from; D and Wt take the same
// operations in the same order as without colour.
template <bool SKIP, bool COLOR>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const std::conditional_t<COLOR, IntegrateColorParams, IntegrateParams> p)
{
    const int x0 = ((int)blockIdx.x * 16 + ((int)threadIdx.x & 15)) * 4;
    const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
    const bool inside = x0 < p.X && y < p.Y;            // X is a multiple of 4: a lane's four voxels are inside or outside together
    const int z_begin = (int)blockIdx.z * ZCHUNK;
    const int z_end = z_begin + ZCHUNK < p.Z ? z_begin + ZCHUNK : p.Z;
    const float fy = (float)y;
    const float fW = (float)p.W, fH = (float)p.H;
    const bool has_conf = p.conf[0] != nullptr;

    for (int z = z_begin; z < z_end; ++z) {
        const float fz = (float)z;
        // COLOR: the per-frame arguments (12 + 3 x 2 SGPRs each, 144 for eight frames) do not fit the scalar registers beside the rest; an
        // offset of zero the compiler cannot see through makes it fetch them from the argument segment where they are used, plane by
        // plane (scalar loads that hit the scalar cache), instead of parking them all in VGPR lanes across the z loop
        int fo = 0;
        if constexpr (COLOR) asm volatile("s_mov_b32 %0, 0" : "=s"(fo));
        float ts[ESTD_TSDF_MAX_FRAMES][4], ws[ESTD_TSDF_MAX_FRAMES][4];
        int px[COLOR ? ESTD_TSDF_MAX_FRAMES : 1][4];
        bool any = false;
#pragma unroll
        for (int t = 0; t < ESTD_TSDF_MAX_FRAMES; ++t) {
#pragma unroll
            for (int v = 0; v < 4; ++v) { ts[t][v] = 0.f; ws[t][v] = 0.f; }
            if (t < p.T && inside) {
                const float* A = p.A[t + fo];
                const float ra = fmaf(A[1], fy, fmaf(A[2], fz, A[3]));
                const float rb = fmaf(A[5], fy, fmaf(A[6], fz, A[7]));
                const float rc = fmaf(A[9], fy, fmaf(A[10], fz, A[11]));
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float fx = (float)(x0 + v);
                    const float c = fmaf(A[8], fx, rc);
                    if (!(c > p.z_near)) continue;
                    const float a = fmaf(A[0], fx, ra), b = fmaf(A[4], fx, rb);
                    // cheap, conservative rejection in front of the two divisions: a projection more than a pixel outside the image
                    // (a / c < -1.5 or > W + 0.5; a rounded product moves the limit by 2^-24 of it) is outside for the exact test below
                    // too, so the result does not change; most waves outside every frustum leave here as a whole
                    if (a < -1.5f * c || a > (fW + 0.5f) * c || b < -1.5f * c || b > (fH + 0.5f) * c) continue;
                    const float u = floorf(a / c + 0.5f), w = floorf(b / c + 0.5f);
                    if (!(u >= 0.f && u < fW && w >= 0.f && w < fH)) continue;
                    const int pix = (int)w * p.W + (int)u;
                    const float d = p.depth[t + fo][pix];
                    if (!(d > 0.f && d < __builtin_inff())) continue;
                    float wgt = 1.f;
                    if (has_conf) {
                        const float cf = p.conf[t + fo][pix];
                        if (cf < p.conf_min) continue;
                        if (p.weighted) wgt = cf;
                        if (!(wgt > 0.f && wgt < __builtin_inff())) continue;       // a sample of zero (or undefined) weight carries nothing
                    }
                    const float sdf = d - c;
                    if (sdf < -p.trunc) continue;
                    ts[t][v] = fminf(1.f, sdf / p.trunc);
                    ws[t][v] = wgt;
                    if constexpr (COLOR) px[t][v] = pix;
                    any = true;
                }
            }
        }
        if (SKIP ? any : inside) {
            const long long off = ((long long)z * p.Y + y) * p.X + x0;
            float4 d4 = *reinterpret_cast<const float4*>(p.D + off);
            float4 w4 = *reinterpret_cast<const float4*>(p.Wt + off);
            float dv[4] = {d4.x, d4.y, d4.z, d4.w}, wv[4] = {w4.x, w4.y, w4.z, w4.w};
            float cv[COLOR ? 3 : 1][4];
            const long long plane = (long long)p.Z * p.Y * p.X;
            const long long hw = (long long)p.H * p.W;
            if constexpr (COLOR) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float4 c4 = *reinterpret_cast<const float4*>(p.C + k * plane + off);
                    cv[k][0] = c4.x; cv[k][1] = c4.y; cv[k][2] = c4.z; cv[k][3] = c4.w;
                }
            }
#pragma unroll
            for (int t = 0; t < ESTD_TSDF_MAX_FRAMES; ++t) {
                if (t < p.T) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        if (ws[t][v] > 0.f) {
                            const float den = wv[v] + ws[t][v];
                            if constexpr (COLOR) {
#pragma unroll
                                for (int k = 0; k < 3; ++k) {
                                    const float col = p.image[t + fo][k * hw + px[t][v]];
                                    cv[k][v] = fmaf(cv[k][v], wv[v], col * ws[t][v]) / den;
                                }
                            }
                            dv[v] = fmaf(dv[v], wv[v], ts[t][v] * ws[t][v]) / den;
                            wv[v] = fminf(den, p.w_max);
                        }
                    }
                }
            }
            *reinterpret_cast<float4*>(p.D + off) = make_float4(dv[0], dv[1], dv[2], dv[3]);
            *reinterpret_cast<float4*>(p.Wt + off) = make_float4(wv[0], wv[1], wv[2], wv[3]);
            if constexpr (COLOR) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    *reinterpret_cast<float4*>(p.C + k * plane + off) = make_float4(cv[k][0], cv[k][1], cv[k][2], cv[k][3]);
            }
        }
    }
}

struct ExtractParams {
    int Z, Y, X;
    float w_min, voxel, origin[3];
    const float* D;
    const float* Wt;
    unsigned long long* counter;
    long long capacity;
    float* xyz;
    float* normal;
    float* weight;
    long long* edge;
};

// gradient of D at voxel (q[0], q[1], q[2]) = (x, y, z) in units per voxel: central difference where both neighbours along an axis exist and
// are observed (Wt >= w_min), the one-sided difference where one does, 0 where neither does
__device__ inline void tsdf_gradient(const ExtractParams& p, const int q[3], float g[3])
{
    const int dims[3] = {p.X, p.Y, p.Z};
    const long long strides[3] = {1, p.X, (long long)p.X * p.Y};
    const long long idx = ((long long)q[2] * p.Y + q[1]) * p.X + q[0];
    const float dq = p.D[idx];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool lo = q[k] > 0 && p.Wt[idx - strides[k]] >= p.w_min;
        const bool hi = q[k] + 1 < dims[k] && p.Wt[idx + strides[k]] >= p.w_min;
        const float dl = lo ? p.D[idx - strides[k]] : dq, dh = hi ? p.D[idx + strides[k]] : dq;
        g[k] = (lo && hi) ? 0.5f * (dh - dl) : dh - dl;
    }
}

// one lane per voxel, lanes along x; a wave is 64 voxels of one row.  Each lane tests its +x, +y, +z edges; the wave then takes ONE
// increment of the counter for all its crossings (three ballots, population counts, lane 0 adds the total) and every crossing finds its
// slot from the counts below its lane.
__global__ __launch_bounds__(256) void tsdf_extract_kernel(const ExtractParams p)
{
    const int lane = (int)threadIdx.x & 63;
    const int q[3] = {(int)blockIdx.x * 64 + lane, (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6), (int)blockIdx.z};
    const int dims[3] = {p.X, p.Y, p.Z};
    const long long strides[3] = {1, p.X, (long long)p.X * p.Y};
    const long long idx = ((long long)q[2] * p.Y + q[1]) * p.X + q[0];
    bool cross[3] = {false, false, false};
    float d0 = 0.f, w0 = 0.f, d1[3] = {0.f, 0.f, 0.f}, w1[3] = {0.f, 0.f, 0.f};
    if (q[0] < p.X && q[1] < p.Y) {
        w0 = p.Wt[idx];
        if (w0 >= p.w_min) {
            d0 = p.D[idx];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (q[k] + 1 < dims[k]) {
                    w1[k] = p.Wt[idx + strides[k]];
                    if (w1[k] >= p.w_min) {
                        d1[k] = p.D[idx + strides[k]];
                        cross[k] = (d0 < 0.f && 0.f <= d1[k]) || (d1[k] < 0.f && 0.f <= d0);
                    }
                }
            }
        }
    }
    const unsigned long long b0 = __ballot(cross[0]), b1 = __ballot(cross[1]), b2 = __ballot(cross[2]);
    const int n0 = __popcll(b0), n1 = __popcll(b1), n2 = __popcll(b2);
    if (n0 + n1 + n2 == 0) return;                       // wave-uniform
    unsigned int base_lo = 0, base_hi = 0;
    if (lane == 0) {
        const unsigned long long base = atomicAdd(p.counter, (unsigned long long)(n0 + n1 + n2));
        base_lo = (unsigned int)base;
        base_hi = (unsigned int)(base >> 32);
    }
    base_lo = __shfl(base_lo, 0);
    base_hi = __shfl(base_hi, 0);
    const long long base = (long long)(((unsigned long long)base_hi << 32) | base_lo);
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long first[3] = {base + __popcll(b0 & below), base + n0 + __popcll(b1 & below), base + n0 + n1 + __popcll(b2 & below)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!cross[k] || first[k] >= p.capacity) continue;        // records past the capacity are dropped; the counter keeps the total
        const long long slot = first[k];
        const float s = d0 / (d0 - d1[k]);
        int qn[3] = {q[0], q[1], q[2]};
        qn[k] += 1;
        float g0[3], g1[3], g[3];
        tsdf_gradient(p, q, g0);
        tsdf_gradient(p, qn, g1);
#pragma unroll
        for (int j = 0; j < 3; ++j) g[j] = fmaf(s, g1[j] - g0[j], g0[j]);
        const float len2 = fmaf(g[2], g[2], fmaf(g[1], g[1], g[0] * g[0]));
        const float len = sqrtf(len2);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            p.normal[slot * 3 + j] = len > 0.f ? g[j] / len : 0.f;
            const float cell = (float)q[j] + 0.5f + (j == k ? s : 0.f);
            p.xyz[slot * 3 + j] = fmaf(cell, p.voxel, p.origin[j]);
        }
        p.weight[slot] = fmaf(s, w1[k] - w0, w0);
        p.edge[slot] = 3 * idx + k;
    }
}

struct EdgeColorParams {
    int Z, Y, X;
    long long n;
    const float* D;
    const float* C;
    const long long* edge;
    float* out;
};

// one lane per record: the colour at the crossing of edge id 3 * voxel + axis, blended with the s the extraction computed from the same
// stored D values; an id outside the volume (or whose far end is) gives zeros
__global__ __launch_bounds__(256) void tsdf_edge_colors_kernel(const EdgeColorParams p)
{
    const long long i = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (i >= p.n) return;
    const long long plane = (long long)p.Z * p.Y * p.X;
    const long long e = p.edge[i];
    float c[3] = {0.f, 0.f, 0.f};
    if (e >= 0 && e < 3 * plane) {
        const long long idx = e / 3;
        const int k = (int)(e - 3 * idx);
        const long long row = idx / p.X;
        const int q[3] = {(int)(idx - row * p.X), (int)(row % p.Y), (int)(row / p.Y)};
        const int dims[3] = {p.X, p.Y, p.Z};
        const long long strides[3] = {1, p.X, (long long)p.X * p.Y};
        if (q[k] + 1 < dims[k]) {
            const long long far = idx + strides[k];
            const float d0 = p.D[idx], d1 = p.D[far];
            const float s = d0 / (d0 - d1);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float c0 = p.C[j * plane + idx], c1 = p.C[j * plane + far];
                c[j] = fmaf(s, c1 - c0, c0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) p.out[i * 3 + j] = c[j];
}

inline int check_dims(int Z, int Y, int X)
{
    if (Z <= 0 || Y <= 0 || X <= 0 || (X & 3)) return ESTD_ERR_ARG;
    // 64-bit offsets inside the kernels; the launch grids (z on blockIdx.z) and the 3 * index + axis edge ids bound each dimension
    if (Z > 65535 || Y > 65535 * 4 || X > (1 << 20)) return ESTD_ERR_UNSUPPORTED;
    return ESTD_OK;
}

// the argument checks and the launch arguments the two integrate entry points share
template <class Desc, class Params>
inline int integrate_setup(const Desc* d, Params& p)
{
    if (!d->tsdf || !d->weight) return ESTD_ERR_ARG;
    if (d->T < 1 || d->T > ESTD_TSDF_MAX_FRAMES || d->H <= 0 || d->W <= 0) return ESTD_ERR_ARG;
    if ((long long)d->H * d->W > 0x7fffffffLL) return ESTD_ERR_ARG;
    if (!finite_pos(d->trunc) || !finite_pos(d->w_max) || !(d->z_near >= 0.f) || !(d->conf_min == d->conf_min)) return ESTD_ERR_ARG;
    for (int t = 0; t < d->T; ++t) {
        if (!d->depth[t]) return ESTD_ERR_ARG;
        if ((d->conf[t] != nullptr) != (d->conf[0] != nullptr)) return ESTD_ERR_ARG;     // a confidence map for every frame or for none
    }
    if (d->weighted && !d->conf[0]) return ESTD_ERR_ARG;
    if (const int st = check_dims(d->Z, d->Y, d->X)) return st;
    p.Z = d->Z; p.Y = d->Y; p.X = d->X; p.T = d->T; p.H = d->H; p.W = d->W; p.weighted = d->weighted != 0;
    p.trunc = d->trunc; p.z_near = d->z_near; p.conf_min = d->conf_min; p.w_max = d->w_max;
    p.D = d->tsdf; p.Wt = d->weight;
    for (int t = 0; t < ESTD_TSDF_MAX_FRAMES; ++t) {
        p.depth[t] = t < d->T ? d->depth[t] : nullptr;
        p.conf[t] = t < d->T ? d->conf[t] : nullptr;
        for (int i = 0; i < 12; ++i) p.A[t][i] = t < d->T ? d->mats[t][i] : 0.f;
    }
    return ESTD_OK;
}

inline dim3 integrate_grid(int Z, int Y, int X)
{
    return dim3((unsigned)estd_ceil_div(X, 64), (unsigned)estd_ceil_div(Y, 16), (unsigned)estd_ceil_div(Z, ZCHUNK));
}

}  // namespace

extern "C" int estd_tsdf_integrate(const estd_tsdf_integrate_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    IntegrateParams p;
    if (const int st = integrate_setup(d, p)) return st;
    const dim3 grid = integrate_grid(d->Z, d->Y, d->X);
    if (d->no_skip)
        hipLaunchKernelGGL((tsdf_integrate_kernel<false, false>), grid, dim3(256), 0, estd_stream(s), p);
    else
        hipLaunchKernelGGL((tsdf_integrate_kernel<true, false>), grid, dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_tsdf_integrate_color(const estd_tsdf_integrate_color_desc* d, estd_stream_t s)
{
    if (!d || !d->color) return ESTD_ERR_ARG;
    for (int t = 0; t < d->T && t < ESTD_TSDF_MAX_FRAMES; ++t)
        if (!d->image[t]) return ESTD_ERR_ARG;
    IntegrateColorParams p;
    if (const int st = integrate_setup(d, p)) return st;
    p.C = d->color;
    for (int t = 0; t < ESTD_TSDF_MAX_FRAMES; ++t) p.image[t] = t < d->T ? d->image[t] : nullptr;
    const dim3 grid = integrate_grid(d->Z, d->Y, d->X);
    if (d->no_skip)
        hipLaunchKernelGGL((tsdf_integrate_kernel<false, true>), grid, dim3(256), 0, estd_stream(s), p);
    else
        hipLaunchKernelGGL((tsdf_integrate_kernel<true, true>), grid, dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_tsdf_edge_colors(const float* tsdf, const float* color, int Z, int Y, int X, const long long* edge, long long n, float* out,
                                     estd_stream_t s)
{
    if (!tsdf || !color || n < 0) return ESTD_ERR_ARG;
    if (n > 0 && (!edge || !out)) return ESTD_ERR_ARG;
    if (const int st = check_dims(Z, Y, X)) return st;
    if (n > 0x7fffffffLL * 256) return ESTD_ERR_UNSUPPORTED;          // one workgroup of 256 records per blockIdx.x
    if (n == 0) return ESTD_OK;
    EdgeColorParams p;
    p.Z = Z; p.Y = Y; p.X = X; p.n = n; p.D = tsdf; p.C = color; p.edge = edge; p.out = out;
    hipLaunchKernelGGL(tsdf_edge_colors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_tsdf_extract_points(const float* tsdf, const float* weight, int Z, int Y, int X, float voxel_size, const float* origin3,
                                        float w_min, unsigned long long* counter, long long capacity, float* xyz, float* normal,
                                        float* point_weight, long long* edge, estd_stream_t s)
{
    if (!tsdf || !weight || !origin3 || !counter || capacity < 0 || !finite_pos(voxel_size) || !(w_min == w_min)) return ESTD_ERR_ARG;
    if (capacity > 0 && (!xyz || !normal || !point_weight || !edge)) return ESTD_ERR_ARG;
    if (const int st = check_dims(Z, Y, X)) return st;
    ExtractParams p;
    p.Z = Z; p.Y = Y; p.X = X; p.w_min = w_min; p.voxel = voxel_size;
    for (int j = 0; j < 3; ++j) p.origin[j] = origin3[j];       // HOST pointer: three floats copied into the launch arguments
    p.D = tsdf; p.Wt = weight; p.counter = counter; p.capacity = capacity;
    p.xyz = xyz; p.normal = normal; p.weight = point_weight; p.edge = edge;
    const dim3 grid((unsigned)estd_ceil_div(X, 64), (unsigned)estd_ceil_div(Y, 4), (unsigned)Z);
    hipLaunchKernelGGL(tsdf_extract_kernel, grid, dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
