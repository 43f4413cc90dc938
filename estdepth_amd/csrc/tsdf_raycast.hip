// tsdf_raycast.hip -- the way back out of the TSDF volume of csrc/tsdf.hip: depth, normal and weight maps of the fused surface as a pinhole
// camera sees it (KinectFusion's surface prediction), by marching one ray per pixel through the volume at a fixed step of z-depth.
//
// estd_tsdf_raycast, per pixel (u, v) (the contract of include/estd_hip.h; M = [R K^-1 / voxel | (c - origin) / voxel - 0.5] on the host):
//     r_j = fma(M[j][0], u, fma(M[j][1], v, M[j][2]));  t_k = fma(k, dt, t_min);  p_j = fma(t_k, r_j, M[j][3])       (voxel-index coordinates)
//     sample k is OBSERVED iff its cell floor(p) lies in [0, dim - 2] on every axis and all eight corner weights are >= w_min;
//     F, Wb = trilinear blends (x, then y, then z, lerp(a, b, f) = fma(f, b - a, a)) of the corner D values / weights, G the interpolant's gradient;
//     hit = the first k with samples k - 1 and k observed and F_{k-1} > 0 >= F_k:  s = F_{k-1} / (F_{k-1} - F_k),  depth = fma(dt, s, t_{k-1}),
//     normal = g / |g| with g = fma(s, G_k - G_{k-1}, G_{k-1}),  weight = fma(s, Wb_k - Wb_{k-1}, Wb_{k-1});  no hit: all zeros.
// Every division is an IEEE division, every fused multiply-add is spelled out and there is no atomic: two calls give the same bits.
//
// Launch shape: one lane per pixel, a wave on an 8 x 8 pixel tile (neighbouring rays walk neighbouring voxels, so the sixteen gathers of a
// wave's sample fall into few cache lines), a workgroup of four waves on 16 x 16 pixels.  Consecutive workgroup ids are dealt round-robin over
// the eight XCDs, each with an L2 of its own; the id is remapped so that the workgroups of one XCD render a contiguous band of image rows and
// the eight L2s hold eight disjoint slabs of the volume instead of eight copies of all of it (for speed only: any placement gives the same
// result).
//
// What the kernel skips, none of which changes a bit of the result:
//   * a ray / box slab test per lane bounds the sample indices that can fall inside the volume; the box is widened by far more than the
//     rounding of p and the index interval by two samples and a relative margin, so every sample left out is provably unobserved (its cell
//     is outside [0, dim - 2]).  The k range of the loop is the union of the lanes' intervals (wave reductions) and so wave-uniform;
//   * the eight weights are probed first; the eight D values are gathered only where all eight weights pass;
//   * a lane is done at its hit or past its interval, and the wave leaves the loop once all its lanes are done.
// The matrix, pointers and constants are kernel arguments (uniform values in SGPRs); the gathers go through the ordinary cached path; offsets
// into the volume are 64-bit.
//
// estd_tsdf_raycast_color: the same kernel with COLOR set.  That instance alone keeps the previous sample's cell base and fractions; at the hit
// -- once per pixel, not per sample -- it gathers the 2 x 8 x 3 corner colours of the two cells, blends each cell the way Wb is blended and
// writes fma(s, Cb_k - Cb_{k-1}, Cb_{k-1}).  Depth, normal and weight take the same operations as without colour.
#include <type_traits>

#include "estd_common.h"
#include "estd_device.h"

namespace {

struct RaycastParams {
    int Z, Y, X, H, W, n_steps, tiles_x, n_blocks;
    float t_min, dt, w_min;
    float M[12];
    const float* D;
    const float* Wt;
    float* depth;
    float* normal;
    float* weight;
    unsigned int* stats;
};

struct RaycastColorParams : RaycastParams {
    const float* C;
    float* color;
};

// the trilinear blend (x, then y, then z: the nesting of Wb) of one plane at the cell whose first corner is c
__device__ inline float blend_cell(const float* c, long long sy, long long sz, float fx, float fy, float fz)
{
    return lerpf(lerpf(lerpf(c[0], c[1], fx), lerpf(c[sy], c[sy + 1], fx), fy),
                 lerpf(lerpf(c[sz], c[sz + 1], fx), lerpf(c[sz + sy], c[sz + sy + 1], fx), fy), fz);
}

__device__ inline int wave_min(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { const int o = __shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}

__device__ inline int wave_max(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { const int o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}

// STATS (the bench tool's counters): per pixel the samples whose weights were probed and the samples whose D values were gathered
template <bool STATS, bool COLOR>
__global__ __launch_bounds__(256) void tsdf_raycast_kernel(const std::conditional_t<COLOR, RaycastColorParams, RaycastParams> p)
{
    // workgroup id -> 16 x 16 tile, row-major within the band of its XCD: ids b, b + 8, b + 16, ... share an XCD
    const int b = (int)blockIdx.x;
    const int per = p.n_blocks >> 3, rem = p.n_blocks & 7;
    const int xcd = b & 7;
    const int tile = xcd * per + (xcd < rem ? xcd : rem) + (b >> 3);
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int u = tx * 16 + (wave & 1) * 8 + (lane & 7);
    const int v = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool valid = u < p.W && v < p.H;

    const float fu = (float)u, fv = (float)v;
    float r[3], o[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        r[j] = fmaf(p.M[4 * j], fu, fmaf(p.M[4 * j + 1], fv, p.M[4 * j + 2]));
        o[j] = p.M[4 * j + 3];
    }

    // conservative interval [k_lo, k_hi] of the samples that can lie inside the volume.  A sample is observed only if the computed
    // p_j = fma(t_k, r_j, o_j) is in [0, dim_j - 1); one rounding moves it by at most 2^-24 dim_j, so the exact o_j + t_k r_j is inside the
    // box widened by eps_j >= 1e-3, and t_k inside the slab interval of the widened box; the interval in k is widened by two samples and
    // 1e-6 of its magnitude (the roundings of t_k, of the two divisions and of the subtractions are a few 2^-24 of it).  NaNs that the
    // infinities of a near-zero r_j can make only DROP a constraint (fmaxf / fminf return the other operand).
    const float dims[3] = {(float)p.X, (float)p.Y, (float)p.Z};
    float klo = 0.f, khi = (float)(p.n_steps - 1);
    bool empty = !valid;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float eps = fmaf(1e-5f, fabsf(o[j]) + dims[j], 1e-3f);
        const float lo = -eps, hi = dims[j] - 1.f + eps;
        if (r[j] == 0.f) {
            if (!(o[j] >= lo && o[j] <= hi)) empty = true;
        } else {
            float t0 = (lo - o[j]) / r[j], t1 = (hi - o[j]) / r[j];
            if (t0 > t1) { const float x = t0; t0 = t1; t1 = x; }
            const float k0 = (t0 - p.t_min) / p.dt - fmaf(1e-6f, (fabsf(t0) + p.t_min) / p.dt, 2.f);
            const float k1 = (t1 - p.t_min) / p.dt + fmaf(1e-6f, (fabsf(t1) + p.t_min) / p.dt, 2.f);
            klo = fmaxf(klo, floorf(k0));
            khi = fminf(khi, ceilf(k1));
        }
    }
    if (!(klo <= khi)) empty = true;
    const int k_lo = empty ? 0x7fffffff : (int)klo;
    const int k_hi = empty ? -1 : (int)khi;
    const int k_begin = wave_min(k_lo), k_end = wave_max(k_hi);          // wave-uniform

    const long long sy = p.X, sz = (long long)p.X * p.Y;
    const float cx = (float)(p.X - 2), cy = (float)(p.Y - 2), cz = (float)(p.Z - 2);
    bool done = empty, obs_p = false;
    float F_p = 0.f, Wb_p = 0.f, G_p[3] = {0.f, 0.f, 0.f}, t_p = 0.f;
    float out_depth = 0.f, out_weight = 0.f, out_n[3] = {0.f, 0.f, 0.f};
    unsigned int n_probed = 0, n_gathered = 0;
    long long base_p = 0;                                   // COLOR only: the previous sample's cell and fractions
    float f_p[3] = {0.f, 0.f, 0.f}, out_c[3] = {0.f, 0.f, 0.f};

    for (int k = k_begin; k <= k_end; ++k) {
        if (__all(done)) break;
        const float t = fmaf((float)k, p.dt, p.t_min);
        bool obs = false;
        float F = 0.f, Wb = 0.f, G[3] = {0.f, 0.f, 0.f};
        long long base_k = 0;
        float f_k[3] = {0.f, 0.f, 0.f};
        if (!done && k >= k_lo) {
            const float px = fmaf(t, r[0], o[0]), py = fmaf(t, r[1], o[1]), pz = fmaf(t, r[2], o[2]);
            const float ix = floorf(px), iy = floorf(py), iz = floorf(pz);
            if (ix >= 0.f && ix <= cx && iy >= 0.f && iy <= cy && iz >= 0.f && iz <= cz) {          // false for a NaN coordinate
                const long long base = ((long long)(int)iz * p.Y + (int)iy) * p.X + (int)ix;
                const float* w = p.Wt + base;
                const float w000 = w[0], w100 = w[1], w010 = w[sy], w110 = w[sy + 1];
                const float w001 = w[sz], w101 = w[sz + 1], w011 = w[sz + sy], w111 = w[sz + sy + 1];
                if (STATS) ++n_probed;
                const float wm = p.w_min;
                if (w000 >= wm && w100 >= wm && w010 >= wm && w110 >= wm && w001 >= wm && w101 >= wm && w011 >= wm && w111 >= wm) {
                    const float* d = p.D + base;
                    const float d000 = d[0], d100 = d[1], d010 = d[sy], d110 = d[sy + 1];
                    const float d001 = d[sz], d101 = d[sz + 1], d011 = d[sz + sy], d111 = d[sz + sy + 1];
                    if (STATS) ++n_gathered;
                    const float fx = px - ix, fy = py - iy, fz = pz - iz;
                    const float c00 = lerpf(d000, d100, fx), c10 = lerpf(d010, d110, fx);
                    const float c01 = lerpf(d001, d101, fx), c11 = lerpf(d011, d111, fx);
                    const float c0 = lerpf(c00, c10, fy), c1 = lerpf(c01, c11, fy);
                    F = lerpf(c0, c1, fz);
                    G[0] = lerpf(lerpf(d100 - d000, d110 - d010, fy), lerpf(d101 - d001, d111 - d011, fy), fz);
                    G[1] = lerpf(c10 - c00, c11 - c01, fz);
                    G[2] = c1 - c0;
                    Wb = lerpf(lerpf(lerpf(w000, w100, fx), lerpf(w010, w110, fx), fy),
                               lerpf(lerpf(w001, w101, fx), lerpf(w011, w111, fx), fy), fz);
                    if constexpr (COLOR) { base_k = base; f_k[0] = fx; f_k[1] = fy; f_k[2] = fz; }
                    obs = true;
                }
            }
        }
        if (obs && obs_p && F_p > 0.f && F <= 0.f) {              // front face: from free space into the surface
            const float s = F_p / (F_p - F);
            out_depth = fmaf(p.dt, s, t_p);
            float g[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) g[j] = fmaf(s, G[j] - G_p[j], G_p[j]);
            const float len = sqrtf(fmaf(g[2], g[2], fmaf(g[1], g[1], g[0] * g[0])));
#pragma unroll
            for (int j = 0; j < 3; ++j) out_n[j] = len > 0.f ? g[j] / len : 0.f;
            out_weight = fmaf(s, Wb - Wb_p, Wb_p);
            if constexpr (COLOR) {
                const long long plane = (long long)p.Z * p.Y * p.X;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float c0 = blend_cell(p.C + j * plane + base_p, sy, sz, f_p[0], f_p[1], f_p[2]);
                    const float c1 = blend_cell(p.C + j * plane + base_k, sy, sz, f_k[0], f_k[1], f_k[2]);
                    out_c[j] = fmaf(s, c1 - c0, c0);
                }
            }
            done = true;
        }
        obs_p = obs; F_p = F; Wb_p = Wb; t_p = t;
#pragma unroll
        for (int j = 0; j < 3; ++j) G_p[j] = G[j];
        if constexpr (COLOR) {
            base_p = base_k;
#pragma unroll
            for (int j = 0; j < 3; ++j) f_p[j] = f_k[j];
        }
        if (k >= k_hi) done = true;
    }

    if (valid) {
        const long long pix = (long long)v * p.W + u;
        p.depth[pix] = out_depth;
        p.weight[pix] = out_weight;
#pragma unroll
        for (int j = 0; j < 3; ++j) p.normal[pix * 3 + j] = out_n[j];
        if constexpr (COLOR) {
#pragma unroll
            for (int j = 0; j < 3; ++j) p.color[pix * 3 + j] = out_c[j];
        }
        if (STATS) {
            p.stats[pix * 2] = n_probed;
            p.stats[pix * 2 + 1] = n_gathered;
        }
    }
}

template <class Desc, class Params>
inline int raycast_setup(const Desc* d, Params& p)
{
    if (!d->tsdf || !d->weight || !d->depth || !d->normal || !d->out_weight) return ESTD_ERR_ARG;
    if (d->H <= 0 || d->W <= 0 || d->n_steps <= 0) return ESTD_ERR_ARG;
    if (!estd_finite(d->dt) || !(d->dt > 0.f) || !estd_finite(d->t_min) || !(d->t_min >= 0.f) || !(d->w_min == d->w_min)) return ESTD_ERR_ARG;
    for (int i = 0; i < 12; ++i)
        if (!estd_finite(d->mat[i])) return ESTD_ERR_ARG;
    if (d->Z <= 0 || d->Y <= 0 || d->X <= 0 || (d->X & 3)) return ESTD_ERR_ARG;
    // the volume limits of the other entry points; one workgroup per 16 x 16 pixels on blockIdx.x; k is exact in fp32 up to 2^24
    if (d->Z > 65535 || d->Y > 65535 * 4 || d->X > (1 << 20)) return ESTD_ERR_UNSUPPORTED;
    if ((long long)d->H * d->W > 0x7fffffffLL || d->n_steps > (1 << 24)) return ESTD_ERR_UNSUPPORTED;
    p.Z = d->Z; p.Y = d->Y; p.X = d->X; p.H = d->H; p.W = d->W; p.n_steps = d->n_steps;
    p.tiles_x = estd_ceil_div(d->W, 16);
    p.n_blocks = p.tiles_x * estd_ceil_div(d->H, 16);
    p.t_min = d->t_min; p.dt = d->dt; p.w_min = d->w_min;
    for (int i = 0; i < 12; ++i) p.M[i] = d->mat[i];
    p.D = d->tsdf; p.Wt = d->weight; p.depth = d->depth; p.normal = d->normal; p.weight = d->out_weight; p.stats = d->stats;
    return ESTD_OK;
}

}  // namespace

extern "C" int estd_tsdf_raycast(const estd_tsdf_raycast_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    RaycastParams p;
    if (const int st = raycast_setup(d, p)) return st;
    if (d->stats)
        hipLaunchKernelGGL((tsdf_raycast_kernel<true, false>), dim3((unsigned)p.n_blocks), dim3(256), 0, estd_stream(s), p);
    else
        hipLaunchKernelGGL((tsdf_raycast_kernel<false, false>), dim3((unsigned)p.n_blocks), dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_tsdf_raycast_color(const estd_tsdf_raycast_color_desc* d, estd_stream_t s)
{
    if (!d || !d->color || !d->out_color) return ESTD_ERR_ARG;
    RaycastColorParams p;
    if (const int st = raycast_setup(d, p)) return st;
    p.C = d->color; p.color = d->out_color;
    if (d->stats)
        hipLaunchKernelGGL((tsdf_raycast_kernel<true, true>), dim3((unsigned)p.n_blocks), dim3(256), 0, estd_stream(s), p);
    else
        hipLaunchKernelGGL((tsdf_raycast_kernel<false, true>), dim3((unsigned)p.n_blocks), dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
