// depth_consistency.hip -- the geometric cross-view check of multi-view stereo pipelines (MVSNet's / COLMAP's filter) in front of the TSDF
// fusion of csrc/tsdf.hip: one target depth map is reprojected into S source views, each source's depth is read there (bilinear), carried
// back into the target view, and a source counts as consistent where it lands within px_max pixels of where it started at a depth within
// rel_max of the target's.  A gather kernel: (1 + S) maps read, four written.
//
// estd_depth_consistency, per target pixel (u, v) (the contract of include/estd_hip.h; F_s = [K_s R_st K_t^-1 | K_s t_st], B_s the same the
// other way, both formed on the host):
//     d = depth_t[v][u]; invalid (all outputs 0) unless finite and > z_near.  For each source in order:
//     (a, b, c)_j = fma(d, fma(F[j][0], u, fma(F[j][1], v, F[j][2])), F[j][3]);  skip unless c > z_near;  us = a / c, vs = b / c;
//     skip unless 0 <= us <= W - 1 and 0 <= vs <= H - 1;  x0 = min(floor(us), W - 2), y0 likewise;  skip unless the four taps are finite
//     and > z_near;  ds = lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy), lerp(a, b, f) = fma(f, b - a, a), fx = us - x0, fy = vs - y0;
//     (a', b', c') from B, us, vs, ds in the same shape;  skip unless c' > z_near;  u' = a' / c', v' = b' / c';  the source is VISIBLE;
//     e2 = fma(u' - u, u' - u, (v' - v)^2),  rel = |c' - d| / d;  CONSISTENT iff e2 < px_max^2 and rel < rel_max.
//     views / visible = the counts;  depth = (d + c'_1 + c'_2 + ...) / (1 + views) over the consistent sources, added in source order;
//     rel_err = (rel_1 + rel_2 + ...) / views, 0 where views = 0.
// Every division is an IEEE division, every fused multiply-add is spelled out and there is no atomic: two calls give the same bits.
//
// Launch shape (csrc/tsdf_raycast.hip's): one lane per pixel, a wave on an 8 x 8 pixel tile -- neighbouring target pixels land on neighbouring
// source pixels, so the four taps of a wave fall into few cache lines -- a workgroup of four waves on 16 x 16 pixels.  The source loop is
// rolled and wave-uniform (S is a kernel argument); the matrices, pointers and constants are kernel arguments, read with scalar loads at
// the loop's index -- unrolled, 8 x 24 matrix values would not fit the scalar registers.  The gathers go through the ordinary cached path;
// pixel offsets are 64-bit.  A lane outside the image, an invalid pixel and a skipped source only mask lanes: no lane leaves the loop early.
#include "estd_common.h"
#include "estd_device.h"

namespace {

struct ConsistencyParams {
    int H, W, S, tiles_x;
    float z_near, px_max2, rel_max;
    const float* target;
    float* views;
    float* visible;
    float* depth;
    float* rel_err;
    const float* source[ESTD_CONSISTENCY_MAX_SOURCES];
    float F[ESTD_CONSISTENCY_MAX_SOURCES][12];
    float B[ESTD_CONSISTENCY_MAX_SOURCES][12];
};

__global__ __launch_bounds__(256) void depth_consistency_kernel(const ConsistencyParams p)
{
    const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int u = tx * 16 + (wave & 1) * 8 + (lane & 7);
    const int v = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = u < p.W && v < p.H;
    const long long pix = (long long)v * p.W + u;
    const float d = inside ? p.target[pix] : 0.f;
    const bool valid = inside && depth_ok(d, p.z_near);

    const float fu = (float)u, fv = (float)v;
    const float x_max = (float)(p.W - 1), y_max = (float)(p.H - 1), x_cell = (float)(p.W - 2), y_cell = (float)(p.H - 2);
    float n_views = 0.f, n_visible = 0.f, sum_depth = d, sum_rel = 0.f;

#pragma unroll 1
    for (int s = 0; s < p.S; ++s) {
        if (!valid) continue;
        const float* F = p.F[s];
        const float c = project_row(F + 8, fu, fv, d);
        if (!(c > p.z_near)) continue;
        const float us = project_row(F, fu, fv, d) / c, vs = project_row(F + 4, fu, fv, d) / c;
        if (!(us >= 0.f && us <= x_max && vs >= 0.f && vs <= y_max)) continue;             // false for a NaN coordinate
        const float x0 = fminf(floorf(us), x_cell), y0 = fminf(floorf(vs), y_cell);         // in [0, W - 2] x [0, H - 2]
        const float* t = p.source[s] + ((long long)(int)y0 * p.W + (int)x0);
        const float t00 = t[0], t10 = t[1], t01 = t[p.W], t11 = t[p.W + 1];
        if (!(depth_ok(t00, p.z_near) && depth_ok(t10, p.z_near) && depth_ok(t01, p.z_near) && depth_ok(t11, p.z_near))) continue;
        const float fx = us - x0, fy = vs - y0;
        const float ds = lerpf(lerpf(t00, t10, fx), lerpf(t01, t11, fx), fy);
        const float* B = p.B[s];
        const float cb = project_row(B + 8, us, vs, ds);
        if (!(cb > p.z_near)) continue;
        const float ub = project_row(B, us, vs, ds) / cb, vb = project_row(B + 4, us, vs, ds) / cb;
        n_visible += 1.f;
        const float du = ub - fu, dv = vb - fv;
        const float e2 = fmaf(du, du, dv * dv);
        const float rel = fabsf(cb - d) / d;
        if (e2 < p.px_max2 && rel < p.rel_max) {
            n_views += 1.f;
            sum_depth += cb;
            sum_rel += rel;
        }
    }

    if (inside) {
        p.views[pix] = n_views;
        p.visible[pix] = n_visible;
        p.depth[pix] = valid ? sum_depth / (1.f + n_views) : 0.f;
        p.rel_err[pix] = n_views > 0.f ? sum_rel / n_views : 0.f;
    }
}

}  // namespace

extern "C" int estd_depth_consistency(const estd_depth_consistency_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    if (!d->target || !d->views || !d->visible || !d->depth || !d->rel_err) return ESTD_ERR_ARG;
    if (d->S < 1 || d->S > ESTD_CONSISTENCY_MAX_SOURCES || d->H < 2 || d->W < 2) return ESTD_ERR_ARG;
    if (!estd_finite(d->px_max) || !(d->px_max > 0.f) || !estd_finite(d->rel_max) || !(d->rel_max > 0.f)) return ESTD_ERR_ARG;
    if (!estd_finite(d->z_near) || !(d->z_near >= 0.f)) return ESTD_ERR_ARG;
    for (int i = 0; i < d->S; ++i) {
        if (!d->source[i]) return ESTD_ERR_ARG;
        for (int j = 0; j < 24; ++j)
            if (!estd_finite(d->mats[i][j / 12][j % 12])) return ESTD_ERR_ARG;
    }
    if ((long long)d->H * d->W > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;         // one workgroup per 16 x 16 pixels on blockIdx.x
    ConsistencyParams p{};
    p.H = d->H; p.W = d->W; p.S = d->S;
    p.tiles_x = estd_ceil_div(d->W, 16);
    p.z_near = d->z_near; p.rel_max = d->rel_max;
    p.px_max2 = d->px_max * d->px_max;                                               // formed once, here
    if (!(p.px_max2 > 0.f) || !estd_finite(p.px_max2)) return ESTD_ERR_ARG;             // a px_max whose square leaves fp32
    p.target = d->target; p.views = d->views; p.visible = d->visible; p.depth = d->depth; p.rel_err = d->rel_err;
    for (int i = 0; i < d->S; ++i) {
        p.source[i] = d->source[i];
        for (int j = 0; j < 12; ++j) { p.F[i][j] = d->mats[i][0][j]; p.B[i][j] = d->mats[i][1][j]; }
    }
    const unsigned n_blocks = (unsigned)p.tiles_x * (unsigned)estd_ceil_div(d->H, 16);
    hipLaunchKernelGGL(depth_consistency_kernel, dim3(n_blocks), dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
