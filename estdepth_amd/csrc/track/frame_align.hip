// frame_align.hip -- projective point-to-plane alignment of ONE live depth map against ONE set of model maps (depth + normals as
// csrc/tsdf_raycast.hip renders them): KinectFusion's tracking step.  One launch forms the Gauss-Newton system of the frame -- the 21 upper
// entries of sum J J^T, the 6 of sum J r, sum r^2 and the match count -- and writes the per-pixel residual and match maps.
//
// estd_frame_align, per live pixel (u, v) (the contract of include/estd_hip.h; L = [R_g K^-1 | c_g], Fm = K_m [R|t]_world->model,
// Bm = [R_m K_m^-1 | c_m], all formed on the host):
//     d = depth[v][u]; skipped unless finite, > z_near and (conf null or conf[v][u] >= conf_min);
//     p_j = fma(d, fma(L[j][0], u, fma(L[j][1], v, L[j][2])), L[j][3]);
//     (a, b, c)_j = fma(Fm[j][0], px, fma(Fm[j][1], py, fma(Fm[j][2], pz, Fm[j][3])));  skipped unless c > z_near;
//     um = floor(a / c + 0.5), vm = floor(b / c + 0.5);  skipped unless 0 <= um < Wm and 0 <= vm < Hm;
//     dm = m_depth[vm][um]; skipped unless dm > 0;  n = m_normal[vm][um];  q_j = the row expression of p with Bm, um, vm, dm;
//     e = q - p;  skipped unless fma(ex, ex, fma(ey, ey, ez ez)) <= dist_max^2;
//     r = fma(nx, ex, fma(ny, ey, nz ez));  J = (nx, ny, nz, fma(py, nz, -(pz ny)), fma(pz, nx, -(px nz)), fma(px, ny, -(py nx))).
// Every division is an IEEE division, every fused multiply-add is spelled out and there is no atomic: two calls give the same bits.
//
// Launch shape (csrc/tsdf_raycast.hip's): one lane per pixel, a wave on an 8 x 8 pixel tile, a workgroup of four waves on 16 x 16 pixels.
// A skipped pixel and a lane outside the image only mask lanes and add zeros.  Each of the 29 per-pixel terms is one fp32 value (a
// product rounded once), widened to float64 and added over the wave by an exclusive-or butterfly (lane distances 32, 16, 8, 4, 2, 1: every
// lane forms the same sums in the same order, so the result does not depend on which lane stores it), then over the four waves in wave
// order through LDS, and stored as one float64 partial per workgroup and term with ordinary vector stores.  frame_align_reduce_kernel
// adds the partials: workgroup k owns term k, lane l adds partials l, l + 64, l + 128, ... in ascending order, and the same butterfly
// joins the lanes.  The matrices, pointers and constants are kernel arguments; pixel offsets are 64-bit.
#include "estd_common.h"
#include "estd_device.h"

namespace {

constexpr int N_SUMS = ESTD_FRAME_ALIGN_SUMS;

struct AlignParams {
    int H, W, Hm, Wm, tiles_x;
    float z_near, conf_min, dist2;
    const float* depth;
    const float* conf;
    const float* m_depth;
    const float* m_normal;
    float* residual;
    int* match;
    double* partials;
    float L[12], F[12], B[12];
};

// row j of a 3x4 matrix applied to the point (x, y, z, 1):  fma(M0, x, fma(M1, y, fma(M2, z, M3)))
__device__ inline float point_row(const float* m, float x, float y, float z) { return fmaf(m[0], x, fmaf(m[1], y, fmaf(m[2], z, m[3]))); }

// the sum of x over the 64 lanes, the same bits in every lane
__device__ inline double wave_sum(double x)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) x += __shfl_xor(x, k, 64);
    return x;
}

__global__ __launch_bounds__(256) void frame_align_kernel(const AlignParams p)
{
    __shared__ double wave_part[4][N_SUMS];
    const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int u = tx * 16 + (wave & 1) * 8 + (lane & 7);
    const int v = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = u < p.W && v < p.H;
    const long long pix = inside ? (long long)v * p.W + u : 0;
    const float d = p.depth[pix];
    bool ok = inside && depth_ok(d, p.z_near);
    if (p.conf) ok = ok && p.conf[pix] >= p.conf_min;                                       // false for a NaN confidence

    float r = 0.f, j0 = 0.f, j1 = 0.f, j2 = 0.f, j3 = 0.f, j4 = 0.f, j5 = 0.f, one = 0.f;
    int hit = -1;
    if (ok) {
        const float fu = (float)u, fv = (float)v;
        const float px = project_row(p.L, fu, fv, d), py = project_row(p.L + 4, fu, fv, d), pz = project_row(p.L + 8, fu, fv, d);
        const float c = point_row(p.F + 8, px, py, pz);
        if (c > p.z_near) {
            const float um = floorf(point_row(p.F, px, py, pz) / c + 0.5f), vm = floorf(point_row(p.F + 4, px, py, pz) / c + 0.5f);
            if (um >= 0.f && vm >= 0.f && um < 2147483648.f && vm < 2147483648.f) {          // false for a NaN; the conversions are exact
                const int iu = (int)um, iv = (int)vm;
                if (iu < p.Wm && iv < p.Hm) {
                    const long long mp = (long long)iv * p.Wm + iu;
                    const float dm = p.m_depth[mp];
                    if (dm > 0.f) {
                        const float nx = p.m_normal[mp * 3], ny = p.m_normal[mp * 3 + 1], nz = p.m_normal[mp * 3 + 2];
                        const float ex = project_row(p.B, um, vm, dm) - px, ey = project_row(p.B + 4, um, vm, dm) - py,
                                    ez = project_row(p.B + 8, um, vm, dm) - pz;
                        if (fmaf(ex, ex, fmaf(ey, ey, ez * ez)) <= p.dist2) {                   // false for a NaN or an infinite model depth
                            r = fmaf(nx, ex, fmaf(ny, ey, nz * ez));
                            j0 = nx; j1 = ny; j2 = nz;
                            j3 = fmaf(py, nz, -(pz * ny));
                            j4 = fmaf(pz, nx, -(px * nz));
                            j5 = fmaf(px, ny, -(py * nx));
                            one = 1.f;
                            hit = (int)mp;
                        }
                    }
                }
            }
        }
    }
    if (inside) {
        p.residual[pix] = r;
        p.match[pix] = hit;
    }

    const float J[6] = {j0, j1, j2, j3, j4, j5};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double s = wave_sum((double)(J[i] * J[j]));
            if (lane == 0) wave_part[wave][k] = s;
            ++k;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double s = wave_sum((double)(J[i] * r));
        if (lane == 0) wave_part[wave][21 + i] = s;
    }
    const double s_rr = wave_sum((double)(r * r)), s_n = wave_sum((double)one);
    if (lane == 0) {
        wave_part[wave][27] = s_rr;
        wave_part[wave][28] = s_n;
    }
    __syncthreads();
    if (threadIdx.x < N_SUMS) {
        const int t = (int)threadIdx.x;
        p.partials[(long long)blockIdx.x * N_SUMS + t] = ((wave_part[0][t] + wave_part[1][t]) + wave_part[2][t]) + wave_part[3][t];
    }
}

// workgroup k (one wave) adds term k of the n_blocks partials
__global__ __launch_bounds__(64) void frame_align_reduce_kernel(const double* partials, int n_blocks, double* sums)
{
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
    double s = 0.0;
    for (int b = lane; b < n_blocks; b += 64) s += partials[(long long)b * N_SUMS + k];
    s = wave_sum(s);
    if (lane == 0) sums[k] = s;
}

inline long long n_tiles(int H, int W) { return (long long)estd_ceil_div(W, 16) * estd_ceil_div(H, 16); }

}  // namespace

extern "C" long long estd_frame_align_partials(int H, int W)
{
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return 0;
    return n_tiles(H, W) * N_SUMS * (long long)sizeof(double);
}

extern "C" int estd_frame_align(const estd_frame_align_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    if (!d->depth || !d->m_depth || !d->m_normal || !d->residual || !d->match || !d->partials || !d->sums) return ESTD_ERR_ARG;
    if (d->H <= 0 || d->W <= 0 || d->Hm <= 0 || d->Wm <= 0) return ESTD_ERR_ARG;
    if (!estd_finite(d->dist_max) || !(d->dist_max > 0.f)) return ESTD_ERR_ARG;
    const float dist2 = d->dist_max * d->dist_max;                                          // formed once, here
    if (!(dist2 > 0.f) || !estd_finite(dist2)) return ESTD_ERR_ARG;                            // a dist_max whose square leaves fp32
    if (!estd_finite(d->z_near) || !(d->z_near >= 0.f)) return ESTD_ERR_ARG;
    if (d->conf && !(d->conf_min == d->conf_min)) return ESTD_ERR_ARG;                       // a NaN threshold
    for (int j = 0; j < 12; ++j)
        if (!estd_finite(d->L[j]) || !estd_finite(d->Fm[j]) || !estd_finite(d->Bm[j])) return ESTD_ERR_ARG;
    if ((long long)d->H * d->W > 0x7fffffffLL || (long long)d->Hm * d->Wm > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    AlignParams p{};
    p.H = d->H; p.W = d->W; p.Hm = d->Hm; p.Wm = d->Wm;
    p.tiles_x = estd_ceil_div(d->W, 16);
    p.z_near = d->z_near; p.conf_min = d->conf_min; p.dist2 = dist2;
    p.depth = d->depth; p.conf = d->conf; p.m_depth = d->m_depth; p.m_normal = d->m_normal;
    p.residual = d->residual; p.match = d->match; p.partials = d->partials;
    for (int j = 0; j < 12; ++j) { p.L[j] = d->L[j]; p.F[j] = d->Fm[j]; p.B[j] = d->Bm[j]; }
    const long long n_blocks = n_tiles(d->H, d->W);                                         // < 2^23
    hipLaunchKernelGGL(frame_align_kernel, dim3((unsigned)n_blocks), dim3(256), 0, estd_stream(s), p);
    hipLaunchKernelGGL(frame_align_reduce_kernel, dim3(N_SUMS), dim3(64), 0, estd_stream(s), (const double*)d->partials, (int)n_blocks, d->sums);
    return ESTD_LAUNCH_CHECK();
}
