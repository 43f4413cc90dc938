// rigid_align.hip -- rigid registration of a point cloud to a cloud or a triangle mesh: moving the cloud and forming the Gauss-Newton
// system of one ICP iteration from correspondences the existing searches found (estd_cloud_nearest: the nearest target point;
// estd_mesh_nearest: the closest surface point and its face).  csrc/track/frame_align.hip does the same for one depth map against
// rendered maps; the sums, their layout and their order of addition are that file's.
//
// estd_rigid_apply (rigid_apply_kernel, one lane per point): moved = T p, moved_normal = R n, T a host 3 x 4 matrix in the launch
// arguments; each coordinate fma(T_j0, x, fma(T_j1, y, fma(T_j2, z, T_j3))), the normal's the same expression without T_j3.
//
// estd_rigid_system (rigid_system_kernel + rigid_reduce_kernel; the contract of include/estd_hip.h), per point i:
//     k = index[i]; skipped unless 0 <= k < Nn (and k < Nt with by_index): an index outside is never turned into an address;
//     m = moved[i]; q = target[by_index ? k : i]; e = q - m; e2 = fma(ex, ex, fma(ey, ey, ez ez)); skipped unless e2 <= dist_max^2;
//     with moved_normal and a finite cos_min: c = fma(nx, sx, fma(ny, sy, nz sz)), n = normal[k], s = moved_normal[i]; skipped unless
//     (two_sided ? fabsf(c) : c) >= cos_min;
//     plane: r = fma(nx, ex, fma(ny, ey, nz ez)), J = (n, q x n), the 29 terms J_i J_j, J_i r, r r, 1 -- frame_align's;
//     point: the 29 terms of J^T J, J^T e, |e|^2, 1 with J = [I | -[q]x]: constants, +-q_k, fma(qy, qy, qz qz), -(qx qy), e_k,
//            fma(qy, ez, -(qz ey)), e2.
// One lane per point, 256 points per workgroup.  Each term is one fp32 value, widened to float64 and added over the wave by an
// exclusive-or butterfly (lane distances 32 .. 1: the same bits in every lane), over the four waves in wave order through LDS, stored as
// one partial per workgroup and term; rigid_reduce_kernel: workgroup k owns term k, lane l adds partials l, l + 64, ... in ascending
// order and the butterfly joins the lanes.  No atomics: two calls give the same bits.  Point offsets are 64-bit.
#include "estd_common.h"
#include "estd_device.h"

namespace {

constexpr int N_SUMS = ESTD_RIGID_SYSTEM_SUMS;

struct ApplyParams {
    long long n;
    const float* src;
    const float* src_normal;
    float* moved;
    float* moved_normal;
    float T[12];
};

struct SystemParams {
    long long n, n_target, n_normal;
    int metric, by_index, two_sided, use_cos;
    float dist2, cos_min;
    const float* moved;
    const float* moved_normal;
    const long long* index;
    const float* target;
    const float* normal;
    float* residual;
    long long* match;
    double* partials;
};

// the sum of x over the 64 lanes, the same bits in every lane
__device__ inline double wave_sum(double x)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) x += __shfl_xor(x, k, 64);
    return x;
}

__global__ __launch_bounds__(256) void rigid_apply_kernel(const ApplyParams p)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const float x = p.src[i * 3], y = p.src[i * 3 + 1], z = p.src[i * 3 + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) p.moved[i * 3 + j] = fmaf(p.T[4 * j], x, fmaf(p.T[4 * j + 1], y, fmaf(p.T[4 * j + 2], z, p.T[4 * j + 3])));
    if (p.src_normal) {
        const float a = p.src_normal[i * 3], b = p.src_normal[i * 3 + 1], c = p.src_normal[i * 3 + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) p.moved_normal[i * 3 + j] = fmaf(p.T[4 * j], a, fmaf(p.T[4 * j + 1], b, p.T[4 * j + 2] * c));
    }
}

__global__ __launch_bounds__(256) void rigid_system_kernel(const SystemParams p)
{
    __shared__ double wave_part[4][N_SUMS];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool inside = i < p.n;

    float t[N_SUMS];
#pragma unroll
    for (int k = 0; k < N_SUMS; ++k) t[k] = 0.f;
    float res = 0.f;
    long long hit = -1;
    const long long k = inside ? p.index[i] : -1;
    if (k >= 0 && k < p.n_normal && (!p.by_index || k < p.n_target)) {
        const long long qi = (p.by_index ? k : i) * 3;
        const float mx = p.moved[i * 3], my = p.moved[i * 3 + 1], mz = p.moved[i * 3 + 2];
        const float qx = p.target[qi], qy = p.target[qi + 1], qz = p.target[qi + 2];
        const float ex = qx - mx, ey = qy - my, ez = qz - mz;
        const float e2 = fmaf(ex, ex, fmaf(ey, ey, ez * ez));
        bool ok = e2 <= p.dist2;                                                             // false for a NaN
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (ok && (p.use_cos || p.metric == ESTD_RIGID_PLANE)) {
            nx = p.normal[k * 3]; ny = p.normal[k * 3 + 1]; nz = p.normal[k * 3 + 2];
        }
        if (ok && p.use_cos) {
            const float c = fmaf(nx, p.moved_normal[i * 3], fmaf(ny, p.moved_normal[i * 3 + 1], nz * p.moved_normal[i * 3 + 2]));
            ok = (p.two_sided ? fabsf(c) : c) >= p.cos_min;                                  // false for a NaN
        }
        if (ok) {
            hit = k;
            if (p.metric == ESTD_RIGID_PLANE) {
                const float r = fmaf(nx, ex, fmaf(ny, ey, nz * ez));
                const float J[6] = {nx, ny, nz, fmaf(qy, nz, -(qz * ny)), fmaf(qz, nx, -(qx * nz)), fmaf(qx, ny, -(qy * nx))};
                int s = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b) t[s++] = J[a] * J[b];
#pragma unroll
                for (int a = 0; a < 6; ++a) t[21 + a] = J[a] * r;
                t[27] = r * r;
                res = r;
            } else {
                t[0] = 1.f; t[4] = qz; t[5] = -qy;                                            // (0,0) (0,4) (0,5)
                t[6] = 1.f; t[8] = -qz; t[10] = qx;                                           // (1,1) (1,3) (1,5)
                t[11] = 1.f; t[12] = qy; t[13] = -qx;                                         // (2,2) (2,3) (2,4)
                t[15] = fmaf(qy, qy, qz * qz); t[16] = -(qx * qy); t[17] = -(qx * qz);        // (3,3) (3,4) (3,5)
                t[18] = fmaf(qx, qx, qz * qz); t[19] = -(qy * qz);                            // (4,4) (4,5)
                t[20] = fmaf(qx, qx, qy * qy);                                                // (5,5)
                t[21] = ex; t[22] = ey; t[23] = ez;
                t[24] = fmaf(qy, ez, -(qz * ey));
                t[25] = fmaf(qz, ex, -(qx * ez));
                t[26] = fmaf(qx, ey, -(qy * ex));
                t[27] = e2;
                res = sqrtf(e2);
            }
            t[28] = 1.f;
        }
    }
    if (inside) {
        p.residual[i] = res;
        p.match[i] = hit;
    }

#pragma unroll
    for (int s = 0; s < N_SUMS; ++s) {
        const double v = wave_sum((double)t[s]);
        if (lane == 0) wave_part[wave][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < N_SUMS) {
        const int s = (int)threadIdx.x;
        p.partials[(long long)blockIdx.x * N_SUMS + s] = ((wave_part[0][s] + wave_part[1][s]) + wave_part[2][s]) + wave_part[3][s];
    }
}

// workgroup k (one wave) adds term k of the n_blocks partials
__global__ __launch_bounds__(64) void rigid_reduce_kernel(const double* partials, int n_blocks, double* sums)
{
    const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
    double s = 0.0;
    for (int b = lane; b < n_blocks; b += 64) s += partials[(long long)b * N_SUMS + k];
    s = wave_sum(s);
    if (lane == 0) sums[k] = s;
}

constexpr long long LIMIT = 0x7fffffffLL;                                                    // sizes stay below 2^31

}  // namespace

extern "C" int estd_rigid_apply(const float* src, const float* src_normal, long long n, const float* T12, float* moved, float* moved_normal,
                                estd_stream_t s)
{
    if (n < 0 || !T12) return ESTD_ERR_ARG;
    for (int j = 0; j < 12; ++j)
        if (!estd_finite(T12[j])) return ESTD_ERR_ARG;
    if (n > 0 && (!src || !moved)) return ESTD_ERR_ARG;
    if (n > 0 && ((src_normal != nullptr) != (moved_normal != nullptr))) return ESTD_ERR_ARG;
    if (n > LIMIT) return ESTD_ERR_UNSUPPORTED;
    if (n == 0) return ESTD_OK;
    ApplyParams p{};
    p.n = n; p.src = src; p.src_normal = src_normal; p.moved = moved; p.moved_normal = moved_normal;
    for (int j = 0; j < 12; ++j) p.T[j] = T12[j];
    hipLaunchKernelGGL(rigid_apply_kernel, dim3((unsigned)estd_ceil_div(n, 256LL)), dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" long long estd_rigid_system_partials(long long n)
{
    if (n <= 0 || n > LIMIT) return 0;
    return ((n + 255) / 256) * N_SUMS * (long long)sizeof(double);
}

extern "C" int estd_rigid_system(const estd_rigid_system_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    if (d->N < 0 || d->Nt < 0 || d->Nn < 0) return ESTD_ERR_ARG;
    if (d->metric != ESTD_RIGID_PLANE && d->metric != ESTD_RIGID_POINT) return ESTD_ERR_ARG;
    if (!estd_finite(d->dist_max) || !(d->dist_max > 0.f)) return ESTD_ERR_ARG;
    const float dist2 = d->dist_max * d->dist_max;                                          // formed once, here
    if (!(dist2 > 0.f) || !estd_finite(dist2)) return ESTD_ERR_ARG;
    if (d->moved_normal && !(d->cos_min == d->cos_min)) return ESTD_ERR_ARG;                 // a NaN threshold
    const bool use_cos = d->moved_normal && estd_finite(d->cos_min);
    if (!d->sums) return ESTD_ERR_ARG;
    if (d->N > 0 && (!d->moved || !d->index || !d->residual || !d->match || !d->partials)) return ESTD_ERR_ARG;
    if (d->N > 0 && d->Nt > 0 && !d->target) return ESTD_ERR_ARG;
    if (d->N > 0 && d->Nn > 0 && !d->normal && (use_cos || d->metric == ESTD_RIGID_PLANE)) return ESTD_ERR_ARG;
    if (!d->by_index && d->Nt < d->N) return ESTD_ERR_ARG;                                   // target is then read at i
    if (d->N > LIMIT || d->Nt > LIMIT || d->Nn > LIMIT) return ESTD_ERR_UNSUPPORTED;
    const long long n_blocks = (d->N + 255) / 256;                                           // < 2^23
    if (d->N > 0) {
        SystemParams p{};
        p.n = d->N; p.n_target = d->Nt; p.n_normal = d->Nn;
        p.metric = d->metric; p.by_index = d->by_index != 0; p.two_sided = d->two_sided != 0; p.use_cos = use_cos;
        p.dist2 = dist2; p.cos_min = d->cos_min;
        p.moved = d->moved; p.moved_normal = d->moved_normal; p.index = d->index; p.target = d->target; p.normal = d->normal;
        p.residual = d->residual; p.match = d->match; p.partials = d->partials;
        hipLaunchKernelGGL(rigid_system_kernel, dim3((unsigned)n_blocks), dim3(256), 0, estd_stream(s), p);
    }
    hipLaunchKernelGGL(rigid_reduce_kernel, dim3(N_SUMS), dim3(64), 0, estd_stream(s), (const double*)d->partials, (int)n_blocks, d->sums);
    return ESTD_LAUNCH_CHECK();
}
