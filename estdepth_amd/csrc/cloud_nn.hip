// cloud_nn.hip -- nearest neighbours between two point clouds and voxel-grid down-sampling: what the 3D scores of a fused reconstruction
// (accuracy, completeness, precision / recall / F-score, chamfer distance: estdepth_amd/cloud_metrics.py) are made of.  The input is the
// cloud csrc/tsdf.hip's extraction produces; nothing here is part of the timed step.
//
// estd_cloud_nearest (the contract of include/estd_hip.h).  Per query q, over ALL targets p, in fp32:
//     dx = qx - px, dy, dz alike;  d2 = fma(dx, dx, fma(dy, dy, dz * dz));  d2min = the smallest d2;  index = the SMALLEST original target
//     index attaining it;  found iff d2min <= r2 = fl(max_dist * max_dist);  dist = sqrt(d2min) (IEEE) or max_dist;  index or -1.
// A minimum and then the smallest index: the result does not depend on the order candidates are met in, so the acceleration structure cannot
// change a bit of it as long as it never skips a candidate that could win or tie.
//
// Structure and search: the uniform grid and the ring walk of csrc/estd_device.h (grid_ring_walk; the argument why no ring is skipped too
// early stands there, once).  What is this file's own: a candidate is ONE target point, its box of cells the one cell
//     c_j = cell_coord(p_j),    key = (c_z dims_y + c_y) dims_x + c_x,
// which cloud_cell_keys_kernel computes for targets and queries alike (a query outside the box gets the clamped cell).  The host sorts the
// targets by key (stable), builds cell_start[key] = the number of targets with a smaller key, and keeps the sorted targets as 16-byte
// records (x, y, z, the bits of the original index): a candidate is ONE 16-byte load.  bound() returns best = the smallest d2 so far,
// starting at r2.  A candidate that ties best is still examined (the walk's comparison is strict), and the smaller index wins it.
//
// Launch shape: one lane per query, the queries taken in the order of THEIR cell key (`order`, sorted by the host): the 64 lanes of a wave
// sit in the same few cells, walk the same rows and load the same records -- broadcast or neighbouring 16-byte loads out of L1 / L2 instead
// of 64 unrelated gathers -- and leave their loops after similar trip counts.  Results are scattered back through `order` (two plain stores
// per query).  The alternative, a workgroup per block of query cells that stages the neighbouring target cells in LDS, needs a bound on the
// records per staged block that a dense table does not give (one cell may hold the whole cloud) and a second path for what does not fit;
// the records a wave shares here are served by the 32 KiB L1 without one.  No LDS, no atomics, no scratch.
//
// estd_cloud_cell_centroids: the voxel-grid down-sampling evaluation protocols apply first.  The host sorts the points by cell key (stable:
// inside a cell the original order is kept) and passes the segment bounds; one lane per (cell, column) adds its column of the cell's points
// in float64 in that order, divides by the count in float64 and rounds to fp32 once.  Cells come out in ascending key order.
#include "estd_common.h"
#include "estd_device.h"

namespace {

struct CloudKeysParams {
    const float* points;
    long long* keys;
    long long n;
    float lo[3];
    float inv_cell;
    int dims[3];
};

__global__ __launch_bounds__(256) void cloud_cell_keys_kernel(const CloudKeysParams p)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const float* q = p.points + 3 * i;
    const long long cx = cell_coord(q[0], p.lo[0], p.inv_cell, p.dims[0]);
    const long long cy = cell_coord(q[1], p.lo[1], p.inv_cell, p.dims[1]);
    const long long cz = cell_coord(q[2], p.lo[2], p.inv_cell, p.dims[2]);
    p.keys[i] = (cz * p.dims[1] + cy) * p.dims[0] + cx;
}

struct CloudNearestParams {
    const float* query;
    const long long* order;
    const float4* records;
    const int* cell_start;
    float* dist;
    long long* index;
    unsigned int* stats;
    int M, N;
    estd_grid grid;
    float max_dist, r2;
};

// STATS (the bench tool's counter): per query the candidates whose distance was evaluated
template <bool STATS>
__global__ __launch_bounds__(256) void cloud_nearest_kernel(const CloudNearestParams p)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= p.M) return;
    const long long qi = p.order ? p.order[i] : (long long)i;
    if ((unsigned long long)qi >= (unsigned long long)p.M) return;           // a malformed permutation writes nothing out of bounds
    const float qx = p.query[3 * qi], qy = p.query[3 * qi + 1], qz = p.query[3 * qi + 2];
    float best = p.r2;
    int best_index = 0x7fffffff;                                             // so that d2 == r2 is found
    unsigned int examined = 0;

    if (p.N > 0) {
        // the records of cells k0 .. k1 of one row
        auto scan = [&](int k0, int k1) {
            const int beg = max(p.cell_start[k0], 0), end = min(p.cell_start[k1 + 1], p.N);
            for (int j = beg; j < end; ++j) {
                const float4 t = p.records[j];
                const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
                const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
                const int idx = __float_as_int(t.w);
                if (d2 < best || (d2 == best && idx < best_index)) {
                    best = d2;
                    best_index = idx;
                }
                if (STATS) ++examined;
            }
        };

        grid_ring_walk(p.grid, qx, qy, qz, [&]() { return best; }, scan);
    }

    const bool found = best_index != 0x7fffffff;
    p.dist[qi] = found ? sqrtf(best) : p.max_dist;
    p.index[qi] = found ? (long long)best_index : -1ll;
    if (STATS) p.stats[qi] = examined;
}

struct CloudCentroidParams {
    const float* points;
    const float* attrs;
    const long long* order;
    const long long* segments;
    float* out_points;
    float* out_attrs;
    long long N, K;
    int C;
};

__global__ __launch_bounds__(256) void cloud_cell_centroids_kernel(const CloudCentroidParams p)
{
    const int cols = 3 + p.C;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.K * cols) return;
    const long long k = i / cols;
    const int col = (int)(i - k * cols);
    const long long beg = max(p.segments[k], 0ll), end = min(p.segments[k + 1], p.N);
    const float* src = col < 3 ? p.points + col : p.attrs + (col - 3);
    const int stride = col < 3 ? 3 : p.C;
    double sum = 0.0;
    long long count = 0;
    for (long long j = beg; j < end; ++j) {
        const long long idx = p.order[j];
        if ((unsigned long long)idx >= (unsigned long long)p.N) continue;
        sum += (double)src[idx * stride];
        ++count;
    }
    const float mean = count > 0 ? (float)(sum / (double)count) : 0.f;
    if (col < 3) p.out_points[3 * k + col] = mean;
    else p.out_attrs[k * p.C + (col - 3)] = mean;
}

}  // namespace

extern "C" int estd_cloud_cell_keys(const float* points, long long n, const float* lo3, float cell, const int* dims3, long long* keys,
                                    estd_stream_t s)
{
    if (n < 0 || !estd_grid_ok(lo3, cell, dims3, ESTD_CLOUD_KEY_MAX_DIM, 0)) return ESTD_ERR_ARG;
    if (n == 0) return ESTD_OK;
    if (!points || !keys) return ESTD_ERR_ARG;
    if (n > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    CloudKeysParams p{};
    p.points = points; p.keys = keys; p.n = n;
    p.inv_cell = estd_inv_cell(cell);
    for (int j = 0; j < 3; ++j) { p.lo[j] = lo3[j]; p.dims[j] = dims3[j]; }
    hipLaunchKernelGGL(cloud_cell_keys_kernel, dim3((unsigned)estd_ceil_div(n, 256)), dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_cloud_nearest(const estd_cloud_nearest_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    if (d->M < 0 || d->N < 0) return ESTD_ERR_ARG;
    CloudNearestParams p{};
    if (estd_search_args(d->max_dist, d->N, d->lo, d->cell, d->dims, d->records, d->cell_start, &p.grid, &p.r2) != ESTD_OK) return ESTD_ERR_ARG;
    if (d->M > 0x7fffffffLL || d->N > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (d->M == 0) return ESTD_OK;
    if (!d->query || !d->dist || !d->index) return ESTD_ERR_ARG;
    p.query = d->query; p.order = d->order; p.records = reinterpret_cast<const float4*>(d->records); p.cell_start = d->cell_start;
    p.dist = d->dist; p.index = d->index; p.stats = d->stats;
    p.M = (int)d->M; p.N = (int)d->N;
    p.max_dist = d->max_dist;
    const dim3 grid((unsigned)estd_ceil_div(d->M, 256));
    if (d->stats) hipLaunchKernelGGL(cloud_nearest_kernel<true>, grid, dim3(256), 0, estd_stream(s), p);
    else hipLaunchKernelGGL(cloud_nearest_kernel<false>, grid, dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_cloud_cell_centroids(const float* points, const float* attrs, int C, long long n, const long long* order,
                                         const long long* segments, long long K, float* out_points, float* out_attrs, estd_stream_t s)
{
    if (n < 0 || K < 0 || K > n || C < 0 || C > ESTD_CLOUD_MAX_ATTRS) return ESTD_ERR_ARG;
    if (K == 0) return ESTD_OK;
    if (!points || !order || !segments || !out_points) return ESTD_ERR_ARG;
    if (C > 0 && (!attrs || !out_attrs)) return ESTD_ERR_ARG;
    if (n > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    CloudCentroidParams p{};
    p.points = points; p.attrs = attrs; p.order = order; p.segments = segments; p.out_points = out_points; p.out_attrs = out_attrs;
    p.N = n; p.K = K; p.C = C;
    hipLaunchKernelGGL(cloud_cell_centroids_kernel, dim3((unsigned)estd_ceil_div(K * (3 + C), 256)), dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
