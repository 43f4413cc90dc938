// cloud_cluster.hip -- density-based clustering of a point cloud (DBSCAN) and the fixed-radius neighbour count behind it: what tells the
// floaters of a fused cloud -- a blob of forty stray points is not part of the scene -- from its surface before the cloud is scored,
// registered or written (estdepth_amd/cloud_metrics.py: PointGrid.count_within, cluster_dbscan, filter_clusters).  Nothing here is part
// of the timed step.
//
// The contract (include/estd_hip.h, estd_cloud_dbscan; its numpy form: tests/cloud_cluster_ref.py), every output defined to the integer:
//     d2(i, j) as estd_cloud_nearest forms it (exactly symmetric: negating dx, dy, dz changes no bit); j is a NEIGHBOUR of i iff
//     d2(i, j) <= r2 = fl(eps * eps), i itself included; count[i] = the neighbours of i; i is CORE iff count[i] >= min_points;
//     clusters = the connected components of the graph on the core points with an edge between two core points that are neighbours;
//     label[core i] = the smallest original index among the core points of its component; label[non-core i] = the label of its nearest
//     core neighbour by the key (d2, original index), -1 (noise) without one; size[r] = the points labelled r; noise = the points labelled -1.
// Counts, a set of edges, a minimum over keys: nothing depends on the order candidates are met in, so the grid, the cell edge and the
// scheduling change no bit.
//
// Structure: PointGrid's records and cell table as csrc/cloud_nn.hip defines them, and the ring walk of csrc/estd_device.h (grid_ring_walk,
// with the argument why no ring is skipped).  One lane per point IN CELL-KEY ORDER: for the cloud against itself lane i takes record i --
// position and original index in one 16-byte load, no `order` array -- so the lanes of a wave sit in the same few cells and walk the
// same rows.  An index read from a record is never an address before in_range() has passed it; a record that fails is skipped.
// The union-find is csrc/estd_device.h's (parent_load, find_root, find_root_halving, unite), the one of csrc/mesh/mesh_components.hip.
//
// Four launches, 256 lanes per workgroup:
//   dbscan_count_kernel    walks with the CONSTANT bound r2 and counts the candidates with d2 <= r2.  For clustering (parent given) it
//                          also stores parent[i] = i and size[i] = 0, and lane 0 of the grid stores noise = 0.  With `query` given it
//                          counts for queries that are not the targets, taken through `order` (estd_cloud_count_within).
//   dbscan_hook_kernel     a core point walks again and unites with every core neighbour of SMALLER original index: each edge once.
//   dbscan_flatten_kernel  one lane per original index: label[i] = core ? find_root(parent, i) : -1; label is not parent, nothing is
//                          read that this launch writes.
//   dbscan_border_kernel   a non-core point walks with the SHRINKING bound best (from r2) over core candidates only and stores
//                          label[best]; core labels are the previous launch's, this one stores non-core labels only.  Then every point
//                          counts: one integer atomicAdd per wave and distinct label (the ballot loop of mesh_cc_count_kernel), one per
//                          wave for the noise.
// A candidate is known to be core by count[index], gathered only for candidates already inside the radius (4 bytes next to a 16-byte
// record that was loaded anyway).  No float atomics, no LDS, no scratch.
#include "estd_common.h"
#include "estd_device.h"

namespace {

constexpr int DB_WG = 256;

struct DbscanParams {
    const float* query;                         // NULL: the cloud against itself, lane i takes record i
    const long long* order;
    const float4* records;
    const int* cell_start;
    int* count;
    int* parent;                                // NULL: counting only
    int* label;
    int* size;
    int* noise;
    int M, N, min_points;
    estd_grid grid;
    float r2;
};

// the candidates of cells k0 .. k1 of one row with d2 <= r2: fn(original index, d2) for each
template <typename Fn>
__device__ __forceinline__ void dbscan_scan(const DbscanParams& p, float qx, float qy, float qz, float reach2, int k0, int k1, Fn&& fn)
{
    const int beg = max(p.cell_start[k0], 0), end = min(p.cell_start[k1 + 1], p.N);
    for (int j = beg; j < end; ++j) {
        const float4 t = p.records[j];
        const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
        const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
        if (d2 <= reach2) fn(__float_as_int(t.w), d2);
    }
}

__global__ __launch_bounds__(DB_WG) void dbscan_count_kernel(const DbscanParams p)
{
    const int i = (int)blockIdx.x * DB_WG + (int)threadIdx.x;
    if (i >= p.M) return;
    if (p.parent) {                                                          // by lane, not by record: complete whatever the records name
        p.parent[i] = i;
        p.size[i] = 0;
        if (i == 0) *p.noise = 0;
    }
    float qx, qy, qz;
    int qi;
    if (p.query) {
        const long long o = p.order ? p.order[i] : (long long)i;
        if ((unsigned long long)o >= (unsigned long long)p.M) return;        // a malformed permutation writes nothing out of bounds
        qi = (int)o;
        qx = p.query[3 * o]; qy = p.query[3 * o + 1]; qz = p.query[3 * o + 2];
    } else {
        const float4 own = p.records[i];
        qi = __float_as_int(own.w);
        if (!in_range(qi, p.N)) return;                                       // never an address
        qx = own.x; qy = own.y; qz = own.z;
    }
    int n = 0;
    if (p.N > 0) {
        const float r2 = p.r2;
        grid_ring_walk(p.grid, qx, qy, qz, [&]() { return r2; },
                       [&](int k0, int k1) { dbscan_scan(p, qx, qy, qz, r2, k0, k1, [&](int, float) { ++n; }); });
    }
    p.count[qi] = n;
}

__global__ __launch_bounds__(DB_WG) void dbscan_hook_kernel(const DbscanParams p)
{
    const int i = (int)blockIdx.x * DB_WG + (int)threadIdx.x;
    if (i >= p.N) return;
    const float4 own = p.records[i];
    const int qi = __float_as_int(own.w);
    if (!in_range(qi, p.N)) return;                                           // never an address
    if (p.count[qi] < p.min_points) return;
    const float r2 = p.r2;
    grid_ring_walk(p.grid, own.x, own.y, own.z, [&]() { return r2; }, [&](int k0, int k1) {
        dbscan_scan(p, own.x, own.y, own.z, r2, k0, k1, [&](int idx, float) {
            if (idx < qi && in_range(idx, p.N) && p.count[idx] >= p.min_points) unite(p.parent, qi, idx);
        });
    });
}

__global__ __launch_bounds__(DB_WG) void dbscan_flatten_kernel(const int* parent, const int* count, int* label, int N, int min_points)
{
    const int i = (int)blockIdx.x * DB_WG + (int)threadIdx.x;
    if (i >= N) return;
    label[i] = count[i] >= min_points ? find_root(parent, i) : -1;
}

__global__ __launch_bounds__(DB_WG) void dbscan_border_kernel(const DbscanParams p)
{
    const int lane = (int)threadIdx.x & 63;
    const int i = (int)blockIdx.x * DB_WG + (int)threadIdx.x;
    bool valid = false;
    int lab = -1;
    if (i < p.N) {
        const float4 own = p.records[i];
        const int qi = __float_as_int(own.w);
        valid = in_range(qi, p.N);                                            // never an address
        if (valid) {
            if (p.count[qi] >= p.min_points) {
                lab = p.label[qi];
            } else {
                float best = p.r2;
                int best_index = 0x7fffffff;                                  // so that d2 == r2 is found
                grid_ring_walk(p.grid, own.x, own.y, own.z, [&]() { return best; }, [&](int k0, int k1) {
                    dbscan_scan(p, own.x, own.y, own.z, best, k0, k1, [&](int idx, float d2) {
                        if ((d2 < best || (d2 == best && idx < best_index)) && in_range(idx, p.N) && p.count[idx] >= p.min_points) {
                            best = d2;
                            best_index = idx;
                        }
                    });
                });
                if (best_index != 0x7fffffff) lab = p.label[best_index];
                p.label[qi] = lab;
            }
        }
    }
    const bool member = valid && in_range(lab, p.N);
    const unsigned long long b_noise = __ballot(valid && !member);
    if (b_noise != 0ull && lane == 0) atomicAdd(p.noise, __popcll(b_noise));
    // one add per distinct label of the wave: the lowest lane still waiting names its label, every lane with that label is served by
    // the one add.  `todo` is wave-uniform and loses at least that lane per round: at most 64 rounds, one for a wave inside one cluster.
    unsigned long long todo = __ballot(member);
    while (todo != 0ull) {
        const int leader = __ffsll(todo) - 1;
        const int r0 = __shfl(lab, leader);
        const unsigned long long same = __ballot(member && lab == r0);
        if (lane == leader) atomicAdd(p.size + r0, __popcll(same));
        todo &= ~same;
    }
}

}  // namespace

extern "C" int estd_cloud_count_within(const estd_cloud_count_within_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    if (d->M < 0 || d->N < 0) return ESTD_ERR_ARG;
    DbscanParams p{};
    if (estd_search_args(d->radius, d->N, d->lo, d->cell, d->dims, d->records, d->cell_start, &p.grid, &p.r2) != ESTD_OK) return ESTD_ERR_ARG;
    if (d->M > 0x7fffffffLL || d->N > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (d->M == 0) return ESTD_OK;
    if (!d->query || !d->count) return ESTD_ERR_ARG;
    p.query = d->query; p.order = d->order; p.records = reinterpret_cast<const float4*>(d->records); p.cell_start = d->cell_start;
    p.count = d->count;
    p.M = (int)d->M; p.N = (int)d->N;
    hipLaunchKernelGGL(dbscan_count_kernel, dim3((unsigned)estd_ceil_div(d->M, DB_WG)), dim3(DB_WG), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_cloud_dbscan(const estd_cloud_dbscan_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    if (d->N < 0 || d->min_points < 1) return ESTD_ERR_ARG;
    DbscanParams p{};
    if (estd_search_args(d->eps, d->N, d->lo, d->cell, d->dims, d->records, d->cell_start, &p.grid, &p.r2) != ESTD_OK) return ESTD_ERR_ARG;
    if (d->N > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (d->N == 0) return ESTD_OK;
    if (!d->count || !d->parent || !d->label || !d->size || !d->noise) return ESTD_ERR_ARG;
    p.records = reinterpret_cast<const float4*>(d->records); p.cell_start = d->cell_start;
    p.count = d->count; p.parent = d->parent; p.label = d->label; p.size = d->size; p.noise = d->noise;
    p.M = p.N = (int)d->N; p.min_points = d->min_points;
    const dim3 grid((unsigned)estd_ceil_div(d->N, DB_WG)), wg(DB_WG);
    hipLaunchKernelGGL(dbscan_count_kernel, grid, wg, 0, estd_stream(s), p);
    hipLaunchKernelGGL(dbscan_hook_kernel, grid, wg, 0, estd_stream(s), p);
    hipLaunchKernelGGL(dbscan_flatten_kernel, grid, wg, 0, estd_stream(s), (const int*)p.parent, (const int*)p.count, p.label, p.N, p.min_points);
    hipLaunchKernelGGL(dbscan_border_kernel, grid, wg, 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
