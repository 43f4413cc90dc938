// mesh_distance.hip -- the distance from a point to a triangle mesh: per query the nearest point of the nearest triangle, so that the 3D
// scores (estdepth_amd/cloud_metrics.py, compare_meshes(exact=True)) measure the distance to a SURFACE and not to its nearest sample.
// The contract: include/estd_hip.h (estd_mesh_tri_bins, estd_mesh_tri_fill, estd_mesh_nearest); its numpy form: tests/mesh_distance_ref.py.
//
// One device function, tri_closest, evaluates a (query, triangle) pair: the region tests of Ericson, Real-Time Collision Detection
// 5.1.5, in fp32 with every product and sum an explicit fmaf nesting or a plain operation (contraction is off in this file's device
// code).  The result of a query is the smallest d2 over ALL valid triangles and among equal d2 the smallest face index: a minimum does
// not depend on the order candidates are met in, nor on how often one is met, so the search structure cannot change a bit of it as
// long as it never skips a candidate that could win or tie.
//
// Structure: the uniform grid and the ring walk of csrc/estd_device.h (grid_ring_walk, with the argument why no ring is skipped too
// early).  A candidate is a TRIANGLE, registered in every cell the bounding box of its three vertices covers (cell_coord of the box's
// two corners, the function estd_cloud_cell_keys uses); a triangle whose box covers more than `big_cells` cells goes on the BIG LIST
// instead, which every query tests in full.
//   mesh_tri_bins_kernel   one lane per triangle: validity (indices, finite vertices, the fp32 normal), the box of cells, the number of
//                          (cell, face) pairs it will write and its flag (0 invalid, 1 grid, 2 big list); the invalid ones are counted
//                          with ONE integer atomic add per wave
//   mesh_tri_fill_kernel   one lane per triangle: recomputes the box and writes its own pairs at its own offset (the host's exclusive
//                          prefix sum of the counts): no atomics, the same bits for every launch; a pair outside [0, n_pairs) is dropped
// The host sorts the pairs by key (stable), builds cell_start by searchsorted and gathers 48-byte records in cell order: the nine
// coordinates, the bits of the face index, two words of padding -- a candidate is three 16-byte loads and a cell's candidates are one
// contiguous range.
//   mesh_nearest_kernel    one lane per query, the queries in the order of their own cell key.  Phase A tests every record of the big
//                          list: the record's address is the same for every lane, so the loads are scalar loads into SGPRs (one per
//                          wave, not 64 identical vector loads).  Phase B is the ring walk over the cell table.
//
// The bound of phase B: bound() returns best = the smallest d2 so far over BOTH phases, starting at r2 = max_dist^2.  A triangle that ties
// best is still examined (the walk's comparison is strict), and the smaller face index wins it; a triangle met in several cells is
// examined several times, which a minimum does not notice.  The walk's argument needs the valid triangles' vertices inside the grid's
// box, which the host layer guarantees (the box is theirs).
//
// No LDS, no scratch, no spinning, nothing between workgroups; the only atomic is the invalid count.
#include "../estd_common.h"
#include "../estd_device.h"

namespace {

constexpr int WG = 256;
constexpr int NO_FACE = 0x7fffffff;

__device__ __forceinline__ float dot3(float x0, float x1, float x2, float y0, float y1, float y2)
{
    return fmaf(x0, y0, fmaf(x1, y1, x2 * y2));
}

// THE per-pair function (include/estd_hip.h, "The pair"): the barycentric pair (v, w) of the point of triangle (a, b, c) closest to q,
// the point p and d2 = |q - p|^2, operation by operation as the header states them.
__device__ __forceinline__ float tri_closest(float qx, float qy, float qz, float ax, float ay, float az, float bx, float by, float bz,
                                             float cx, float cy, float cz, float& v, float& w, float& px, float& py, float& pz)
{
#pragma clang fp contract(off)
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float apx = qx - ax, apy = qy - ay, apz = qz - az;
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    const float bpx = qx - bx, bpy = qy - by, bpz = qz - bz;
    const float d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    const float cpx = qx - cx, cpy = qy - cy, cpz = qz - cz;
    const float d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    const float vc = fmaf(d1, d4, -(d3 * d2)), vb = fmaf(d5, d2, -(d1 * d6)), va = fmaf(d3, d6, -(d5 * d4));
    const float e43 = d4 - d3, e56 = d5 - d6;
    // every region needs at most ONE division: its operands are selected first, so that the lanes of a wave divide once, together
    float num = 0.f, den = 1.f;
    int region;
    if (d1 <= 0.f && d2 <= 0.f) {                                   // vertex A
        region = 0;
    } else if (d3 >= 0.f && d4 <= d3) {                             // vertex B
        region = 1;
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {               // edge AB: v = d1 / (d1 - d3)
        region = 2; num = d1; den = d1 - d3;
    } else if (d6 >= 0.f && d5 <= d6) {                             // vertex C
        region = 3;
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {               // edge AC: w = d2 / (d2 - d6)
        region = 4; num = d2; den = d2 - d6;
    } else if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) {             // edge BC: w = e43 / (e43 + e56)
        region = 5; num = e43; den = e43 + e56;
    } else {                                                        // the interior: denom = 1 / ((va + vb) + vc)
        region = 6; num = 1.f; den = (va + vb) + vc;
    }
    const float r = num / den;
    v = region == 1 ? 1.f : region == 2 ? r : region == 5 ? 1.f - r : region == 6 ? vb * r : 0.f;
    w = region == 3 ? 1.f : (region == 4 || region == 5) ? r : region == 6 ? vc * r : 0.f;
    px = fmaf(w, acx, fmaf(v, abx, ax));
    py = fmaf(w, acy, fmaf(v, aby, ay));
    pz = fmaf(w, acz, fmaf(v, abz, az));
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}

struct TriGrid {
    float lo[3];
    float inv_cell;
    int dims[3];
    int big_cells;
};

// the validity of face f and its box of cells c0 .. c1 (inclusive) -> the number of cells, 0 for an invalid face; never an address from
// an index outside [0, V)
__device__ __forceinline__ int tri_box(const float* xyz, int V, const int* faces, long long f, const TriGrid& g, int c0[3], int c1[3])
{
#pragma clang fp contract(off)
    const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    if (!(in_range(v0, V) && in_range(v1, V) && in_range(v2, V))) return 0;
    const float* a = xyz + 3ll * v0;
    const float* b = xyz + 3ll * v1;
    const float* c = xyz + 3ll * v2;
    const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
    if (!(finite_f32(ax) && finite_f32(ay) && finite_f32(az) && finite_f32(bx) && finite_f32(by) && finite_f32(bz) && finite_f32(cx) &&
          finite_f32(cy) && finite_f32(cz)))
        return 0;
    const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    // two ROUNDED products and their difference, no fma: a face that names a vertex twice (ab == ac, or one of them 0) gives exactly 0
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    if (fmaf(nx, nx, fmaf(ny, ny, nz * nz)) == 0.f) return 0;       // degenerate
    const float l[3] = {fminf(fminf(ax, bx), cx), fminf(fminf(ay, by), cy), fminf(fminf(az, bz), cz)};
    const float h[3] = {fmaxf(fmaxf(ax, bx), cx), fmaxf(fmaxf(ay, by), cy), fmaxf(fmaxf(az, bz), cz)};
    int n = 1;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c0[j] = cell_coord(l[j], g.lo[j], g.inv_cell, g.dims[j]);
        c1[j] = cell_coord(h[j], g.lo[j], g.inv_cell, g.dims[j]);
        n *= c1[j] - c0[j] + 1;                                     // at most dims[0] dims[1] dims[2] <= 2^24
    }
    return n;
}

__global__ __launch_bounds__(WG) void mesh_tri_bins_kernel(const float* xyz, int V, const int* faces, long long F, const TriGrid g, int* count,
                                                           int* flag, unsigned long long* invalid)
{
    const int lane = (int)threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * WG + threadIdx.x;
    bool bad = false;
    if (f < F) {
        int c0[3], c1[3];
        const int n = tri_box(xyz, V, faces, f, g, c0, c1);
        bad = n == 0;
        const bool big = n > g.big_cells;
        count[f] = (bad || big) ? 0 : n;
        flag[f] = bad ? 0 : (big ? 2 : 1);
    }
    const unsigned long long b_bad = __ballot(bad);
    if (b_bad != 0ull && lane == 0) atomicAdd(invalid, (unsigned long long)__popcll(b_bad));
}

__global__ __launch_bounds__(WG) void mesh_tri_fill_kernel(const float* xyz, int V, const int* faces, long long F, const TriGrid g,
                                                           const long long* offset, long long n_pairs, long long* keys, int* pair_face)
{
    const long long f = (long long)blockIdx.x * WG + threadIdx.x;
    if (f >= F) return;
    int c0[3], c1[3];
    const int n = tri_box(xyz, V, faces, f, g, c0, c1);
    if (n == 0 || n > g.big_cells) return;
    long long o = offset[f];
#pragma unroll 1
    for (int z = c0[2]; z <= c1[2]; ++z)
#pragma unroll 1
        for (int y = c0[1]; y <= c1[1]; ++y)
#pragma unroll 1
            for (int x = c0[0]; x <= c1[0]; ++x, ++o)
                if ((unsigned long long)o < (unsigned long long)n_pairs) {      // a foreign offset writes nothing out of bounds
                    keys[o] = ((long long)z * g.dims[1] + y) * g.dims[0] + x;
                    pair_face[o] = (int)f;
                }
}

struct MeshNearestParams {
    const float* query;
    const long long* order;
    const float4* big;              // [B][3]
    const float4* records;          // [P][3]
    const int* cell_start;
    float* dist;
    int* face;
    float* bary;
    float* closest;
    int M, B, P;
    estd_grid grid;
    float max_dist, r2;
};

__global__ __launch_bounds__(WG) void mesh_nearest_kernel(const MeshNearestParams p)
{
    const int i = (int)blockIdx.x * WG + (int)threadIdx.x;
    if (i >= p.M) return;
    const long long qi = p.order ? p.order[i] : (long long)i;
    if ((unsigned long long)qi >= (unsigned long long)p.M) return;           // a malformed permutation writes nothing out of bounds
    const float qx = p.query[3 * qi], qy = p.query[3 * qi + 1], qz = p.query[3 * qi + 2];
    float best = p.r2;
    int best_face = NO_FACE;                                                 // so that d2 == r2 is found
    const float4* best_rec = nullptr;                                        // the winner's record: v, w and p are formed again from it
    float v, w, px, py, pz;

    auto test = [&](const float4* rec) {
        const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
        const float d2 = tri_closest(qx, qy, qz, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, v, w, px, py, pz);
        const int idx = __float_as_int(r2.y);
        if (d2 < best || (d2 == best && idx < best_face)) {
            best = d2;
            best_face = idx;
            best_rec = rec;
        }
    };

    // phase A: the big list, the same record for every lane (a uniform address: scalar loads)
#pragma unroll 1
    for (int j = 0; j < p.B; ++j) test(p.big + 3ll * j);

    // phase B: the rings over the cell table
    if (p.P > 0) {
        auto scan = [&](int k0, int k1) {
            const int beg = max(p.cell_start[k0], 0), end = min(p.cell_start[k1 + 1], p.P);
#pragma unroll 1
            for (int j = beg; j < end; ++j) test(p.records + 3ll * j);
        };

        grid_ring_walk(p.grid, qx, qy, qz, [&]() { return best; }, scan);
    }

    const bool found = best_face != NO_FACE;
    p.dist[qi] = found ? sqrtf(best) : p.max_dist;
    p.face[qi] = found ? best_face : -1;
    if (p.bary || p.closest) {
        v = w = px = py = pz = 0.f;
        if (found) {
            const float4 r0 = best_rec[0], r1 = best_rec[1], r2 = best_rec[2];
            (void)tri_closest(qx, qy, qz, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, v, w, px, py, pz);
        }
        if (p.bary) {
            p.bary[2 * qi] = v;
            p.bary[2 * qi + 1] = w;
        }
        if (p.closest) {
            p.closest[3 * qi] = px;
            p.closest[3 * qi + 1] = py;
            p.closest[3 * qi + 2] = pz;
        }
    }
}

inline TriGrid tri_grid(const float* lo3, float cell, const int* dims3, int big_cells)
{
    TriGrid g{};
    g.inv_cell = estd_inv_cell(cell);
    for (int j = 0; j < 3; ++j) { g.lo[j] = lo3[j]; g.dims[j] = dims3[j]; }
    g.big_cells = big_cells;
    return g;
}

}  // namespace

extern "C" int estd_mesh_tri_bins(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const float* lo3, float cell,
                                  const int* dims3, int big_cells, int* count, int* flag, long long* invalid, estd_stream_t s)
{
    if (n_faces < 0 || n_vertices < 0 || big_cells < 0 || !invalid) return ESTD_ERR_ARG;
    if (!estd_grid_ok(lo3, cell, dims3, ESTD_CLOUD_MAX_DIM, ESTD_CLOUD_MAX_CELLS)) return ESTD_ERR_ARG;
    if ((n_vertices > 0 && !xyz) || (n_faces > 0 && (!faces || !count || !flag))) return ESTD_ERR_ARG;
    if (n_vertices > 0x7fffffffLL || n_faces > 0x7fffffffLL / 3) return ESTD_ERR_UNSUPPORTED;
    if (hipMemsetAsync(invalid, 0, sizeof(long long), estd_stream(s)) != hipSuccess) return ESTD_ERR_LAUNCH;
    if (n_faces > 0)
        hipLaunchKernelGGL(mesh_tri_bins_kernel, dim3((unsigned)((n_faces + WG - 1) / WG)), dim3(WG), 0, estd_stream(s), xyz, (int)n_vertices,
                           faces, n_faces, tri_grid(lo3, cell, dims3, big_cells), count, flag, reinterpret_cast<unsigned long long*>(invalid));
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_mesh_tri_fill(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const float* lo3, float cell,
                                  const int* dims3, int big_cells, const long long* offset, long long n_pairs, long long* keys, int* pair_face,
                                  estd_stream_t s)
{
    if (n_faces < 0 || n_vertices < 0 || big_cells < 0 || n_pairs < 0) return ESTD_ERR_ARG;
    if (!estd_grid_ok(lo3, cell, dims3, ESTD_CLOUD_MAX_DIM, ESTD_CLOUD_MAX_CELLS)) return ESTD_ERR_ARG;
    if (n_vertices > 0x7fffffffLL || n_faces > 0x7fffffffLL / 3 || n_pairs > ESTD_MESH_DISTANCE_MAX_PAIRS) return ESTD_ERR_UNSUPPORTED;
    if (n_pairs == 0 || n_faces == 0) return ESTD_OK;
    if (!xyz || !faces || !offset || !keys || !pair_face) return ESTD_ERR_ARG;
    hipLaunchKernelGGL(mesh_tri_fill_kernel, dim3((unsigned)((n_faces + WG - 1) / WG)), dim3(WG), 0, estd_stream(s), xyz, (int)n_vertices,
                       faces, n_faces, tri_grid(lo3, cell, dims3, big_cells), offset, n_pairs, keys, pair_face);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_mesh_nearest(const estd_mesh_nearest_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    if (d->M < 0 || d->B < 0 || d->P < 0) return ESTD_ERR_ARG;
    MeshNearestParams p{};
    if (estd_search_args(d->max_dist, d->P, d->lo, d->cell, d->dims, d->records, d->cell_start, &p.grid, &p.r2) != ESTD_OK) return ESTD_ERR_ARG;
    if (d->B > 0 && (!d->big_records || (reinterpret_cast<unsigned long long>(d->big_records) & 15ull))) return ESTD_ERR_ARG;
    if (d->M > 0x7fffffffLL || d->B > ESTD_MESH_DISTANCE_MAX_PAIRS || d->P > ESTD_MESH_DISTANCE_MAX_PAIRS) return ESTD_ERR_UNSUPPORTED;
    if (d->M == 0) return ESTD_OK;
    if (!d->query || !d->dist || !d->face) return ESTD_ERR_ARG;
    p.query = d->query; p.order = d->order;
    p.big = reinterpret_cast<const float4*>(d->big_records); p.records = reinterpret_cast<const float4*>(d->records);
    p.cell_start = d->cell_start; p.dist = d->dist; p.face = d->face; p.bary = d->bary; p.closest = d->closest;
    p.M = (int)d->M; p.B = (int)d->B; p.P = (int)d->P;
    p.max_dist = d->max_dist;
    hipLaunchKernelGGL(mesh_nearest_kernel, dim3((unsigned)estd_ceil_div(d->M, WG)), dim3(WG), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
