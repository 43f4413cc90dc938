// mesh_simplify.hip -- vertex clustering with quadric placement (Rossignac-Borrel clusters, Lindstrom's representative vertex): the two
// device stages of fusion3d.simplify_mesh.  The contract: include/estd_hip.h (estd_mesh_cluster_faces, estd_mesh_cluster_quadrics); its
// numpy form: tests/mesh_simplify_ref.py.  The clusters themselves (the ranks of the occupied grid keys) and the two stable sorts between
// the launches are the host's.
//
// Two launches, 256 lanes per workgroup, 64-bit offsets throughout:
//   mesh_cluster_faces_kernel    one lane per input face: the clusters of its three corners (a face with an index outside [0, V) is
//                                never an address, its corner records get cluster K), the triple rotated so that the smallest cluster
//                                comes first with the winding kept, or (-1, -1, -1) for an invalid or collapsed face.  Two counters,
//                                each raised with ONE integer atomic add per wave (ballot + population count).
//   mesh_cluster_quadric_kernel  GROUP = 8 neighbouring lanes per cluster (eight clusters per wave).  Lane l of a group adds the terms of
//                                the segment's records l, l + 8, l + 16, ... in ascending order, from 0, as one chain per accumulator;
//                                an exclusive-or butterfly over the lane distances 4, 2, 1 joins the eight chains (the same bits in
//                                all eight lanes); every lane solves the 3 x 3 system and lane 0 of the group stores the seven values.
//                                Every operation is one IEEE float64 operation in the order the header states, never contracted.
//
// The gather: a record names a face, the face three vertices, so a term costs one 8-byte, one 12-byte and three 12-byte reads through two
// indirections.  A segment holds the corners of neighbouring faces in ascending face order, so the eight lanes of a group read neighbouring
// rows of `faces` and mostly neighbouring vertices; a lane per cluster would read 64 unrelated segments per wave and leave a cluster of 300
// records to one lane.  No LDS, no float atomics, no inline assembly; the outputs are plain vector stores.
#include "../estd_common.h"
#include "../estd_device.h"

namespace {

constexpr int WG = 256;
constexpr int GROUP = 8;                            // lanes per cluster in mesh_cluster_quadric_kernel; the reference's sum tree depends on it

__global__ __launch_bounds__(WG) void mesh_cluster_faces_kernel(const int* faces, long long F, int V, const int* cluster, int K, int* corner,
                                                                int* triple, unsigned long long* counts)
{
    const int lane = (int)threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * WG + threadIdx.x;
    bool bad = false, flat = false;
    if (f < F) {
        const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
        int c0 = K, c1 = K, c2 = K, t0 = -1, t1 = -1, t2 = -1;
        bad = !(in_range(v0, V) && in_range(v1, V) && in_range(v2, V));           // never an address
        if (!bad) {
            c0 = cluster[v0]; c1 = cluster[v1]; c2 = cluster[v2];
            flat = c0 == c1 || c1 == c2 || c2 == c0;
            if (!flat) {
                if (c0 < c1 && c0 < c2) { t0 = c0; t1 = c1; t2 = c2; }
                else if (c1 < c2)       { t0 = c1; t1 = c2; t2 = c0; }
                else                    { t0 = c2; t1 = c0; t2 = c1; }
            }
        }
        corner[3 * f] = c0; corner[3 * f + 1] = c1; corner[3 * f + 2] = c2;
        triple[3 * f] = t0; triple[3 * f + 1] = t1; triple[3 * f + 2] = t2;
    }
    const unsigned long long b_bad = __ballot(bad), b_flat = __ballot(flat);
    if (b_bad != 0ull && lane == 0) atomicAdd(counts, (unsigned long long)__popcll(b_bad));
    if (b_flat != 0ull && lane == 0) atomicAdd(counts + 1, (unsigned long long)__popcll(b_flat));
}

struct QuadricParams {
    const float* xyz;
    const int* faces;
    const long long* order;
    const long long* segments;
    const long long* cell_key;
    const float* mean;
    float* out_xyz;
    float* out_normal;
    unsigned char* placed;
    long long F, K;
    int V;
    int dims[3];
    float lo[3];
    float cell;
    double reg;
};

// the eight chains of a group joined: lane distances 4, 2, 1, every lane ends with the same bits
__device__ __forceinline__ double group_sum(double x)
{
#pragma clang fp contract(off)
    for (int k = GROUP / 2; k >= 1; k >>= 1) x += __shfl_xor(x, k, 64);
    return x;
}

__global__ __launch_bounds__(WG) void mesh_cluster_quadric_kernel(const QuadricParams p)
{
#pragma clang fp contract(off)
    const int sub = (int)threadIdx.x & (GROUP - 1);
    const long long k = (long long)blockIdx.x * (WG / GROUP) + ((int)threadIdx.x / GROUP);
    const bool live = k < p.K;                                                    // a dead group walks no records but joins the shuffles
    const long long n3 = 3 * p.F;
    long long beg = 0, end = 0;
    double centre[3] = {0.0, 0.0, 0.0};
    if (live) {
        beg = max(p.segments[k], 0ll);
        end = min(p.segments[k + 1], n3);
        const long long key = p.cell_key[k], plane = (long long)p.dims[0] * p.dims[1];
        const long long gz = key / plane, rest = key - gz * plane, gy = rest / p.dims[0], gx = rest - gy * p.dims[0];
        centre[0] = (double)p.lo[0] + ((double)gx + 0.5) * (double)p.cell;
        centre[1] = (double)p.lo[1] + ((double)gy + 0.5) * (double)p.cell;
        centre[2] = (double)p.lo[2] + ((double)gz + 0.5) * (double)p.cell;
    }
    double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, bx = 0.0, by = 0.0, bz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
#pragma unroll 1
    for (long long j = beg + sub; j < end; j += GROUP) {
        const long long r = p.order[j];
        if ((unsigned long long)r >= (unsigned long long)n3) continue;            // a malformed permutation is never an address
        const long long f = r / 3;
        const int v0 = p.faces[3 * f], v1 = p.faces[3 * f + 1], v2 = p.faces[3 * f + 2];
        if (!(in_range(v0, p.V) && in_range(v1, p.V) && in_range(v2, p.V))) continue;
        const float* a = p.xyz + 3ll * v0;
        const float* b = p.xyz + 3ll * v1;
        const float* c = p.xyz + 3ll * v2;
        const double ax = a[0], ay = a[1], az = a[2];
        const double e1x = (double)b[0] - ax, e1y = (double)b[1] - ay, e1z = (double)b[2] - az;
        const double e2x = (double)c[0] - ax, e2y = (double)c[1] - ay, e2z = (double)c[2] - az;
        const double mx = e1y * e2z - e1z * e2y, my = e1z * e2x - e1x * e2z, mz = e1x * e2y - e1y * e2x;
        const double px = ax - centre[0], py = ay - centre[1], pz = az - centre[2];
        const double delta = (mx * px + my * py) + mz * pz;
        axx += mx * mx; axy += mx * my; axz += mx * mz; ayy += my * my; ayz += my * mz; azz += mz * mz;
        bx += delta * mx; by += delta * my; bz += delta * mz;
        nx += mx; ny += my; nz += mz;
    }
    axx = group_sum(axx); axy = group_sum(axy); axz = group_sum(axz); ayy = group_sum(ayy); ayz = group_sum(ayz); azz = group_sum(azz);
    bx = group_sum(bx); by = group_sum(by); bz = group_sum(bz);
    nx = group_sum(nx); ny = group_sum(ny); nz = group_sum(nz);
    if (!live || sub != 0) return;

    const unsigned* mean_bits = reinterpret_cast<const unsigned*>(p.mean) + 3 * k;
    const unsigned m0 = mean_bits[0], m1 = mean_bits[1], m2 = mean_bits[2];
    const double t = (axx + ayy) + azz;
    const double lam = t * p.reg;
    const double gx = (double)__uint_as_float(m0) - centre[0], gy = (double)__uint_as_float(m1) - centre[1], gz = (double)__uint_as_float(m2) - centre[2];
    const double M00 = axx + lam, M11 = ayy + lam, M22 = azz + lam, M10 = axy, M20 = axz, M21 = ayz;
    const double r0 = bx + lam * gx, r1 = by + lam * gy, r2 = bz + lam * gz;
    // M = L D L^T without pivoting
    const double d0 = M00;
    const double l10 = M10 / d0, l20 = M20 / d0;
    const double d1 = M11 - l10 * M10;
    const double u21 = M21 - l20 * M10;
    const double l21 = u21 / d1;
    const double d2 = (M22 - l20 * M20) - l21 * u21;
    const double y0 = r0, y1 = r1 - l10 * y0, y2 = (r2 - l20 * y0) - l21 * y1;
    const double z0 = y0 / d0, z1 = y1 / d1, z2 = y2 / d2;
    const double s2 = z2, s1 = z1 - l21 * s2, s0 = (z0 - l10 * s1) - l20 * s2;
    const double half = 0.5 * (double)p.cell;
    const bool ok = t > 0.0 && d0 > 0.0 && d1 > 0.0 && d2 > 0.0 && fabs(s0) <= half && fabs(s1) <= half && fabs(s2) <= half;      // false for a NaN
    unsigned* ox = reinterpret_cast<unsigned*>(p.out_xyz) + 3 * k;
    ox[0] = ok ? __float_as_uint((float)(centre[0] + s0)) : m0;
    ox[1] = ok ? __float_as_uint((float)(centre[1] + s1)) : m1;
    ox[2] = ok ? __float_as_uint((float)(centre[2] + s2)) : m2;
    p.placed[k] = ok ? 1 : 0;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const bool flat = len == 0.0;
    float* on = p.out_normal + 3 * k;
    on[0] = flat ? 0.f : (float)(nx / len);
    on[1] = flat ? 0.f : (float)(ny / len);
    on[2] = flat ? 0.f : (float)(nz / len);
}

}  // namespace

extern "C" int estd_mesh_cluster_faces(const int* faces, long long n_faces, long long n_vertices, const int* cluster, long long n_clusters,
                                       int* corner, int* triple, long long* counts, estd_stream_t s)
{
    if (n_faces < 0 || n_vertices < 0 || n_clusters < 0 || n_clusters > n_vertices || !counts) return ESTD_ERR_ARG;
    if ((n_faces > 0 && (!faces || !corner || !triple)) || (n_vertices > 0 && !cluster)) return ESTD_ERR_ARG;
    if (n_vertices > 0x7fffffffLL || n_faces > 0x7fffffffLL / 3) return ESTD_ERR_UNSUPPORTED;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(long long), estd_stream(s)) != hipSuccess) return ESTD_ERR_LAUNCH;
    if (n_faces == 0 || n_clusters == 0) return ESTD_OK;
    hipLaunchKernelGGL(mesh_cluster_faces_kernel, dim3((unsigned)estd_ceil_div(n_faces, WG)), dim3(WG), 0, estd_stream(s), faces, n_faces,
                       (int)n_vertices, cluster, (int)n_clusters, corner, triple, reinterpret_cast<unsigned long long*>(counts));
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_mesh_cluster_quadrics(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const long long* order,
                                          const long long* segments, const long long* cell_key, long long n_clusters, const float* mean,
                                          const float* lo3, float cell, const int* dims3, double reg, float* out_xyz, float* out_normal,
                                          unsigned char* placed, estd_stream_t s)
{
    if (n_faces < 0 || n_vertices < 0 || n_clusters < 0 || n_clusters > n_vertices) return ESTD_ERR_ARG;
    if (!estd_grid_ok(lo3, cell, dims3, ESTD_CLOUD_KEY_MAX_DIM, 0)) return ESTD_ERR_ARG;      // the grid estd_cloud_cell_keys accepts
    if (!(reg >= 0.0 && reg < (double)__builtin_inf())) return ESTD_ERR_ARG;     // negative, infinite or a NaN
    if ((n_vertices > 0 && !xyz) || (n_faces > 0 && (!faces || !order))) return ESTD_ERR_ARG;
    if (n_clusters > 0 && (!segments || !cell_key || !mean || !out_xyz || !out_normal || !placed)) return ESTD_ERR_ARG;
    if (n_vertices > 0x7fffffffLL || n_faces > 0x7fffffffLL / 3) return ESTD_ERR_UNSUPPORTED;
    if (n_faces == 0 || n_clusters == 0) return ESTD_OK;
    QuadricParams p{};
    p.xyz = xyz; p.faces = faces; p.order = order; p.segments = segments; p.cell_key = cell_key; p.mean = mean;
    p.out_xyz = out_xyz; p.out_normal = out_normal; p.placed = placed;
    p.F = n_faces; p.K = n_clusters; p.V = (int)n_vertices;
    p.cell = cell; p.reg = reg;
    for (int j = 0; j < 3; ++j) { p.lo[j] = lo3[j]; p.dims[j] = dims3[j]; }
    hipLaunchKernelGGL(mesh_cluster_quadric_kernel, dim3((unsigned)estd_ceil_div(n_clusters, WG / GROUP)), dim3(WG), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
