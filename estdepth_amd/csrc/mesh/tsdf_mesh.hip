// tsdf_mesh.hip -- the fused surface of a TSDF volume (csrc/tsdf.hip) as a triangle mesh by naive surface nets: one vertex per surface
// cell, one quad per sign-changing voxel edge.  No case table; every topological decision compares stored fp32 values (D < 0,
// Wt >= w_min), so the vertex set and the face list are defined to the integer.  The contract: include/estd_hip.h
// (estd_tsdf_mesh_vertices, estd_tsdf_mesh_faces); its float64 form: tests/tsdf_mesh_ref.py.
//
// Volume: planes of [Z][Y][X] fp32 voxels, x fastest, any X (the accesses here are four bytes per lane: a lane is one voxel).  Offsets
// are 64-bit; ids are 32-bit clean because the entry points refuse more than 2^31 - 1 voxels.
//
// surface_net_cells_kernel<COLOR>: a wave reads 64 consecutive voxels of a row and owns the 63 cells between them -- the +x corner of a
// lane's cell is its neighbour's voxel, fetched with one lane shuffle instead of a second, misaligned load; lane 63 only lends its
// voxels.  A workgroup of four waves covers four cell rows (each wave reads its row and the next) and marches ZCHUNK cell planes along z,
// keeping the upper plane of one step as the lower plane of the next: two row loads per plane and wave for Wt and two for D, each a
// contiguous 256 bytes; D is read only where the weight passes (an unobserved voxel's D decides nothing), so the unobserved bulk of a
// volume costs its weight plane alone.  An active cell's vertex is computed in registers (twelve edges, fully unrolled: no indexed
// array survives); the colour planes are read by active lanes only.  Append: ONE increment of the counter per wave and plane (ballot +
// population count, lane 0 adds, device scope), every record finds its slot from the count below its lane; no float atomics.
//
// surface_net_faces_kernel: one lane per voxel, lanes along x as in tsdf_extract_kernel.  A lane whose voxel is observed tests its +x,
// +y, +z edges on D alone (four loads); only a lane with a crossing reads the 3 x 3 x 2 weights round the edge that decide whether the
// four cells exist and are observed.  It appends {edge id, the four cell ids in winding order} the same way.
#include "../estd_common.h"

namespace {

constexpr int ZCHUNK = 8;          // cell planes a workgroup marches along z

struct CellParams {
    int Z, Y, X;
    float w_min, voxel, origin[3];
    const float* D;
    const float* Wt;
    const float* C;                // [3][Z][Y][X], COLOR only
    unsigned long long* counter;
    long long capacity;
    long long* cell;
    float* xyz;
    float* normal;
    float* weight;
    float* color;
};

// one wave-wide reservation of `n` slots (n is wave-uniform and > 0): lane 0 adds, every lane gets the base
__device__ inline long long wave_reserve(unsigned long long* counter, int lane, int n)
{
    unsigned int lo = 0, hi = 0;
    if (lane == 0) {
        const unsigned long long base = atomicAdd(counter, (unsigned long long)n);
        lo = (unsigned int)base;
        hi = (unsigned int)(base >> 32);
    }
    lo = __shfl(lo, 0);
    hi = __shfl(hi, 0);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// the crossing of one cell edge, D0 at the lower-index end: exactly one end negative -> s = D0 / (D0 - D1)
__device__ inline bool edge_cross(float d0, float d1, float& s)
{
    const bool c = (d0 < 0.f) != (d1 < 0.f);
    s = c ? d0 / (d0 - d1) : 0.f;
    return c;
}

template <bool COLOR>
__global__ __launch_bounds__(256) void surface_net_cells_kernel(const CellParams p)
{
    const int lane = (int)threadIdx.x & 63;
    const int x = (int)blockIdx.x * 63 + lane;                         // this lane's voxel column; its cell when lane < 63
    const int y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);      // the cell row; voxel rows y and y + 1
    const bool in0 = x < p.X && y < p.Y, in1 = x < p.X && y + 1 < p.Y;
    const bool is_cell = lane < 63 && x + 1 < p.X && y + 1 < p.Y;
    const long long row = p.X, plane = (long long)p.X * p.Y;
    const int z_begin = (int)blockIdx.z * ZCHUNK;
    const int z_end = z_begin + ZCHUNK < p.Z - 1 ? z_begin + ZCHUNK : p.Z - 1;     // cell planes z_begin .. z_end - 1
    const long long col = (long long)y * row + x;

    // d[dz][dy][dx], w likewise: dx = 1 comes from the neighbouring lane
    float d[2][2][2], w[2][2][2];
    {
        const long long o = (long long)z_begin * plane + col;
        const float w0 = in0 ? p.Wt[o] : 0.f, w1 = in1 ? p.Wt[o + row] : 0.f;
        const float d0 = in0 && w0 >= p.w_min ? p.D[o] : 0.f, d1 = in1 && w1 >= p.w_min ? p.D[o + row] : 0.f;
        d[1][0][0] = d0; d[1][1][0] = d1; w[1][0][0] = w0; w[1][1][0] = w1;
        d[1][0][1] = __shfl_down(d0, 1); d[1][1][1] = __shfl_down(d1, 1);
        w[1][0][1] = __shfl_down(w0, 1); w[1][1][1] = __shfl_down(w1, 1);
    }
    for (int z = z_begin; z < z_end; ++z) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { d[0][j][i] = d[1][j][i]; w[0][j][i] = w[1][j][i]; }
        }
        {
            const long long o = (long long)(z + 1) * plane + col;
            const float w0 = in0 ? p.Wt[o] : 0.f, w1 = in1 ? p.Wt[o + row] : 0.f;
            const float d0 = in0 && w0 >= p.w_min ? p.D[o] : 0.f, d1 = in1 && w1 >= p.w_min ? p.D[o + row] : 0.f;
            d[1][0][0] = d0; d[1][1][0] = d1; w[1][0][0] = w0; w[1][1][0] = w1;
            d[1][0][1] = __shfl_down(d0, 1); d[1][1][1] = __shfl_down(d1, 1);
            w[1][0][1] = __shfl_down(w0, 1); w[1][1][1] = __shfl_down(w1, 1);
        }
        bool observed = is_cell, neg = false, pos = false;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    observed = observed && w[k][j][i] >= p.w_min;
                    neg = neg || d[k][j][i] < 0.f;
                    pos = pos || !(d[k][j][i] < 0.f);
                }
            }
        }
        const bool active = observed && neg && pos;
        const unsigned long long b = __ballot(active);
        const int n_wave = __popcll(b);
        if (n_wave == 0) continue;                                   // wave-uniform
        const long long slot = wave_reserve(p.counter, lane, n_wave) + __popcll(b & ((1ull << lane) - 1ull));
        if (!active || slot >= p.capacity) continue;                 // records past the capacity are dropped; the counter keeps the total

        // the twelve edges: the four x-edges, then y, then z; within an axis the lower end's linear index ascends (the lower of the two
        // other axes varies fastest).  sum[k]: the cell-local crossing points added in that order; g[k]: the sum of D1 - D0 over axis k
        float sum[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f}, csum[3] = {0.f, 0.f, 0.f};
        int n = 0;
        const long long id = (long long)z * plane + col;
        const long long vplane = (long long)p.Z * plane;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // offsets of the edge's lower end on the two other axes (lo = the lower of them, hi the higher)
                const int lo = e & 1, hi = e >> 1;
                const int ox = a == 0 ? 0 : lo, oy = a == 0 ? lo : (a == 1 ? 0 : hi), oz = a == 2 ? 0 : hi;
                const float d0 = d[oz][oy][ox], d1 = d[oz + (a == 2)][oy + (a == 1)][ox + (a == 0)];
                g[a] += d1 - d0;
                float s;
                if (edge_cross(d0, d1, s)) {
                    sum[0] += a == 0 ? s : (float)ox;
                    sum[1] += a == 1 ? s : (float)oy;
                    sum[2] += a == 2 ? s : (float)oz;
                    n += 1;
                    if constexpr (COLOR) {
                        const long long v0 = id + oz * plane + oy * row + ox;
                        const long long v1 = v0 + (a == 0 ? 1 : (a == 1 ? row : plane));
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const float c0 = p.C[k * vplane + v0], c1 = p.C[k * vplane + v1];
                            csum[k] += fmaf(s, c1 - c0, c0);
                        }
                    }
                }
            }
        }
        const float fn = (float)n;
        const int cidx[3] = {x, y, z};
        const float len = sqrtf(fmaf(g[2], g[2], fmaf(g[1], g[1], g[0] * g[0])));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p.xyz[slot * 3 + k] = fmaf((float)cidx[k] + 0.5f + sum[k] / fn, p.voxel, p.origin[k]);
            p.normal[slot * 3 + k] = len > 0.f ? g[k] / len : 0.f;
            if constexpr (COLOR) p.color[slot * 3 + k] = csum[k] / fn;
        }
        float ws = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) ws += w[k][j][i];
            }
        }
        p.weight[slot] = ws * 0.125f;
        p.cell[slot] = id;
    }
}

struct FaceParams {
    int Z, Y, X;
    float w_min;
    const float* D;
    const float* Wt;
    unsigned long long* counter;
    long long capacity;
    long long* edge;
    int* quad;
};

__global__ __launch_bounds__(256) void surface_net_faces_kernel(const FaceParams p)
{
    const int lane = (int)threadIdx.x & 63;
    const int q[3] = {(int)blockIdx.x * 64 + lane, (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6), (int)blockIdx.z};
    const int dims[3] = {p.X, p.Y, p.Z};
    const long long strides[3] = {1, p.X, (long long)p.X * p.Y};
    const long long idx = ((long long)q[2] * p.Y + q[1]) * p.X + q[0];
    bool face[3] = {false, false, false};
    float d0 = 0.f;
    // an unobserved voxel is a corner of every cell round its edges: no face, and D is not read
    if (q[0] < p.X && q[1] < p.Y && p.Wt[idx] >= p.w_min) {
        d0 = p.D[idx];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            // the four cells round the +a edge exist: q - e_b - e_c is a voxel and q + e_a + e_b + e_c is one
            if (q[a] + 1 >= dims[a] || q[b] < 1 || q[c] < 1 || q[b] + 1 >= dims[b] || q[c] + 1 >= dims[c]) continue;
            const float d1 = p.D[idx + strides[a]];
            if ((d0 < 0.f) == (d1 < 0.f)) continue;
            // all four observed: the 3 x 3 x 2 voxels round the edge
            bool observed = true;
#pragma unroll
            for (int ia = 0; ia < 2; ++ia) {
#pragma unroll
                for (int ib = -1; ib < 2; ++ib) {
#pragma unroll
                    for (int ic = -1; ic < 2; ++ic)
                        observed = observed && p.Wt[idx + ia * strides[a] + ib * strides[b] + ic * strides[c]] >= p.w_min;
                }
            }
            face[a] = observed;
        }
    }
    const unsigned long long b0 = __ballot(face[0]), b1 = __ballot(face[1]), b2 = __ballot(face[2]);
    const int n0 = __popcll(b0), n1 = __popcll(b1), n2 = __popcll(b2);
    if (n0 + n1 + n2 == 0) return;                       // wave-uniform
    const long long base = wave_reserve(p.counter, lane, n0 + n1 + n2);
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long first[3] = {base + __popcll(b0 & below), base + n0 + __popcll(b1 & below), base + n0 + n1 + __popcll(b2 & below)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!face[a] || first[a] >= p.capacity) continue;
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const int c0 = (int)(idx - strides[b] - strides[c]), c1 = (int)(idx - strides[c]), c2 = (int)idx, c3 = (int)(idx - strides[b]);
        // free space on the +a side (D0 < 0): q0 q1 q2 q3; on the other: q3 q2 q1 q0 -- the triangles are (0, 1, 2), (0, 2, 3) of this order
        const int4 rec = d0 < 0.f ? make_int4(c0, c1, c2, c3) : make_int4(c3, c2, c1, c0);
        *reinterpret_cast<int4*>(p.quad + first[a] * 4) = rec;
        p.edge[first[a]] = 3 * idx + a;
    }
}

// any X; the launch grids bound each dimension and the 32-bit cell ids the number of voxels
inline int check_dims(int Z, int Y, int X)
{
    if (Z <= 0 || Y <= 0 || X <= 0) return ESTD_ERR_ARG;
    if (Z > 65535 || Y > 65535 * 4 || X > (1 << 20)) return ESTD_ERR_UNSUPPORTED;
    if ((long long)Z * Y * X > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    return ESTD_OK;
}

}  // namespace

extern "C" int estd_tsdf_mesh_vertices(const float* tsdf, const float* weight, const float* color, int Z, int Y, int X, float voxel_size,
                                       const float* origin3, float w_min, unsigned long long* counter, long long capacity, long long* cell,
                                       float* xyz, float* normal, float* vertex_weight, float* vertex_color, estd_stream_t s)
{
    if (!tsdf || !weight || !origin3 || !counter || capacity < 0 || !finite_pos(voxel_size) || !(w_min == w_min)) return ESTD_ERR_ARG;
    if (capacity > 0 && (!cell || !xyz || !normal || !vertex_weight || (color && !vertex_color))) return ESTD_ERR_ARG;
    if (const int st = check_dims(Z, Y, X)) return st;
    if (Z < 2 || Y < 2 || X < 2) return ESTD_OK;                // no cells: nothing to launch, the counter stays as the caller zeroed it
    CellParams p;
    p.Z = Z; p.Y = Y; p.X = X; p.w_min = w_min; p.voxel = voxel_size;
    for (int j = 0; j < 3; ++j) p.origin[j] = origin3[j];       // HOST pointer: three floats copied into the launch arguments
    p.D = tsdf; p.Wt = weight; p.C = color; p.counter = counter; p.capacity = capacity;
    p.cell = cell; p.xyz = xyz; p.normal = normal; p.weight = vertex_weight; p.color = vertex_color;
    const dim3 grid((unsigned)estd_ceil_div(X - 1, 63), (unsigned)estd_ceil_div(Y - 1, 4), (unsigned)estd_ceil_div(Z - 1, ZCHUNK));
    if (color)
        hipLaunchKernelGGL(surface_net_cells_kernel<true>, grid, dim3(256), 0, estd_stream(s), p);
    else
        hipLaunchKernelGGL(surface_net_cells_kernel<false>, grid, dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_tsdf_mesh_faces(const float* tsdf, const float* weight, int Z, int Y, int X, float w_min, unsigned long long* counter,
                                    long long capacity, long long* edge, int* quad, estd_stream_t s)
{
    if (!tsdf || !weight || !counter || capacity < 0 || !(w_min == w_min)) return ESTD_ERR_ARG;
    if (capacity > 0 && (!edge || !quad)) return ESTD_ERR_ARG;
    if (const int st = check_dims(Z, Y, X)) return st;
    if (Z < 2 || Y < 2 || X < 2) return ESTD_OK;
    FaceParams p;
    p.Z = Z; p.Y = Y; p.X = X; p.w_min = w_min; p.D = tsdf; p.Wt = weight; p.counter = counter; p.capacity = capacity;
    p.edge = edge; p.quad = quad;
    const dim3 grid((unsigned)estd_ceil_div(X, 64), (unsigned)estd_ceil_div(Y, 4), (unsigned)Z);
    hipLaunchKernelGGL(surface_net_faces_kernel, grid, dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
