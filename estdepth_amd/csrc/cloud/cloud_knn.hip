// cloud_knn.hip -- the k nearest neighbours of every query in a point cloud, and normals by a PCA plane fit over them: what gives a cloud
// that arrives without normals (a laser scan, a PLY without nx ny nz) a normal score and a point-to-plane registration
// (estdepth_amd/cloud_metrics.py: knn, estimate_normals, remove_outliers).  Nothing here is part of the timed step.
//
// estd_cloud_knn (the contract of include/estd_hip.h).  Per query q, over ALL targets p, in fp32, d2 exactly as estd_cloud_nearest forms
// it: dx = qx - px, dy, dz alike; d2 = fma(dx, dx, fma(dy, dy, dz * dz)).  A candidate's key is the pair (d2, original index), ordered
// lexicographically; the result is the k smallest keys among the candidates with d2 <= r2 = fl(max_dist^2), ascending; count = how many
// there are.  dist = sqrt(d2) (IEEE), slots from count on hold max_dist and -1.  A set of smallest keys and then a sort: the result does
// not depend on the order candidates are met in, so the grid, the cell edge and the order of the queries change no bit.
//
// Structure: PointGrid's records, cell table and cell-sorted query order as csrc/cloud_nn.hip defines them (a candidate is one target
// point in one cell), one lane per query, and the ring walk of csrc/estd_device.h (grid_ring_walk, with the argument why no ring is
// skipped too early).  bound() returns kth = the d2 of the current k-th key once the list is full and r2 before that: while the list is
// not full every candidate within r2 enters, and afterwards a candidate further away than the k-th key can neither enter the list nor tie
// its last place.  A candidate that ties the k-th d2 is still examined (the walk's comparison is strict), and the index decides.
//
// The list: 64-bit keys  bits(d2) << 32 | index  (d2 is not negative and never NaN for finite inputs, so unsigned integer order is the
// pair's order; csrc/mesh/mesh_raster.hip's trick) in LDS, slot-major: keys[slot][lane], so the 64 lanes of the wave touch consecutive
// 8-byte words of one slot -- a per-lane array indexed at run time would live in scratch.  One wave per workgroup, 64 lanes x 32 slots x
// 8 B = 16 KiB, each lane reads and writes its own column only: no barrier.  Maintenance: the worst key and its slot stay in registers;
// a candidate that beats the worst replaces it and the column is rescanned for the new worst (k LDS reads).  At the end the column is
// sorted in place by selection (k^2 / 2 reads) and written out.  One instance serves every k in 1 .. 32 (the trip counts are run-time
// values); the STATS instance counts the candidates examined for the bench tool.
//
// estd_cloud_normals.  One lane per query; the neighbours in list order.  With c = count:
//     mean_j = (sum_i (double)p_i[j]) / c;   x_i = (double)p_i - mean;   C_ab = sum_i (x_ia * x_ib), each product rounded, then added
// (no contraction: numpy reproduces the bits), ab = xx, xy, xz, yy, yz, zz.  The symmetric 3 x 3 eigenproblem is solved in float64 by the
// CYCLIC JACOBI method: JACOBI_SWEEPS sweeps over (0,1), (0,2), (1,2) with the rotation of Rutishauser (t = sgn(theta) / (|theta| +
// sqrt(theta^2 + 1)), an off-diagonal that is exactly 0 is skipped), matrix and vectors in named registers.  The eigenvalues are sorted,
// clamped at 0 from below and rounded to fp32 once; the normal is the unit eigenvector of the smallest, normalised in float64 and rounded
// once.  valid iff c >= 3, every used index in [0, N), l2 > 0 and (l1 - l0) > 2^-16 l2 (on the clamped float64 values).  An index out of
// range is never an address: the row is invalid, counted, and gets zeros.  Sign: with `toward` the fp32 normal is flipped so that
// sum_j n_j ((double)v_j - (double)q_j) >= 0 in float64; without it, or when that sum is exactly 0, the component of largest magnitude
// is positive (the lowest axis among equal magnitudes).  The invalid rows are counted with one integer atomic per wave.
#include "estd_common.h"
#include "estd_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int KNN_WAVE = 64;                    // one wave per workgroup: a lane owns a column of the list
constexpr int JACOBI_SWEEPS = 8;                // quadratic convergence: a 3 x 3 matrix is diagonal to float64 after 5 or 6

struct KnnParams {
    const float* query;
    const long long* order;
    const float4* records;
    const int* cell_start;
    float* dist;
    int* index;
    int* count;
    unsigned int* stats;
    int M, N, k;
    estd_grid grid;
    float max_dist, r2;
};

template <bool STATS>
__global__ __launch_bounds__(KNN_WAVE) void knn_search_kernel(const KnnParams p)
{
    __shared__ unsigned long long keys[ESTD_CLOUD_KNN_MAX * KNN_WAVE];       // [slot][lane]
    const int lane = (int)threadIdx.x;
    const int i = (int)blockIdx.x * KNN_WAVE + lane;
    if (i >= p.M) return;
    const long long qi = p.order ? p.order[i] : (long long)i;
    if ((unsigned long long)qi >= (unsigned long long)p.M) return;           // a malformed permutation writes nothing out of bounds
    const float qx = p.query[3 * qi], qy = p.query[3 * qi + 1], qz = p.query[3 * qi + 2];
    const int k = p.k;
    unsigned long long* col = keys + lane;
    int n = 0;                                                               // keys in the list
    unsigned long long worst = 0ull;                                         // the largest key of a FULL list ...
    int worst_slot = 0;                                                      // ... and where it sits
    float kth = p.r2;                                                        // the d2 the ring bound is compared to
    unsigned int examined = 0;

    if (p.N > 0) {
        // the largest key of the column and its slot, once the list is full
        auto rescan = [&]() {
            unsigned long long w = col[0];
            int ws = 0;
            for (int s = 1; s < k; ++s) {
                const unsigned long long v = col[s * KNN_WAVE];
                if (v > w) { w = v; ws = s; }
            }
            worst = w; worst_slot = ws;
            kth = __uint_as_float((unsigned int)(w >> 32));
        };

        // the records of cells k0 .. k1 of one row
        auto scan = [&](int k0, int k1) {
            const int beg = max(p.cell_start[k0], 0), end = min(p.cell_start[k1 + 1], p.N);
            for (int j = beg; j < end; ++j) {
                const float4 t = p.records[j];
                const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
                const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
                const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)__float_as_uint(t.w);
                if (STATS) ++examined;
                if (n < k) {
                    if (d2 <= p.r2) {                                        // so that d2 == r2 is found
                        col[n * KNN_WAVE] = key;
                        if (++n == k) rescan();
                    }
                } else if (key < worst) {
                    col[worst_slot * KNN_WAVE] = key;
                    rescan();
                }
            }
        };

        grid_ring_walk(p.grid, qx, qy, qz, [&]() { return kth; }, scan);
    }

    // ascending: selection sort of the lane's column, each place written out as it is settled
    float* dist = p.dist + (long long)qi * k;
    int* index = p.index + (long long)qi * k;
    for (int a = 0; a < n; ++a) {
        unsigned long long m = col[a * KNN_WAVE];
        int ms = a;
        for (int s = a + 1; s < n; ++s) {
            const unsigned long long v = col[s * KNN_WAVE];
            if (v < m) { m = v; ms = s; }
        }
        if (ms != a) {
            col[ms * KNN_WAVE] = col[a * KNN_WAVE];
            col[a * KNN_WAVE] = m;
        }
        dist[a] = sqrtf(__uint_as_float((unsigned int)(m >> 32)));
        index[a] = (int)(unsigned int)(m & 0xffffffffull);
    }
    for (int a = n; a < k; ++a) {
        dist[a] = p.max_dist;
        index[a] = -1;
    }
    p.count[qi] = n;
    if (STATS) p.stats[qi] = examined;
}

struct NormalsParams {
    const float* points;
    const float* query;
    const int* index;
    const int* count;
    const float* toward;
    float* normal;
    float* eig;
    unsigned char* valid;
    unsigned long long* invalid;
    double* cov;
    int M, N, k, toward_stride;
};

// one Jacobi rotation in the plane (p, q) of the symmetric matrix: app, aqq the diagonal entries, apq the off-diagonal one, arp / arq the
// entries that couple the third index r to p and q; v?p / v?q the two columns of the vectors
__device__ inline void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                     double& v0p, double& v0q, double& v1p, double& v1q, double& v2p, double& v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
}

__device__ inline void swap_cols(double& la, double& lb, double& a0, double& a1, double& a2, double& b0, double& b1, double& b2)
{
    if (lb < la) {
        double t = la; la = lb; lb = t;
        t = a0; a0 = b0; b0 = t;
        t = a1; a1 = b1; b1 = t;
        t = a2; a2 = b2; b2 = t;
    }
}

__global__ __launch_bounds__(256) void knn_normals_kernel(const NormalsParams p)
{
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const bool active = q < p.M;
    bool ok = false, bad = false;
    if (active) {
        const int c = min(max(p.count[q], 0), p.k);
        const int* idx = p.index + (long long)q * p.k;
        bool in_range = true;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int i = 0; i < c; ++i) {
            const int j = idx[i];
            if ((unsigned int)j >= (unsigned int)p.N) { in_range = false; break; }       // never an address
            const float* t = p.points + 3ll * j;
            sx += (double)t[0]; sy += (double)t[1]; sz += (double)t[2];
        }
        double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
        if (in_range && c > 0) {
            const double mx = sx / (double)c, my = sy / (double)c, mz = sz / (double)c;
            for (int i = 0; i < c; ++i) {
                const float* t = p.points + 3ll * idx[i];
                const double x = (double)t[0] - mx, y = (double)t[1] - my, z = (double)t[2] - mz;
                cxx += x * x; cxy += x * y; cxz += x * z; cyy += y * y; cyz += y * z; czz += z * z;
            }
        }
        if (p.cov) {
            double* o = p.cov + 6ll * q;
            o[0] = cxx; o[1] = cxy; o[2] = cxz; o[3] = cyy; o[4] = cyz; o[5] = czz;
        }
        // cyclic Jacobi: a = the matrix, v = the vectors (columns)
        double a00 = cxx, a01 = cxy, a02 = cxz, a11 = cyy, a12 = cyz, a22 = czz;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
            jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        double l0 = a00, l1 = a11, l2 = a22;
        swap_cols(l0, l1, v00, v10, v20, v01, v11, v21);
        swap_cols(l1, l2, v01, v11, v21, v02, v12, v22);
        swap_cols(l0, l1, v00, v10, v20, v01, v11, v21);
        l0 = fmax(l0, 0.0); l1 = fmax(l1, 0.0); l2 = fmax(l2, 0.0);
        ok = in_range && c >= 3 && l2 > 0.0 && (l1 - l0) > 0x1p-16 * l2;
        bad = !ok;
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (ok) {
            const double len = sqrt(v00 * v00 + v10 * v10 + v20 * v20);
            nx = (float)(v00 / len); ny = (float)(v10 / len); nz = (float)(v20 / len);
            double side = 0.0;
            if (p.toward) {
                const float* v = p.toward + (long long)p.toward_stride * q;
                const float* o = p.query + 3ll * q;
                side = (double)nx * ((double)v[0] - (double)o[0]) + (double)ny * ((double)v[1] - (double)o[1]);
                side = side + (double)nz * ((double)v[2] - (double)o[2]);
            }
            bool flip = side < 0.0;
            if (side == 0.0) {
                const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
                const float lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
                flip = lead < 0.f;
            }
            if (flip) { nx = -nx; ny = -ny; nz = -nz; }
        }
        p.normal[3ll * q] = nx; p.normal[3ll * q + 1] = ny; p.normal[3ll * q + 2] = nz;
        const bool keep = in_range;                                                      // an out-of-range row reports zeros
        p.eig[3ll * q] = keep ? (float)l0 : 0.f; p.eig[3ll * q + 1] = keep ? (float)l1 : 0.f; p.eig[3ll * q + 2] = keep ? (float)l2 : 0.f;
        p.valid[q] = ok ? 1 : 0;
    }
    const unsigned long long b = __ballot(bad);
    if (b != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(p.invalid, (unsigned long long)__popcll(b));
}

}  // namespace

extern "C" int estd_cloud_knn(const estd_cloud_knn_desc* d, estd_stream_t s)
{
    if (!d) return ESTD_ERR_ARG;
    if (d->M < 0 || d->N < 0) return ESTD_ERR_ARG;
    if (d->k < 1 || d->k > ESTD_CLOUD_KNN_MAX) return ESTD_ERR_ARG;
    KnnParams p{};
    if (estd_search_args(d->max_dist, d->N, d->lo, d->cell, d->dims, d->records, d->cell_start, &p.grid, &p.r2) != ESTD_OK) return ESTD_ERR_ARG;
    if (d->M > 0x7fffffffLL || d->N > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (d->M == 0) return ESTD_OK;
    if (!d->query || !d->dist || !d->index || !d->count) return ESTD_ERR_ARG;
    p.query = d->query; p.order = d->order; p.records = reinterpret_cast<const float4*>(d->records); p.cell_start = d->cell_start;
    p.dist = d->dist; p.index = d->index; p.count = d->count; p.stats = d->stats;
    p.M = (int)d->M; p.N = (int)d->N; p.k = d->k;
    p.max_dist = d->max_dist;
    const dim3 grid((unsigned)estd_ceil_div(d->M, KNN_WAVE));
    if (d->stats) hipLaunchKernelGGL(knn_search_kernel<true>, grid, dim3(KNN_WAVE), 0, estd_stream(s), p);
    else hipLaunchKernelGGL(knn_search_kernel<false>, grid, dim3(KNN_WAVE), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_cloud_normals(const float* points, long long n, const float* query, long long m, const int* index, const int* count, int k,
                                  const float* toward, int toward_per_query, float* normal, float* eig, unsigned char* valid,
                                  long long* invalid, double* cov, estd_stream_t s)
{
    if (n < 0 || m < 0 || k < 1 || k > ESTD_CLOUD_KNN_MAX) return ESTD_ERR_ARG;
    if (m > 0 && (!query || !index || !count || !normal || !eig || !valid || !invalid)) return ESTD_ERR_ARG;
    if (m > 0 && n > 0 && !points) return ESTD_ERR_ARG;
    if (n > 0x7fffffffLL || m > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (m == 0) return ESTD_OK;                                               // nothing to count: `invalid` is the caller's zero
    if (hipMemsetAsync(invalid, 0, sizeof(long long), estd_stream(s)) != hipSuccess) return ESTD_ERR_LAUNCH;
    NormalsParams p{};
    p.points = points; p.query = query; p.index = index; p.count = count; p.toward = toward; p.toward_stride = toward_per_query ? 3 : 0;
    p.normal = normal; p.eig = eig; p.valid = valid; p.invalid = reinterpret_cast<unsigned long long*>(invalid); p.cov = cov;
    p.M = (int)m; p.N = (int)n; p.k = k;
    hipLaunchKernelGGL(knn_normals_kernel, dim3((unsigned)estd_ceil_div(m, 256)), dim3(256), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
