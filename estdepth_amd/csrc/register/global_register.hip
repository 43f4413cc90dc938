// global_register.hip -- the stage in front of ICP (estdepth_amd/registration.py: fpfh, match_features, ransac_pairs, register_global):
// pose-invariant local descriptors of a point cloud, their nearest neighbours in descriptor space, and a hypothesise-and-verify search
// over the correspondences.  The contract, with the order of every sum and product: include/estd_hip.h (estd_cloud_spfh,
// estd_cloud_fpfh, estd_feature_match, estd_ransac_pairs); its numpy form: tests/global_reg_ref.py.  Nothing here is part of the timed step.
//
//   greg_spfh_kernel<ORIENTED>  one lane per point: the pair features of the point with its neighbours (estd_cloud_knn's lists) in
//                          float64, uncontracted, binned into 3 x 11 counters.  The counters are bytes of six 64-bit registers (a count
//                          is at most 32): no per-lane array, so nothing in scratch and no LDS.
//   greg_fpfh_kernel       one lane per point: the weighted sum of the neighbours' histograms, 33 float64 accumulators in registers (the
//                          loops over the bins are unrolled, every index is a constant), one division per neighbour; the rows without
//                          a descriptor are counted with one integer atomic per wave.
//   greg_match_kernel      brute force in 33 dimensions: 64 query rows per workgroup, each held by one lane of EVERY of its four waves
//                          with its 33 values in registers; the rows of b are staged through LDS in tiles of MATCH_TILE, each wave
//                          takes every fourth row of a tile (every lane reads the same LDS address: a broadcast, no bank conflict) and
//                          the four partial (best, second) pairs are joined through LDS by the key (d2, j).  With one query per lane
//                          of a 256-lane workgroup the first timing showed 3 000 queries on 12 of 256 compute units, nine times
//                          slower than torch.cdist + argmin; this shape launches four times the workgroups for a quarter of the work.
//                          The distance is the fma chain of the header, not |a|^2 + |b|^2 - 2 a.b: the bits are the contract.
//   greg_ransac_kernel     one wave per hypothesis, four per workgroup (no LDS, no barrier): the three draws, the status tests and the
//                          closed-form transform are wave-uniform, so a rejected hypothesis costs three pairs of loads; the lanes stride
//                          over the correspondences, each with its own chain of r2, and an exclusive-or butterfly joins them.  The winner
//                          is an integer atomic maximum of (count, ~h).
#include "../estd_common.h"
#include "../estd_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int GREG_WG = 256;
constexpr int BINS = ESTD_FPFH_BINS;            // 3 groups of 11
constexpr int MATCH_TILE = 128;                 // rows of b per LDS tile
constexpr int MATCH_WAVES = GREG_WG / 64;        // the waves of a workgroup share its 64 queries and split the rows of every tile
constexpr int MATCH_STRIDE = 36;               // floats per staged row: 33 padded to a multiple of four, so that a row starts 16-byte aligned

struct D3 { double x, y, z; };

__device__ inline D3 load3(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ inline D3 sub3(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline double dot3(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline D3 cross3(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline D3 div3(D3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ inline bool zero3(D3 a) { return a.x == 0.0 && a.y == 0.0 && a.z == 0.0; }
// clamped in float64 BEFORE the conversion (a NaN or a huge value from normals that are not finite has no int): NaN -> bin 0
__device__ inline int bin11(double v) { return (int)fmin(fmax(floor(v), 0.0), 10.0); }

// one more in counter `b` of a group: counters 0..7 are the bytes of lo, 8..10 those of hi
__device__ inline void count_bin(unsigned long long& lo, unsigned long long& hi, int b)
{
    if (b < 8) lo += 1ull << (8 * b);
    else hi += 1ull << (8 * (b - 8));
}

template <bool ORIENTED>
__global__ __launch_bounds__(GREG_WG) void greg_spfh_kernel(const float* points, const float* normal, int n, const int* index, const int* count,
                                                            int k, int* hist, int* pairs)
{
    const int s = (int)blockIdx.x * GREG_WG + (int)threadIdx.x;
    if (s >= n) return;
    const D3 ps = load3(points + 3ll * s), u = load3(normal + 3ll * s);
    const bool own = !zero3(u);
    const int c = own ? min(max(count[s], 0), k) : 0;
    const int* idx = index + (long long)s * k;
    unsigned long long a_lo = 0, a_hi = 0, f_lo = 0, f_hi = 0, t_lo = 0, t_hi = 0;
    int np = 0;
    for (int i = 0; i < c; ++i) {
        const int t = idx[i];
        if (t == s || (unsigned int)t >= (unsigned int)n) continue;              // never an address
        const D3 nt = load3(normal + 3ll * t);
        if (zero3(nt)) continue;
        const D3 d = sub3(load3(points + 3ll * t), ps);
        const double len = sqrt(dot3(d, d));
        if (len == 0.0) continue;
        const D3 dn = div3(d, len);
        double phi = dot3(u, dn);
        D3 v = cross3(dn, u);
        const double vl = sqrt(dot3(v, v));
        if (vl == 0.0) continue;
        v = div3(v, vl);
        const D3 w = cross3(u, v);
        double alpha = dot3(v, nt), y = dot3(w, nt), x = dot3(u, nt);
        int ba, bf, bt = 5;
        if (ORIENTED) {
            ba = bin11((fmin(fmax(alpha, -1.0), 1.0) + 1.0) * 5.5);
            bf = bin11((fmin(fmax(phi, -1.0), 1.0) + 1.0) * 5.5);
            const double q = fabs(x) + fabs(y);
            if (q != 0.0) {
                const double r = y / q;
                const double pa = x >= 0.0 ? r : (y >= 0.0 ? 2.0 - r : -2.0 - r);
                bt = bin11((pa + 2.0) * 2.75);
            }
        } else {
            alpha = fabs(alpha); phi = fabs(phi); y = fabs(y); x = fabs(x);
            ba = bin11(fmin(alpha, 1.0) * 11.0);
            bf = bin11(fmin(phi, 1.0) * 11.0);
            const double q = x + y;
            if (q != 0.0) bt = bin11((y / q) * 11.0);
        }
        count_bin(a_lo, a_hi, ba);
        count_bin(f_lo, f_hi, bf);
        count_bin(t_lo, t_hi, bt);
        ++np;
    }
    int* h = hist + (long long)s * BINS;
#pragma unroll
    for (int b = 0; b < 11; ++b) {
        h[b] = (int)(((b < 8 ? a_lo >> (8 * b) : a_hi >> (8 * (b - 8)))) & 0xffull);
        h[11 + b] = (int)(((b < 8 ? f_lo >> (8 * b) : f_hi >> (8 * (b - 8)))) & 0xffull);
        h[22 + b] = (int)(((b < 8 ? t_lo >> (8 * b) : t_hi >> (8 * (b - 8)))) & 0xffull);
    }
    pairs[s] = np;
}

__global__ __launch_bounds__(GREG_WG) void greg_fpfh_kernel(const float* points, const float* normal, int n, const int* index, const int* count,
                                                            int k, const int* hist, const int* pairs, float* desc, unsigned char* valid,
                                                            unsigned long long* invalid)
{
    const int i = (int)blockIdx.x * GREG_WG + (int)threadIdx.x;
    bool bad = false;
    if (i < n) {
        const D3 pi = load3(points + 3ll * i);
        const int c = min(max(count[i], 0), k);
        const int* idx = index + (long long)i * k;
        double acc[BINS];
#pragma unroll
        for (int b = 0; b < BINS; ++b) acc[b] = 0.0;
        int m = 0;
        for (int a = 0; a < c; ++a) {
            const int j = idx[a];
            if (j == i || (unsigned int)j >= (unsigned int)n) continue;          // never an address
            const int pj = pairs[j];
            if (pj <= 0) continue;
            const D3 d = sub3(load3(points + 3ll * j), pi);
            const double d2 = dot3(d, d);
            if (!(d2 > 0.0)) continue;
            const double wj = 1.0 / ((double)pj * d2);
            const int* hj = hist + (long long)j * BINS;
#pragma unroll
            for (int b = 0; b < BINS; ++b) acc[b] = acc[b] + (double)hj[b] * wj;
            ++m;
        }
        const int pi_n = pairs[i];
        const int* hi = hist + (long long)i * BINS;
        float* out = desc + (long long)i * BINS;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            double F[11];
            double sum = 0.0;
#pragma unroll
            for (int b = 0; b < 11; ++b) {
                const double own = pi_n > 0 ? (double)hi[11 * g + b] / (double)pi_n : 0.0;
                const double nb = m > 0 ? acc[11 * g + b] / (double)m : 0.0;
                F[b] = own + nb;
                sum = b == 0 ? F[0] : sum + F[b];
            }
#pragma unroll
            for (int b = 0; b < 11; ++b) out[11 * g + b] = sum == 0.0 ? 0.f : (float)(F[b] / sum);
        }
        const float* nn = normal + 3ll * i;
        const bool ok = !(nn[0] == 0.f && nn[1] == 0.f && nn[2] == 0.f) && pi_n >= 3;
        valid[i] = ok ? 1 : 0;
        bad = !ok;
    }
    const unsigned long long b_bad = __ballot(bad);
    if (b_bad != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(invalid, (unsigned long long)__popcll(b_bad));
}

__global__ __launch_bounds__(GREG_WG) void greg_match_kernel(const float* a, int m, const float* b, int n, const unsigned char* a_valid,
                                                             const unsigned char* b_valid, int* index, float* d2_out, float* d2_second)
{
    __shared__ __attribute__((aligned(16))) float tile[MATCH_TILE * MATCH_STRIDE];
    __shared__ int use[MATCH_TILE];
    __shared__ float part_best[MATCH_WAVES][64], part_second[MATCH_WAVES][64];
    __shared__ int part_j[MATCH_WAVES][64];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = (int)blockIdx.x * 64 + lane;                                   // the four waves hold the SAME 64 queries
    const bool row = i < m && (!a_valid || a_valid[i] != 0);
    float q[BINS];
#pragma unroll
    for (int c = 0; c < BINS; ++c) q[c] = row ? a[(long long)i * BINS + c] : 0.f;
    const float inf = __builtin_inff();
    float best = inf, second = inf;
    int best_j = -1;
    for (int base = 0; base < n; base += MATCH_TILE) {
        const int rows = min(MATCH_TILE, n - base);
        __syncthreads();                                                         // the previous tile has been read by every lane
        for (int e = tid; e < rows * BINS; e += GREG_WG) {
            const int r = e / BINS, c = e - r * BINS;
            tile[r * MATCH_STRIDE + c] = b[(long long)(base + r) * BINS + c];
        }
        if (tid < MATCH_TILE) use[tid] = tid < rows && (!b_valid || b_valid[base + tid] != 0);
        __syncthreads();
        if (row) {
            for (int r = wave; r < rows; r += MATCH_WAVES) {                     // each wave a quarter of the tile's rows
                if (!use[r]) continue;                                           // wave-uniform
                const float* t = tile + r * MATCH_STRIDE;
                const float e0 = q[0] - t[0];
                float d2 = e0 * e0;
#pragma unroll
                for (int c = 1; c < BINS; ++c) {
                    const float e = q[c] - t[c];
                    d2 = fmaf(e, e, d2);
                }
                if (d2 < best) {                                                 // a wave's rows come in ascending j: an equal d2 does not displace
                    second = best; best = d2; best_j = base + r;
                } else if (d2 < second) {
                    second = d2;
                }
            }
        }
    }
    // the four partial results of a query meet in LDS; wave 0 joins them in wave order by the key (d2, j): the two smallest d2 of the
    // union are among the four waves' two smallest, and the outcome does not depend on which wave saw which row
    part_best[wave][lane] = best; part_second[wave][lane] = second; part_j[wave][lane] = best_j;
    __syncthreads();
    if (wave == 0 && i < m) {
#pragma unroll
        for (int w = 1; w < MATCH_WAVES; ++w) {
            const float ob = part_best[w][lane], os = part_second[w][lane];
            const int oj = part_j[w][lane];
            if (oj < 0) continue;                                                // that wave found nothing
            if (best_j < 0 || ob < best || (ob == best && oj < best_j)) {
                second = best; best = ob; best_j = oj;
            } else if (ob < second) {
                second = ob;
            }
            if (os < second) second = os;
        }
        index[i] = best_j;
        d2_out[i] = best;
        d2_second[i] = second;
    }
}

struct RansacParams {
    const float* P;
    const float* Q;
    int C, H;
    unsigned long long seed;
    double dist2, edge_ratio;
    int* count;
    unsigned char* status;
    double* ssq;
    double* T;
    unsigned long long* best;
};

// the frame of three points: e1 along a -> b, e3 the triangle's normal, e2 = e3 x e1; false when it does not exist
__device__ inline bool frame3(D3 a, D3 b, D3 c, D3& e1, D3& e2, D3& e3)
{
    const D3 ab = sub3(b, a);
    const double l1 = sqrt(dot3(ab, ab));
    if (l1 == 0.0) return false;
    e1 = div3(ab, l1);
    const D3 nrm = cross3(e1, sub3(c, a));
    const double l3 = sqrt(dot3(nrm, nrm));
    if (l3 == 0.0) return false;
    e3 = div3(nrm, l3);
    e2 = cross3(e3, e1);
    return true;
}

__device__ inline double edge_len(D3 a, D3 b) { const D3 d = sub3(b, a); return sqrt(dot3(d, d)); }
__device__ inline bool finite_d(double v) { return v - v == 0.0; }

__global__ __launch_bounds__(GREG_WG) void greg_ransac_kernel(const RansacParams p)
{
    const int lane = (int)threadIdx.x & 63;
    const int h = (int)blockIdx.x * (GREG_WG / 64) + ((int)threadIdx.x >> 6);
    if (h >= p.H) return;                                                        // the whole wave
    int status = 0;
    double R[9], t[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    if (p.C <= 0) {
        status = 1;
    } else {
        const unsigned long long C = (unsigned long long)p.C, hh = (unsigned long long)h;
        const long long c0 = (long long)(h64(p.seed, hh, 0ull) % C), c1 = (long long)(h64(p.seed, hh, 1ull) % C), c2 = (long long)(h64(p.seed, hh, 2ull) % C);
        if (c0 == c1 || c0 == c2 || c1 == c2) {
            status = 1;
        } else {
            const D3 pa = load3(p.P + 3 * c0), pb = load3(p.P + 3 * c1), pc = load3(p.P + 3 * c2);
            const D3 qa = load3(p.Q + 3 * c0), qb = load3(p.Q + 3 * c1), qc = load3(p.Q + 3 * c2);
            const double lp0 = edge_len(pa, pb), lp1 = edge_len(pb, pc), lp2 = edge_len(pc, pa);
            const double lq0 = edge_len(qa, qb), lq1 = edge_len(qb, qc), lq2 = edge_len(qc, qa);
            const double er = p.edge_ratio;
            D3 e1p, e2p, e3p, e1q, e2q, e3q;
            if (lp0 < er * lq0 || lq0 < er * lp0 || lp1 < er * lq1 || lq1 < er * lp1 || lp2 < er * lq2 || lq2 < er * lp2) {
                status = 2;
            } else if (!frame3(pa, pb, pc, e1p, e2p, e3p) || !frame3(qa, qb, qc, e1q, e2q, e3q)) {
                status = 3;
            } else {
                const double a1[3] = {e1q.x, e1q.y, e1q.z}, a2[3] = {e2q.x, e2q.y, e2q.z}, a3[3] = {e3q.x, e3q.y, e3q.z};
                const double b1[3] = {e1p.x, e1p.y, e1p.z}, b2[3] = {e2p.x, e2p.y, e2p.z}, b3[3] = {e3p.x, e3p.y, e3p.z};
                const double cp[3] = {((pa.x + pb.x) + pc.x) / 3.0, ((pa.y + pb.y) + pc.y) / 3.0, ((pa.z + pb.z) + pc.z) / 3.0};
                const double cq[3] = {((qa.x + qb.x) + qc.x) / 3.0, ((qa.y + qb.y) + qc.y) / 3.0, ((qa.z + qb.z) + qc.z) / 3.0};
                bool fin = true;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        R[3 * i + j] = (a1[i] * b1[j] + a2[i] * b2[j]) + a3[i] * b3[j];
                        fin = fin && finite_d(R[3 * i + j]);
                    }
                    t[i] = cq[i] - ((R[3 * i] * cp[0] + R[3 * i + 1] * cp[1]) + R[3 * i + 2] * cp[2]);
                    fin = fin && finite_d(t[i]);
                }
                if (!fin) {
                    status = 3;
#pragma unroll
                    for (int j = 0; j < 9; ++j) R[j] = 0.0;
                    t[0] = t[1] = t[2] = 0.0;
                }
            }
        }
    }
    int cnt = 0;
    double ssq = 0.0;
    if (status == 0) {
        for (int r = lane; r < p.C; r += 64) {
            const D3 s = load3(p.P + 3ll * r), q = load3(p.Q + 3ll * r);
            const double ex = (((R[0] * s.x + R[1] * s.y) + R[2] * s.z) + t[0]) - q.x;
            const double ey = (((R[3] * s.x + R[4] * s.y) + R[5] * s.z) + t[1]) - q.y;
            const double ez = (((R[6] * s.x + R[7] * s.y) + R[8] * s.z) + t[2]) - q.z;
            const double r2 = (ex * ex + ey * ey) + ez * ez;
            if (r2 <= p.dist2) { ++cnt; ssq = ssq + r2; }
        }
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) {
            ssq += __shfl_xor(ssq, k, 64);
            cnt += __shfl_xor(cnt, k, 64);
        }
    }
    if (lane == 0) {
        p.count[h] = cnt;
        p.status[h] = (unsigned char)status;
        p.ssq[h] = ssq;
        if (status == 0) atomicMax(p.best, ((unsigned long long)(unsigned int)cnt << 32) | (unsigned long long)(0xffffffffu - (unsigned int)h));
        double* T = p.T + 12ll * h;                                              // constant indices only: R and t stay in registers
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            T[4 * i] = R[3 * i]; T[4 * i + 1] = R[3 * i + 1]; T[4 * i + 2] = R[3 * i + 2]; T[4 * i + 3] = t[i];
        }
    }
}

inline int rows_ok(long long n, int k) { return n < 0 || k < 1 || k > ESTD_CLOUD_KNN_MAX ? ESTD_ERR_ARG : ESTD_OK; }

}  // namespace

extern "C" int estd_cloud_spfh(const float* points, const float* normal, long long n, const int* index, const int* count, int k, int oriented,
                               int* hist, int* pairs, estd_stream_t s)
{
    if (rows_ok(n, k) != ESTD_OK) return ESTD_ERR_ARG;
    if (n > 0 && (!points || !normal || !index || !count || !hist || !pairs)) return ESTD_ERR_ARG;
    if (n > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (n == 0) return ESTD_OK;
    const dim3 grid((unsigned)estd_ceil_div(n, GREG_WG));
    if (oriented) hipLaunchKernelGGL(greg_spfh_kernel<true>, grid, dim3(GREG_WG), 0, estd_stream(s), points, normal, (int)n, index, count, k, hist, pairs);
    else hipLaunchKernelGGL(greg_spfh_kernel<false>, grid, dim3(GREG_WG), 0, estd_stream(s), points, normal, (int)n, index, count, k, hist, pairs);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_cloud_fpfh(const float* points, const float* normal, long long n, const int* index, const int* count, int k, const int* hist,
                               const int* pairs, float* desc, unsigned char* valid, long long* invalid, estd_stream_t s)
{
    if (rows_ok(n, k) != ESTD_OK) return ESTD_ERR_ARG;
    if (n > 0 && (!points || !normal || !index || !count || !hist || !pairs || !desc || !valid || !invalid)) return ESTD_ERR_ARG;
    if (n > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (n == 0) return ESTD_OK;                                                  // nothing to count: `invalid` is the caller's zero
    if (hipMemsetAsync(invalid, 0, sizeof(long long), estd_stream(s)) != hipSuccess) return ESTD_ERR_LAUNCH;
    hipLaunchKernelGGL(greg_fpfh_kernel, dim3((unsigned)estd_ceil_div(n, GREG_WG)), dim3(GREG_WG), 0, estd_stream(s), points, normal, (int)n, index,
                       count, k, hist, pairs, desc, valid, reinterpret_cast<unsigned long long*>(invalid));
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_feature_match(const float* a, long long m, const float* b, long long n, const unsigned char* a_valid, const unsigned char* b_valid,
                                  int* index, float* d2, float* d2_second, estd_stream_t s)
{
    if (m < 0 || n < 0) return ESTD_ERR_ARG;
    if (m > 0 && (!a || !index || !d2 || !d2_second)) return ESTD_ERR_ARG;
    if (m > 0 && n > 0 && !b) return ESTD_ERR_ARG;
    if (m > 0x7fffffffLL || n > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (m == 0) return ESTD_OK;
    hipLaunchKernelGGL(greg_match_kernel, dim3((unsigned)estd_ceil_div(m, 64)), dim3(GREG_WG), 0, estd_stream(s), a, (int)m, b, (int)n, a_valid,
                       b_valid, index, d2, d2_second);
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_ransac_pairs(const float* P, const float* Q, long long c, long long hypotheses, unsigned long long seed, double dist_max,
                                 double edge_ratio, int* count, unsigned char* status, double* ssq, double* T, unsigned long long* best,
                                 estd_stream_t s)
{
    if (c < 0 || hypotheses < 0) return ESTD_ERR_ARG;
    if (!(dist_max >= 0.0) || !(dist_max - dist_max == 0.0)) return ESTD_ERR_ARG;
    if (!(edge_ratio >= 0.0 && edge_ratio <= 1.0)) return ESTD_ERR_ARG;
    if (hypotheses > 0 && (!count || !status || !ssq || !T || !best)) return ESTD_ERR_ARG;
    if (hypotheses > 0 && c > 0 && (!P || !Q)) return ESTD_ERR_ARG;
    if (c > 0x7fffffffLL || hypotheses > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    if (hypotheses == 0) return ESTD_OK;
    if (hipMemsetAsync(best, 0, sizeof(unsigned long long), estd_stream(s)) != hipSuccess) return ESTD_ERR_LAUNCH;
    RansacParams p{};
    p.P = P; p.Q = Q; p.C = (int)c; p.H = (int)hypotheses; p.seed = seed; p.dist2 = dist_max * dist_max; p.edge_ratio = edge_ratio;
    p.count = count; p.status = status; p.ssq = ssq; p.T = T; p.best = best;
    hipLaunchKernelGGL(greg_ransac_kernel, dim3((unsigned)estd_ceil_div(hypotheses, GREG_WG / 64)), dim3(GREG_WG), 0, estd_stream(s), p);
    return ESTD_LAUNCH_CHECK();
}
