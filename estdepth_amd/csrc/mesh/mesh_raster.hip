// mesh_raster.hip -- a z-buffer rasteriser for triangle lists: the depth, face, barycentric and facing maps of a mesh in one camera.
// The contract: include/estd_hip.h (estd_mesh_raster, estd_mesh_raster_resolve); its numpy form: tests/mesh_raster_ref.py.  No clipping
// stage and no case table: the per-pixel test is a ray-triangle test in the space q = M (x, 1), where pixel (u, v) is the ray (u, v, 1),
// and every decision is one IEEE float64 operation in the order the header states, never contracted into an fma.
//
// Two launches, 256 lanes per workgroup, 64-bit offsets throughout:
//   mesh_raster_kernel<PRE>  one WAVE per triangle: its three vertices projected, the three edge normals and det formed (the same values
//                            in all 64 lanes), then the lanes sweep the triangle's screen box in 8 x 8 pixel blocks aligned to the image
//                            (a lane row = 8 neighbouring keys = one 64-byte segment).  A covered pixel merges key = bits(d) << 32 | f
//                            into keys[H][W] with a 64-bit unsigned atomic minimum at agent scope.  PRE = 1 puts a relaxed agent-scope
//                            load in front and skips the atomic when key >= the value read: keys only decrease, so a value read is never
//                            smaller than the current one and the skip never loses a winner (it pays where many triangles want the
//                            same keys and costs a round trip per block elsewhere: off by default).  A triangle with an index outside
//                            [0, V) is never an address and is counted with one integer atomic per wave.  With few triangles
//                            (F < 8192) gridDim.y = min(64, 8192 / F) waves share each triangle: wave `part` takes the blocks part,
//                            part + parts, ... of its box -- which wave visits a pixel changes no bit of a minimum.
//   mesh_resolve_kernel      one lane per pixel: unpacks the key and recomputes the winner's edge functions (the same operations, the
//                            same bits) for the barycentric pair and the facing; writes every pixel of all four maps
//
// The box: with all three q_z > z_near the projections' bounding box with a one-pixel margin, clamped to the image before any address
// is formed; the whole image otherwise (a triangle that crosses the camera plane).  A triangle whose det is 0 or not finite is skipped:
// c = det / S is then 0, infinite or a NaN for every S, and contributes to no pixel.  No float atomics, no LDS, no inline assembly.
#include "../estd_common.h"
#include "../estd_device.h"

namespace {

constexpr int WG = 256;
constexpr long long RASTER_SPLIT_WAVES = 8192;      // below this many triangles each one's blocks are dealt to RASTER_SPLIT_WAVES / F waves,
constexpr long long RASTER_MAX_PARTS = 64;          // at most this many

struct RasterMat { double m[12]; };

// q_j = ((M_j0 x + M_j1 y) + M_j2 z) + M_j3
__device__ __forceinline__ void project(const RasterMat& M, const float* p, double* q)
{
#pragma clang fp contract(off)
    const double x = p[0], y = p[1], z = p[2];
    for (int j = 0; j < 3; ++j) q[j] = ((M.m[4 * j] * x + M.m[4 * j + 1] * y) + M.m[4 * j + 2] * z) + M.m[4 * j + 3];
}

// n = a x b, each component two rounded products and one difference: exactly antisymmetric in a, b
__device__ __forceinline__ void cross(const double* a, const double* b, double* n)
{
#pragma clang fp contract(off)
    n[0] = a[1] * b[2] - a[2] * b[1];
    n[1] = a[2] * b[0] - a[0] * b[2];
    n[2] = a[0] * b[1] - a[1] * b[0];
}

struct Setup { double n[3][3]; double det; };

__device__ __forceinline__ void setup(const double* q0, const double* q1, const double* q2, Setup& t)
{
#pragma clang fp contract(off)
    cross(q1, q2, t.n[0]);
    cross(q2, q0, t.n[1]);
    cross(q0, q1, t.n[2]);
    t.det = (t.n[0][0] * q0[0] + t.n[0][1] * q0[1]) + t.n[0][2] * q0[2];
}

// the edge functions and their sum at pixel (u, v) -> covered
__device__ __forceinline__ bool edges(const Setup& t, double u, double v, double* E, double& S)
{
#pragma clang fp contract(off)
    for (int k = 0; k < 3; ++k) E[k] = (t.n[k][0] * u + t.n[k][1] * v) + t.n[k][2];
    S = (E[0] + E[1]) + E[2];
    return (E[0] >= 0.0 && E[1] >= 0.0 && E[2] >= 0.0 && S > 0.0) || (E[0] <= 0.0 && E[1] <= 0.0 && E[2] <= 0.0 && S < 0.0);
}

template <int PRE>
__global__ __launch_bounds__(WG) void mesh_raster_kernel(const float* xyz, int V, const int* faces, long long face_first, long long face_count,
                                                         RasterMat M, int H, int W, float z_near, unsigned long long* keys,
                                                         unsigned long long* invalid)
{
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (WG / 64) + ((int)threadIdx.x >> 6);
    const int part = (int)blockIdx.y, parts = (int)gridDim.y;                     // the triangle's blocks part, part + parts, ... are this wave's
    if (w >= face_count) return;
    const long long f = face_first + w;
    const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    if (!(in_range(v0, V) && in_range(v1, V) && in_range(v2, V))) {                // never an address
        if (lane == 0 && part == 0) atomicAdd(invalid, 1ull);
        return;
    }
    double q0[3], q1[3], q2[3];
    project(M, xyz + 3ll * v0, q0);
    project(M, xyz + 3ll * v1, q1);
    project(M, xyz + 3ll * v2, q2);
    Setup t;
    setup(q0, q1, q2, t);
    if (!(fabs(t.det) < __builtin_inf()) || t.det == 0.0) return;                 // det / S is 0, infinite or a NaN whatever S is
    // the pixels that can be covered: u0..u1 x r0..r1, inside the image
    int u0 = 0, u1 = W - 1, r0 = 0, r1 = H - 1;
    const double zn = (double)z_near;
    if (q0[2] > zn && q1[2] > zn && q2[2] > zn) {
        const double x0 = q0[0] / q0[2], x1 = q1[0] / q1[2], x2 = q2[0] / q2[2];
        const double y0 = q0[1] / q0[2], y1 = q1[1] / q1[2], y2 = q2[1] / q2[2];
        // clamped as doubles first: a projection may be infinite (never a NaN: det is finite, so every q is)
        const double lo_x = fmax(floor(fmin(fmin(x0, x1), x2)) - 1.0, 0.0), hi_x = fmin(ceil(fmax(fmax(x0, x1), x2)) + 1.0, (double)(W - 1));
        const double lo_y = fmax(floor(fmin(fmin(y0, y1), y2)) - 1.0, 0.0), hi_y = fmin(ceil(fmax(fmax(y0, y1), y2)) + 1.0, (double)(H - 1));
        if (!(lo_x <= hi_x && lo_y <= hi_y)) return;                              // off the image
        u0 = (int)lo_x; u1 = (int)hi_x; r0 = (int)lo_y; r1 = (int)hi_y;
    }
    const int lx = lane & 7, ly = lane >> 3;
    const int bx0 = u0 >> 3, by0 = r0 >> 3, nbx = (u1 >> 3) - bx0 + 1, nb = nbx * ((r1 >> 3) - by0 + 1);
    for (int k = part; k < nb; k += parts) {
        const int r = (by0 + k / nbx) * 8 + ly, u = (bx0 + k % nbx) * 8 + lx;
        if (u < u0 || u > u1 || r < r0 || r > r1) continue;
        double E[3], S;
        if (!edges(t, (double)u, (double)r, E, S)) continue;
        const double c = t.det / S;
        const float d = (float)c;
        if (!(d > z_near && d < __builtin_inff())) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(unsigned)f;
        unsigned long long* slot = keys + ((long long)r * W + u);
        if (PRE && key >= __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;
        __hip_atomic_fetch_min(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(WG) void mesh_resolve_kernel(const float* xyz, int V, const int* faces, long long F, RasterMat M, int H, int W,
                                                          const unsigned long long* keys, float* depth, int* face, float* bary, int* facing)
{
#pragma clang fp contract(off)
    const long long p = (long long)blockIdx.x * WG + threadIdx.x;
    if (p >= (long long)H * W) return;
    const unsigned long long key = keys[p];
    float d = 0.f, b1 = 0.f, b2 = 0.f;
    int fo = -1, side = 0;
    const long long f = (long long)(key & 0xffffffffull);
    if (key != ~0ull && f < F) {
        const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
        if (in_range(v0, V) && in_range(v1, V) && in_range(v2, V)) {              // false only for keys that are not this mesh's
            double q0[3], q1[3], q2[3], E[3], S;
            project(M, xyz + 3ll * v0, q0);
            project(M, xyz + 3ll * v1, q1);
            project(M, xyz + 3ll * v2, q2);
            Setup t;
            setup(q0, q1, q2, t);
            edges(t, (double)(p % W), (double)(p / W), E, S);
            d = __uint_as_float((unsigned)(key >> 32));
            fo = (int)f;
            b1 = (float)(E[1] / S);
            b2 = (float)(E[2] / S);
            side = S < 0.0 ? 1 : (S > 0.0 ? -1 : 0);                             // S < 0: counter-clockwise seen from the camera
        }
    }
    depth[p] = d;
    face[p] = fo;
    bary[2 * p] = b1;
    bary[2 * p + 1] = b2;
    facing[p] = side;
}

bool mat_finite(const double* mat)
{
    for (int i = 0; i < 12; ++i)
        if (!(mat[i] - mat[i] == 0.0)) return false;
    return true;
}

// the checks both entry points share; -> ESTD_OK or the refusal
int check_raster_args(const float* xyz, long long V, const int* faces, long long F, const double* mat, int H, int W)
{
    if (V < 0 || F < 0 || H <= 0 || W <= 0 || !mat) return ESTD_ERR_ARG;
    if ((V > 0 && !xyz) || (F > 0 && !faces) || !mat_finite(mat)) return ESTD_ERR_ARG;
    if (V > 0x7fffffffLL || F > 0x7fffffffLL / 3 || (long long)H * W > 0x7fffffffLL) return ESTD_ERR_UNSUPPORTED;
    return ESTD_OK;
}

}  // namespace

extern "C" int estd_mesh_raster(const float* xyz, long long n_vertices, const int* faces, long long n_faces, long long face_first,
                                long long face_count, const double* mat, int H, int W, float z_near, int flags, unsigned long long* keys,
                                long long* invalid, estd_stream_t s)
{
    const int st = check_raster_args(xyz, n_vertices, faces, n_faces, mat, H, W);
    if (st != ESTD_OK) return st;
    if (!keys || !invalid || !(z_near >= 0.f && z_near < __builtin_inff()) || (flags & ~(ESTD_MESH_RASTER_PRELOAD | ESTD_MESH_RASTER_CLEAR)))
        return ESTD_ERR_ARG;
    if (face_first < 0 || face_count < 0 || face_first > n_faces || face_count > n_faces - face_first) return ESTD_ERR_ARG;
    if (hipMemsetAsync(invalid, 0, sizeof(long long), estd_stream(s)) != hipSuccess) return ESTD_ERR_LAUNCH;
    if ((flags & ESTD_MESH_RASTER_CLEAR) && hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * (size_t)H * (size_t)W, estd_stream(s)) != hipSuccess)
        return ESTD_ERR_LAUNCH;
    if (face_count > 0) {
        RasterMat M;
        for (int i = 0; i < 12; ++i) M.m[i] = mat[i];
        // few triangles: the blocks of each are dealt to several waves, so that one that fills the image does not leave the device to one wave
        const long long parts = RASTER_SPLIT_WAVES / face_count;
        const dim3 grid((unsigned)((face_count + WG / 64 - 1) / (WG / 64)), (unsigned)(parts < 1 ? 1 : (parts > RASTER_MAX_PARTS ? RASTER_MAX_PARTS : parts)));
        auto* inv = reinterpret_cast<unsigned long long*>(invalid);
        if (!(flags & ESTD_MESH_RASTER_PRELOAD))
            hipLaunchKernelGGL(mesh_raster_kernel<0>, grid, dim3(WG), 0, estd_stream(s), xyz, (int)n_vertices, faces, face_first, face_count, M, H, W,
                               z_near, keys, inv);
        else
            hipLaunchKernelGGL(mesh_raster_kernel<1>, grid, dim3(WG), 0, estd_stream(s), xyz, (int)n_vertices, faces, face_first, face_count, M, H, W,
                               z_near, keys, inv);
    }
    return ESTD_LAUNCH_CHECK();
}

extern "C" int estd_mesh_raster_resolve(const float* xyz, long long n_vertices, const int* faces, long long n_faces, const double* mat, int H,
                                        int W, const unsigned long long* keys, float* depth, int* face, float* bary, int* facing,
                                        estd_stream_t s)
{
    const int st = check_raster_args(xyz, n_vertices, faces, n_faces, mat, H, W);
    if (st != ESTD_OK) return st;
    if (!keys || !depth || !face || !bary || !facing) return ESTD_ERR_ARG;
    RasterMat M;
    for (int i = 0; i < 12; ++i) M.m[i] = mat[i];
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, estd_stream(s), xyz, (int)n_vertices, faces, n_faces, M,
                       H, W, keys, depth, face, bary, facing);
    return ESTD_LAUNCH_CHECK();
}
