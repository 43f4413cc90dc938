// mesh_components.hip -- the connected components of a triangle mesh by a single-pass, lock-free union-find over all workgroups (the
// ECL-CC scheme).  The contract: include/estd_hip.h (estd_mesh_components); its numpy form: tests/mesh_components_ref.py.  Every output is
// defined to the integer: label[v] = the smallest vertex index of v's component, triangles[r] = the triangles of root r.
//
// Four launches, 256 lanes per workgroup, 64-bit offsets throughout:
//   mesh_cc_init_kernel     one lane per vertex: parent[v] = v, triangles[v] = 0; lane 0 of the grid writes the start value of `invalid`
//   mesh_cc_hook_kernel     one lane per triangle: union(v0, v1), union(v0, v2); a triangle with an index outside [0, V) is skipped
//   mesh_cc_flatten_kernel  one lane per vertex: label[v] = find(v), in place over parent[]
//   mesh_cc_count_kernel    one lane per triangle: +1 at triangles[label[v0]], the lanes of a wave that share a root send ONE atomic add;
//                           a triangle with an index outside [0, V) is counted in `invalid` (one add per wave) and nowhere else
//
// The union-find itself (parent_load, find_root, find_root_halving, unite) is csrc/estd_device.h's, with the argument for the forest's
// invariant, the termination of every loop and the visibility of every read and write, stated there once.  Here the elements are the
// vertices, and the edges hooked are (v0, v1) and (v0, v2) of every triangle.
#include "../estd_common.h"
#include "../estd_device.h"

namespace {

constexpr int WG = 256;

__global__ __launch_bounds__(WG) void mesh_cc_init_kernel(int* parent, int* triangles, long long* invalid, long long invalid_start, int V)
{
    const long long v = (long long)blockIdx.x * WG + threadIdx.x;
    if (v == 0) *invalid = invalid_start;
    if (v < V) {
        parent[v] = (int)v;
        triangles[v] = 0;
    }
}

__global__ __launch_bounds__(WG) void mesh_cc_hook_kernel(const int* faces, long long F, int* parent, int V)
{
    const long long f = (long long)blockIdx.x * WG + threadIdx.x;
    if (f >= F) return;
    const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    if (!in_range(v0, V) || !in_range(v1, V) || !in_range(v2, V)) return;       // never an address
    unite(parent, v0, v1);
    unite(parent, v0, v2);
}

// In place: label[] is parent[].  A lane reads what the hook launch left or what another lane of THIS launch has already stored, the
// root of that vertex; either is a smaller member of the tree, and a root keeps parent[r] == r, so the walk ends at the same root both ways.
__global__ __launch_bounds__(WG) void mesh_cc_flatten_kernel(int* label, int V)
{
    const long long v = (long long)blockIdx.x * WG + threadIdx.x;
    if (v >= V) return;
    const int r = find_root(label, (int)v);
    if (r != (int)v) __hip_atomic_store(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(WG) void mesh_cc_count_kernel(const int* faces, long long F, const int* label, int* triangles,
                                                           unsigned long long* invalid, int V)
{
    const int lane = (int)threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * WG + threadIdx.x;
    bool valid = false, bad = false;
    int root = 0;
    if (f < F) {
        const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
        valid = in_range(v0, V) && in_range(v1, V) && in_range(v2, V);
        bad = !valid;
        if (valid) root = label[v0];
    }
    const unsigned long long b_bad = __ballot(bad);
    if (b_bad != 0ull && lane == 0) atomicAdd(invalid, (unsigned long long)__popcll(b_bad));
    // one add per distinct root of the wave: the lowest lane still waiting names its root, every lane with that root is served by the
    // one add.  `todo` is wave-uniform and loses at least that lane per round: at most 64 rounds, one for a wave inside one component.
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {
        const int leader = __ffsll(todo) - 1;
        const int r0 = __shfl(root, leader);
        const unsigned long long same = __ballot(valid && root == r0);
        if (lane == leader) atomicAdd(triangles + r0, __popcll(same));
        todo &= ~same;
    }
}

}  // namespace

extern "C" int estd_mesh_components(const int* faces, long long n_faces, long long n_vertices, int* label, int* triangles,
                                    long long* invalid, estd_stream_t s)
{
    if (n_faces < 0 || n_vertices < 0 || !invalid) return ESTD_ERR_ARG;
    if ((n_faces > 0 && !faces) || (n_vertices > 0 && (!label || !triangles))) return ESTD_ERR_ARG;
    if (n_vertices > 0x7fffffffLL || n_faces > 0x7fffffffLL / 3) return ESTD_ERR_UNSUPPORTED;
    const int V = (int)n_vertices;
    const long long F = n_faces;
    const unsigned v_blocks = (unsigned)((n_vertices + WG - 1) / WG), f_blocks = (unsigned)((F + WG - 1) / WG);
    // without vertices every triangle is out of range: the init launch alone defines the outputs
    hipLaunchKernelGGL(mesh_cc_init_kernel, dim3(v_blocks ? v_blocks : 1u), dim3(WG), 0, estd_stream(s), label, triangles, invalid, V ? 0LL : F, V);
    if (V > 0 && F > 0) {
        hipLaunchKernelGGL(mesh_cc_hook_kernel, dim3(f_blocks), dim3(WG), 0, estd_stream(s), faces, F, label, V);
        hipLaunchKernelGGL(mesh_cc_flatten_kernel, dim3(v_blocks), dim3(WG), 0, estd_stream(s), label, V);
        hipLaunchKernelGGL(mesh_cc_count_kernel, dim3(f_blocks), dim3(WG), 0, estd_stream(s), faces, F, (const int*)label, triangles,
                           reinterpret_cast<unsigned long long*>(invalid), V);
    }
    return ESTD_LAUNCH_CHECK();
}
