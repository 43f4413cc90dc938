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
// The forest.  parent[v] only ever holds v itself or a smaller member of v's tree, and it only ever decreases: the init launch stores v;
// a HOOK, the successful atomicCAS(&parent[a], a, b) with b < a, is the one store that joins two trees; a SHORTCUT, atomicMin(&parent[v],
// g) with g a member of v's tree below parent[v], joins nothing.  So every path strictly descends and ends at a root (parent[r] == r),
// the root is the smallest member of its tree, a vertex that has been hooked never becomes a root again, and once every triangle is
// hooked the trees are the components: the labels do not depend on the order in which the lanes ran.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed, so the hook kernel takes nothing from a load for
// granted: every write of parent[] is an agent-scope atomic (atomicCAS, atomicMin), every read a relaxed agent-scope atomic load (served
// by the L2, never the L1), and ANY value a read returns -- fresh or stale -- was stored at that address at some time, hence is v's own
// index or a smaller member of v's tree.  A stale read costs steps, never correctness: the one decision that takes effect is the CAS,
// which compares against the memory's value.  The launches are ordered by the stream; what one launch stored, the next one reads.
#include "../estd_common.h"
#include "../estd_device.h"

namespace {

constexpr int WG = 256;

__device__ __forceinline__ int parent_load(const int* parent, int v)
{
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v's tree as far as this lane can see.  Terminates whatever the loads return: a value read at parent[v] is <= v, the loop
// goes on only while it is < v, and indices are not negative -- at most v steps.  The result is v itself or a smaller member of v's
// tree; it was a root when the value read at it was stored, not necessarily now.
__device__ __forceinline__ int find_root(const int* parent, int v)
{
    int p = parent_load(parent, v);
    while (p != v) {
        v = p;
        p = parent_load(parent, v);
    }
    return v;
}

// find_root with path halving, for the hook kernel: every vertex on the way is pointed at its grandparent, so the chains that the first
// round of hooks builds (every lane starts on a forest of single vertices at once) are not walked at full length again.  The shortcut
// is an agent-scope atomicMin -- parent[v] only ever DEcreases -- and it is applied to v only after a read showed parent[v] = p != v, so
// v is no root and never becomes one again: a shortcut cannot undo or pre-empt a hook.  g was read at parent[p] and p at parent[v],
// so g is a member of v's tree and g < p < v: the invariant of the forest holds.  Termination as in find_root: v strictly decreases.
__device__ __forceinline__ int find_root_halving(int* parent, int v)
{
    int p = parent_load(parent, v);
    while (p != v) {
        const int g = parent_load(parent, p);
        if (g != p) atomicMin(parent + v, g);
        v = p;
        p = g;
    }
    return v;
}

// merge the trees of a and b.  Invariant: a and b are in the trees of the two vertices the call was given (each is replaced by an
// ancestor of itself only).  Termination: every iteration ends the loop (a == b: one tree already; or the CAS put root a under b < a),
// or replaces a, the larger of the two, by a strictly smaller index >= 0 -- the CAS failed, so it returned parent[a] != a, hence < a, and
// the search goes on from THAT value (find_root_halving only descends further).  a + b strictly decreases and is bounded below: no
// iteration waits for another lane, none repeats a state.  b need not be a root: hooking a root under any smaller member of the other
// tree keeps every path descending.  Every tree has exactly one root, its smallest member (all paths descend to it), so a root a and a
// smaller b are never in one tree: a successful CAS always merges two trees and removes exactly one root.
__device__ __forceinline__ void unite(int* parent, int a, int b)
{
    a = find_root_halving(parent, a);
    b = find_root_halving(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) break;
        a = find_root_halving(parent, old);
    }
}

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
