// Device-side primitives shared by the kernel sources of libestd_hip.so (gfx950 only): each one is written here once, at global scope.
// Every function is __forceinline__, so a kernel compiles to the same code as with a private copy.  A helper that only one file uses
// stays in that file, and so do the kernel-specific constants (tile sizes, LDS budgets, the ESTD_* A/B switches and their notes).
// tests/test_kernel_helpers_cpu.py keeps the .hip files from defining any of these names again.
#ifndef ESTD_DEVICE_H
#define ESTD_DEVICE_H

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "estd_common.h"                        // estd_grid
#include "estd_hip.h"

// ---- vector types ----
typedef float f32x4 __attribute__((ext_vector_type(4)));            // an MFMA accumulator
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((__vector_size__(16)));    // the type raw_buffer_load_b128 returns (GCC vector)
typedef unsigned int u32x3 __attribute__((__vector_size__(12)));
typedef unsigned int u32x2 __attribute__((__vector_size__(8)));
typedef __bf16 bf16x8 __attribute__((__vector_size__(16)));         // the bf16 MFMA operand of the operand-split kernels
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr unsigned OOB_OFFSET = 0xFFFFFF00u;    // beyond num_records of any descriptor: loads return 0, stores are dropped

// ---- casts ----
__device__ __forceinline__ float4 as_float4(u32x4 v)
{
    // NB: __builtin_bit_cast(float, v[i]) on a vector element is miscompiled by this clang (every lane reads
    // element 0); a whole-object copy is the safe form.
    float4 f;
    __builtin_memcpy(&f, &v, 16);
    return f;
}
__device__ __forceinline__ float2 as_float2(u32x2 v) { float2 f; __builtin_memcpy(&f, &v, 8); return f; }
__device__ __forceinline__ u32x4 as_u32x4(float4 f) { u32x4 v; __builtin_memcpy(&v, &f, 16); return v; }

// ---- buffer descriptors: the name states the unit of the extent (a descriptor sized in the wrong unit either reaches past the
// buffer, where the hardware no longer clamps, or returns zeros for loads that are in range) ----
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_f32(const float* base, size_t elems)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)(elems * 4), 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_bytes(const void* base, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// Workgroup barrier that only orders LDS traffic.  __syncthreads() would also drain vmcnt, i.e. wait for the
// previous tile's output stores (and the in-flight prefetch) to complete on every tile.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- LDS swizzles ----
// byte offset of 16-byte chunk c of LDS voxel record v; CM = channels of a record: 32 -> 128-byte records, key (v >> 1) & 7;
// 16 -> 64-byte records, key (v >> 2) & 3
template <int CM>
__device__ __forceinline__ int lds_chunk_off(int v, int c)
{
    if (CM == 32) return v * 128 + ((c ^ ((v >> 1) & 7)) << 4);
    else          return v * 64 + ((c ^ ((v >> 2) & 3)) << 4);
}
// The swizzle key taken from the COLUMN of the haloed slice only -- (col >> 1) & 7; IN_W is even, so the bank half (voxel & 1) is the
// column's parity and the 8 even / 8 odd columns a fragment read touches still have 8 distinct keys -- which makes the byte offset of
// (row, col, chunk) = row * IN_W * 128 + f(col, chunk): the fragment reads of a tap loop then need one address register per (column
// tap, channel chunk) and immediates for the halo row and the depth slice, instead of one register per (row, column tap) plus an XOR
// per second-chunk read.
__device__ __forceinline__ int lds_colkey_off(int col, int c) { return col * 128 + ((c ^ ((col >> 1) & 7)) << 4); }

// ---- DPP row sums ----
// sum over the 16 lanes of a DPP row (every lane gets the total): two quad permutations + two row rotations, all folded into v_add_f32
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float v)
{
    v = dpp_add<0xB1>(v);      // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);      // quad_perm [2,3,0,1]
    v = dpp_add<0x124>(v);     // row_ror:4
    v = dpp_add<0x128>(v);     // row_ror:8
    return v;
}
// sum of a double over the 16 lanes of a DPP row, every lane gets the total: two quad permutations + two row rotations of the two
// dwords (v_mov_b32 with a DPP modifier: no LDS round trip) and one v_add_f64 per level
template <int CTRL>
__device__ __forceinline__ double dpp_add_f64(double v)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xf, 0xf, false);
    return v + __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double row16_sum_f64(double v)
{
    v = dpp_add_f64<0xB1>(v);      // quad_perm [1,0,3,2]
    v = dpp_add_f64<0x4E>(v);      // quad_perm [2,3,0,1]
    v = dpp_add_f64<0x124>(v);     // row_ror:4
    v = dpp_add_f64<0x128>(v);     // row_ror:8
    return v;
}

// ---- activations ----
// tanh x = 1 - 2 / (exp(2x) + 1) on the transcendental units (v_exp_f32, v_rcp_f32: 1 ulp each; five instructions instead of the device
// library's ~30).  Absolute error <= 2e-7 over the whole range (cancellation near 0 costs relative, not absolute accuracy); +-inf -> +-1.
__device__ __forceinline__ float tanh_fast(float x)
{
    const float t = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(t + 1.0f);
}
// sigmoid the same way: four instructions where expf + an IEEE division take ~20
__device__ __forceinline__ float sigmoid_fast(float v) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f)); }
// the activation of an epilogue that branches per output element; tanh is the device library's, as in the oracle ...
__device__ __forceinline__ float act_apply(float v, int act)
{
    if (act == ESTD_ACT_RELU) return v > 0.0f ? v : 0.0f;
    if (act == ESTD_ACT_TANH) return tanhf(v);
    return v;
}
// ... and with tanh_fast (csrc/conv3d_wino3.hip): a call site chooses its numerics by name
__device__ __forceinline__ float act_apply_fast(float v, int act)
{
    if (act == ESTD_ACT_RELU) return v > 0.0f ? v : 0.0f;
    if (act == ESTD_ACT_TANH) return tanh_fast(v);
    return v;
}

__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ---- 3 x bf16 operand split (csrc/conv3d_split_bf16.hip, csrc/conv2d_split_bf16.hip) ----
// x0, x1 -> three packed bf16 pairs with x = h + m + l (exact unless x is within 2^-24 of the bf16 range limits)
__device__ __forceinline__ void split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l)
{
    const bf16x2 hb = {(__bf16)x0, (__bf16)x1};
    h = __builtin_bit_cast(unsigned, hb);
    float r0 = x0 - __builtin_bit_cast(float, h << 16);
    float r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
    const bf16x2 mb = {(__bf16)r0, (__bf16)r1};
    m = __builtin_bit_cast(unsigned, mb);
    r0 -= __builtin_bit_cast(float, m << 16);
    r1 -= __builtin_bit_cast(float, m & 0xffff0000u);
    const bf16x2 lb = {(__bf16)r0, (__bf16)r1};
    l = __builtin_bit_cast(unsigned, lb);
}
// 8 channels (two float4) of one voxel -> LDS, one 16-byte write per piece (o1 - o0 = o2 - o1 = PIECE_BYTES for real items)
__device__ __forceinline__ void fill_item(char* smem, int o0, int o1, int o2, float4 a, float4 b)
{
    u32x4 h, m, l;
    unsigned th, tm, tl;
    split2(a.x, a.y, th, tm, tl); h[0] = th; m[0] = tm; l[0] = tl;
    split2(a.z, a.w, th, tm, tl); h[1] = th; m[1] = tm; l[1] = tl;
    split2(b.x, b.y, th, tm, tl); h[2] = th; m[2] = tm; l[2] = tl;
    split2(b.z, b.w, th, tm, tl); h[3] = th; m[3] = tm; l[3] = tl;
    *reinterpret_cast<u32x4*>(smem + o0) = h;
    *reinterpret_cast<u32x4*>(smem + o1) = m;
    *reinterpret_cast<u32x4*>(smem + o2) = l;
}
// compile-time tap index: a "#pragma unroll" loop gets peeled (some taps are special) and is then no longer fully unrolled
template <typename F, int... I>
__device__ __forceinline__ void for_each_tap(F&& f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}

// ---- reconstruction kernels ----
__device__ __forceinline__ float lerpf(float a, float b, float f) { return fmaf(f, b - a, a); }
// row j of a 3x4 matrix applied to (x, y, 1) z + column 3:  fma(z, fma(M0, x, fma(M1, y, M2)), M3)
__device__ __forceinline__ float project_row(const float* m, float x, float y, float z) { return fmaf(z, fmaf(m[0], x, fmaf(m[1], y, m[2])), m[3]); }
__device__ __forceinline__ bool depth_ok(float d, float z_near) { return d > z_near && d < __builtin_inff(); }          // false for a NaN

// ---- counter-based random numbers (csrc/mesh/mesh_sample.hip, csrc/register/global_register.hip) ----
// the finaliser of SplitMix64 (Steele, Lea, Flood 2014)
__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}
// two rounds over (seed, i, stream), all arithmetic modulo 2^64: no state, so element i is a function of (seed, i, stream) alone
__device__ __forceinline__ unsigned long long h64(unsigned long long seed, unsigned long long i, unsigned long long stream)
{
    return mix64(mix64(seed + (i + 1ull) * 0x9e3779b97f4a7c15ull) + (stream + 1ull) * 0xd1b54a32d192ed03ull);
}

// ---- never an address from a foreign index or a value that is no number ----
__device__ __forceinline__ bool in_range(int i, int V) { return (unsigned)i < (unsigned)V; }
__device__ __forceinline__ bool finite_f32(float v) { return v - v == 0.f; }

// ---- the uniform-grid search (csrc/cloud_nn.hip, csrc/cloud/cloud_knn.hip, csrc/mesh/mesh_distance.hip) ----
// The structure: a uniform grid (estd_grid, csrc/estd_common.h) with a dense cell table.  A CANDIDATE (a point, a triangle) is registered in
// every cell of its BOX OF CELLS, the product of the intervals cell_coord(low corner) .. cell_coord(high corner) of its bounding box per
// axis -- for a point the box of one cell.  The records of a cell are contiguous and the cells of one grid row follow each other:
// cell_start[key] .. cell_start[key + 1], key = (c_z dims_y + c_y) dims_x + c_x.  A query searches from ITS cell_coord; outside the grid's
// box that is the clamped cell.
//
// The walk: ring r = the cells at Chebyshev distance r from the query's cell, r = 0, 1, 2, ..., row by row: a row on the ring's z or y
// face is one range (x - r .. x + r), any other row contributes its two end cells.  It stops in front of ring r >= 2 when
//     LB_SCALE * ((r - 1) * cell)^2 > bound(),
// bound() = the d2 a candidate has to reach to change the result (it starts at r2 = max_dist^2, so max_dist bounds the search as well), and
// after ring r_max, the last one that meets the grid.
//
// Why nothing is skipped.  cell_coord is monotone in the coordinate, so every point of a candidate (a convex combination of what spans its
// bounding box) has per axis a cell coordinate inside the candidate's box of cells.  A candidate not met in rings 0 .. r - 1 has no cell
// within Chebyshev distance r - 1 of the query's cell; its box is a product of intervals, so along ONE axis the whole interval is r or
// more cells away.  With dims_j <= 1024 (ESTD_CLOUD_MAX_DIM, estd_grid_ok) the fp32 cell coordinate is off by at most
// 3 * 2^-24 * 1024 < 2^-12 cells from the real one, for the query and for the corner that bounds the box on that side, so every point of
// the candidate is at least (r - 1 - 2^-11) cell edges from the query along that axis -- also for a clamped query, which lies further
// out than its cell on the clamped axis, provided the candidates lie inside the grid's box (the host layer takes the box from them).
// LB_SCALE = 1 - 2^-5: the 2^-11 and the roundings of the bound need 1 - 2^-10, the margin is 32 times that.  The comparison is STRICT: a
// candidate whose d2 EQUALS bound() is still examined, so a rule that breaks ties by index sees every tie.  The result is then a function
// of the candidate set alone and the cell edge is a tuning parameter only.
constexpr float LB_SCALE = 0.96875f;            // 1 - 2^-5

// the clamped cell coordinate; the clamp is done in float so that a far query (or an infinite product) converts safely.  Never contracted,
// whatever the including file sets: keys, bins and searches have to agree on every bit (there is no multiply-add to fuse; this keeps it so)
__device__ __forceinline__ int cell_coord(float p, float lo, float inv_cell, int dim)
{
#pragma clang fp contract(off)
    const float t = floorf((p - lo) * inv_cell);
    return (int)fminf(fmaxf(t, 0.f), (float)(dim - 1));
}

// bound(): the d2 the lower bound is compared to, read anew in front of every ring; scan(k0, k1): visits the records of cells k0 .. k1 of
// one row (k0 <= k1, both inside the table)
template <typename Bound, typename Scan>
__device__ __forceinline__ void grid_ring_walk(const estd_grid& g, float qx, float qy, float qz, Bound&& bound, Scan&& scan)
{
    const int X = g.dims[0], Y = g.dims[1], Z = g.dims[2];
    const int cx = cell_coord(qx, g.lo[0], g.inv_cell, X);
    const int cy = cell_coord(qy, g.lo[1], g.inv_cell, Y);
    const int cz = cell_coord(qz, g.lo[2], g.inv_cell, Z);
    const int r_max = max(max(max(cx, X - 1 - cx), max(cy, Y - 1 - cy)), max(cz, Z - 1 - cz));      // the last ring that meets the grid
#pragma unroll 1
    for (int r = 0; r <= r_max; ++r) {
        if (r >= 2) {
            const float reach = (float)(r - 1) * g.cell;
            if (reach * reach * LB_SCALE > bound()) break;
        }
        const int z0 = max(cz - r, 0), z1 = min(cz + r, Z - 1), y0 = max(cy - r, 0), y1 = min(cy + r, Y - 1);
        const int xa = cx - r, xb = cx + r;
#pragma unroll 1
        for (int z = z0; z <= z1; ++z) {
            const bool z_face = z - cz == r || cz - z == r;
#pragma unroll 1
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * Y + y) * X;
                if (z_face || y - cy == r || cy - y == r) {
                    scan(row + max(xa, 0), row + min(xb, X - 1));
                } else {
                    if (xa >= 0) scan(row + xa, row + xa);
                    if (xb <= X - 1) scan(row + xb, row + xb);
                }
            }
        }
    }
}

// ---- the lock-free union-find (csrc/mesh/mesh_components.hip, csrc/cloud/cloud_cluster.hip) ----
// The forest.  parent[v] only ever holds v itself or a smaller member of v's tree, and it only ever decreases: an init launch stores v;
// a HOOK, the successful atomicCAS(&parent[a], a, b) with b < a, is the one store that joins two trees; a SHORTCUT, atomicMin(&parent[v],
// g) with g a member of v's tree below parent[v], joins nothing.  So every path strictly descends and ends at a root (parent[r] == r),
// the root is the smallest member of its tree, an element that has been hooked never becomes a root again, and once every edge is
// hooked the trees are the components: the labels do not depend on the order in which the lanes ran.
//
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed, so a hook kernel takes nothing from a load for
// granted: every write of parent[] is an agent-scope atomic (atomicCAS, atomicMin), every read a relaxed agent-scope atomic load (served
// by the L2, never the L1), and ANY value a read returns -- fresh or stale -- was stored at that address at some time, hence is v's own
// index or a smaller member of v's tree.  A stale read costs steps, never correctness: the one decision that takes effect is the CAS,
// which compares against the memory's value.  The launches are ordered by the stream; what one launch stored, the next one reads.
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

// find_root with path halving, for a hook kernel: every element on the way is pointed at its grandparent, so the chains that the first
// round of hooks builds (every lane starts on a forest of single elements at once) are not walked at full length again.  The shortcut
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

// merge the trees of a and b.  Invariant: a and b are in the trees of the two elements the call was given (each is replaced by an
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

#endif
