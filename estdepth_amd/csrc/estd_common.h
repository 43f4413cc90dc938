// Shared helpers for the HIP translation units of libestd_hip.so (gfx950 only).
#ifndef ESTD_COMMON_H
#define ESTD_COMMON_H

#include <hip/hip_runtime.h>

#include "estd_hip.h"

#define ESTD_LAUNCH_CHECK() (hipGetLastError() == hipSuccess ? ESTD_OK : ESTD_ERR_LAUNCH)

static inline hipStream_t estd_stream(estd_stream_t s) { return static_cast<hipStream_t>(s); }

// Activation as a per-channel floor in the straight-line epilogues: out = fmaxf(v, floor) (one v_max_f32).  ReLU: floor 0.
// Activation "none": the floor is a quiet NaN -- v_max_f32 is IEEE maxNum, max(v, NaN) = v for every v and max(NaN, NaN) = NaN, so
// a NaN produced by the convolution still reaches the output as the reference's conv3d + BatchNorm would deliver it (with -inf as
// the floor a NaN came out as -inf).  Same instruction count.
#define ESTD_NO_FLOOR __builtin_nanf("")

// persistent-grid size of a kernel with `per_cu` resident workgroups per CU: the compute units of the CURRENT device (256 on an
// MI355X; queried once per device ordinal -- partitioned / other gfx950 parts report their own count) minus the reserve of
// estd_set_reserved_cus
extern "C" int estd_get_reserved_cus(void);
#include <atomic>
#include <stdio.h>
static inline int estd_device_cus(void)
{
    static std::atomic<int> cus[64];            // zero-initialised; 0 = not queried yet (relaxed: every thread would store the same value)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    int n = 0;
    const bool cached = (unsigned)dev < 64u;    // ordinals beyond the table are queried every time instead of aliasing a slot
    if (cached && (n = cus[dev].load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true))
            fprintf(stderr, "libestd_hip: hipDeviceGetAttribute(MultiprocessorCount) failed for device %d: persistent grids sized for 256 CUs\n", dev);
        return 256;                             // not cached: a later call may succeed
    }
    if (cached) cus[dev].store(n, std::memory_order_relaxed);
    return n;
}
static inline int estd_persistent_wgs(int per_cu)
{
    const int cus = estd_device_cus() - estd_get_reserved_cus();
    return (cus > 8 ? cus : 8) * per_cu;
}
// grid of a persistent kernel over `total` work items: one workgroup per item up to the resident ones; from 8 on a multiple of 8, which the
// kernels' XCD-aware blockIdx -> item mapping needs (a grid that is no multiple of 8 takes their plain mapping)
static inline int estd_persistent_grid(long long total, int per_cu)
{
    const int slots = estd_persistent_wgs(per_cu);
    int grid = total < slots ? (int)total : slots;
    if (grid >= 8) grid &= ~7;
    return grid;
}

// the buffer descriptors of the 3x3x3 kernels address ONE volume of the batch with 32-bit byte offsets: its widest record has to fit
static inline bool estd_conv3d_volume_fits_rsrc(const estd_conv3d_desc& d)
{
    const long long vox = (long long)d.D * d.H * d.W;
    const int widest = d.in_stride > d.out_stride ? d.in_stride : d.out_stride;
    return vox * widest * 4 < 0x7fffff00LL;
}

// read-back streams of a 3x3x3 epilogue (the kernels' RBK): 0 none; 1 = running sum only (out += result); 2 = residual (+ residual2) + scale; 3 = both
static inline int estd_conv3d_readback_kind(bool res_any, bool accumulate)
{
    return (!res_any && !accumulate) ? 0 : (!res_any ? 1 : (!accumulate ? 2 : 3));
}

// a positive finite float (false for a NaN)
static inline bool finite_pos(float v) { return v > 0.f && v < __builtin_inff(); }

// finite (false for a NaN and for either infinity)
static inline bool estd_finite(float v) { return v - v == 0.f; }

// ---- the uniform grid of the 3D back end: the host side of its one set of checks (the device side: csrc/estd_device.h) ----
// the reciprocal of the cell edge, formed here alone: keys, bins and searches multiply by the same fp32 value
static inline float estd_inv_cell(float cell) { return 1.0f / cell; }

// lo finite, cell and its fp32 reciprocal positive and finite, 1 <= dims_j <= max_dim, at most max_cells cells (0: no cap on the product)
static inline bool estd_grid_ok(const float* lo3, float cell, const int* dims3, int max_dim, long long max_cells)
{
    if (!lo3 || !dims3) return false;
    if (!estd_finite(cell) || !(cell > 0.f)) return false;
    const float inv = estd_inv_cell(cell);
    if (!estd_finite(inv) || !(inv > 0.f)) return false;
    for (int j = 0; j < 3; ++j)
        if (!estd_finite(lo3[j]) || dims3[j] < 1 || dims3[j] > max_dim) return false;
    return max_cells <= 0 || (long long)dims3[0] * dims3[1] * dims3[2] <= max_cells;
}

// what a ring search reads of its grid (grid_ring_walk, csrc/estd_device.h); a member of the search kernels' parameter blocks
struct estd_grid {
    int dims[3];
    float lo[3];
    float cell, inv_cell;
};

// The arguments the grid searches share -> ESTD_OK or ESTD_ERR_ARG.  max_dist positive and finite; *r2 = max_dist^2, formed here alone, finite
// (not a max_dist whose square leaves fp32); with n > 0 candidates in the cell table: the grid rules, `records` and `cell_start` given,
// `records` 16-byte aligned (a record is read with 16-byte loads), and *g filled.  With n == 0 *g stays as it is: the kernels never read it.
static inline int estd_search_args(float max_dist, long long n, const float* lo3, float cell, const int* dims3, const void* records,
                                   const int* cell_start, estd_grid* g, float* r2)
{
    if (!estd_finite(max_dist) || !(max_dist > 0.f)) return ESTD_ERR_ARG;
    *r2 = max_dist * max_dist;
    if (!estd_finite(*r2)) return ESTD_ERR_ARG;
    if (n > 0) {
        if (!estd_grid_ok(lo3, cell, dims3, ESTD_CLOUD_MAX_DIM, ESTD_CLOUD_MAX_CELLS)) return ESTD_ERR_ARG;
        if (!records || !cell_start || (reinterpret_cast<unsigned long long>(records) & 15ull)) return ESTD_ERR_ARG;
        g->cell = cell; g->inv_cell = estd_inv_cell(cell);
        for (int j = 0; j < 3; ++j) { g->lo[j] = lo3[j]; g->dims[j] = dims3[j]; }
    }
    return ESTD_OK;
}

// csrc/conv3d_wino2_c16.hip: the 16 -> 16 + head instance behind estd_conv3d_k3_wino2 (arguments validated by the caller)
int estd_wino2_c16_launch(const estd_conv3d_desc& d, hipStream_t stream);

static inline int estd_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (function, device): raise it once per device ordinal and
// kernel instantiation.  One atomic bit mask per instantiation -- thread-safe, and correct when a process drives
// several devices (launches under graph capture find the bit already set by the warm-up launch).
template <auto Kernel>
static inline void estd_allow_dynamic_lds(int bytes)
{
    static std::atomic<unsigned long long> done{0ull};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        done.fetch_or(bit, std::memory_order_release);
    }
}

#endif
