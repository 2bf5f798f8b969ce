// What the volume primitives (morphology.hip, quality.hip, mass_effect.hip, normal_structures.hip, components.hip) share: the
// argument checks and launch arithmetic of their entry points, the wave reductions and the index split of their kernels, and the
// read-back every entry point with a host result ends with (percentile.hip, extras.hip and radix_select.h take only that).
// Kernels stay in their files: device code is not linked across files, and a kernel defined here would be emitted once per file
// that includes it.  A helper that one file alone uses stays in that file.
#pragma once
#include "kernels.h"

namespace mi355 {

// ---- host ----------------------------------------------------------------------------------------------------------------
static inline int check_volume(const char *what, int d0, int d1, int d2, int64_t *V) {
    MI355_REQUIRE(d0 >= 1 && d1 >= 1 && d2 >= 1, "%s: bad shape %dx%dx%d", what, d0, d1, d2);
    *V = (int64_t)d0 * d1 * d2;
    MI355_REQUIRE(*V < (1ll << 31), "%s: %dx%dx%d has 2^31 voxels or more", what, d0, d1, d2);
    return MI355_OK;
}
// a selection of voxels by their flag byte: every bit of `require`, no bit of `forbid`
static inline int check_selection(const char *what, int require, int forbid) {
    MI355_REQUIRE(require >= 0 && require <= 255 && forbid >= 0 && forbid <= 255 && (require & forbid) == 0,
                  "%s: require %d, forbid %d (masks of flag bits, 0..255, that share no bit)", what, require, forbid);
    return MI355_OK;
}
// workgroups for n items, per_block each, between 1 and cap
static inline unsigned grid_for(int64_t n, int per_block, int64_t cap) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
static inline size_t pad256(size_t b) { return (b + 255) / 256 * 256; }
static inline int aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The tail of an entry point that hands a result to the host: the error of the launches before it, then the copy, then the wait
// for the copy - in this order, so that the host words are never read while the copy is in flight.
static inline int read_back(void *host, const void *dev, size_t bytes, hipStream_t s) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    MI355_HIP(e);
    return MI355_OK;
}

// ---- device --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);  // a fixed tree: the same bits in every lane, every run
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
// linear C-order index of a [d0][d1][d2] volume with fewer than 2^31 voxels -> its three coordinates
__device__ __forceinline__ void coords(int64_t i, int d1, int d2, int &c0, int &c1, int &c2) {
    const unsigned u = (unsigned)i;
    const unsigned zy = u / (unsigned)d2;
    c2 = (int)(u - zy * (unsigned)d2);
    c0 = (int)(zy / (unsigned)d1);
    c1 = (int)(zy - (unsigned)c0 * (unsigned)d1);
}

}  // namespace mi355
