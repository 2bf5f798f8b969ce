// Surface distances between two label maps (what nnU-Net v1's evaluator reports beside Dice - the 95 % Hausdorff
// distance, the average symmetric surface distance - and the surface Dice): the surfaces of up to four regions of both maps in one
// pass, the exact squared PHYSICAL distance to the nearest surface voxel inside an index box, and an ordered gather of that map.
// brats_amd.evaluate takes the square roots and the order statistics on the host.
//
// All volumes are [d0][d1][d2] C-order with fewer than 2^31 voxels.  A box is [lo, hi) per axis inside the volume; the distance map
// is dense over the box, [hi0 - lo0][hi1 - lo1][hi2 - lo2] doubles.  No workgroup waits for another one: every ordering is a launch
// boundary.  Nothing here takes device scratch: the flag volume, the distance map, the gather's block counts and the count word
// are the caller's, and every word of them that is read was written by the same call before (no result depends on what they held).
//
// Squared distance = three separable passes over the fp64 map, in place - the decomposition of edt_axis{0,1,2}_kernel in
// morphology.hip (lower envelope by brute force over an LDS tile) with doubles and +infinity as the explicit "no site yet" value:
//   1  axis 0   a thread per (i1, i2) column of the box scans down and up: (steps to the nearest site of the column * spacing0)^2,
//               +inf while the column has none; lanes run along axis 2
//   2  axis 1   a workgroup stages an [n1][TX] tile (TX = 64 .. 8 neighbours along axis 2, SD_TILE_BYTES in all) and every thread
//               computes four outputs of one column per sweep: one conflict-free ds_read_b64 per four (multiply, multiply, add, min)
//   3  axis 2   a workgroup stages TY whole lines (one contiguous chunk of memory); a thread computes one output and reads the line
//               two entries at a time (ds_read_b128, the same address in every lane of a line: a broadcast)
// The value of a voxel is min over the sites y of fl(fl((D0 s0)^2 + (D1 s1)^2) + (D2 s2)^2), D = x - y: rounding is monotonic, so
// taking the minimum axis by axis is taking it over all sites, and the three terms are added in scipy's order (axis 0, 1, 2).  The
// file is compiled without contraction: an fma of the square into the sum would round once where scipy rounds twice.
// LDS: SD_TILE_BYTES = 32 KiB per workgroup of 256 threads, so five workgroups (20 waves) share the 160 KiB of a CU.
#include "volume_common.h"

#pragma clang fp contract(off)

namespace mi355 {

constexpr int SD_MAX_LINE = MI355_SURFACE_EDT_MAX_LINE;  // longest axis-1 / axis-2 line of a box: a [512][8] fp64 tile
constexpr int SD_TILE_BYTES = 32 * 1024;
constexpr int SD_GATHER_CHUNK = MI355_GATHER_CHUNK;      // box voxels per workgroup of the gather (8 per thread)
static_assert(SD_MAX_LINE * 8 * 8 == SD_TILE_BYTES && SD_MAX_LINE >= 256, "the axis-1 tile of the longest line is 8 columns wide");
static_assert(SD_GATHER_CHUNK % 256 == 0, "whole rounds of 256 threads");

struct RegionTables { uint8_t pred[256], gt[256]; };
struct Box { int lo[3], n[3]; };

__device__ __forceinline__ double sd_inf() { return __builtin_huge_val(); }

// volume index of box voxel (b0, b1, b2)
__device__ __forceinline__ int64_t box_to_volume(const Box &b, int d1, int d2, int b0, int b1, int b2) {
    return ((int64_t)(b.lo[0] + b0) * d1 + (b.lo[1] + b1)) * d2 + (b.lo[2] + b2);
}

// ------------------------------------------------------------------------------------------- surfaces
// flags[i] bit r (r = 0..3) = voxel i is in region r of the prediction and one of its six neighbours is not (a position outside
// the volume is not); bit 4 + r the same for the ground truth.  A region bit survives the AND over the neighbours where the voxel
// is interior, so surface = centre & ~(AND of the six): scipy's mask & ~binary_erosion(mask), border_value = 0, for eight masks at once.
__global__ __launch_bounds__(256) void region_surfaces_kernel(const uint8_t *pred, const uint8_t *gt, int d0, int d1, int d2, RegionTables tab,
                                                              uint8_t *flags) {
    __shared__ uint8_t tp[256], tg[256];
    tp[threadIdx.x] = tab.pred[threadIdx.x];
    tg[threadIdx.x] = tab.gt[threadIdx.x];
    __syncthreads();
    const int64_t V = (int64_t)d0 * d1 * d2;
    const int64_t s1 = d2, s0 = (int64_t)d1 * d2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        int z, y, x;
        coords(i, d1, d2, z, y, x);
        const int cp = tp[pred[i]], cg = tg[gt[i]];
        int ap = cp, ag = cg;  // bits of the regions that the voxel and all six neighbours belong to
        if (cp | cg) {
            const int64_t nb[6] = {x > 0 ? i - 1 : -1, x + 1 < d2 ? i + 1 : -1, y > 0 ? i - s1 : -1, y + 1 < d1 ? i + s1 : -1, z > 0 ? i - s0 : -1,
                                   z + 1 < d0 ? i + s0 : -1};
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                ap &= nb[k] >= 0 ? tp[pred[nb[k]]] : 0;
                ag &= nb[k] >= 0 ? tg[gt[nb[k]]] : 0;
            }
        }
        flags[i] = (uint8_t)((cp & ~ap) | ((cg & ~ag) << 4));
    }
}

// ------------------------------------------------------------------------------------------- squared distance to the flagged voxels
__global__ __launch_bounds__(256) void count_flagged_kernel(const uint8_t *flags, int d1, int d2, Box box, int select, unsigned *count) {
    const int64_t n = (int64_t)box.n[0] * box.n[1] * box.n[2];
    int c = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int b0, b1, b2;
        coords(i, box.n[1], box.n[2], b0, b1, b2);
        c += (flags[box_to_volume(box, d1, d2, b0, b1, b2)] & select) != 0;
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned)c);  // integers: the sum does not depend on the order
}

__global__ __launch_bounds__(256) void sd_axis0_kernel(const uint8_t *flags, int d1, int d2, Box box, int select, double s0, double *g) {
    const int plane = box.n[1] * box.n[2];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= plane) return;
    const int b1 = c / box.n[2], b2 = c - b1 * box.n[2];
    const uint8_t *f = flags + box_to_volume(box, d1, d2, 0, b1, b2);
    const int64_t fs = (int64_t)d1 * d2;
    double *col = g + c;
    int run = -1;  // steps since the last site of the column, -1 before the first
    for (int z = 0; z < box.n[0]; ++z) {
        run = (f[z * fs] & select) ? 0 : (run < 0 ? -1 : run + 1);
        col[(int64_t)z * plane] = (double)run;
    }
    run = -1;
    for (int z = box.n[0] - 1; z >= 0; --z) {
        const int down = (int)col[(int64_t)z * plane];
        run = down == 0 ? 0 : (run < 0 ? -1 : run + 1);
        const int d = down < 0 ? run : (run < 0 ? down : min(down, run));
        const double t = (double)d * s0;
        col[(int64_t)z * plane] = d < 0 ? sd_inf() : t * t;
    }
}

// g + (d * s)^2: two roundings for the square, one for the sum; +inf stays +inf
__device__ __forceinline__ double sd_min_plus(double acc, double g, int d, double s) {
    const double t = (double)d * s;
    return fmin(acc, g + t * t);
}

// in place: every workgroup reads its whole tile into LDS before it writes, and nobody else touches the tile
__global__ __launch_bounds__(256) void sd_axis1_kernel(double *g, int n1, int n2, int nbx, int tx_log2, double s1) {
    extern __shared__ __attribute__((aligned(16))) double sd_tile[];  // [n1][TX]
    const int TX = 1 << tx_log2;
    const int z = blockIdx.x / nbx, x0 = (blockIdx.x - z * nbx) * TX;
    double *base = g + (int64_t)z * n1 * n2;
    for (int i = threadIdx.x; i < n1 * TX; i += 256) {
        const int y = i >> tx_log2, x = x0 + (i & (TX - 1));
        sd_tile[i] = x < n2 ? base[(int64_t)y * n2 + x] : sd_inf();
    }
    __syncthreads();
    const int xl = threadIdx.x & (TX - 1), x = x0 + xl;
    const int groups = 256 >> tx_log2;
    for (int y0 = (threadIdx.x >> tx_log2) * 4; y0 < n1; y0 += groups * 4) {
        double a0 = sd_inf(), a1 = sd_inf(), a2 = sd_inf(), a3 = sd_inf();
        for (int j = 0; j < n1; ++j) {
            const double v = sd_tile[(j << tx_log2) + xl];
            const int d = y0 - j;
            a0 = sd_min_plus(a0, v, d, s1); a1 = sd_min_plus(a1, v, d + 1, s1); a2 = sd_min_plus(a2, v, d + 2, s1); a3 = sd_min_plus(a3, v, d + 3, s1);
        }
        if (x >= n2) continue;
        double *o = base + (int64_t)y0 * n2 + x;
        o[0] = a0;
        if (y0 + 1 < n1) o[n2] = a1;
        if (y0 + 2 < n1) o[2 * (int64_t)n2] = a2;
        if (y0 + 3 < n1) o[3 * (int64_t)n2] = a3;
    }
}

__global__ __launch_bounds__(256) void sd_axis2_kernel(double *g, int64_t lines, int n2, int pitch, int ty, double s2) {
    extern __shared__ __attribute__((aligned(16))) double sd_tile[];  // [ty][pitch], pitch = n2 rounded up to 2, the tail = +inf
    const int64_t line0 = (int64_t)blockIdx.x * ty;
    const int nl = (int)min((int64_t)ty, lines - line0);
    double *base = g + line0 * n2;
    const int n = nl * n2;
    for (int i = threadIdx.x; i < nl * pitch; i += 256) {
        const int l = i / pitch, x = i - l * pitch;
        sd_tile[i] = x < n2 ? base[l * n2 + x] : sd_inf();
    }
    __syncthreads();
    const double2 *tile2 = (const double2 *)sd_tile;
    const int p2 = pitch >> 1;
    for (int o = threadIdx.x; o < n; o += 256) {
        const int l = o / n2, x = o - l * n2;
        double acc = sd_inf();
        const double2 *row = tile2 + l * p2;
        for (int j2 = 0; j2 < p2; ++j2) {
            const double2 v = row[j2];
            const int d = x - 2 * j2;
            acc = sd_min_plus(acc, v.x, d, s2); acc = sd_min_plus(acc, v.y, d - 1, s2);
        }
        base[o] = acc;
    }
}

// ------------------------------------------------------------------------------------------- ordered gather
// Workgroup b owns box voxels [b * CHUNK, (b + 1) * CHUNK) in raster order, thread t of round r voxel b * CHUNK + r * 256 + t.
__device__ __forceinline__ bool gather_selected(const uint8_t *flags, int d1, int d2, const Box &box, int select, int64_t n, int64_t i) {
    if (i >= n) return false;
    int b0, b1, b2;
    coords(i, box.n[1], box.n[2], b0, b1, b2);
    return (flags[box_to_volume(box, d1, d2, b0, b1, b2)] & select) != 0;
}

__global__ __launch_bounds__(256) void gather_count_kernel(const uint8_t *flags, int d1, int d2, Box box, int select, unsigned *block_counts) {
    __shared__ int wred[4];
    const int64_t n = (int64_t)box.n[0] * box.n[1] * box.n[2];
    int c = 0;
    for (int r = 0; r < SD_GATHER_CHUNK / 256; ++r)
        c += gather_selected(flags, d1, d2, box, select, n, (int64_t)blockIdx.x * SD_GATHER_CHUNK + r * 256 + threadIdx.x);
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = (unsigned)(wred[0] + wred[1] + wred[2] + wred[3]);
}

// one workgroup: counts[0 .. n) -> their exclusive prefix sums in place, counts[n] = the total (64-bit carry, 32-bit results: the
// total is at most the number of box voxels, < 2^31)
__global__ __launch_bounds__(256) void gather_scan_kernel(unsigned *counts, int n) {
    __shared__ unsigned wsum[4];
    __shared__ unsigned carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        const unsigned v = i < n ? counts[i] : 0;
        unsigned incl = v;  // inclusive scan of the wave
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned up = __shfl_up(incl, m);
            if (lane >= m) incl += up;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        unsigned before = carry_s;
        for (int k = 0; k < w; ++k) before += wsum[k];
        if (i < n) counts[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) carry_s += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[n] = carry_s;
}

// out[offset of the block + number of selected voxels in front of this one inside the block] = the voxel's value: positions follow
// from counts alone, never from the order in which threads arrive
__global__ __launch_bounds__(256) void gather_scatter_kernel(const double *values, const uint8_t *flags, int d1, int d2, Box box, int select,
                                                             const unsigned *block_offsets, double *out) {
    __shared__ int wcnt[4];
    const int64_t n = (int64_t)box.n[0] * box.n[1] * box.n[2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned pos = block_offsets[blockIdx.x];
    for (int r = 0; r < SD_GATHER_CHUNK / 256; ++r) {
        const int64_t i = (int64_t)blockIdx.x * SD_GATHER_CHUNK + r * 256 + threadIdx.x;
        const bool on = gather_selected(flags, d1, d2, box, select, n, i);
        const unsigned long long mask = __ballot(on);
        if (lane == 0) wcnt[w] = __popcll(mask);
        __syncthreads();
        unsigned before = 0;
        for (int k = 0; k < w; ++k) before += wcnt[k];
        const unsigned total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (on) out[pos + before + __popcll(mask & ((1ull << lane) - 1ull))] = values[i];
        pos += total;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------- host
static inline int check_box(const char *what, int d0, int d1, int d2, const int32_t *lo, const int32_t *hi, Box *box, int64_t *n) {
    MI355_REQUIRE(lo && hi, "%s: null box", what);
    const int d[3] = {d0, d1, d2};
    for (int k = 0; k < 3; ++k) {
        MI355_REQUIRE(lo[k] >= 0 && lo[k] < hi[k] && hi[k] <= d[k], "%s: box [%d, %d) along axis %d of a %dx%dx%d volume", what, lo[k], hi[k], k, d0, d1, d2);
        box->lo[k] = lo[k];
        box->n[k] = hi[k] - lo[k];
    }
    *n = (int64_t)box->n[0] * box->n[1] * box->n[2];
    return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_region_surfaces(const uint8_t *pred_dev, const uint8_t *gt_dev, int d0, int d1, int d2, const uint8_t *pred_table256_host,
                                     const uint8_t *gt_table256_host, uint8_t *flags_dev, int64_t flags_bytes, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("region_surfaces", d0, d1, d2, &V));
    MI355_REQUIRE(pred_dev && gt_dev && pred_table256_host && gt_table256_host && flags_dev, "region_surfaces: null pointer");
    MI355_REQUIRE(flags_dev != pred_dev && flags_dev != gt_dev, "region_surfaces: the flag volume must not be one of the label maps");
    MI355_REQUIRE(flags_bytes >= V, "region_surfaces: the flag volume has %lld bytes, %dx%dx%d needs %lld", (long long)flags_bytes, d0, d1, d2, (long long)V);
    RegionTables tab;
    for (int i = 0; i < 256; ++i) {
        MI355_REQUIRE(pred_table256_host[i] <= 15 && gt_table256_host[i] <= 15, "region_surfaces: table entry %d names a region beyond the four (bits 0..3)", i);
        tab.pred[i] = pred_table256_host[i];
        tab.gt[i] = gt_table256_host[i];
    }
    MI355_TRY(bind_device());
    hipLaunchKernelGGL(region_surfaces_kernel, dim3(grid_for(V, 256, 16384)), dim3(256), 0, (hipStream_t)stream, pred_dev, gt_dev, d0, d1, d2, tab, flags_dev);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_edt_to_flagged_f64(const uint8_t *flags_dev, int d0, int d1, int d2, const int32_t *lo_host, const int32_t *hi_host, int select,
                                        const double *spacing_host, double *dist2_dev, int64_t dist2_capacity, uint32_t *count_dev, void *stream) {
    int64_t V = 0, n = 0;
    Box box;
    MI355_TRY(check_volume("edt_to_flagged_f64", d0, d1, d2, &V));
    MI355_REQUIRE(flags_dev && spacing_host && dist2_dev && count_dev, "edt_to_flagged_f64: null pointer");
    MI355_TRY(check_box("edt_to_flagged_f64", d0, d1, d2, lo_host, hi_host, &box, &n));
    MI355_REQUIRE(select >= 1 && select <= 255, "edt_to_flagged_f64: select %d (a mask of the flag bits that mark a site, 1..255)", select);
    for (int k = 0; k < 3; ++k)
        MI355_REQUIRE(spacing_host[k] > 0 && spacing_host[k] <= 1.7976931348623157e308, "edt_to_flagged_f64: spacing %g along axis %d (finite and positive)",
                      spacing_host[k], k);
    MI355_REQUIRE(box.n[1] <= SD_MAX_LINE && box.n[2] <= SD_MAX_LINE,
                  "edt_to_flagged_f64: a %dx%dx%d box: axes 1 and 2 may have %d entries at most (one line per LDS tile)", box.n[0], box.n[1], box.n[2], SD_MAX_LINE);
    MI355_REQUIRE(dist2_capacity >= n, "edt_to_flagged_f64: the distance map holds %lld doubles, the %dx%dx%d box needs %lld", (long long)dist2_capacity,
                  box.n[0], box.n[1], box.n[2], (long long)n);
    hipStream_t s = (hipStream_t)stream;
    MI355_TRY(bind_device());
    MI355_HIP(hipMemsetAsync(count_dev, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(count_flagged_kernel, dim3(grid_for(n, 256 * 16, 2048)), dim3(256), 0, s, flags_dev, d1, d2, box, select, (unsigned *)count_dev);
    unsigned sites = 0;
    MI355_TRY(read_back(&sites, count_dev, sizeof(unsigned), s));
    MI355_REQUIRE(sites > 0, "edt_to_flagged_f64: no site: no voxel of the %dx%dx%d box has a bit of select %d, there is no distance to measure", box.n[0],
                  box.n[1], box.n[2], select);
    const int plane = box.n[1] * box.n[2];
    hipLaunchKernelGGL(sd_axis0_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, flags_dev, d1, d2, box, select, spacing_host[0], dist2_dev);
    if (box.n[1] > 1) {
        int tx_log2 = 6;  // the widest tile of n1 rows within SD_TILE_BYTES: 64 columns up to 64 rows, 8 columns up to 512
        while (((size_t)box.n[1] << (tx_log2 + 3)) > (size_t)SD_TILE_BYTES) --tx_log2;
        const int nbx = ceil_div(box.n[2], 1 << tx_log2);  // nbx * n0 <= n < 2^31
        hipLaunchKernelGGL(sd_axis1_kernel, dim3((unsigned)nbx * (unsigned)box.n[0]), dim3(256), (size_t)box.n[1] << (tx_log2 + 3), s, dist2_dev, box.n[1],
                           box.n[2], nbx, tx_log2, spacing_host[1]);
    }
    if (box.n[2] > 1) {
        const int pitch = (box.n[2] + 1) & ~1;
        int ty = SD_TILE_BYTES / 8 / pitch;  // >= 8 lines
        ty = ty > 32 ? 32 : ty;
        const int64_t lines = (int64_t)box.n[0] * box.n[1];
        hipLaunchKernelGGL(sd_axis2_kernel, dim3((unsigned)((lines + ty - 1) / ty)), dim3(256), (size_t)ty * pitch * 8, s, dist2_dev, lines, box.n[2], pitch, ty,
                           spacing_host[2]);
    }
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_gather_flagged_f64(const double *values_dev, const uint8_t *flags_dev, int d0, int d1, int d2, const int32_t *lo_host,
                                        const int32_t *hi_host, int select, double *out_dev, int64_t capacity, uint32_t *block_counts_dev, int64_t block_words,
                                        int64_t *count_host, void *stream) {
    int64_t V = 0, n = 0;
    Box box;
    MI355_TRY(check_volume("gather_flagged_f64", d0, d1, d2, &V));
    MI355_REQUIRE(flags_dev && block_counts_dev && count_host && capacity >= 0 && (out_dev ? values_dev != nullptr : capacity == 0),
                  "gather_flagged_f64: null pointer or negative capacity");
    MI355_TRY(check_box("gather_flagged_f64", d0, d1, d2, lo_host, hi_host, &box, &n));
    MI355_REQUIRE(select >= 1 && select <= 255, "gather_flagged_f64: select %d (a mask of flag bits, 1..255)", select);
    const int nblocks = (int)((n + SD_GATHER_CHUNK - 1) / SD_GATHER_CHUNK);
    MI355_REQUIRE(block_words >= (int64_t)nblocks + 1, "gather_flagged_f64: %lld words for the block counts, the %dx%dx%d box needs %d (one per %d voxels and one)",
                  (long long)block_words, box.n[0], box.n[1], box.n[2], nblocks + 1, SD_GATHER_CHUNK);
    hipStream_t s = (hipStream_t)stream;
    MI355_TRY(bind_device());
    unsigned *counts = (unsigned *)block_counts_dev;
    hipLaunchKernelGGL(gather_count_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, flags_dev, d1, d2, box, select, counts);
    hipLaunchKernelGGL(gather_scan_kernel, dim3(1), dim3(256), 0, s, counts, nblocks);
    unsigned total = 0;
    MI355_TRY(read_back(&total, counts + nblocks, sizeof(unsigned), s));
    *count_host = (int64_t)total;
    if (!out_dev) return MI355_OK;  // a count-only call
    MI355_REQUIRE((int64_t)total <= capacity, "gather_flagged_f64: %u voxels are selected, the output holds %lld: nothing was written", total, (long long)capacity);
    if (total == 0) return MI355_OK;
    hipLaunchKernelGGL(gather_scatter_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, values_dev, flags_dev, d1, d2, box, select, (const unsigned *)counts, out_dev);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}
