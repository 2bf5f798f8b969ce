// City-block distance transform, integer-valued flag predicates, int32 order statistics and a column-count maximum: the primitives
// behind the reference's step 6 (feature_extraction/step6_normal_structures.py) that components.hip, morphology.hip, percentile.hip
// and mass_effect.hip do not already cover - what that file gets from binary_dilation(mask, iterations=5 / 10) (:152, :215, :345),
// from comparing distance_transform_edt with two of its own percentiles (:206-210, :224), from `inferior_brain[:, :, k:] = False`
// (:306-308) and from np.max(np.sum(mask[:, y:, :], axis=0)) (:130-131).  Nothing here knows about step 6.
//
// The rules of morphology.hip hold: volumes are [d0][d1][d2] C-order, the lanes of a wave sit on adjacent addresses of axis 2 for
// every global access, no workgroup waits for another one (every ordering is a launch boundary), and every result is
// deterministic: there is no float in this file, every voxel of a map is written by one thread, and the two reductions meet in
// integer atomics, which commute.
//
// City-block (L1, taxicab) distance = what `iterations` steps of the 6-neighbour cross reach: dist <= n is binary_dilation(mask,
// iterations=n) and, measured to the background with everything outside the volume counted as background, dist > n is
// binary_erosion(mask, iterations=n), for every n at once.  L1 separates into one pass per axis, and along a line
// min_j(g[j] + |i - j|) is a forward and a backward running minimum, run = min(g[i], run + 1): O(line), in place, no min-plus loop.
//   axis 0, 1   a thread per column, lanes along axis 2; the axis-0 pass reads the mask instead of the map
//   axis 2      a workgroup stages whole lines in LDS (one contiguous chunk of memory, as edt_axis2_kernel does), a thread walks
//               one line there (the pitch is odd: the lanes of a wave read 64 different banks), and the chunk is written back
// Values are uint32 with CB_FAR = 2^30 (MI355_CITYBLOCK_FAR) for "no source anywhere": a finite distance is below d0 + d1 + d2
// <= 2^30 (checked), run + 1 is clamped to CB_FAR, so nothing wraps.
#include "radix_select.h"
#include "volume_common.h"

namespace mi355 {
namespace ns {

constexpr unsigned CB_FAR = MI355_CITYBLOCK_FAR;
constexpr int CB_TILE_WORDS = 16 * 1024;  // 64 KiB of LDS per workgroup of the axis-2 pass
constexpr int CB_MAX_LINES = 256;         // lines per workgroup: one thread each
constexpr int CB_COLUMN_THREADS = 64;     // one wave per workgroup of the column passes: a plane of 240 x 155 columns is 582 of them
constexpr int CB_AHEAD = 8;               // loads in flight per column

__device__ __forceinline__ unsigned cb_step(unsigned v, unsigned run) { return min(v, min(run + 1u, CB_FAR)); }

// column c = (o, i): the voxels base + k * stride, k < len, base = o * outer_stride + i.  Axis 0: one o, i over a plane; axis 1:
// o = i0, i = i2.  FIRST: the map is not read, a voxel starts at 0 where it is a source (to_foreground: the mask is nonzero;
// else: it is zero) and at CB_FAR elsewhere.  start = the running minimum a line begins with at either end: CB_FAR (nothing
// outside the volume) or 0 (a source just outside: the first voxel is at most 1 away from it).
template <bool FIRST>
__global__ __launch_bounds__(CB_COLUMN_THREADS) void cb_column_kernel(const uint8_t *mask, int to_foreground, unsigned *g, unsigned columns, unsigned inner,
                                                                      int64_t outer_stride, int len, int64_t stride, unsigned start) {
    const unsigned c = blockIdx.x * (unsigned)CB_COLUMN_THREADS + threadIdx.x;
    if (c >= columns) return;
    const unsigned o = c / inner;
    unsigned *col = g + (int64_t)o * outer_stride + (c - o * inner);
    const uint8_t *mcol = FIRST ? mask + (int64_t)o * outer_stride + (c - o * inner) : nullptr;
    // CB_AHEAD voxels are loaded before the first of them is stored: the running minimum is a dependent chain, the loads are not
    unsigned run = start;
    for (int k0 = 0; k0 < len; k0 += CB_AHEAD) {
        unsigned v[CB_AHEAD];
#pragma unroll
        for (int j = 0; j < CB_AHEAD; ++j) {
            const int64_t p = (int64_t)min(k0 + j, len - 1) * stride;
            v[j] = FIRST ? (((mcol[p] != 0) == (to_foreground != 0)) ? 0u : CB_FAR) : col[p];
        }
#pragma unroll
        for (int j = 0; j < CB_AHEAD; ++j)
            if (k0 + j < len) {
                run = cb_step(v[j], run);
                col[(k0 + j) * stride] = run;
            }
    }
    run = start;
    for (int k0 = len - 1; k0 >= 0; k0 -= CB_AHEAD) {
        unsigned v[CB_AHEAD];
#pragma unroll
        for (int j = 0; j < CB_AHEAD; ++j) v[j] = col[(int64_t)max(k0 - j, 0) * stride];
#pragma unroll
        for (int j = 0; j < CB_AHEAD; ++j)
            if (k0 - j >= 0) {
                run = cb_step(v[j], run);
                col[(k0 - j) * stride] = run;
            }
    }
}

// in place: every workgroup reads its lines into LDS before it writes, and nobody else touches them
__global__ __launch_bounds__(256) void cb_axis2_kernel(unsigned *g, int64_t lines, int d2, int pitch, int per_block, unsigned start) {
    extern __shared__ unsigned tile[];  // [per_block][pitch]
    const int64_t line0 = (int64_t)blockIdx.x * per_block;
    const int nl = (int)min((int64_t)per_block, lines - line0);
    unsigned *base = g + line0 * d2;
    const int n = nl * d2;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int l = i / d2;
        tile[l * pitch + (i - l * d2)] = base[i];
    }
    __syncthreads();
    if ((int)threadIdx.x < nl) {
        unsigned *row = tile + threadIdx.x * pitch;
        unsigned run = start;
        for (int x = 0; x < d2; ++x) { run = cb_step(row[x], run); row[x] = run; }
        run = start;
        for (int x = d2 - 1; x >= 0; --x) { run = cb_step(row[x], run); row[x] = run; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int l = i / d2;
        base[i] = tile[l * pitch + (i - l * d2)];
    }
}

// ------------------------------------------------------------------------------------------- flag predicates
__device__ __forceinline__ unsigned flag_i32(unsigned f, int v, unsigned bitmask, unsigned require, unsigned forbid, int lo, int hi) {
    const bool on = (f & require) == require && !(f & forbid) && lo <= v && v <= hi;
    return (f & ~bitmask) | (on ? bitmask : 0u);
}

// a thread takes 4 consecutive voxels: one 4-byte load of the flags and one 16-byte load of the values where both pointers are
// aligned for it (vec), byte and word loads otherwise and on the last, partial group
__global__ __launch_bounds__(256) void flag_from_i32_kernel(uint8_t *flags, unsigned bitmask, unsigned require, unsigned forbid, const int *values, int lo,
                                                            int hi, int64_t n, int vec) {
    const int64_t groups = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += (int64_t)gridDim.x * 256) {
        const int64_t i = q * 4;
        if (vec && i + 4 <= n) {
            const unsigned f = *reinterpret_cast<const unsigned *>(flags + i);
            const int4 v = *reinterpret_cast<const int4 *>(values + i);
            const unsigned r = flag_i32(f & 255u, v.x, bitmask, require, forbid, lo, hi) | flag_i32((f >> 8) & 255u, v.y, bitmask, require, forbid, lo, hi) << 8 |
                               flag_i32((f >> 16) & 255u, v.z, bitmask, require, forbid, lo, hi) << 16 | flag_i32(f >> 24, v.w, bitmask, require, forbid, lo, hi) << 24;
            *reinterpret_cast<unsigned *>(flags + i) = r;
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) flags[i + j] = (uint8_t)flag_i32(flags[i + j], values[i + j], bitmask, require, forbid, lo, hi);
        }
    }
}

struct Box { int lo[3], hi[3]; };  // half-open, clipped to the volume

__global__ __launch_bounds__(256) void flag_from_box_kernel(uint8_t *flags, unsigned bitmask, unsigned require, unsigned forbid, int d1, int d2, int64_t V, Box b) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        const unsigned u = (unsigned)i;
        const unsigned zy = u / (unsigned)d2;
        const int c2 = (int)(u - zy * (unsigned)d2), c0 = (int)(zy / (unsigned)d1), c1 = (int)(zy - (unsigned)c0 * (unsigned)d1);
        const unsigned f = flags[i];
        const bool on = (f & require) == require && !(f & forbid) && c0 >= b.lo[0] && c0 < b.hi[0] && c1 >= b.lo[1] && c1 < b.hi[1] && c2 >= b.lo[2] &&
                        c2 < b.hi[2];
        flags[i] = (uint8_t)((f & ~bitmask) | (on ? bitmask : 0u));
    }
}

// ------------------------------------------------------------------------------------------- column-count maximum
// The columns (i1, i2) with i1 >= i1_from are the last `columns` entries of a plane: a thread per column counts down axis 0, the
// lanes of a wave on adjacent addresses; *best = the largest count (starts at 0)
__global__ __launch_bounds__(256) void column_count_max_kernel(const uint8_t *flags, unsigned require, unsigned both, int d0, int64_t plane, int64_t first,
                                                               unsigned columns, unsigned *best) {
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    unsigned cnt = 0;
    if (c < columns) {
        const uint8_t *col = flags + first + c;
        for (int z = 0; z < d0; ++z) cnt += (col[z * plane] & both) == require ? 1u : 0u;
    }
    for (int m = 1; m < 64; m <<= 1) cnt = max(cnt, (unsigned)__shfl_xor((int)cnt, m));
    if ((threadIdx.x & 63) == 0 && cnt) atomicMax(best, cnt);
}

// ------------------------------------------------------------------------------------------- int32 order statistics
// a non-negative int32 is its own order-preserving key; a negative one is counted on the side (the call is then refused)
struct NonNegativeKey {
    __device__ static __forceinline__ int classify(unsigned bits, double, double, unsigned &key) {
        if (bits & 0x80000000u) return PCT_ASIDE;
        key = bits;
        return PCT_KEYED;
    }
};

static inline int check_flag_args(const char *what, int bit, int require, int forbid) {
    MI355_REQUIRE(bit >= 0 && bit < 8 && require >= 0 && require <= 255 && forbid >= 0 && forbid <= 255, "%s: bit %d, require %d, forbid %d", what, bit, require,
                  forbid);
    return MI355_OK;
}

}  // namespace ns
}  // namespace mi355

using namespace mi355;
using namespace mi355::ns;

extern "C" int mi355_cityblock_distance(const uint8_t *mask_dev, int d0, int d1, int d2, int to_foreground, int32_t *dist_dev, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("cityblock_distance", d0, d1, d2, &V));
    MI355_REQUIRE(mask_dev && dist_dev, "cityblock_distance: null pointer");
    MI355_REQUIRE((int64_t)d0 + d1 + d2 <= (int64_t)CB_FAR, "cityblock_distance: %dx%dx%d: a distance could reach the value that stands for 'no source' (2^30)", d0,
                  d1, d2);
    const int pitch = d2 | 1;
    MI355_REQUIRE(pitch <= CB_TILE_WORDS, "cityblock_distance: %dx%dx%d: axis 2 may have %d entries at most (one line per LDS tile)", d0, d1, d2,
                  CB_TILE_WORDS - 1);
    MI355_TRY(bind_device());
    hipStream_t s = (hipStream_t)stream;
    unsigned *g = (unsigned *)dist_dev;
    const int64_t plane = (int64_t)d1 * d2;
    const unsigned start = to_foreground ? CB_FAR : 0u;  // measured to the background, a source lies just outside every face
    hipLaunchKernelGGL(cb_column_kernel<true>, dim3((unsigned)((plane + CB_COLUMN_THREADS - 1) / CB_COLUMN_THREADS)), dim3(CB_COLUMN_THREADS), 0, s, mask_dev, to_foreground, g, (unsigned)plane, (unsigned)plane,
                       (int64_t)0, d0, plane, start);
    const int64_t columns1 = (int64_t)d0 * d2;
    hipLaunchKernelGGL(cb_column_kernel<false>, dim3((unsigned)((columns1 + CB_COLUMN_THREADS - 1) / CB_COLUMN_THREADS)), dim3(CB_COLUMN_THREADS), 0, s, (const uint8_t *)nullptr, to_foreground, g,
                       (unsigned)columns1, (unsigned)d2, plane, d1, (int64_t)d2, start);
    int per_block = CB_TILE_WORDS / pitch;
    per_block = per_block > CB_MAX_LINES ? CB_MAX_LINES : per_block;
    const int64_t lines = (int64_t)d0 * d1;
    hipLaunchKernelGGL(cb_axis2_kernel, dim3((unsigned)((lines + per_block - 1) / per_block)), dim3(256), (size_t)per_block * pitch * sizeof(unsigned), s, g, lines,
                       d2, pitch, per_block, start);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_flag_from_i32(uint8_t *flags_dev, int bit, int require, int forbid, const int32_t *values_dev, int32_t lo, int32_t hi, int64_t n,
                                   void *stream) {
    MI355_REQUIRE(flags_dev && values_dev && n >= 0, "flag_from_i32: bad argument");
    MI355_TRY(check_flag_args("flag_from_i32", bit, require, forbid));
    MI355_TRY(bind_device());
    const int vec = ((uintptr_t)flags_dev & 3) == 0 && ((uintptr_t)values_dev & 15) == 0;
    hipLaunchKernelGGL(flag_from_i32_kernel, dim3(grid_for(n, 1024, 8192)), dim3(256), 0, (hipStream_t)stream, flags_dev, 1u << bit, (unsigned)require,
                       (unsigned)forbid, (const int *)values_dev, lo, hi, n, vec);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_flag_from_box(uint8_t *flags_dev, int bit, int require, int forbid, int d0, int d1, int d2, const int32_t *box_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("flag_from_box", d0, d1, d2, &V));
    MI355_REQUIRE(flags_dev && box_host, "flag_from_box: null pointer");
    MI355_TRY(check_flag_args("flag_from_box", bit, require, forbid));
    const int dims[3] = {d0, d1, d2};
    Box b;
    for (int k = 0; k < 3; ++k) {  // clipped to the volume; lo >= hi on an axis: an empty box
        b.lo[k] = box_host[2 * k] < 0 ? 0 : box_host[2 * k];
        b.hi[k] = box_host[2 * k + 1] > dims[k] ? dims[k] : box_host[2 * k + 1];
    }
    MI355_TRY(bind_device());
    hipLaunchKernelGGL(flag_from_box_kernel, dim3(grid_for(V, 256, 8192)), dim3(256), 0, (hipStream_t)stream, flags_dev, 1u << bit, (unsigned)require,
                       (unsigned)forbid, d1, d2, V, b);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// scratch slot SCR_MORPHOLOGY, per stream lane: the table of the radix select (radix_select.h)
extern "C" int mi355_masked_order_stats_i32(const int32_t *values_dev, int64_t n, const uint8_t *flags_dev, int require, int forbid, const double *q_host, int nq,
                                            int64_t *count_host, int32_t *below_host, int32_t *above_host, void *stream) {
    MI355_REQUIRE(values_dev && q_host && count_host && below_host && above_host, "masked_order_stats_i32: null pointer");
    MI355_REQUIRE(n >= 1 && n < (1ll << 31), "masked_order_stats_i32: n = %lld (1 <= n < 2^31)", (long long)n);
    MI355_REQUIRE(nq >= 1 && nq <= PCT_MAX_Q, "masked_order_stats_i32: %d percentiles (1..%d per call)", nq, PCT_MAX_Q);
    for (int j = 0; j < nq; ++j)
        MI355_REQUIRE(q_host[j] >= 0.0 && q_host[j] <= 100.0, "masked_order_stats_i32: percentile %d is %g (0..100, not NaN)", j, q_host[j]);
    MI355_TRY(check_selection("masked_order_stats_i32", require, forbid));
    int64_t counts[2] = {0, 0};
    unsigned below[PCT_MAX_Q], above[PCT_MAX_Q];
    MI355_TRY(radix_select<NonNegativeKey>("masked_order_stats_i32", (const unsigned *)values_dev, n, flags_dev, require, forbid, 0.0, 0.0, q_host, nq, counts, below,
                                           above, (hipStream_t)stream));
    MI355_REQUIRE(counts[1] == 0, "masked_order_stats_i32: %lld of the selected values are negative (keys are the values in [0, 2^31))", (long long)counts[1]);
    count_host[0] = counts[0];
    if (counts[0] == 0) return MI355_OK;
    for (int j = 0; j < nq; ++j) {
        below_host[j] = (int32_t)below[j];
        above_host[j] = (int32_t)above[j];
    }
    return MI355_OK;
}

// scratch slot SCR_MORPHOLOGY, per stream lane: the result word
extern "C" int mi355_column_count_max(const uint8_t *flags_dev, int require, int forbid, int d0, int d1, int d2, int i1_from, int64_t *out_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("column_count_max", d0, d1, d2, &V));
    MI355_REQUIRE(flags_dev && out_host, "column_count_max: null pointer");
    MI355_TRY(check_selection("column_count_max", require, forbid));
    MI355_REQUIRE(i1_from >= 0, "column_count_max: i1_from %d (0 or more; at or above d1 = %d the slab is empty and the result 0)", i1_from, d1);
    out_host[0] = 0;
    if (i1_from >= d1) return MI355_OK;
    hipStream_t s = (hipStream_t)stream;
    unsigned *best = nullptr, h = 0;
    MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, 256, (void **)&best));
    MI355_HIP(hipMemsetAsync(best, 0, sizeof(unsigned), s));
    const int64_t plane = (int64_t)d1 * d2, first = (int64_t)i1_from * d2, columns = plane - first;
    hipLaunchKernelGGL(column_count_max_kernel, dim3((unsigned)((columns + 255) / 256)), dim3(256), 0, s, flags_dev, (unsigned)require, (unsigned)(require | forbid),
                       d0, plane, first, (unsigned)columns, best);
    MI355_TRY(read_back(&h, best, sizeof(unsigned), s));
    out_host[0] = (int64_t)h;
    return MI355_OK;
}
