// Axis profiles, box counts, ranked picks, the distance between two point sets and a masked minimum: the primitives behind the
// reference's step 2 (feature_extraction/step2_mass_effect.py) that morphology.hip, percentile.hip and quality.hip do not already
// cover - what that file gets from np.where(mask)[0].min() / .max() / .mean() and ndimage.center_of_mass of a half (:54-99), from
// `(tumor_mask & lobe_mask).sum()` over sliced lobe masks (:472-518), from indexing np.where with np.random.choice (:214-225) and
// from a Python loop over 1000 x 1000 distances (:227-232).  Nothing here knows about step 2.
//
// Conventions as in morphology.hip and quality.hip: volumes are [d0][d1][d2] C-order, a voxel is selected when its flag byte has
// every bit of `require` and no bit of `forbid`, no workgroup waits for another one, and every result is deterministic: there is
// no float in this file, counts and minima meet in integer atomics (which commute) or are combined in a fixed order (the scan).
//
// All kernels but the pair distance are one pass over one flag byte per voxel: a thread takes 16 consecutive voxels with one
// 16-byte load (byte loads when the pointer is not 16-byte aligned and on the last, partial group), turns them into a 16-bit
// mask and does nothing more where the mask is zero - most of a head volume.  Counters live in LDS (axis_counts, box_counts) or
// in registers and are flushed to global memory once per workgroup.
#include "volume_common.h"

namespace mi355 {
namespace me {

constexpr int VPT = 16;          // voxels per thread and step
constexpr int TILE = 256 * VPT;  // voxels per workgroup and step; the block of select_ranked
constexpr int SCAN = 256;        // block counts per segment of the scan
constexpr int MAX_SEGMENTS = 2048;  // 2^31 voxels / TILE / SCAN
constexpr int B_CHUNK = 2048;    // points of list b per workgroup of the pair distance

// (require and forbid share no bit: one comparison)
__device__ __forceinline__ unsigned picked(unsigned byte, unsigned require, unsigned both) { return (byte & both) == require ? 1u : 0u; }

// bit j = voxel i + j is selected, for the 16 voxels from i on that lie below n
__device__ __forceinline__ unsigned select16(const uint8_t *flags, int64_t i, int64_t n, bool vec, unsigned require, unsigned forbid) {
    const unsigned both = require | forbid;
    unsigned m = 0;
    if (vec && i + VPT <= n) {
        const uint4 q = *reinterpret_cast<const uint4 *>(flags + i);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int b = 0; b < 4; ++b) m |= picked((w[k] >> (8 * b)) & 255u, require, both) << (4 * k + b);
    } else {
        for (int j = 0; j < VPT && i + j < n; ++j) m |= picked(flags[i + j], require, both) << j;
    }
    return m;
}

// the coordinates of a voxel, moved forward through the C order
struct Walk {
    int c0, c1, c2;
    __device__ __forceinline__ void forward(int by, int d1, int d2) {
        c2 += by;
        while (c2 >= d2) {
            c2 -= d2;
            if (++c1 == d1) { c1 = 0; ++c0; }
        }
    }
};

// ------------------------------------------------------------------------------------------- axis counts
// hist = d0 + d1 + d2 LDS counters.  Axis 2 takes one LDS atomic per selected voxel; along axis 0 and 1 a thread's 16 voxels
// are a few runs, added once each.  A workgroup sees at most ceil(tiles / grid) * 4096 < 2^32 voxels.
__global__ __launch_bounds__(256) void axis_counts_kernel(const uint8_t *flags, unsigned require, unsigned forbid, int d0, int d1, int d2, int vec,
                                                          unsigned long long *counts) {
    extern __shared__ unsigned hist[];
    const int64_t V = (int64_t)d0 * d1 * d2, tiles = (V + TILE - 1) / TILE;
    const int nh = d0 + d1 + d2;
    for (int k = threadIdx.x; k < nh; k += 256) hist[k] = 0;
    __syncthreads();
    unsigned *h0 = hist, *h1 = hist + d0, *h2 = hist + d0 + d1;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t i = tile * TILE + (int64_t)threadIdx.x * VPT;
        unsigned m = i < V ? select16(flags, i, V, vec != 0, require, forbid) : 0u;
        if (!m) continue;
        Walk w;
        coords(i, d1, d2, w.c0, w.c1, w.c2);
        int a0 = w.c0, a1 = w.c1, prev = 0;
        unsigned n0 = 0, n1 = 0;
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            w.forward(j - prev, d1, d2);
            prev = j;
            if (w.c0 != a0 || w.c1 != a1) {
                if (n1) atomicAdd(h1 + a1, n1);
                n1 = 0; a1 = w.c1;
                if (w.c0 != a0) {
                    if (n0) atomicAdd(h0 + a0, n0);
                    n0 = 0; a0 = w.c0;
                }
            }
            atomicAdd(h2 + w.c2, 1u);
            ++n0; ++n1;
        }
        atomicAdd(h1 + a1, n1);
        atomicAdd(h0 + a0, n0);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nh; k += 256)
        if (hist[k]) atomicAdd(counts + k, (unsigned long long)hist[k]);
}

// ------------------------------------------------------------------------------------------- box counts
struct Boxes {
    int b[MI355_MAX_BOXES][6];  // lo0, hi0, lo1, hi1, lo2, hi2; the entries past nb are empty boxes
};

__global__ __launch_bounds__(256) void box_counts_kernel(const uint8_t *flags, unsigned require, unsigned forbid, int d0, int d1, int d2, int vec,
                                                         Boxes bx, int nb, unsigned long long *counts) {
    __shared__ unsigned wg[MI355_MAX_BOXES];
    const int64_t V = (int64_t)d0 * d1 * d2, tiles = (V + TILE - 1) / TILE;
    if (threadIdx.x < MI355_MAX_BOXES) wg[threadIdx.x] = 0;
    __syncthreads();
    int cnt[MI355_MAX_BOXES];
#pragma unroll
    for (int b = 0; b < MI355_MAX_BOXES; ++b) cnt[b] = 0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t i = tile * TILE + (int64_t)threadIdx.x * VPT;
        unsigned m = i < V ? select16(flags, i, V, vec != 0, require, forbid) : 0u;
        if (!m) continue;
        Walk w;
        coords(i, d1, d2, w.c0, w.c1, w.c2);
        int prev = 0;
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            w.forward(j - prev, d1, d2);
            prev = j;
#pragma unroll
            for (int b = 0; b < MI355_MAX_BOXES; ++b)
                cnt[b] += (w.c0 >= bx.b[b][0] && w.c0 < bx.b[b][1] && w.c1 >= bx.b[b][2] && w.c1 < bx.b[b][3] && w.c2 >= bx.b[b][4] && w.c2 < bx.b[b][5]) ? 1 : 0;
        }
    }
#pragma unroll
    for (int b = 0; b < MI355_MAX_BOXES; ++b) {
        const int r = wave_sum(cnt[b]);
        if ((threadIdx.x & 63) == 0 && r) atomicAdd(wg + b, (unsigned)r);
    }
    __syncthreads();
    if ((int)threadIdx.x < nb && wg[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)wg[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------- ranked picks
// block_count[b] = the selected voxels among [b * TILE, (b + 1) * TILE): one write per workgroup, no atomic
__global__ __launch_bounds__(256) void block_count_kernel(const uint8_t *flags, unsigned require, unsigned forbid, int64_t n, int vec, unsigned *block_count) {
    __shared__ int wred[4];
    const int64_t i = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * VPT;
    const int c = wave_sum(i < n ? (int)__popc(select16(flags, i, n, vec != 0, require, forbid)) : 0);
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (unsigned)(wred[0] + wred[1] + wred[2] + wred[3]);
}

// exclusive prefix of one value per thread over the 256 threads of a workgroup, and the total
__device__ __forceinline__ unsigned long long scan256(unsigned long long v, unsigned long long &total) {
    __shared__ unsigned long long s[SCAN];
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < SCAN; d <<= 1) {
        const unsigned long long a = t >= d ? s[t - d] : 0ull;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    total = s[SCAN - 1];
    return s[t] - v;
}

// level 1: offset[b] = the selected voxels in the blocks of b's segment before b; segment_sum[seg] = those of the segment
__global__ __launch_bounds__(256) void scan_blocks_kernel(const unsigned *block_count, int nblocks, unsigned *offset, unsigned *segment_sum) {
    const int b = blockIdx.x * SCAN + threadIdx.x;
    unsigned long long total;
    const unsigned long long excl = scan256(b < nblocks ? block_count[b] : 0u, total);
    if (b < nblocks) offset[b] = (unsigned)excl;  // a segment holds SCAN * TILE = 2^20 voxels
    if (threadIdx.x == 0) segment_sum[blockIdx.x] = (unsigned)total;
}

// level 2, one workgroup: segment_base[s] = the selected voxels before segment s, segment_base[nseg] = all of them
__global__ __launch_bounds__(256) void scan_segments_kernel(const unsigned *segment_sum, int nseg, unsigned long long *segment_base) {
    constexpr int PER = MAX_SEGMENTS / SCAN;
    unsigned v[PER];
    unsigned long long mine = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int s = threadIdx.x * PER + q;
        v[q] = s < nseg ? segment_sum[s] : 0u;
        mine += v[q];
    }
    unsigned long long total, run = scan256(mine, total);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int s = threadIdx.x * PER + q;
        if (s < nseg) segment_base[s] = run;
        run += v[q];
    }
    if (threadIdx.x == 0) segment_base[nseg] = total;
}

// one wave per rank (all of them below the total: the host has checked).  The owning block is the LAST one whose base does not
// exceed the rank (empty blocks share their base with the next block); inside it, four steps of 64 lanes x 16 voxels: popcount,
// inclusive wave scan, and the lane whose range holds the rank walks to its bit.  Same voxels per lane as block_count_kernel.
__global__ __launch_bounds__(64) void pick_kernel(const uint8_t *flags, unsigned require, unsigned forbid, int64_t n, int vec, const unsigned *offset,
                                                  const unsigned long long *segment_base, int nblocks, const long long *ranks, long long *index) {
    const unsigned long long r = (unsigned long long)ranks[blockIdx.x];
    int lo = 0, hi = nblocks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segment_base[mid / SCAN] + offset[mid] <= r) lo = mid; else hi = mid - 1;
    }
    int t = (int)(r - (segment_base[lo / SCAN] + offset[lo]));
    const int lane = threadIdx.x;
    for (int step = 0; step < TILE / (64 * VPT); ++step) {
        const int64_t i = (int64_t)lo * TILE + step * (64 * VPT) + lane * VPT;
        unsigned m = i < n ? select16(flags, i, n, vec != 0, require, forbid) : 0u;
        const int c = __popc(m);
        int incl = c;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        const int total = __shfl(incl, 63);
        if (t < total) {
            int skip = t - (incl - c);
            if (skip >= 0 && skip < c) {
                while (skip--) m &= m - 1;
                index[blockIdx.x] = i + (__ffs(m) - 1);
            }
            return;
        }
        t -= total;
    }
}

// ------------------------------------------------------------------------------------------- pair distance
// res[0] = min d^2 (starts as all ones), res[1] = nonzero when an index lies outside the volume.  grid (a in 256s, b in
// B_CHUNKs); the b points of a chunk pass through LDS 256 at a time.  T = unsigned when no axis exceeds 32768 (three squares
// below 2^30 each), else unsigned long long
template <typename T>
__global__ __launch_bounds__(256) void min_pair_kernel(const long long *a, int ka, const long long *b, int kb, int d0, int d1, int d2, unsigned long long *res) {
    __shared__ int sb[3][256];
    const int64_t V = (int64_t)d0 * d1 * d2;
    const int ia = blockIdx.x * 256 + threadIdx.x;
    int a0 = 0, a1 = 0, a2 = 0;
    bool live = ia < ka, bad = false;
    if (live) {
        const long long idx = a[ia];
        if (idx < 0 || idx >= V) { bad = true; live = false; }
        else coords(idx, d1, d2, a0, a1, a2);
    }
    const int b_lo = blockIdx.y * B_CHUNK, b_hi = min(kb, b_lo + B_CHUNK);
    T best = ~(T)0;
    for (int t0 = b_lo; t0 < b_hi; t0 += 256) {
        __syncthreads();
        const int ib = t0 + threadIdx.x;
        if (ib < b_hi) {
            const long long idx = b[ib];
            int c0 = 0, c1 = 0, c2 = 0;
            if (idx < 0 || idx >= V) bad = true;
            else coords(idx, d1, d2, c0, c1, c2);
            sb[0][threadIdx.x] = c0; sb[1][threadIdx.x] = c1; sb[2][threadIdx.x] = c2;
        }
        __syncthreads();
        const int cnt = min(256, b_hi - t0);
        if (live)
            for (int q = 0; q < cnt; ++q) {
                const int x = a0 - sb[0][q], y = a1 - sb[1][q], z = a2 - sb[2][q];
                const T d = (T)((T)(x * (long long)x) + (T)(y * (long long)y) + (T)(z * (long long)z));
                best = d < best ? d : best;
            }
    }
    unsigned long long wide = live ? (unsigned long long)best : ~0ull;
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned long long o = __shfl_xor(wide, m);
        wide = o < wide ? o : wide;
    }
    if ((threadIdx.x & 63) == 0 && wide != ~0ull) atomicMin(res, wide);
    if (bad) atomicOr(res + 1, 1ull);
}

// ------------------------------------------------------------------------------------------- masked minimum
// res[0] = the number of selected voxels, the low word of res[1] = the smallest key seen, key = value ^ 2^31 (unsigned order =
// signed order of the values; starts as all ones)
__global__ __launch_bounds__(256) void masked_min_kernel(const int *values, const uint8_t *flags, unsigned require, unsigned forbid, int64_t n, int vec,
                                                         unsigned long long *res) {
    const int64_t tiles = (n + TILE - 1) / TILE;
    unsigned best = ~0u;
    int cnt = 0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t i = tile * TILE + (int64_t)threadIdx.x * VPT;
        unsigned m = i < n ? select16(flags, i, n, vec != 0, require, forbid) : 0u;
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            const unsigned key = (unsigned)values[i + j] ^ 0x80000000u;
            best = key < best ? key : best;
            ++cnt;
        }
    }
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned o = __shfl_xor(best, m);
        best = o < best ? o : best;
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicAdd(res, (unsigned long long)cnt);
        atomicMin(reinterpret_cast<unsigned *>(res + 1), best);
    }
}

}  // namespace me
}  // namespace mi355

using namespace mi355;
using namespace mi355::me;

// scratch slot SCR_MASS_EFFECT, per stream lane: the result words of a call, and for a ranked pick [block counts | offsets |
// segment sums | segment bases | ranks]
extern "C" int mi355_axis_counts(const uint8_t *flags_dev, int require, int forbid, int d0, int d1, int d2, int64_t *counts_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("axis_counts", d0, d1, d2, &V));
    MI355_TRY(check_selection("axis_counts", require, forbid));
    MI355_REQUIRE(flags_dev && counts_host, "axis_counts: null pointer");
    MI355_REQUIRE(d0 <= MI355_AXIS_COUNTS_MAX && d1 <= MI355_AXIS_COUNTS_MAX && d2 <= MI355_AXIS_COUNTS_MAX,
                  "axis_counts: %dx%dx%d has an axis longer than %d (the three profiles are counted in 48 KiB of LDS)", d0, d1, d2, MI355_AXIS_COUNTS_MAX);
    hipStream_t s = (hipStream_t)stream;
    const int nh = d0 + d1 + d2;
    unsigned long long *counts = nullptr;
    MI355_TRY(device_scratch(SCR_MASS_EFFECT, s, (size_t)nh * sizeof(unsigned long long), (void **)&counts));
    MI355_HIP(hipMemsetAsync(counts, 0, (size_t)nh * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(axis_counts_kernel, dim3(grid_for(V, TILE, 1024)), dim3(256), (size_t)nh * sizeof(unsigned), s, flags_dev, (unsigned)require,
                       (unsigned)forbid, d0, d1, d2, aligned16(flags_dev), counts);
    MI355_TRY(read_back(counts_host, counts, (size_t)nh * sizeof(int64_t), s));
    return MI355_OK;
}

extern "C" int mi355_box_counts(const uint8_t *flags_dev, int require, int forbid, int d0, int d1, int d2, const int32_t *boxes_host, int nb,
                                int64_t *counts_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("box_counts", d0, d1, d2, &V));
    MI355_TRY(check_selection("box_counts", require, forbid));
    MI355_REQUIRE(flags_dev && boxes_host && counts_host, "box_counts: null pointer");
    MI355_REQUIRE(nb >= 1 && nb <= MI355_MAX_BOXES, "box_counts: %d boxes (1..%d)", nb, MI355_MAX_BOXES);
    const int dims[3] = {d0, d1, d2};
    Boxes bx;
    for (int b = 0; b < MI355_MAX_BOXES; ++b)
        for (int k = 0; k < 6; ++k) bx.b[b][k] = 0;
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < 3; ++k) {
            const int lo = boxes_host[b * 6 + 2 * k], hi = boxes_host[b * 6 + 2 * k + 1];
            MI355_REQUIRE(lo >= 0 && hi <= dims[k], "box_counts: box %d spans [%d, %d) on axis %d of length %d", b, lo, hi, k, dims[k]);
            bx.b[b][2 * k] = lo;
            bx.b[b][2 * k + 1] = hi;
        }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *counts = nullptr;
    MI355_TRY(device_scratch(SCR_MASS_EFFECT, s, 256, (void **)&counts));
    MI355_HIP(hipMemsetAsync(counts, 0, MI355_MAX_BOXES * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(box_counts_kernel, dim3(grid_for(V, TILE, 1024)), dim3(256), 0, s, flags_dev, (unsigned)require, (unsigned)forbid, d0, d1, d2,
                       aligned16(flags_dev), bx, nb, counts);
    MI355_TRY(read_back(counts_host, counts, (size_t)nb * sizeof(int64_t), s));
    return MI355_OK;
}

extern "C" int mi355_select_ranked(const uint8_t *flags_dev, int require, int forbid, int64_t n, const int64_t *ranks_host, int k,
                                   int64_t *index_dev, int64_t *count_host, void *stream) {
    MI355_REQUIRE(n >= 1 && n < (1ll << 31), "select_ranked: n = %lld (1..2^31-1)", (long long)n);
    MI355_TRY(check_selection("select_ranked", require, forbid));
    MI355_REQUIRE(flags_dev && ranks_host && index_dev && count_host, "select_ranked: null pointer");
    MI355_REQUIRE(k >= 1 && k <= MI355_MAX_POINTS, "select_ranked: %d ranks (1..%d)", k, MI355_MAX_POINTS);
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (int)((n + TILE - 1) / TILE), nseg = (nblocks + SCAN - 1) / SCAN;
    const size_t count_bytes = pad256((size_t)nblocks * sizeof(unsigned)), seg_bytes = pad256((size_t)nseg * sizeof(unsigned)),
                 base_bytes = pad256((size_t)(nseg + 1) * sizeof(unsigned long long));
    char *scr = nullptr;
    MI355_TRY(device_scratch(SCR_MASS_EFFECT, s, 2 * count_bytes + seg_bytes + base_bytes + (size_t)k * sizeof(long long), (void **)&scr));
    unsigned *block_count = (unsigned *)scr, *offset = (unsigned *)(scr + count_bytes), *segment_sum = (unsigned *)(scr + 2 * count_bytes);
    unsigned long long *segment_base = (unsigned long long *)(scr + 2 * count_bytes + seg_bytes);
    long long *ranks = (long long *)(scr + 2 * count_bytes + seg_bytes + base_bytes);
    const int vec = aligned16(flags_dev);
    hipLaunchKernelGGL(block_count_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, flags_dev, (unsigned)require, (unsigned)forbid, n, vec, block_count);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3((unsigned)nseg), dim3(256), 0, s, (const unsigned *)block_count, nblocks, offset, segment_sum);
    hipLaunchKernelGGL(scan_segments_kernel, dim3(1), dim3(256), 0, s, (const unsigned *)segment_sum, nseg, segment_base);
    unsigned long long m = 0;
    MI355_TRY(read_back(&m, segment_base + nseg, sizeof(m), s));
    count_host[0] = (int64_t)m;
    for (int j = 0; j < k; ++j)
        MI355_REQUIRE(ranks_host[j] >= 0 && (unsigned long long)ranks_host[j] < m, "select_ranked: rank %lld (entry %d) of %llu selected voxels",
                      (long long)ranks_host[j], j, m);
    hipError_t e = hipMemcpyAsync(ranks, ranks_host, (size_t)k * sizeof(long long), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pick_kernel, dim3((unsigned)k), dim3(64), 0, s, flags_dev, (unsigned)require, (unsigned)forbid, n, vec, (const unsigned *)offset,
                           (const unsigned long long *)segment_base, nblocks, (const long long *)ranks, (long long *)index_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    MI355_HIP(e);
    return MI355_OK;
}

extern "C" int mi355_min_pair_dist2(const int64_t *a_index_dev, int ka, const int64_t *b_index_dev, int kb, int d0, int d1, int d2,
                                    int64_t *min_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("min_pair_dist2", d0, d1, d2, &V));
    MI355_REQUIRE(a_index_dev && b_index_dev && min_host, "min_pair_dist2: null pointer");
    MI355_REQUIRE(ka >= 1 && ka <= MI355_MAX_POINTS && kb >= 1 && kb <= MI355_MAX_POINTS, "min_pair_dist2: lists of %d and %d points (1..%d each)", ka, kb,
                  MI355_MAX_POINTS);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *res = nullptr, h[2] = {0, 0};
    MI355_TRY(device_scratch(SCR_MASS_EFFECT, s, 256, (void **)&res));
    MI355_HIP(hipMemsetAsync(res, 0xFF, sizeof(unsigned long long), s));
    MI355_HIP(hipMemsetAsync(res + 1, 0, sizeof(unsigned long long), s));
    const dim3 grid((unsigned)((ka + 255) / 256), (unsigned)((kb + B_CHUNK - 1) / B_CHUNK));
    const long long *a = (const long long *)a_index_dev, *b = (const long long *)b_index_dev;
    if (d0 <= 32768 && d1 <= 32768 && d2 <= 32768)
        hipLaunchKernelGGL(min_pair_kernel<unsigned>, grid, dim3(256), 0, s, a, ka, b, kb, d0, d1, d2, res);
    else
        hipLaunchKernelGGL(min_pair_kernel<unsigned long long>, grid, dim3(256), 0, s, a, ka, b, kb, d0, d1, d2, res);
    MI355_TRY(read_back(h, res, sizeof(h), s));
    MI355_REQUIRE(h[1] == 0, "min_pair_dist2: an index lies outside the %dx%dx%d volume", d0, d1, d2);
    min_host[0] = (int64_t)h[0];
    return MI355_OK;
}

extern "C" int mi355_masked_min_i32(const int32_t *values_dev, const uint8_t *flags_dev, int require, int forbid, int64_t n, int32_t *min_host,
                                    int64_t *count_host, void *stream) {
    MI355_REQUIRE(n >= 1 && n < (1ll << 31), "masked_min_i32: n = %lld (1..2^31-1)", (long long)n);
    MI355_TRY(check_selection("masked_min_i32", require, forbid));
    MI355_REQUIRE(values_dev && flags_dev && min_host && count_host, "masked_min_i32: null pointer");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *res = nullptr, h[2] = {0, 0};
    MI355_TRY(device_scratch(SCR_MASS_EFFECT, s, 256, (void **)&res));
    MI355_HIP(hipMemsetAsync(res, 0, sizeof(unsigned long long), s));
    MI355_HIP(hipMemsetAsync(res + 1, 0xFF, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(masked_min_kernel, dim3(grid_for(n, TILE, 2048)), dim3(256), 0, s, (const int *)values_dev, flags_dev, (unsigned)require,
                       (unsigned)forbid, n, aligned16(flags_dev), res);
    MI355_TRY(read_back(h, res, sizeof(h), s));
    count_host[0] = (int64_t)h[0];
    if (h[0]) min_host[0] = (int32_t)((unsigned)(h[1] & 0xFFFFFFFFull) ^ 0x80000000u);
    return MI355_OK;
}
