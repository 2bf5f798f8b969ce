// Exact masked order statistics of a float32 volume: what the reference gets from np.percentile
// (feature_extraction/utils.py:48-49, :57, :67; step2_mass_effect.py:179; step4_morphology.py:317-320; step5_quality.py:194-212;
// step6_normal_structures.py:48-50, :129, :207, :224, :313) after it has copied `data[mask]` out of the volume and sorted it.
//
// Radix select, most significant digit first, 8 bits per pass, on the order-preserving 32-bit key of a float: sign bit set ->
// all bits inverted, else the sign bit set; -0.0 takes the key of +0.0.  Nothing is sorted and no selected value is copied:
// every pass reads the volume and the flag byte again (5 bytes per voxel) and counts, per wanted rank, the voxels whose key
// starts with the digits found so far, by their next digit.  A call wants up to 16 ranks (below / above of 8 percentiles); ranks
// whose keys share the digits found so far share one 256-bin histogram ("group"), so a voxel adds to one bin at most.
//
//   pass 0   one group, no prefix: the histogram of the top digit of every selected voxel; its total is the count m from which
//            the host derives the ranks floor((m - 1) q / 100) and that + 1, in IEEE double as numpy does.  The NaN among the
//            voxels the flag test alone selects are counted on the side.
//   pass p   the host reads the table of pass p - 1 back (the call is synchronous anyway: it returns host values), walks each
//            rank's histogram to its bin, subtracts what lies below and extends the prefix: at most 16 prefixes for pass p.
//
// Counting: a workgroup owns a contiguous chunk of voxels, counts into LDS and adds its nonzero bins to the global table with
// integer atomics.  Integer adds commute, so two calls are bit-equal.  MR intensities put nearly every voxel of a wave into two
// or three bins of the top digit and a constant volume puts all of them into one bin in every pass; 64 LDS atomics on one word
// serialise.  So the lanes of a wave first agree on equal bins: up to AGG_ROUNDS times the first pending lane announces its
// bin, the lanes with that bin are counted by a ballot and ONE lane adds the count; what is still pending after that is
// spread over many bins and goes to LDS lane by lane.  A constant volume costs one round and one atomic per wave and load.
#include <cmath>
#include <cstring>

#include "kernels.h"

namespace mi355 {

constexpr int PCT_MAX_Q = 8;                    // percentiles per call
constexpr int PCT_MAX_GROUPS = 2 * PCT_MAX_Q;   // distinct prefixes per pass: below and above of each
constexpr int PCT_CHUNK = 8192;                 // voxels per workgroup (32 per thread)
constexpr int PCT_UNROLL = 4;                   // loads in flight per thread
constexpr int AGG_ROUNDS = 4;

struct PctGroups {
    int count;
    unsigned mask;                       // the digits found so far: the top 8 p bits (0 in pass 0)
    unsigned prefix[PCT_MAX_GROUPS];     // key & mask of each group, all different
};

__host__ __device__ __forceinline__ unsigned pct_key(unsigned bits) {
    if (bits == 0x80000000u) bits = 0;  // -0.0 == +0.0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
static inline unsigned pct_bits_of_key(unsigned key) { return (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key; }

// every lane of the wave calls this (slot < 0: nothing to add)
__device__ __forceinline__ void wave_hist_add(unsigned *hist, int slot, int lane) {
    bool pending = slot >= 0;
#pragma unroll
    for (int r = 0; r < AGG_ROUNDS; ++r) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;  // (the same in every lane)
        const int leader = __ffsll(act) - 1;
        const int s = __builtin_amdgcn_readlane(slot, leader);
        const unsigned long long same = __ballot(pending && slot == s);
        if (lane == leader) atomicAdd(&hist[s], (unsigned)__popcll(same));
        pending = pending && slot != s;
    }
    if (pending) atomicAdd(&hist[slot], 1u);
}

// table[g * 256 + d] += voxels of the block's chunk that are selected, whose key starts with prefix g and goes on with digit d;
// table[PCT_MAX_GROUPS * 256] += the NaN among the flag-selected voxels (pass 0 only: count_nan)
__global__ __launch_bounds__(256) void pct_hist_kernel(const float *x, const uint8_t *flags, int64_t n, int require, int forbid, double lo, double hi,
                                                       PctGroups groups, int shift, int count_nan, unsigned *table) {
    __shared__ unsigned hist[PCT_MAX_GROUPS * 256];
    __shared__ unsigned nan_count;
    const int bins = groups.count * 256;
    for (int i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
    if (threadIdx.x == 0) nan_count = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * PCT_CHUNK + threadIdx.x;
    int nans = 0;
    for (int it = 0; it < PCT_CHUNK / 256; it += PCT_UNROLL) {  // (no lane leaves the loop early: the ballots need the whole wave)
        unsigned bits[PCT_UNROLL];
        int f[PCT_UNROLL];
#pragma unroll
        for (int u = 0; u < PCT_UNROLL; ++u) {
            const int64_t i = base + (int64_t)(it + u) * 256;
            const bool in = i < n;
            bits[u] = in ? __float_as_uint(x[i]) : 0u;
            f[u] = in ? (flags ? (int)flags[i] : 0) : -1;
        }
#pragma unroll
        for (int u = 0; u < PCT_UNROLL; ++u) {
            int slot = -1;
            if (f[u] >= 0 && (f[u] & require) == require && !(f[u] & forbid)) {
                const float v = __uint_as_float(bits[u]);
                if (v != v) {
                    nans += count_nan;
                } else if (lo < (double)v && (double)v < hi) {
                    const unsigned key = pct_key(bits[u]);
                    const unsigned head = key & groups.mask;
                    for (int g = 0; g < groups.count; ++g)
                        if (head == groups.prefix[g]) slot = g * 256 + (int)((key >> shift) & 255u);
                }
            }
            wave_hist_add(hist, slot, lane);
        }
    }
    if (nans) atomicAdd(&nan_count, (unsigned)nans);
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256) {
        const unsigned h = hist[i];
        if (h) atomicAdd(table + i, h);
    }
    if (threadIdx.x == 0 && nan_count) atomicAdd(table + PCT_MAX_GROUPS * 256, nan_count);
}

}  // namespace mi355

using namespace mi355;

// scratch slot SCR_MORPHOLOGY, per stream lane: the table of 16 x 256 counters and the NaN counter
extern "C" int mi355_masked_percentiles(const float *x_dev, int64_t n, const uint8_t *flags_dev, int require, int forbid, double lo, double hi,
                                        const double *q_host, int nq, int64_t *count_host, float *below_host, float *above_host, void *stream) {
    MI355_REQUIRE(x_dev && q_host && count_host && below_host && above_host, "masked_percentiles: null pointer");
    MI355_REQUIRE(n >= 1 && n < (1ll << 31), "masked_percentiles: n = %lld (1 <= n < 2^31)", (long long)n);
    MI355_REQUIRE(nq >= 1 && nq <= PCT_MAX_Q, "masked_percentiles: %d percentiles (1..%d per call)", nq, PCT_MAX_Q);
    for (int j = 0; j < nq; ++j)
        MI355_REQUIRE(q_host[j] >= 0.0 && q_host[j] <= 100.0, "masked_percentiles: percentile %d is %g (0..100, not NaN)", j, q_host[j]);
    MI355_REQUIRE(!(lo != lo) && !(hi != hi), "masked_percentiles: a bound is NaN");
    MI355_REQUIRE(require >= 0 && require <= 255 && forbid >= 0 && forbid <= 255 && !(require & forbid),
                  "masked_percentiles: require %d, forbid %d (masks of flag bits, 0..255, that share no bit)", require, forbid);
    hipStream_t s = (hipStream_t)stream;
    constexpr int TABLE = PCT_MAX_GROUPS * 256 + 1;
    unsigned *table = nullptr;
    MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, (size_t)TABLE * sizeof(unsigned), (void **)&table));
    static thread_local unsigned h[TABLE];
    const unsigned blocks = (unsigned)((n + PCT_CHUNK - 1) / PCT_CHUNK);

    const int nt = 2 * nq;                // target t = 2 j: below of percentile j, 2 j + 1: above
    int64_t rank[PCT_MAX_GROUPS];         // rank among the voxels that share the target's prefix
    unsigned prefix[PCT_MAX_GROUPS];
    int group[PCT_MAX_GROUPS];
    PctGroups groups;
    groups.count = 1;
    groups.mask = 0;
    for (int g = 0; g < PCT_MAX_GROUPS; ++g) groups.prefix[g] = 0;
    for (int t = 0; t < nt; ++t) { rank[t] = 0; prefix[t] = 0; group[t] = 0; }

    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        MI355_HIP(hipMemsetAsync(table, 0, (size_t)TABLE * sizeof(unsigned), s));
        hipLaunchKernelGGL(pct_hist_kernel, dim3(blocks), dim3(256), 0, s, x_dev, flags_dev, n, require, forbid, lo, hi, groups, shift, pass == 0 ? 1 : 0, table);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h, table, (size_t)TABLE * sizeof(unsigned), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        MI355_HIP(e);
        if (pass == 0) {
            int64_t m = 0;
            for (int d = 0; d < 256; ++d) m += h[d];
            count_host[0] = m;
            count_host[1] = h[PCT_MAX_GROUPS * 256];
            if (m == 0) return MI355_OK;
            for (int j = 0; j < nq; ++j) {  // numpy's virtual index (m - 1) * true_divide(q, 100), in double
                const double v = (double)(m - 1) * (q_host[j] / 100.0);
                const int64_t r = (int64_t)floor(v);
                rank[2 * j] = r;
                rank[2 * j + 1] = r + 1 < m - 1 ? r + 1 : m - 1;
            }
        }
        for (int t = 0; t < nt; ++t) {
            const unsigned *hist = h + group[t] * 256;
            int64_t below = 0;
            int d = 0;
            while (d < 255 && below + hist[d] <= rank[t]) below += hist[d++];
            MI355_REQUIRE(below + hist[d] > rank[t], "masked_percentiles: pass %d lost rank %lld (the volume or the flags changed during the call?)", pass,
                          (long long)rank[t]);
            rank[t] -= below;
            prefix[t] |= (unsigned)d << shift;
        }
        groups.mask = 0xFFFFFFFFu << shift;
        groups.count = 0;
        for (int t = 0; t < nt; ++t) {
            int g = 0;
            while (g < groups.count && groups.prefix[g] != prefix[t]) ++g;
            if (g == groups.count) groups.prefix[groups.count++] = prefix[t];
            group[t] = g;
        }
    }
    for (int j = 0; j < nq; ++j) {
        const unsigned b = pct_bits_of_key(prefix[2 * j]), a = pct_bits_of_key(prefix[2 * j + 1]);
        memcpy(below_host + j, &b, sizeof(float));
        memcpy(above_host + j, &a, sizeof(float));
    }
    return MI355_OK;
}
