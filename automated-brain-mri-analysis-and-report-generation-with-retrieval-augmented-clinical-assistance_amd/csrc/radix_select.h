// The radix select behind mi355_masked_percentiles (percentile.hip, float32 values) and mi355_masked_order_stats_i32
// (normal_structures.hip, int32 values): one histogram kernel and one host driver, templated on how a 32-bit word of the volume
// becomes an order-preserving 32-bit key.  The method is described at the top of percentile.hip.  Beside them the histogram kernel
// of the batched float32 select (mi355_masked_percentiles_multi), which shares PctGroups, wave_hist_add and the Key classifier.
#pragma once
#include <cmath>

#include "volume_common.h"

namespace mi355 {

constexpr int PCT_MAX_Q = 8;                    // percentiles per call
constexpr int PCT_MAX_GROUPS = 2 * PCT_MAX_Q;   // distinct prefixes per pass: below and above of each
constexpr int PCT_CHUNK = 8192;                 // voxels per workgroup (32 per thread)
constexpr int PCT_UNROLL = 4;                   // loads in flight per thread
constexpr int AGG_ROUNDS = 4;
constexpr int PCT_TABLE = PCT_MAX_GROUPS * 256 + 1;  // 16 x 256 counters and the side counter

struct PctGroups {
    int count;
    unsigned mask;                       // the digits found so far: the top 8 p bits (0 in pass 0)
    unsigned prefix[PCT_MAX_GROUPS];     // key & mask of each group, all different
};

// What a word of the volume is to the select: KEYED (it takes part, with this key), SKIPPED, or ASIDE (it does not take part and
// is counted on the side: a NaN, a negative integer)
enum { PCT_SKIPPED = 0, PCT_KEYED = 1, PCT_ASIDE = 2 };

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
// table[PCT_MAX_GROUPS * 256] += the words set ASIDE among the flag-selected voxels (pass 0 only: count_aside)
template <class Key>
__global__ __launch_bounds__(256) void pct_hist_kernel(const unsigned *x, const uint8_t *flags, int64_t n, int require, int forbid, double lo, double hi,
                                                       PctGroups groups, int shift, int count_aside, unsigned *table) {
    __shared__ unsigned hist[PCT_MAX_GROUPS * 256];
    __shared__ unsigned aside_count;
    const int bins = groups.count * 256;
    for (int i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
    if (threadIdx.x == 0) aside_count = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * PCT_CHUNK + threadIdx.x;
    int aside = 0;
    for (int it = 0; it < PCT_CHUNK / 256; it += PCT_UNROLL) {  // (no lane leaves the loop early: the ballots need the whole wave)
        unsigned bits[PCT_UNROLL];
        int f[PCT_UNROLL];
#pragma unroll
        for (int u = 0; u < PCT_UNROLL; ++u) {
            const int64_t i = base + (int64_t)(it + u) * 256;
            const bool in = i < n;
            bits[u] = in ? x[i] : 0u;
            f[u] = in ? (flags ? (int)flags[i] : 0) : -1;
        }
#pragma unroll
        for (int u = 0; u < PCT_UNROLL; ++u) {
            int slot = -1;
            if (f[u] >= 0 && (f[u] & require) == require && !(f[u] & forbid)) {
                unsigned key = 0;
                const int kind = Key::classify(bits[u], lo, hi, key);
                if (kind == PCT_ASIDE) {
                    aside += count_aside;
                } else if (kind == PCT_KEYED) {
                    const unsigned head = key & groups.mask;
                    for (int g = 0; g < groups.count; ++g)
                        if (head == groups.prefix[g]) slot = g * 256 + (int)((key >> shift) & 255u);
                }
            }
            wave_hist_add(hist, slot, lane);
        }
    }
    if (aside) atomicAdd(&aside_count, (unsigned)aside);
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256) {
        const unsigned h = hist[i];
        if (h) atomicAdd(table + i, h);
    }
    if (threadIdx.x == 0 && aside_count) atomicAdd(table + PCT_MAX_GROUPS * 256, aside_count);
}

// ---- the batched form: up to PCT_MAX_VOLUMES volumes of one length that share the flag byte (mi355_masked_percentiles_multi,
// percentile.hip).  One launch counts for all of them: a thread loads the flag byte of a voxel once and the word of a volume only
// when the byte passes that volume's flag test.  The histogram of a launch is the groups of its volumes one after the other
// (`base`), then one side counter per volume, in LDS and in the global table alike; LDS is dynamic and sized by those groups.
constexpr int PCT_MAX_VOLUMES = 4;
constexpr int PCT_MULTI_WORDS = PCT_MAX_VOLUMES * (PCT_MAX_GROUPS * 256 + 1);  // the most a pass can count

struct PctMultiVolume {
    const unsigned *x;
    double lo, hi;
    int require, forbid;
    int base;            // first counter of the volume's groups within the launch's histogram
    PctGroups groups;
};
struct PctMultiArgs {
    int count;           // volumes of this launch
    int bins;            // 256 x the groups of all of them; the side counter of volume v is counter bins + v
    PctMultiVolume vol[PCT_MAX_VOLUMES];
};

// table[vol[v].base + g * 256 + d] and table[bins + v]: what pct_hist_kernel counts, per volume of the launch.  Dynamic LDS:
// (bins + count) words.  Per wave, then per block, then one global integer atomic per nonzero counter, as pct_hist_kernel.
template <class Key>
__global__ __launch_bounds__(256) void pct_hist_multi_kernel(PctMultiArgs a, const uint8_t *flags, int64_t n, int shift, int count_aside, unsigned *table) {
    extern __shared__ unsigned multi_hist[];
    const int words = a.bins + a.count;
    for (int i = threadIdx.x; i < words; i += 256) multi_hist[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * PCT_CHUNK + threadIdx.x;
    int aside[PCT_MAX_VOLUMES] = {0, 0, 0, 0};
    int f[PCT_UNROLL], f_next[PCT_UNROLL];
#pragma unroll
    for (int u = 0; u < PCT_UNROLL; ++u) {
        const int64_t i = base + (int64_t)u * 256;
        f[u] = i < n ? (flags ? (int)flags[i] : 0) : -1;
    }
    for (int it = 0; it < PCT_CHUNK / 256; it += PCT_UNROLL) {  // (no lane leaves the loop early: the ballots need the whole wave)
        unsigned bits[PCT_MAX_VOLUMES][PCT_UNROLL];
        unsigned pass[PCT_MAX_VOLUMES];   // bit u: the flag byte of voxel u passes the volume's test
#pragma unroll
        for (int v = 0; v < PCT_MAX_VOLUMES; ++v) {
            pass[v] = 0;
            if (v < a.count) {            // (the same in every lane)
#pragma unroll
                for (int u = 0; u < PCT_UNROLL; ++u) {
                    const bool p = f[u] >= 0 && (f[u] & a.vol[v].require) == a.vol[v].require && !(f[u] & a.vol[v].forbid);
                    bits[v][u] = p ? a.vol[v].x[base + (int64_t)(it + u) * 256] : 0u;
                    pass[v] |= (unsigned)p << u;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PCT_UNROLL; ++u) {  // the flag bytes of the next round, in flight behind the words of this one
            const int64_t i = base + (int64_t)(it + PCT_UNROLL + u) * 256;
            f_next[u] = (it + PCT_UNROLL < PCT_CHUNK / 256 && i < n) ? (flags ? (int)flags[i] : 0) : -1;
        }
#pragma unroll
        for (int u = 0; u < PCT_UNROLL; ++u) {
#pragma unroll
            for (int v = 0; v < PCT_MAX_VOLUMES; ++v) {
                if (v < a.count) {
                    int slot = -1;
                    if (pass[v] >> u & 1u) {
                        unsigned key = 0;
                        const int kind = Key::classify(bits[v][u], a.vol[v].lo, a.vol[v].hi, key);
                        if (kind == PCT_ASIDE) {
                            aside[v] += count_aside;
                        } else if (kind == PCT_KEYED) {
                            const unsigned head = key & a.vol[v].groups.mask;
                            for (int g = 0; g < a.vol[v].groups.count; ++g)
                                if (head == a.vol[v].groups.prefix[g]) slot = a.vol[v].base + g * 256 + (int)((key >> shift) & 255u);
                        }
                    }
                    wave_hist_add(multi_hist, slot, lane);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PCT_UNROLL; ++u) f[u] = f_next[u];
    }
#pragma unroll
    for (int v = 0; v < PCT_MAX_VOLUMES; ++v)
        if (v < a.count && aside[v]) atomicAdd(&multi_hist[a.bins + v], (unsigned)aside[v]);
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += 256) {
        const unsigned h = multi_hist[i];
        if (h) atomicAdd(table + i, h);
    }
}

// count_host[0] = m, the voxels that take part, count_host[1] = the words set aside; below_key[j] / above_key[j] = the keys of
// rank floor(v) and min(floor(v) + 1, m - 1), v = (m - 1) * (q_host[j] / 100) in IEEE double as numpy forms it.  m = 0 leaves the
// keys untouched and succeeds.  The arguments have been checked by the caller.  Scratch slot SCR_MORPHOLOGY, per stream lane.
template <class Key>
int radix_select(const char *what, const unsigned *x_dev, int64_t n, const uint8_t *flags_dev, int require, int forbid, double lo, double hi,
                 const double *q_host, int nq, int64_t *count_host, unsigned *below_key, unsigned *above_key, hipStream_t s) {
    unsigned *table = nullptr;
    MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, (size_t)PCT_TABLE * sizeof(unsigned), (void **)&table));
    static thread_local unsigned h[PCT_TABLE];
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
        MI355_HIP(hipMemsetAsync(table, 0, (size_t)PCT_TABLE * sizeof(unsigned), s));
        hipLaunchKernelGGL(pct_hist_kernel<Key>, dim3(blocks), dim3(256), 0, s, x_dev, flags_dev, n, require, forbid, lo, hi, groups, shift, pass == 0 ? 1 : 0,
                           table);
        MI355_TRY(read_back(h, table, (size_t)PCT_TABLE * sizeof(unsigned), s));
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
            MI355_REQUIRE(below + hist[d] > rank[t], "%s: pass %d lost rank %lld (the volume or the flags changed during the call?)", what, pass,
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
        below_key[j] = prefix[2 * j];
        above_key[j] = prefix[2 * j + 1];
    }
    return MI355_OK;
}

}  // namespace mi355
