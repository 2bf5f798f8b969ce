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
//
// The kernel and the host walk live in radix_select.h, templated on the key: mi355_masked_order_stats_i32 (normal_structures.hip)
// runs them on int32 values.
//
// The batched form (mi355_masked_percentiles_multi) selects in up to 4 volumes that share the flag byte: each of the four passes
// is one launch over the voxels (pct_hist_multi_kernel) and one read-back for all volumes, and the host walk above runs per
// volume on that volume's part of the table.  A volume that selects nothing leaves after pass 0; the others go on.
#include <atomic>
#include <cstring>

#include "radix_select.h"

namespace mi355 {

__host__ __device__ __forceinline__ unsigned pct_key(unsigned bits) {
    if (bits == 0x80000000u) bits = 0;  // -0.0 == +0.0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
static inline unsigned pct_bits_of_key(unsigned key) { return (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key; }

// a float32 takes part when lo < x < hi; a NaN is counted on the side
struct FloatKey {
    __device__ static __forceinline__ int classify(unsigned bits, double lo, double hi, unsigned &key) {
        const float v = __uint_as_float(bits);
        if (v != v) return PCT_ASIDE;
        if (!(lo < (double)v && (double)v < hi)) return PCT_SKIPPED;
        key = pct_key(bits);
        return PCT_KEYED;
    }
};

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
    unsigned below[PCT_MAX_Q], above[PCT_MAX_Q];
    MI355_TRY(radix_select<FloatKey>("masked_percentiles", (const unsigned *)x_dev, n, flags_dev, require, forbid, lo, hi, q_host, nq, count_host, below, above,
                                     (hipStream_t)stream));
    if (count_host[0] == 0) return MI355_OK;
    for (int j = 0; j < nq; ++j) {
        const unsigned b = pct_bits_of_key(below[j]), a = pct_bits_of_key(above[j]);
        memcpy(below_host + j, &b, sizeof(float));
        memcpy(above_host + j, &a, sizeof(float));
    }
    return MI355_OK;
}

namespace mi355 {

// the host walk of radix_select for one volume of a batch
struct PctWalk {
    int nq = 0, nt = 0;
    bool live = true;
    int64_t m = 0;
    int64_t rank[PCT_MAX_GROUPS];
    unsigned prefix[PCT_MAX_GROUPS];
    int group[PCT_MAX_GROUPS];
    PctGroups groups;

    void start(int nq_) {
        nq = nq_;
        nt = 2 * nq_;
        groups.count = 1;
        groups.mask = 0;
        for (int g = 0; g < PCT_MAX_GROUPS; ++g) groups.prefix[g] = 0;
        for (int t = 0; t < PCT_MAX_GROUPS; ++t) { rank[t] = 0; prefix[t] = 0; group[t] = 0; }
    }
    void set_ranks(const double *q) {  // numpy's virtual index (m - 1) * true_divide(q, 100), in double
        for (int j = 0; j < nq; ++j) {
            const double v = (double)(m - 1) * (q[j] / 100.0);
            const int64_t r = (int64_t)floor(v);
            rank[2 * j] = r;
            rank[2 * j + 1] = r + 1 < m - 1 ? r + 1 : m - 1;
        }
    }
    int walk(const unsigned *h, int pass, int volume) {
        const int shift = 24 - 8 * pass;
        for (int t = 0; t < nt; ++t) {
            const unsigned *hist = h + group[t] * 256;
            int64_t below = 0;
            int d = 0;
            while (d < 255 && below + hist[d] <= rank[t]) below += hist[d++];
            MI355_REQUIRE(below + hist[d] > rank[t], "masked_percentiles_multi: volume %d, pass %d lost rank %lld (a volume or the flags changed during the call?)",
                          volume, pass, (long long)rank[t]);
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
        return MI355_OK;
    }
};

// LDS a workgroup may ask for, as the device reports it
static int lds_per_workgroup(size_t *bytes) {
    int dev = 0, v = 0;
    MI355_HIP(hipGetDevice(&dev));
    MI355_HIP(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    MI355_REQUIRE(v >= (int)((PCT_MAX_GROUPS * 256 + 1) * sizeof(unsigned)), "masked_percentiles_multi: the device offers %d bytes of LDS per workgroup, one volume needs %d",
                  v, (int)((PCT_MAX_GROUPS * 256 + 1) * sizeof(unsigned)));
    *bytes = (size_t)v;
    return MI355_OK;
}

}  // namespace mi355

// scratch slot SCR_MORPHOLOGY, per stream lane: the counters of a pass, launch after launch
extern "C" int mi355_masked_percentiles_multi(const float *const *x_dev, int nvol, int64_t n, const uint8_t *flags_dev, const int *require, const int *forbid,
                                              const double *lo, const double *hi, const double *const *q_host, const int *nq, int64_t *count_host,
                                              float *below_host, float *above_host, int *launches_host, void *stream) {
    MI355_REQUIRE(nvol >= 1 && nvol <= PCT_MAX_VOLUMES, "masked_percentiles_multi: nvol = %d (1..%d volumes per call)", nvol, PCT_MAX_VOLUMES);
    MI355_REQUIRE(x_dev && require && forbid && lo && hi && q_host && nq && count_host && below_host && above_host, "masked_percentiles_multi: null pointer");
    MI355_REQUIRE(n >= 1 && n < (1ll << 31), "masked_percentiles_multi: n = %lld (1 <= n < 2^31)", (long long)n);
    for (int v = 0; v < nvol; ++v) {
        MI355_REQUIRE(x_dev[v] && q_host[v], "masked_percentiles_multi: volume %d: null pointer", v);
        MI355_REQUIRE(nq[v] >= 1 && nq[v] <= PCT_MAX_Q, "masked_percentiles_multi: volume %d: nq = %d (1..%d percentiles per volume)", v, nq[v], PCT_MAX_Q);
        for (int j = 0; j < nq[v]; ++j)
            MI355_REQUIRE(q_host[v][j] >= 0.0 && q_host[v][j] <= 100.0, "masked_percentiles_multi: volume %d: percentile %d is %g (0..100, not NaN)", v, j,
                          q_host[v][j]);
        MI355_REQUIRE(!(lo[v] != lo[v]) && !(hi[v] != hi[v]), "masked_percentiles_multi: volume %d: a bound (lo, hi) is NaN", v);
        MI355_REQUIRE(require[v] >= 0 && require[v] <= 255 && forbid[v] >= 0 && forbid[v] <= 255 && !(require[v] & forbid[v]),
                      "masked_percentiles_multi: volume %d: require %d, forbid %d (masks of flag bits, 0..255, that share no bit)", v, require[v], forbid[v]);
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned *table = nullptr;
    MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, (size_t)PCT_MULTI_WORDS * sizeof(unsigned), (void **)&table));
    size_t lds_limit = 0;
    MI355_TRY(lds_per_workgroup(&lds_limit));
    static thread_local unsigned h[PCT_MULTI_WORDS];
    static std::atomic<size_t> lds_allowed{64 * 1024};  // what a launch may ask for without saying so first
    const unsigned blocks = (unsigned)((n + PCT_CHUNK - 1) / PCT_CHUNK);

    PctWalk walk[PCT_MAX_VOLUMES];
    for (int v = 0; v < nvol; ++v) {
        walk[v].start(nq[v]);
        count_host[2 * v] = count_host[2 * v + 1] = 0;
    }
    int launches = 0;
    for (int pass = 0; pass < 4; ++pass) {
        // the launches of the pass: the live volumes in order, a new launch where the next volume's groups no longer fit the LDS
        PctMultiArgs args[PCT_MAX_VOLUMES];
        int start[PCT_MAX_VOLUMES];    // first counter of the launch in the table
        int where[PCT_MAX_VOLUMES][2]; // volume -> (launch, place in it)
        int nl = 0, total = 0;
        for (int v = 0; v < nvol; ++v) {
            if (!walk[v].live) continue;
            const int bins = walk[v].groups.count * 256;
            if (nl == 0 || (size_t)(args[nl - 1].bins + bins + args[nl - 1].count + 1) * sizeof(unsigned) > lds_limit) {
                args[nl].count = 0;
                args[nl].bins = 0;
                ++nl;
            }
            PctMultiArgs &a = args[nl - 1];
            PctMultiVolume &mv = a.vol[a.count];
            mv.x = (const unsigned *)x_dev[v];
            mv.lo = lo[v];
            mv.hi = hi[v];
            mv.require = require[v];
            mv.forbid = forbid[v];
            mv.base = a.bins;
            mv.groups = walk[v].groups;
            where[v][0] = nl - 1;
            where[v][1] = a.count++;
            a.bins += bins;
        }
        if (nl == 0) break;  // nothing is selected in any volume
        for (int l = 0; l < nl; ++l) {
            start[l] = total;
            total += args[l].bins + args[l].count;
        }
        MI355_REQUIRE(total <= PCT_MULTI_WORDS, "masked_percentiles_multi: pass %d wants %d counters, the table holds %d", pass, total, PCT_MULTI_WORDS);
        MI355_HIP(hipMemsetAsync(table, 0, (size_t)total * sizeof(unsigned), s));
        for (int l = 0; l < nl; ++l) {
            const size_t lds = (size_t)(args[l].bins + args[l].count) * sizeof(unsigned);
            if (lds > lds_allowed.load()) {
                MI355_HIP(hipFuncSetAttribute((const void *)pct_hist_multi_kernel<FloatKey>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit));
                lds_allowed.store(lds_limit);
            }
            hipLaunchKernelGGL(pct_hist_multi_kernel<FloatKey>, dim3(blocks), dim3(256), lds, s, args[l], flags_dev, n, 24 - 8 * pass, pass == 0 ? 1 : 0,
                               table + start[l]);
            MI355_HIP(hipGetLastError());
            ++launches;
        }
        MI355_TRY(read_back(h, table, (size_t)total * sizeof(unsigned), s));
        for (int v = 0; v < nvol; ++v) {
            if (!walk[v].live) continue;
            const PctMultiArgs &a = args[where[v][0]];
            const unsigned *launch = h + start[where[v][0]];
            const unsigned *hist = launch + a.vol[where[v][1]].base;
            if (pass == 0) {
                int64_t m = 0;
                for (int d = 0; d < 256; ++d) m += hist[d];
                walk[v].m = count_host[2 * v] = m;
                count_host[2 * v + 1] = launch[a.bins + where[v][1]];
                if (m == 0) {  // this volume is done; the others go on
                    walk[v].live = false;
                    continue;
                }
                walk[v].set_ranks(q_host[v]);
            }
            MI355_TRY(walk[v].walk(hist, pass, v));
        }
    }
    for (int v = 0; v < nvol; ++v) {
        if (walk[v].m == 0) continue;
        for (int j = 0; j < nq[v]; ++j) {
            const unsigned b = pct_bits_of_key(walk[v].prefix[2 * j]), a = pct_bits_of_key(walk[v].prefix[2 * j + 1]);
            memcpy(below_host + v * PCT_MAX_Q + j, &b, sizeof(float));
            memcpy(above_host + v * PCT_MAX_Q + j, &a, sizeof(float));
        }
    }
    if (launches_host) *launches_host = launches;
    return MI355_OK;
}
