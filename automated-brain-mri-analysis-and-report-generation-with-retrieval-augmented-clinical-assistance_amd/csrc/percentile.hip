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
