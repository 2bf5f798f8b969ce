// Ensemble uncertainty from the two moments the sliding window keeps (aggregate.hip, the M2 aggregation kernels): per-voxel
// standard deviation and entropy maps, and the per-channel counts and sums a region summary is built from.  The reference has no
// counterpart: its confidence (feature_extraction/step5_quality.py:457-500) is a table of literals that depend on nothing.
#include <cmath>
#include <cstring>
#include <vector>

#include "volume_common.h"

namespace mi355 {

constexpr int UNC_MAX_CH = 8;
constexpr int UNC_MAX_THR = 8;
constexpr int UNC_NSUM = 6;                    // sum of mean, var, entropy over all voxels, then over F = {mean > 0.5}
constexpr int UNC_NCNT = UNC_MAX_THR + 1;      // #{mean > t} per threshold, then |F|
constexpr int UNC_STATS_BLOCKS = 1024;

// -x log2 x with 0 log 0 = 0 (x in [0, 1]; a negative x, which only rounding could make, counts as 0)
__device__ __forceinline__ float plogp(float x) { return x > 0.f ? -x * log2f(x) : 0.f; }

struct UncMaps {
    const float *mean_a, *m2_a, *mean_b, *m2_b;  // *_b null: one member
    float *std_out, *ent_out;                    // [C][Z][Y][X], either may be null
    float *std_max, *ent_max;                    // [full], either may be null
};

// One thread per voxel of the crop box.  mean = (a + b) / 2 and m2 likewise for two members (the moments over the union of both
// members' samples), var = max(m2 - mean^2, 0) with the product rounded before the subtraction (no fused multiply-add: m2 = fl(mean^2)
// gives exactly 0), std = sqrt(var).  Entropy in bits: binary per channel for sigmoid heads; for softmax heads the categorical
// entropy over the channels divided by log2 C, the same value in every channel of ent_out.
__global__ void uncertainty_maps_kernel(UncMaps a, int C, int Z, int Y, int X, int softmax, float inv_log2c, int bz, int by, int bx, int FY, int FX) {
    const int64_t ZYX = (int64_t)Z * Y * X;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < ZYX; v += (int64_t)gridDim.x * blockDim.x) {
        float smax = 0.f, emax = 0.f, cat = 0.f;
        float ent[UNC_MAX_CH];
#pragma unroll
        for (int k = 0; k < UNC_MAX_CH; ++k) {
            ent[k] = 0.f;
            if (k >= C) continue;
            float mu = a.mean_a[k * ZYX + v], m2 = a.m2_a[k * ZYX + v];
            if (a.mean_b) {
                mu = (mu + a.mean_b[k * ZYX + v]) / 2.0f;
                m2 = (m2 + a.m2_b[k * ZYX + v]) / 2.0f;
            }
            const float sd = sqrtf(fmaxf(__fsub_rn(m2, __fmul_rn(mu, mu)), 0.f));
            if (a.std_out) a.std_out[k * ZYX + v] = sd;
            smax = fmaxf(smax, sd);
            if (softmax) cat += plogp(mu);
            else {
                ent[k] = fminf(fmaxf(plogp(mu) + plogp(1.0f - mu), 0.f), 1.0f);
                emax = fmaxf(emax, ent[k]);
            }
        }
        if (softmax) emax = fminf(fmaxf(cat * inv_log2c, 0.f), 1.0f);
        if (a.ent_out) {
#pragma unroll
            for (int k = 0; k < UNC_MAX_CH; ++k)
                if (k < C) a.ent_out[k * ZYX + v] = softmax ? emax : ent[k];
        }
        if (a.std_max || a.ent_max) {
            int z, y, x;
            coords(v, Y, X, z, y, x);
            const int64_t fi = ((int64_t)(z + bz) * FY + (y + by)) * FX + (x + bx);
            if (a.std_max) a.std_max[fi] = smax;
            if (a.ent_max) a.ent_max[fi] = emax;
        }
    }
}

struct UncThresholds {
    int n;
    float t[UNC_MAX_THR];
};

// Stage 1: block (b, c) reduces its grid-strided voxels of channel c to one slot of partials - sums [UNC_NSUM] fp64, counts
// [UNC_NCNT] int64, max var fp32 - through a fixed tree (wave_sum, then the four waves in order).  No atomics.
__global__ __launch_bounds__(256) void uncertainty_stats_kernel(const float *mean, const float *var, const float *ent, int64_t n, UncThresholds th,
                                                                double *psum, long long *pcnt, float *pmax) {
    const int c = blockIdx.y;
    const float *m = mean + c * n, *vr = var + c * n, *en = ent + c * n;
    double s[UNC_NSUM];
    long long k[UNC_NCNT];
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < UNC_NSUM; ++i) s[i] = 0.0;
#pragma unroll
    for (int i = 0; i < UNC_NCNT; ++i) k[i] = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float mu = m[i], va = vr[i], e = en[i];
        s[0] += (double)mu; s[1] += (double)va; s[2] += (double)e;
        if (mu > 0.5f) {  // strict, as regions_to_labels_kernel thresholds
            s[3] += (double)mu; s[4] += (double)va; s[5] += (double)e;
            k[UNC_MAX_THR] += 1;
        }
#pragma unroll
        for (int t = 0; t < UNC_MAX_THR; ++t)
            if (t < th.n && mu > th.t[t]) k[t] += 1;
        mx = fmaxf(mx, va);
    }
    __shared__ double ws[4][UNC_NSUM];
    __shared__ long long wk[4][UNC_NCNT];
    __shared__ float wm[4];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < UNC_NSUM; ++i) s[i] = wave_sum(s[i]);
#pragma unroll
    for (int i = 0; i < UNC_NCNT; ++i) k[i] = wave_sum(k[i]);
    for (int off = 1; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < UNC_NSUM; ++i) ws[wave][i] = s[i];
#pragma unroll
        for (int i = 0; i < UNC_NCNT; ++i) wk[wave][i] = k[i];
        wm[wave] = mx;
    }
    __syncthreads();
    const size_t slot = (size_t)c * gridDim.x + blockIdx.x;
    if (threadIdx.x < UNC_NSUM) psum[slot * UNC_NSUM + threadIdx.x] = ((ws[0][threadIdx.x] + ws[1][threadIdx.x]) + ws[2][threadIdx.x]) + ws[3][threadIdx.x];
    if (threadIdx.x < UNC_NCNT) pcnt[slot * UNC_NCNT + threadIdx.x] = wk[0][threadIdx.x] + wk[1][threadIdx.x] + wk[2][threadIdx.x] + wk[3][threadIdx.x];
    if (threadIdx.x == 0) pmax[slot] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}

// Stage 2: one wave per (channel, quantity) adds the block slots lane-strided in slot order, then the fixed tree.
// out_sum [C][UNC_NSUM + 1] (the last: max var), out_cnt [C][UNC_NCNT].
__global__ __launch_bounds__(64) void uncertainty_stats_finish_kernel(const double *psum, const long long *pcnt, const float *pmax, int nblocks, double *out_sum,
                                                                      long long *out_cnt) {
    const int c = blockIdx.x, q = blockIdx.y, lane = threadIdx.x;
    const size_t base = (size_t)c * nblocks;
    if (q < UNC_NSUM) {
        double a = 0.0;
        for (int b = lane; b < nblocks; b += 64) a += psum[(base + b) * UNC_NSUM + q];
        a = wave_sum(a);
        if (lane == 0) out_sum[c * (UNC_NSUM + 1) + q] = a;
    } else if (q == UNC_NSUM) {
        float a = 0.f;
        for (int b = lane; b < nblocks; b += 64) a = fmaxf(a, pmax[base + b]);
        for (int off = 1; off < 64; off <<= 1) a = fmaxf(a, __shfl_xor(a, off));
        if (lane == 0) out_sum[c * (UNC_NSUM + 1) + UNC_NSUM] = (double)a;
    } else {
        const int t = q - UNC_NSUM - 1;
        long long a = 0;
        for (int b = lane; b < nblocks; b += 64) a += pcnt[(base + b) * UNC_NCNT + t];
        a = wave_sum(a);
        if (lane == 0) out_cnt[c * UNC_NCNT + t] = a;
    }
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_uncertainty_maps(const float *mean_a, const float *m2_a, const float *mean_b, const float *m2_b, int C, int Z, int Y, int X, int nonlin,
                                      float *std_dev, float *entropy_dev, const int32_t bbox_lo[3], const int32_t full[3], float *std_max_dev,
                                      float *entropy_max_dev, void *stream) {
    MI355_REQUIRE(mean_a && m2_a && !mean_b == !m2_b, "uncertainty_maps: a member is its mean and its second moment");
    MI355_REQUIRE(C >= 1 && C <= UNC_MAX_CH, "uncertainty_maps: %d channels (1..%d)", C, UNC_MAX_CH);
    MI355_REQUIRE(nonlin == MI355_NONLIN_SIGMOID || nonlin == MI355_NONLIN_SOFTMAX,
                  "uncertainty_maps: nonlin %d has no probabilities (sigmoid or softmax)", nonlin);
    MI355_REQUIRE(std_dev || entropy_dev || std_max_dev || entropy_max_dev, "uncertainty_maps: no output asked for");
    int64_t V;
    MI355_TRY(check_volume("uncertainty_maps", Z, Y, X, &V));
    MI355_TRY(bind_device());
    hipStream_t s = (hipStream_t)stream;
    int FY = 0, FX = 0, lo[3] = {0, 0, 0};
    if (std_max_dev || entropy_max_dev) {
        MI355_REQUIRE(bbox_lo && full, "uncertainty_maps: the reduced maps need the crop box and the full shape");
        int64_t FV;
        MI355_TRY(check_volume("uncertainty_maps (full volume)", full[0], full[1], full[2], &FV));
        MI355_REQUIRE(bbox_lo[0] >= 0 && bbox_lo[1] >= 0 && bbox_lo[2] >= 0 && bbox_lo[0] + Z <= full[0] && bbox_lo[1] + Y <= full[1] &&
                          bbox_lo[2] + X <= full[2],
                      "uncertainty_maps: crop box does not fit the full volume");
        if (std_max_dev) MI355_HIP(hipMemsetAsync(std_max_dev, 0, (size_t)FV * sizeof(float), s));
        if (entropy_max_dev) MI355_HIP(hipMemsetAsync(entropy_max_dev, 0, (size_t)FV * sizeof(float), s));
        FY = full[1]; FX = full[2];
        for (int k = 0; k < 3; ++k) lo[k] = bbox_lo[k];
    }
    UncMaps a = {mean_a, m2_a, mean_b, m2_b, std_dev, entropy_dev, std_max_dev, entropy_max_dev};
    const float inv_log2c = C > 1 ? (float)(1.0 / std::log2((double)C)) : 0.f;
    hipLaunchKernelGGL(uncertainty_maps_kernel, dim3(grid_for(V, 256, 8192)), dim3(256), 0, s, a, C, Z, Y, X, nonlin == MI355_NONLIN_SOFTMAX ? 1 : 0,
                       inv_log2c, lo[0], lo[1], lo[2], FY, FX);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_uncertainty_stats(const float *mean_dev, const float *var_dev, const float *entropy_dev, int C, int64_t n,
                                       const float *thresholds_host, int n_thr, int64_t *counts_host, double *sums_host, void *stream) {
    MI355_REQUIRE(mean_dev && var_dev && entropy_dev && counts_host && sums_host && n >= 1, "uncertainty_stats: bad argument");
    MI355_REQUIRE(C >= 1 && C <= UNC_MAX_CH, "uncertainty_stats: %d channels (1..%d)", C, UNC_MAX_CH);
    MI355_REQUIRE(n_thr >= 0 && n_thr <= UNC_MAX_THR && (n_thr == 0 || thresholds_host), "uncertainty_stats: %d thresholds (0..%d)", n_thr, UNC_MAX_THR);
    UncThresholds th = {};
    th.n = n_thr;
    for (int i = 0; i < n_thr; ++i) {
        MI355_REQUIRE(thresholds_host[i] == thresholds_host[i], "uncertainty_stats: threshold %d is NaN", i);
        th.t[i] = thresholds_host[i];
    }
    MI355_TRY(bind_device());
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (int)grid_for(n, 256, UNC_STATS_BLOCKS);
    const size_t slots = (size_t)C * blocks;
    const size_t b_psum = slots * UNC_NSUM * sizeof(double), b_pcnt = slots * UNC_NCNT * sizeof(long long), b_pmax = pad256(slots * sizeof(float));
    const size_t b_osum = (size_t)C * (UNC_NSUM + 1) * sizeof(double), b_ocnt = (size_t)C * UNC_NCNT * sizeof(long long);
    // working memory of its own for the length of the call (a few hundred KiB; the call ends in a read-back anyway): the library's
    // scratch slots belong to the entry points that had them, and nothing here outlives the call
    DeviceAllocs mem;  // (freed on every exit: the read-back below has synchronised the stream by then)
    char *scr = nullptr;
    MI355_TRY(mem.alloc(b_psum + b_pcnt + b_pmax + b_osum + b_ocnt, &scr));
    double *psum = (double *)scr;
    long long *pcnt = (long long *)(scr + b_psum);
    float *pmax = (float *)(scr + b_psum + b_pcnt);
    double *osum = (double *)(scr + b_psum + b_pcnt + b_pmax);
    long long *ocnt = (long long *)(scr + b_psum + b_pcnt + b_pmax + b_osum);
    hipLaunchKernelGGL(uncertainty_stats_kernel, dim3((unsigned)blocks, (unsigned)C), dim3(256), 0, s, mean_dev, var_dev, entropy_dev, n, th, psum, pcnt, pmax);
    hipLaunchKernelGGL(uncertainty_stats_finish_kernel, dim3((unsigned)C, UNC_NSUM + 1 + UNC_NCNT), dim3(64), 0, s, (const double *)psum,
                       (const long long *)pcnt, (const float *)pmax, blocks, osum, ocnt);
    // one read-back: the sums [C][7] and the counts [C][9] lie next to each other
    std::vector<char> host(b_osum + b_ocnt);
    MI355_TRY(read_back(host.data(), osum, b_osum + b_ocnt, s));   // (synchronises the stream: the kernels are done with scr)
    memcpy(sums_host, host.data(), b_osum);
    const long long *cnt = (const long long *)(host.data() + b_osum);
    for (int c = 0; c < C; ++c) {  // thresholds first, then |F|
        for (int t = 0; t < n_thr; ++t) counts_host[c * (n_thr + 1) + t] = cnt[c * UNC_NCNT + t];
        counts_host[c * (n_thr + 1) + n_thr] = cnt[c * UNC_NCNT + UNC_MAX_THR];
    }
    return MI355_OK;
}
