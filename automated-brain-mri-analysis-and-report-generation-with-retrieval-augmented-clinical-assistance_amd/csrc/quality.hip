// Hole filling, Sobel gradient statistics, radial shells and face slabs: the primitives behind the reference's step 5
// (feature_extraction/step5_quality.py) that components.hip, morphology.hip and percentile.hip do not already cover - what that
// file gets from scipy.ndimage.binary_fill_holes (:103), three scipy.ndimage.sobel passes over a float64 copy of T1 (:413-416),
// np.where + a distance per brain voxel (:280-300) and `t1_data[:5].max() > 0` on four faces (:385-390).  Nothing here knows
// about step 5.
//
// Conventions as in morphology.hip: volumes are [d0][d1][d2] C-order, a uint8 mask is foreground where nonzero, no workgroup
// waits for another one, and every result is deterministic:
//   * masks are written by exactly one thread per voxel;
//   * integer reductions (filled voxels, face counts, the maximum of non-negative doubles taken on their bit patterns) meet in
//     integer atomics, which commute;
//   * fp64 sums never meet in an atomic: a thread owns fixed voxels, a workgroup reduces its threads in a fixed tree and writes
//     ONE partial, and one wave sums the partials in a fixed order.
//
// Fill holes = label the COMPLEMENT with the union-find of components.hip at connectivity 1 (mi355_label_components, called
// through), mark every component that owns a voxel on one of the six faces, and write mask | (background whose component is
// unmarked).  One labelling whatever the shape of the channels: there is no sweep that repeats until nothing changes, hence no
// round count to cap.  Per voxel: 1 B read + 1 B written (complement), the labelling's own traffic, 4 B read on the faces
// (mark), 5 B read + 1 B written (write-out).
//
// Contraction is off for the whole file: numpy rounds every square of `(c - centre)**2` before it adds them, and a fused
// multiply-add in shell_dist would move max_dist by an ulp.
#include <cstring>

#include "volume_common.h"

#pragma clang fp contract(off)

namespace mi355 {
namespace qc {

// (sum_columns_kernel repeats morphology.hip's sum_partials_kernel: device code is not linked across files)
constexpr int RED_CHUNK = 8192;  // voxels per workgroup in the fp64 reductions (32 per thread)

// partial[block][ncols] -> out[k] = the sum of column k: lane l adds rows l, l + 64, ... in that order, then the wave's fixed
// butterfly.  grid ncols, one wave each
__global__ __launch_bounds__(64) void sum_columns_kernel(const double *partial, int nblocks, int ncols, double *out) {
    const int k = blockIdx.x;
    double s = 0;
    for (int b = threadIdx.x; b < nblocks; b += 64) s += partial[(int64_t)b * ncols + k];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[k] = s;
}

// NCOLS per-thread values -> partial[block * NCOLS + k], the waves of the workgroup added in the order 0, 1, 2, 3
template <int NCOLS>
__device__ __forceinline__ void block_partial(const double (&v)[NCOLS], double *partial) {
    __shared__ double wred[4][NCOLS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NCOLS; ++k) {
        const double r = wave_sum(v[k]);
        if (lane == 0) wred[w][k] = r;
    }
    __syncthreads();
    if (threadIdx.x < NCOLS)
        partial[(int64_t)blockIdx.x * NCOLS + threadIdx.x] = ((wred[0][threadIdx.x] + wred[1][threadIdx.x]) + wred[2][threadIdx.x]) + wred[3][threadIdx.x];
}

// ------------------------------------------------------------------------------------------- fill holes
__global__ void complement_kernel(const uint8_t *mask, int64_t V, uint8_t *comp) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) comp[i] = mask[i] == 0;
}

// mark[l] = 1 for every component l of the complement with a voxel on a face of the volume (an OR: order cannot matter).  The
// relaxed load spares the atomic once the word is set: the outside of a brain owns nearly every face voxel.  (Measured: 0.43 ms
// per 240 x 240 x 155 volume all the same, the loads and the first atomics queue on that one word.)
__global__ void face_mark_kernel(const int *labels, int d0, int d1, int d2, int n, unsigned *mark) {
    const int64_t V = (int64_t)d0 * d1 * d2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
        int c0, c1, c2;
        coords(i, d1, d2, c0, c1, c2);
        if (c0 && c0 != d0 - 1 && c1 && c1 != d1 - 1 && c2 && c2 != d2 - 1) continue;
        const int l = labels[i];
        if (l < 1 || l > n) continue;
        if (__hip_atomic_load(mark + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(mark + l, 1u);
    }
}

__global__ __launch_bounds__(256) void fill_write_kernel(const uint8_t *mask, const int *labels, const unsigned *mark, int n, int64_t V,
                                                         uint8_t *out, unsigned long long *filled) {
    int cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        const bool fg = mask[i] != 0;
        const int l = labels[i];
        const bool hole = !fg && l >= 1 && l <= n && mark[l] == 0;
        out[i] = fg || hole;
        cnt += hole;
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(filled, (unsigned long long)cnt);
}

// ------------------------------------------------------------------------------------------- Sobel magnitude
// scipy's `reflect` for a stencil of radius 1: -1 reads 0, len reads len - 1
__device__ __forceinline__ int reflect1(int c, int len) { return c < 0 ? 0 : (c >= len ? len - 1 : c); }

// partial[block] = {n, sum(|g| - shift), sum((|g| - shift)^2)} over the block's selected voxels
__global__ __launch_bounds__(256) void sobel_stats_kernel(const float *x, const uint8_t *flags, int select, int d0, int d1, int d2, double shift,
                                                          double *partial) {
    const int64_t V = (int64_t)d0 * d1 * d2, s0 = (int64_t)d1 * d2;
    double acc[3] = {0, 0, 0};
    for (int it = 0; it < RED_CHUNK / 256; ++it) {
        const int64_t i = (int64_t)blockIdx.x * RED_CHUNK + it * 256 + threadIdx.x;
        if (i >= V) break;
        if (!(flags[i] & select)) continue;
        int c0, c1, c2;
        coords(i, d1, d2, c0, c1, c2);
        const int64_t o0[3] = {reflect1(c0 - 1, d0) * s0, c0 * s0, reflect1(c0 + 1, d0) * s0};
        const int64_t o1[3] = {(int64_t)reflect1(c1 - 1, d1) * d2, (int64_t)c1 * d2, (int64_t)reflect1(c1 + 1, d1) * d2};
        const int o2[3] = {reflect1(c2 - 1, d2), c2, reflect1(c2 + 1, d2)};
        double v[3][3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[a][b][c] = (double)x[o0[a] + o1[b] + o2[c]];
        // the difference along the axis first, then [1, 2, 1] along the other two in axis order, as scipy chains its 1-D passes
        double t[3][3], u[3];
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int c = 0; c < 3; ++c) t[b][c] = v[2][b][c] - v[0][b][c];
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = (t[0][c] + t[2][c]) + 2.0 * t[1][c];
        const double g0 = (u[0] + u[2]) + 2.0 * u[1];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) t[a][c] = v[a][2][c] - v[a][0][c];
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = (t[0][c] + t[2][c]) + 2.0 * t[1][c];
        const double g1 = (u[0] + u[2]) + 2.0 * u[1];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) t[a][b] = v[a][b][2] - v[a][b][0];
#pragma unroll
        for (int b = 0; b < 3; ++b) u[b] = (t[0][b] + t[2][b]) + 2.0 * t[1][b];
        const double g2 = (u[0] + u[2]) + 2.0 * u[1];
        const double m = sqrt((g0 * g0 + g1 * g1) + g2 * g2) - shift;
        acc[0] += 1.0; acc[1] += m; acc[2] += m * m;
    }
    block_partial<3>(acc, partial);
}

// ------------------------------------------------------------------------------------------- radial shells
// numpy's np.sqrt((c0 - m0)**2 + (c1 - m1)**2 + (c2 - m2)**2): every square rounded, then two additions from the left
__device__ __forceinline__ double shell_dist(int c0, int c1, int c2, double m0, double m1, double m2) {
    const double a = (double)c0 - m0, b = (double)c1 - m1, c = (double)c2 - m2;
    const double aa = a * a, bb = b * b, cc = c * c;
    return sqrt((aa + bb) + cc);
}

// res[0] = the bit pattern of the largest distance (non-negative doubles order as their bit patterns), res[1] = the number of
// selected voxels
__global__ __launch_bounds__(256) void shell_max_kernel(const uint8_t *flags, int require, int d0, int d1, int d2, double m0, double m1, double m2,
                                                        unsigned long long *res) {
    const int64_t V = (int64_t)d0 * d1 * d2;
    double best = 0.0;
    int cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        if ((flags[i] & require) != require) continue;
        int c0, c1, c2;
        coords(i, d1, d2, c0, c1, c2);
        const double d = shell_dist(c0, c1, c2, m0, m1, m2);
        best = d > best ? d : best;
        ++cnt;
    }
    for (int m = 1; m < 64; m <<= 1) {
        const double o = __shfl_xor(best, m);
        best = o > best ? o : best;
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicMax(res, (unsigned long long)__double_as_longlong(best));
        atomicAdd(res + 1, (unsigned long long)cnt);
    }
}

// partial[block] = {n_inner, sum_inner, n_outer, sum_outer} of x over the block's selected voxels with dist < t_in / dist > t_out
__global__ __launch_bounds__(256) void shell_moments_kernel(const float *x, const uint8_t *flags, int require, int d0, int d1, int d2, double m0,
                                                            double m1, double m2, double t_in, double t_out, double *partial) {
    const int64_t V = (int64_t)d0 * d1 * d2;
    double acc[4] = {0, 0, 0, 0};
    for (int it = 0; it < RED_CHUNK / 256; ++it) {
        const int64_t i = (int64_t)blockIdx.x * RED_CHUNK + it * 256 + threadIdx.x;
        if (i >= V) break;
        if ((flags[i] & require) != require) continue;
        int c0, c1, c2;
        coords(i, d1, d2, c0, c1, c2);
        const double d = shell_dist(c0, c1, c2, m0, m1, m2);
        const bool in = d < t_in, out = d > t_out;
        if (!in && !out) continue;
        const double v = (double)x[i];
        acc[0] += in ? 1.0 : 0.0; acc[1] += in ? v : 0.0;
        acc[2] += out ? 1.0 : 0.0; acc[3] += out ? v : 0.0;
    }
    block_partial<4>(acc, partial);
}

// ------------------------------------------------------------------------------------------- face slabs
__global__ __launch_bounds__(256) void face_slab_kernel(const float *x, int d0, int d1, int d2, int margin, unsigned long long *counts) {
    const int64_t V = (int64_t)d0 * d1 * d2;
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        int c0, c1, c2;
        coords(i, d1, d2, c0, c1, c2);
        const bool in[6] = {c0 < margin, c0 >= d0 - margin, c1 < margin, c1 >= d1 - margin, c2 < margin, c2 >= d2 - margin};
        if (!(in[0] || in[1] || in[2] || in[3] || in[4] || in[5])) continue;
        if (!(x[i] > 0.0f)) continue;
#pragma unroll
        for (int k = 0; k < 6; ++k) cnt[k] += in[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int r = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && r) atomicAdd(counts + k, (unsigned long long)r);
    }
}

}  // namespace qc
}  // namespace mi355

using namespace mi355;
using namespace mi355::qc;

// scratch slot SCR_QUALITY, per stream lane: for a hole filling [filled u64, pad to 256 B | complement u8 V | labels i32 V |
// marks u32, one per component and one spare]; for a reduction its result words or partial sums
extern "C" int mi355_binary_fill_holes(const uint8_t *mask_dev, int d0, int d1, int d2, uint8_t *out_dev, int64_t *filled_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("binary_fill_holes", d0, d1, d2, &V));
    MI355_REQUIRE(mask_dev && out_dev && filled_host && mask_dev != out_dev, "binary_fill_holes: null or aliased pointers (out must not be the input)");
    hipStream_t s = (hipStream_t)stream;
    // a 6-connected component of the complement has no 6-neighbour in another one: at most every second voxel starts one
    const int64_t max_components = V / 2 + 1;
    const size_t comp_bytes = pad256((size_t)V), labels_bytes = pad256((size_t)V * sizeof(int)), mark_bytes = (size_t)(max_components + 1) * sizeof(unsigned);
    char *scr = nullptr;
    MI355_TRY(device_scratch(SCR_QUALITY, s, 256 + comp_bytes + labels_bytes + mark_bytes, (void **)&scr));
    unsigned long long *filled = (unsigned long long *)scr;
    uint8_t *comp = (uint8_t *)(scr + 256);
    int *labels = (int *)(scr + 256 + comp_bytes);
    unsigned *mark = (unsigned *)(scr + 256 + comp_bytes + labels_bytes);
    const unsigned blocks = grid_for(V, 256, 16384);
    hipLaunchKernelGGL(complement_kernel, dim3(blocks), dim3(256), 0, s, mask_dev, V, comp);
    MI355_HIP(hipGetLastError());
    int32_t n = 0;
    MI355_TRY(mi355_label_components(comp, d0, d1, d2, 1, labels, &n, stream));
    MI355_REQUIRE(n >= 0 && n <= max_components, "binary_fill_holes: %d components of the complement of %dx%dx%d (at most %lld can exist)", n, d0, d1, d2,
                  (long long)max_components);
    MI355_HIP(hipMemsetAsync(filled, 0, sizeof(unsigned long long), s));
    MI355_HIP(hipMemsetAsync(mark, 0, (size_t)(n + 1) * sizeof(unsigned), s));
    hipLaunchKernelGGL(face_mark_kernel, dim3(blocks), dim3(256), 0, s, (const int *)labels, d0, d1, d2, (int)n, mark);
    hipLaunchKernelGGL(fill_write_kernel, dim3(blocks), dim3(256), 0, s, mask_dev, (const int *)labels, (const unsigned *)mark, (int)n, V, out_dev, filled);
    unsigned long long h = 0;
    MI355_TRY(read_back(&h, filled, sizeof(h), s));
    *filled_host = (int64_t)h;
    return MI355_OK;
}

extern "C" int mi355_sobel_magnitude_stats(const float *x_dev, const uint8_t *flags_dev, int select, int d0, int d1, int d2, double *stats_host,
                                           void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("sobel_magnitude_stats", d0, d1, d2, &V));
    MI355_REQUIRE(x_dev && flags_dev && stats_host, "sobel_magnitude_stats: null pointer");
    MI355_REQUIRE(select >= 1 && select <= 255, "sobel_magnitude_stats: select %d (a mask of the bits that mark the voxels, 255 = any)", select);
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (int)((V + RED_CHUNK - 1) / RED_CHUNK);
    double *partial = nullptr;
    MI355_TRY(device_scratch(SCR_QUALITY, s, ((size_t)nblocks * 3 + 4) * sizeof(double), (void **)&partial));
    double *total = partial + (size_t)nblocks * 3, h[3] = {0, 0, 0};
    double mean = 0;
    for (int pass = 0; pass < 2; ++pass) {  // pass 0: n and the mean; pass 1: the sums about that mean
        hipLaunchKernelGGL(sobel_stats_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, x_dev, flags_dev, select, d0, d1, d2, mean, partial);
        hipLaunchKernelGGL(sum_columns_kernel, dim3(3), dim3(64), 0, s, (const double *)partial, nblocks, 3, total);
        MI355_TRY(read_back(h, total, sizeof(h), s));
        if (h[0] == 0) { stats_host[0] = stats_host[1] = stats_host[2] = 0; return MI355_OK; }
        if (pass == 0) mean = h[1] / h[0];
    }
    const double dm = h[1] / h[0];  // what rounding left of the mean of (|g| - mean)
    const double var = h[2] / h[0] - dm * dm;
    stats_host[0] = h[0];
    stats_host[1] = mean + dm;
    stats_host[2] = var > 0 ? sqrt(var) : 0.0;
    return MI355_OK;
}

extern "C" int mi355_radial_shell_moments(const float *x_dev, const uint8_t *flags_dev, int require, int d0, int d1, int d2, const double centre[3],
                                          double inner_frac, double outer_frac, double *out_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("radial_shell_moments", d0, d1, d2, &V));
    MI355_REQUIRE(x_dev && flags_dev && centre && out_host, "radial_shell_moments: null pointer");
    MI355_REQUIRE(require >= 0 && require <= 255, "radial_shell_moments: require %d (a mask of flag bits, 0..255)", require);
    MI355_REQUIRE(centre[0] == centre[0] && centre[1] == centre[1] && centre[2] == centre[2] && inner_frac == inner_frac && outer_frac == outer_frac,
                  "radial_shell_moments: the centre or a fraction is NaN");
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (int)((V + RED_CHUNK - 1) / RED_CHUNK);
    char *scr = nullptr;
    MI355_TRY(device_scratch(SCR_QUALITY, s, 256 + ((size_t)nblocks * 4 + 4) * sizeof(double), (void **)&scr));
    unsigned long long *res = (unsigned long long *)scr, hres[2] = {0, 0};
    double *partial = (double *)(scr + 256), *total = partial + (size_t)nblocks * 4, h[4] = {0, 0, 0, 0};
    for (int k = 0; k < 5; ++k) out_host[k] = 0;
    MI355_HIP(hipMemsetAsync(res, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(shell_max_kernel, dim3(grid_for(V, 256 * 16, 4096)), dim3(256), 0, s, flags_dev, require, d0, d1, d2, centre[0], centre[1], centre[2], res);
    MI355_TRY(read_back(hres, res, sizeof(hres), s));
    if (hres[1] == 0) return MI355_OK;
    double max_dist;
    static_assert(sizeof(max_dist) == sizeof(hres[0]), "a double is 64 bits");
    memcpy(&max_dist, &hres[0], sizeof(max_dist));
    const double t_in = max_dist * inner_frac, t_out = max_dist * outer_frac;  // step5_quality.py:293-294
    hipLaunchKernelGGL(shell_moments_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, x_dev, flags_dev, require, d0, d1, d2, centre[0], centre[1], centre[2],
                       t_in, t_out, partial);
    hipLaunchKernelGGL(sum_columns_kernel, dim3(4), dim3(64), 0, s, (const double *)partial, nblocks, 4, total);
    MI355_TRY(read_back(h, total, sizeof(h), s));
    out_host[0] = max_dist;
    for (int k = 0; k < 4; ++k) out_host[1 + k] = h[k];
    return MI355_OK;
}

extern "C" int mi355_face_slab_counts(const float *x_dev, int d0, int d1, int d2, int margin, int64_t *counts_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("face_slab_counts", d0, d1, d2, &V));
    MI355_REQUIRE(x_dev && counts_host, "face_slab_counts: null pointer");
    MI355_REQUIRE(margin >= 1, "face_slab_counts: margin %d (1 or more)", margin);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *counts = nullptr;
    MI355_TRY(device_scratch(SCR_QUALITY, s, 256, (void **)&counts));
    MI355_HIP(hipMemsetAsync(counts, 0, 6 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(face_slab_kernel, dim3(grid_for(V, 256 * 16, 4096)), dim3(256), 0, s, x_dev, d0, d1, d2, margin, counts);
    MI355_TRY(read_back(counts_host, counts, 6 * sizeof(int64_t), s));
    return MI355_OK;
}
