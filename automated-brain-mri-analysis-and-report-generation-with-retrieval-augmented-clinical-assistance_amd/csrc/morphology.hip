// Binary morphology, exact squared Euclidean distance transform and the mask reductions behind the reference's step 4
// (feature_extraction/step4_morphology.py): what that file gets from scipy.ndimage.binary_erosion /
// binary_dilation (:42, :149, :227, :252, :254), distance_transform_edt (:160-161), np.gradient over the whole volume
// (:167-172), np.where + np.cov (:84-100) and boolean-mask indexing of the four modalities (:231-262, :324-338).
// step2_mass_effect.py uses the same erosion and dilation (:19, :373): nothing here knows about step 4.
//
// All volumes are [d0][d1][d2] C-order; a uint8 mask is foreground where nonzero (as in components.hip).  No workgroup
// waits for another one: every ordering is a launch boundary.  Every result is deterministic:
//   * the masks and the distance map are integers written by exactly one thread each;
//   * integer reductions (coordinate moments) meet in integer atomics, which commute;
//   * fp64 reductions (gradient statistics, intensity moments) never meet in an atomic: a thread owns fixed voxels, a
//     workgroup reduces its threads in a fixed tree and writes ONE partial, and one wave sums the partials in a fixed order.
//
// Squared EDT = three separable passes over the int32 map, in place (Felzenszwalb & Huttenlocher's decomposition with the
// lower envelope evaluated by brute force: lines are a few hundred voxels at most, so min_j(g[j] + (i - j)^2) is a plain
// min-plus loop over a tile in LDS - exact, no branches, no per-line stack):
//   1  axis 0   a thread per (i1, i2) column scans down and up: squared distance to the nearest background voxel of the
//               column (EDT_INF when it has none); lanes run along axis 2
//   2  axis 1   a workgroup stages a [d1][TX] tile (TX = 64, 32 or 16 neighbours along axis 2) and every thread computes
//               four outputs of one column per sweep over the tile: one conflict-free ds_read_b32 per four min-adds
//   3  axis 2   a workgroup stages TY whole lines (one contiguous chunk of memory); a thread computes one output and reads
//               the line four entries at a time (ds_read_b128, the same address in every lane of a line: a broadcast)
// In all three the lanes of a wave sit on adjacent addresses of axis 2 for every global access.  Values are uint32 with
// EDT_INF = 2^31: a finite value is at most the squared diagonal (< 2^31, checked), so EDT_INF + (i - j)^2 never wraps and
// never wins against a finite candidate; every pass clamps to EDT_INF again.
#include "volume_common.h"

namespace mi355 {

constexpr unsigned EDT_INF = 0x80000000u;
constexpr int EDT_MAX_LINE = 1024;             // longest axis-1 / axis-2 line: a [1024][16] uint32 tile is 64 KiB of LDS
constexpr int EDT_TILE_BYTES = 64 * 1024;
constexpr int RED_CHUNK = 8192;                // voxels per workgroup in the reductions (32 per thread)
constexpr int MM_BITS = 8, MM_MAX_CHANNELS = 8;  // masked moments: region bits of a flag byte, channels per call

struct ByteSet { uint8_t m[256]; };

// ------------------------------------------------------------------------------------------- erosion / dilation
// one step with the 6-neighbour cross, everything outside the volume = 0 (scipy's border_value); out = 0 / 1
template <bool DILATE>
__global__ __launch_bounds__(256) void morph_step_kernel(const uint8_t *in, int d0, int d1, int d2, uint8_t *out) {
    const int64_t V = (int64_t)d0 * d1 * d2;
    const int64_t s1 = d2, s0 = (int64_t)d1 * d2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        const unsigned u = (unsigned)i;
        const unsigned zy = u / (unsigned)d2;
        const int x = (int)(u - zy * (unsigned)d2), z = (int)(zy / (unsigned)d1), y = (int)(zy - (unsigned)z * (unsigned)d1);
        const bool c = in[i] != 0;
        const bool xm = x > 0 && in[i - 1], xp = x + 1 < d2 && in[i + 1];
        const bool ym = y > 0 && in[i - s1], yp = y + 1 < d1 && in[i + s1];
        const bool zm = z > 0 && in[i - s0], zp = z + 1 < d0 && in[i + s0];
        out[i] = DILATE ? (c || xm || xp || ym || yp || zm || zp) : (c && xm && xp && ym && yp && zm && zp);
    }
}

// ------------------------------------------------------------------------------------------- squared EDT
__global__ __launch_bounds__(256) void count_background_kernel(const uint8_t *mask, int64_t V, unsigned *count) {
    int n = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) n += mask[i] == 0;
    for (int m = 1; m < 64; m <<= 1) n += __shfl_xor(n, m);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, (unsigned)n);
}

__global__ __launch_bounds__(256) void edt_axis0_kernel(const uint8_t *mask, int d0, int64_t plane, unsigned *g) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= plane) return;
    unsigned run = EDT_INF;  // steps since the last background voxel of the column, EDT_INF before the first
    for (int z = 0; z < d0; ++z) {
        const bool fg = mask[z * plane + c] != 0;
        run = fg ? (run == EDT_INF ? EDT_INF : run + 1) : 0;
        g[z * plane + c] = run;
    }
    run = EDT_INF;
    for (int z = d0 - 1; z >= 0; --z) {
        const unsigned down = g[z * plane + c];
        run = down ? (run == EDT_INF ? EDT_INF : run + 1) : 0;
        const unsigned d = min(down, run);
        g[z * plane + c] = d == EDT_INF ? EDT_INF : d * d;  // d <= d0 - 1 and (d0 - 1)^2 < 2^31 (checked by the caller)
    }
}

__device__ __forceinline__ unsigned min_plus(unsigned acc, unsigned g, int d) { return min(acc, g + (unsigned)__mul24(d, d)); }

// in place: every workgroup reads its whole tile into LDS before it writes, and nobody else touches the tile
__global__ __launch_bounds__(256) void edt_axis1_kernel(unsigned *g, int d1, int d2, int nbx, int tx_log2) {
    extern __shared__ unsigned tile[];  // [d1][TX]
    const int TX = 1 << tx_log2;
    const int z = blockIdx.x / nbx, x0 = (blockIdx.x - z * nbx) * TX;
    unsigned *base = g + (int64_t)z * d1 * d2;
    for (int i = threadIdx.x; i < d1 * TX; i += 256) {
        const int y = i >> tx_log2, x = x0 + (i & (TX - 1));
        tile[i] = x < d2 ? base[(int64_t)y * d2 + x] : EDT_INF;
    }
    __syncthreads();
    const int xl = threadIdx.x & (TX - 1), x = x0 + xl;
    const int groups = 256 >> tx_log2;
    for (int y0 = (threadIdx.x >> tx_log2) * 4; y0 < d1; y0 += groups * 4) {
        unsigned a0 = EDT_INF, a1 = EDT_INF, a2 = EDT_INF, a3 = EDT_INF;
        for (int j = 0; j < d1; ++j) {
            const unsigned v = tile[(j << tx_log2) + xl];
            const int d = y0 - j;
            a0 = min_plus(a0, v, d); a1 = min_plus(a1, v, d + 1); a2 = min_plus(a2, v, d + 2); a3 = min_plus(a3, v, d + 3);
        }
        if (x >= d2) continue;
        unsigned *o = base + (int64_t)y0 * d2 + x;
        o[0] = min(a0, EDT_INF);
        if (y0 + 1 < d1) o[d2] = min(a1, EDT_INF);
        if (y0 + 2 < d1) o[2 * (int64_t)d2] = min(a2, EDT_INF);
        if (y0 + 3 < d1) o[3 * (int64_t)d2] = min(a3, EDT_INF);
    }
}

__global__ __launch_bounds__(256) void edt_axis2_kernel(unsigned *g, int64_t lines, int d2, int pitch, int ty) {
    extern __shared__ unsigned tile[];  // [ty][pitch], pitch = d2 rounded up to 4, the tail = EDT_INF
    const int64_t line0 = (int64_t)blockIdx.x * ty;
    const int nl = (int)min((int64_t)ty, lines - line0);
    unsigned *base = g + line0 * d2;
    const int n = nl * d2;
    for (int i = threadIdx.x; i < nl * pitch; i += 256) {
        const int l = i / pitch, x = i - l * pitch;
        tile[i] = x < d2 ? base[l * d2 + x] : EDT_INF;
    }
    __syncthreads();
    const uint4 *tile4 = (const uint4 *)tile;
    const int p4 = pitch >> 2;
    for (int o = threadIdx.x; o < n; o += 256) {
        const int l = o / d2, x = o - l * d2;
        unsigned acc = EDT_INF;
        const uint4 *row = tile4 + l * p4;
        for (int j4 = 0; j4 < p4; ++j4) {
            const uint4 v = row[j4];
            const int d = x - 4 * j4;
            acc = min_plus(acc, v.x, d); acc = min_plus(acc, v.y, d - 1); acc = min_plus(acc, v.z, d - 2); acc = min_plus(acc, v.w, d - 3);
        }
        base[o] = min(acc, EDT_INF);
    }
}

// ------------------------------------------------------------------------------------------- reductions
// np.gradient's stencil along one axis of the signed distance sqrt(d2_in) - sqrt(d2_out): central difference / 2 inside,
// one-sided first difference at both ends (the axis has at least 2 entries)
__device__ __forceinline__ double signed_dist(const int *din, const int *dout, int64_t i) {
    return sqrt((double)din[i]) - sqrt((double)dout[i]);
}
__device__ __forceinline__ double axis_gradient(const int *din, const int *dout, int64_t i, int c, int len, int64_t stride) {
    if (c == 0) return signed_dist(din, dout, i + stride) - signed_dist(din, dout, i);
    if (c == len - 1) return signed_dist(din, dout, i) - signed_dist(din, dout, i - stride);
    return (signed_dist(din, dout, i + stride) - signed_dist(din, dout, i - stride)) / 2.0;
}

// partial[block] = {n, sum(|grad| - shift), sum((|grad| - shift)^2)} over the block's surface voxels
__global__ __launch_bounds__(256) void grad_stats_kernel(const int *din, const int *dout, const uint8_t *surface, int select, int d0, int d1,
                                                         int d2, double shift, double *partial) {
    __shared__ double wred[4][3];
    const int64_t V = (int64_t)d0 * d1 * d2, s0 = (int64_t)d1 * d2;
    double n = 0, a = 0, b = 0;
    for (int it = 0; it < RED_CHUNK / 256; ++it) {
        const int64_t i = (int64_t)blockIdx.x * RED_CHUNK + it * 256 + threadIdx.x;
        if (i >= V) break;
        if (!(surface[i] & select)) continue;
        const unsigned u = (unsigned)i;
        const unsigned zy = u / (unsigned)d2;
        const int x = (int)(u - zy * (unsigned)d2), z = (int)(zy / (unsigned)d1), y = (int)(zy - (unsigned)z * (unsigned)d1);
        const double gz = axis_gradient(din, dout, i, z, d0, s0), gy = axis_gradient(din, dout, i, y, d1, d2), gx = axis_gradient(din, dout, i, x, d2, 1);
        const double m = sqrt(gz * gz + gy * gy + gx * gx) - shift;
        n += 1.0; a += m; b += m * m;
    }
    n = wave_sum(n); a = wave_sum(a); b = wave_sum(b);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { wred[w][0] = n; wred[w][1] = a; wred[w][2] = b; }
    __syncthreads();
    if (threadIdx.x < 3) partial[(int64_t)blockIdx.x * 3 + threadIdx.x] = ((wred[0][threadIdx.x] + wred[1][threadIdx.x]) + wred[2][threadIdx.x]) + wred[3][threadIdx.x];
}

// out[k] = the sum of column k of the partials: lane l adds rows l, l + 64, ... in that order, then the wave's fixed butterfly.
// grid ncols, one wave each
__global__ __launch_bounds__(64) void sum_partials_kernel(const double *partial, int nblocks, int ncols, double *out) {
    const int k = blockIdx.x;
    double s = 0;
    for (int b = threadIdx.x; b < nblocks; b += 64) s += partial[(int64_t)b * ncols + k];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[k] = s;
}

// n, sum of c0 c1 c2, sum of c0^2 c1^2 c2^2, sum of c0 c1, c0 c2, c1 c2 over the foreground (int64, exact)
__global__ __launch_bounds__(256) void second_moments_kernel(const uint8_t *mask, int d0, int d1, int d2, unsigned long long *out) {
    __shared__ long long wred[4][10];
    const int64_t V = (int64_t)d0 * d1 * d2;
    long long v[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) v[k] = 0;
    for (int it = 0; it < RED_CHUNK / 256; ++it) {
        const int64_t i = (int64_t)blockIdx.x * RED_CHUNK + it * 256 + threadIdx.x;
        if (i >= V) break;
        if (!mask[i]) continue;
        const unsigned u = (unsigned)i;
        const unsigned zy = u / (unsigned)d2;
        const long long c2 = u - zy * (unsigned)d2, c0 = zy / (unsigned)d1, c1 = zy - (unsigned)c0 * (unsigned)d1;
        v[0] += 1; v[1] += c0; v[2] += c1; v[3] += c2;
        v[4] += c0 * c0; v[5] += c1 * c1; v[6] += c2 * c2;
        v[7] += c0 * c1; v[8] += c0 * c2; v[9] += c1 * c2;
    }
    if (!__syncthreads_or(v[0] != 0)) return;  // nothing of the mask in this chunk
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const long long r = wave_sum(v[k]);
        if (lane == 0) wred[w][k] = r;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        const long long r = wred[0][threadIdx.x] + wred[1][threadIdx.x] + wred[2][threadIdx.x] + wred[3][threadIdx.x];
        if (r) atomicAdd(out + threadIdx.x, (unsigned long long)r);
    }
}

// grid (chunks, C): partial[(c * chunks + chunk) * 16 + k]: k = 2 b, 2 b + 1 the sum and the sum of squares of channel c over
// the chunk's voxels with flag bit b; the c == 0 row also writes counts[chunk * 8 + b], the chunk's voxels with bit b
__global__ __launch_bounds__(256) void masked_moments_kernel(const float *vols, const uint8_t *flags, int64_t n, double *partial, int *counts) {
    __shared__ double wred[4][2 * MM_BITS];
    __shared__ int wcnt[4][MM_BITS];
    const float *vol = vols + (int64_t)blockIdx.y * n;
    double s[2 * MM_BITS];
    int cnt[MM_BITS];
#pragma unroll
    for (int k = 0; k < 2 * MM_BITS; ++k) s[k] = 0;
#pragma unroll
    for (int b = 0; b < MM_BITS; ++b) cnt[b] = 0;
    for (int it = 0; it < RED_CHUNK / 256; ++it) {
        const int64_t i = (int64_t)blockIdx.x * RED_CHUNK + it * 256 + threadIdx.x;
        if (i >= n) break;
        const int f = flags[i];
        if (!f) continue;
        const double v = (double)vol[i], vv = v * v;
#pragma unroll
        for (int b = 0; b < MM_BITS; ++b) {
            const bool on = (f >> b) & 1;
            s[2 * b] += on ? v : 0.0;
            s[2 * b + 1] += on ? vv : 0.0;
            cnt[b] += on;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 2 * MM_BITS; ++k) {
        const double r = wave_sum(s[k]);
        if (lane == 0) wred[w][k] = r;
    }
#pragma unroll
    for (int b = 0; b < MM_BITS; ++b) {
        int r = cnt[b];
        for (int m = 1; m < 64; m <<= 1) r += __shfl_xor(r, m);
        if (lane == 0) wcnt[w][b] = r;
    }
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x < 2 * MM_BITS) partial[row * (2 * MM_BITS) + threadIdx.x] = ((wred[0][threadIdx.x] + wred[1][threadIdx.x]) + wred[2][threadIdx.x]) + wred[3][threadIdx.x];
    if (blockIdx.y == 0 && threadIdx.x < MM_BITS) counts[(int64_t)blockIdx.x * MM_BITS + threadIdx.x] = wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
}

// out[(b * C + c) * 3 + {0, 1, 2}] = count of bit b, sum, sum of squares of channel c.  grid (C, 24), one wave each: value k of
// channel c over the chunks, lane l taking chunks l, l + 64, ... in that order, then the wave's fixed butterfly
__global__ __launch_bounds__(64) void masked_moments_finish_kernel(const double *partial, const int *counts, int chunks, int C, double *out) {
    const int c = blockIdx.x, k = blockIdx.y;
    if (k < 2 * MM_BITS) {
        double s = 0;
        for (int j = threadIdx.x; j < chunks; j += 64) s += partial[((int64_t)c * chunks + j) * (2 * MM_BITS) + k];
        s = wave_sum(s);
        if (threadIdx.x == 0) out[((k >> 1) * C + c) * 3 + 1 + (k & 1)] = s;
    } else {
        const int b = k - 2 * MM_BITS;
        long long t = 0;
        for (int j = threadIdx.x; j < chunks; j += 64) t += counts[(int64_t)j * MM_BITS + b];
        t = wave_sum(t);
        if (threadIdx.x == 0) out[(b * C + c) * 3] = (double)t;
    }
}

// ------------------------------------------------------------------------------------------- flag helpers
__global__ void flag_from_labels_kernel(const uint8_t *labels, ByteSet set, int bitmask, uint8_t *flags, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = (uint8_t)((flags[i] & ~bitmask) | (set.m[labels[i]] ? bitmask : 0));
}
__global__ void flag_from_flags_kernel(uint8_t *flags, int bitmask, int require, int forbid, const float *x, double lo, double hi, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = flags[i];
        bool on = (f & require) == require && !(f & forbid);
        if (on && x) {
            const double v = (double)x[i];
            on = lo < v && v < hi;
        }
        flags[i] = (uint8_t)((f & ~bitmask) | (on ? bitmask : 0));
    }
}

}  // namespace mi355

using namespace mi355;

// scratch slot SCR_MORPHOLOGY, per stream lane: the second buffer of the erosion / dilation ping-pong, or the partial sums of
// a reduction followed by its few result words
extern "C" int mi355_binary_morphology(const uint8_t *mask_dev, int d0, int d1, int d2, int dilate, int iterations, uint8_t *out_dev,
                                       void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("binary_morphology", d0, d1, d2, &V));
    MI355_REQUIRE(mask_dev && out_dev && mask_dev != out_dev, "binary_morphology: null or aliased pointers (out must not be the input)");
    MI355_REQUIRE(iterations >= 1 && iterations <= 65535, "binary_morphology: iterations %d (1 or more; scipy's 'until nothing changes' (< 1) is not offered)", iterations);
    hipStream_t s = (hipStream_t)stream;
    uint8_t *tmp = nullptr;
    if (iterations > 1) MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, (size_t)V, (void **)&tmp));
    else MI355_TRY(bind_device());
    const unsigned blocks = grid_for(V, 256, 16384);
    const uint8_t *src = mask_dev;
    for (int it = 0; it < iterations; ++it) {
        uint8_t *dst = (iterations - 1 - it) % 2 == 0 ? out_dev : tmp;  // the last step writes out_dev
        if (dilate) hipLaunchKernelGGL(morph_step_kernel<true>, dim3(blocks), dim3(256), 0, s, src, d0, d1, d2, dst);
        else hipLaunchKernelGGL(morph_step_kernel<false>, dim3(blocks), dim3(256), 0, s, src, d0, d1, d2, dst);
        src = dst;
    }
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_edt_squared(const uint8_t *mask_dev, int d0, int d1, int d2, int32_t *dist2_dev, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("edt_squared", d0, d1, d2, &V));
    MI355_REQUIRE(mask_dev && dist2_dev, "edt_squared: null pointer");
    const int64_t diag2 = (int64_t)(d0 - 1) * (d0 - 1) + (int64_t)(d1 - 1) * (d1 - 1) + (int64_t)(d2 - 1) * (d2 - 1);
    MI355_REQUIRE(diag2 < (1ll << 31), "edt_squared: the squared diagonal of %dx%dx%d (%lld) does not fit int32", d0, d1, d2, (long long)diag2);
    MI355_REQUIRE(d1 <= EDT_MAX_LINE && d2 <= EDT_MAX_LINE, "edt_squared: %dx%dx%d: axes 1 and 2 may have %d entries at most (one line per LDS tile)",
                  d0, d1, d2, EDT_MAX_LINE);
    hipStream_t s = (hipStream_t)stream;
    unsigned *count = nullptr;
    MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, 256, (void **)&count));
    MI355_HIP(hipMemsetAsync(count, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(count_background_kernel, dim3(grid_for(V, 256 * 16, 2048)), dim3(256), 0, s, mask_dev, V, count);
    unsigned background = 0;
    MI355_TRY(read_back(&background, count, sizeof(unsigned), s));
    MI355_REQUIRE(background > 0, "edt_squared: the %dx%dx%d volume has no background voxel: there is no distance to measure", d0, d1, d2);
    unsigned *g = (unsigned *)dist2_dev;
    const int64_t plane = (int64_t)d1 * d2;
    hipLaunchKernelGGL(edt_axis0_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, mask_dev, d0, plane, g);
    if (d1 > 1) {
        const int tx_log2 = d1 <= 256 ? 6 : (d1 <= 512 ? 5 : 4);
        const int nbx = ceil_div(d2, 1 << tx_log2);  // nbx * d0 <= V < 2^31
        hipLaunchKernelGGL(edt_axis1_kernel, dim3((unsigned)nbx * (unsigned)d0), dim3(256), (size_t)d1 << (tx_log2 + 2), s, g, d1, d2, nbx, tx_log2);
    }
    if (d2 > 1) {
        const int pitch = (d2 + 3) & ~3;
        int ty = EDT_TILE_BYTES / 4 / (4 * pitch);  // a quarter of the LDS a workgroup may have: four workgroups per CU and more
        ty = ty < 1 ? 1 : (ty > 16 ? 16 : ty);
        const int64_t lines = (int64_t)d0 * d1;
        hipLaunchKernelGGL(edt_axis2_kernel, dim3((unsigned)((lines + ty - 1) / ty)), dim3(256), (size_t)ty * pitch * 4, s, g, lines, d2, pitch, ty);
    }
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_surface_gradient_stats(const int32_t *d2_in_dev, const int32_t *d2_out_dev, const uint8_t *surface_dev, int select, int d0,
                                            int d1, int d2, double *stats_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("surface_gradient_stats", d0, d1, d2, &V));
    MI355_REQUIRE(d2_in_dev && d2_out_dev && surface_dev && stats_host, "surface_gradient_stats: null pointer");
    MI355_REQUIRE(d0 >= 2 && d1 >= 2 && d2 >= 2, "surface_gradient_stats: %dx%dx%d: np.gradient needs at least 2 entries along every axis", d0, d1, d2);
    MI355_REQUIRE(select >= 1 && select <= 255, "surface_gradient_stats: select %d (a mask of the bits that mark the surface, 255 = any)", select);
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (int)((V + RED_CHUNK - 1) / RED_CHUNK);
    double *partial = nullptr;
    MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, ((size_t)nblocks * 3 + 4) * sizeof(double), (void **)&partial));
    double *total = partial + (size_t)nblocks * 3, h[3] = {0, 0, 0};
    double mean = 0;
    for (int pass = 0; pass < 2; ++pass) {  // pass 0: n and the mean; pass 1: the sums about that mean
        hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, (const int *)d2_in_dev, (const int *)d2_out_dev, surface_dev, select,
                           d0, d1, d2, mean, partial);
        hipLaunchKernelGGL(sum_partials_kernel, dim3(3), dim3(64), 0, s, (const double *)partial, nblocks, 3, total);
        MI355_TRY(read_back(h, total, sizeof(h), s));
        if (h[0] == 0) { stats_host[0] = stats_host[1] = stats_host[2] = 0; return MI355_OK; }
        if (pass == 0) mean = h[1] / h[0];
    }
    const double dm = h[1] / h[0];  // what rounding left of the mean of (|grad| - mean)
    const double var = h[2] / h[0] - dm * dm;
    stats_host[0] = h[0];
    stats_host[1] = mean + dm;
    stats_host[2] = var > 0 ? sqrt(var) : 0.0;
    return MI355_OK;
}

extern "C" int mi355_mask_second_moments(const uint8_t *mask_dev, int d0, int d1, int d2, int64_t *moments_host, void *stream) {
    int64_t V = 0;
    MI355_TRY(check_volume("mask_second_moments", d0, d1, d2, &V));
    MI355_REQUIRE(mask_dev && moments_host, "mask_second_moments: null pointer");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *out = nullptr;
    MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, 256, (void **)&out));
    MI355_HIP(hipMemsetAsync(out, 0, 10 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(second_moments_kernel, dim3((unsigned)((V + RED_CHUNK - 1) / RED_CHUNK)), dim3(256), 0, s, mask_dev, d0, d1, d2, out);
    MI355_TRY(read_back(moments_host, out, 10 * sizeof(int64_t), s));
    return MI355_OK;
}

extern "C" int mi355_masked_moments(const float *vols_dev, int C, const uint8_t *flags_dev, int64_t n, double *out_host, void *stream) {
    MI355_REQUIRE(vols_dev && flags_dev && out_host && n >= 1 && n < (1ll << 31), "masked_moments: bad argument (1 <= n < 2^31)");
    MI355_REQUIRE(C >= 1 && C <= MM_MAX_CHANNELS, "masked_moments: %d channels (1..%d)", C, MM_MAX_CHANNELS);
    hipStream_t s = (hipStream_t)stream;
    const int chunks = (int)((n + RED_CHUNK - 1) / RED_CHUNK);
    const size_t partial_bytes = (size_t)C * chunks * 2 * MM_BITS * sizeof(double), counts_bytes = ((size_t)chunks * MM_BITS * sizeof(int) + 7) / 8 * 8;
    const size_t out_count = (size_t)MM_BITS * C * 3;
    char *scr = nullptr;
    MI355_TRY(device_scratch(SCR_MORPHOLOGY, s, partial_bytes + counts_bytes + out_count * sizeof(double), (void **)&scr));
    double *partial = (double *)scr, *out = (double *)(scr + partial_bytes + counts_bytes);
    int *counts = (int *)(scr + partial_bytes);
    hipLaunchKernelGGL(masked_moments_kernel, dim3((unsigned)chunks, (unsigned)C), dim3(256), 0, s, vols_dev, flags_dev, n, partial, counts);
    hipLaunchKernelGGL(masked_moments_finish_kernel, dim3((unsigned)C, 3 * MM_BITS), dim3(64), 0, s, (const double *)partial, (const int *)counts, chunks, C, out);
    MI355_TRY(read_back(out_host, out, out_count * sizeof(double), s));
    return MI355_OK;
}

extern "C" int mi355_flag_from_labels(const uint8_t *labels_dev, const uint8_t *set256_host, int bit, uint8_t *flags_dev, int64_t n, void *stream) {
    MI355_REQUIRE(labels_dev && set256_host && flags_dev && n >= 0, "flag_from_labels: bad argument");
    MI355_REQUIRE(bit >= 0 && bit < MM_BITS, "flag_from_labels: bit %d (0..%d)", bit, MM_BITS - 1);
    MI355_TRY(bind_device());
    ByteSet set;
    for (int i = 0; i < 256; ++i) set.m[i] = set256_host[i];
    hipLaunchKernelGGL(flag_from_labels_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, labels_dev, set, 1 << bit, flags_dev, n);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

extern "C" int mi355_flag_from_flags(uint8_t *flags_dev, int bit, int require, int forbid, const float *x_dev, double lo, double hi, int64_t n,
                                     void *stream) {
    MI355_REQUIRE(flags_dev && n >= 0, "flag_from_flags: bad argument");
    MI355_REQUIRE(bit >= 0 && bit < MM_BITS && require >= 0 && require <= 255 && forbid >= 0 && forbid <= 255, "flag_from_flags: bit %d, require %d, forbid %d", bit,
                  require, forbid);
    MI355_REQUIRE(!(lo != lo) && !(hi != hi), "flag_from_flags: a threshold is NaN");
    MI355_TRY(bind_device());
    hipLaunchKernelGGL(flag_from_flags_kernel, dim3(grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream, flags_dev, 1 << bit, require, forbid, x_dev, lo,
                       hi, n);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}
