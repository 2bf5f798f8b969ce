// The 1x1x1 segmentation head and the sliding-window aggregation: logits from the last decoder feature map, one tile's (or one
// forward's tiles') mirror-averaged sigmoid / softmax scattered Gaussian-weighted into the padded grid - from features or from
// logits, with or without the second moment, all over ONE per-voxel term (mirror_step, grid_add) -, the normaliser alone, and the finish
// that divides by it and crops.  16 B per lane where the layout allows it.
#include "kernels.h"

#include <algorithm>
#include <type_traits>

namespace mi355 {

// ------------------------------------------------------------------ segmentation head
int head_weights_upload(DeviceAllocs &mem, const float *w_host, const float *b_host, int cin, int ncls, HeadWeights *out) {
    MI355_REQUIRE(ncls >= 1 && ncls <= 8, "head: %d classes unsupported (max 8)", ncls);
    MI355_REQUIRE(cin % 8 == 0, "head: cin %d not a multiple of 8", cin);
    HeadWeights h;
    h.cin = cin; h.ncls = ncls;
    MI355_TRY(mem.upload(w_host, (size_t)ncls * cin * sizeof(float), &h.w_dev));
    float bias[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // [8] on the device whatever ncls is
    if (b_host) std::copy(b_host, b_host + ncls, bias);
    MI355_TRY(mem.upload(bias, sizeof(bias), &h.b_dev));
    *out = h;
    return MI355_OK;
}

constexpr int HEAD_MAX_CLS = 8;

// One thread per voxel: the whole channel vector of the voxel is read with 16-B loads (every byte of every
// line is used, consecutive lanes = consecutive voxels), the ncls x C head weights are wave-uniform (scalar loads),
// no cross-lane traffic.  The aggregate / normaliser read-modify-writes are then fully coalesced along x.
// NORM: the feature map is the RAW output of the last decoder conv and its Instance/GroupNorm (+ LeakyReLU) is applied here,
// per channel with this sample's scale / shift (wave-uniform: scalar loads) - generic_UNet.py:62-72 is one expression,
// lrelu(instnorm(conv(x))), and this kernel reads every feature exactly once anyway (round 3: removes the norm_apply pass
// over the widest-resolution tensor of the decoder).
// `feat` = this sample's feature map, `v` = the voxel, V = voxels per sample.  fp32 tensors are plain NDHWC ([V][C]), fp16
// tensors channel-blocked ([C / 8][V][8], common.h): either way consecutive lanes (voxels) read consecutive 16-B pieces.
// CC > 0: the channel count is a compile-time constant (32: every head of the two BraTS networks) - the piece loop is unrolled and ALL
// 16-B pieces of the voxel are loaded before the first is used (round 3: as a run-time loop each piece was load -> wait -> use,
// one load in flight per thread, and head_aggregate ran at 2.0 TB/s with its lanes idle on memory latency).  Same order of
// additions either way: bit-identical logits.
template <typename T, bool NORM, int CC>
__device__ __forceinline__ void head_dot_impl(const T *feat, int64_t v, int64_t V, const float *__restrict__ w, const float *__restrict__ b,
                                              int Crt, int ncls, float *logit, const float *__restrict__ sc, const float *__restrict__ sh, float nslope) {
    const int C = CC > 0 ? CC : Crt;
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) logit[k] = (k < ncls) ? b[k] : 0.f;
    constexpr bool F16 = std::is_same<T, _Float16>::value;
    constexpr int CW = F16 ? 8 : 4;  // channels per 16-B piece
    constexpr int NP = CC > 0 ? CC / CW : 1;
    typedef typename std::conditional<F16, f16x8, f32x4>::type piece_t;
    piece_t pre[NP];
    if constexpr (CC > 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if constexpr (F16) pre[i] = *(const f16x8 *)(feat + ((int64_t)i * V + v) * 8);
            else pre[i] = *(const f32x4 *)(feat + v * C + i * 4);
        }
    }
#pragma unroll
    for (int c = 0; c < C; c += CW) {
        float f[CW];
        piece_t h;
        if constexpr (CC > 0) h = pre[c / CW];
        else if constexpr (F16) h = *(const f16x8 *)(feat + ((int64_t)(c >> 3) * V + v) * 8);
        else h = *(const f32x4 *)(feat + v * C + c);
#pragma unroll
        for (int j = 0; j < CW; ++j) f[j] = (float)h[j];
        if constexpr (NORM) {
#pragma unroll
            for (int j = 0; j < CW; ++j) {
                const float y = fmaf(f[j], sc[c + j], sh[c + j]);
                f[j] = fmaxf(y, y * nslope);  // nslope = 1: no activation (max(y, y) = y)
            }
        }
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k)
            if (k < ncls) {
                const float *wk = w + k * C + c;
                // (same association as round 2: channels c+3, c+2, c+1, c innermost to outermost, 4 at a time)
#pragma unroll
                for (int q4 = 0; q4 < CW; q4 += 4)
                    logit[k] = fmaf(f[q4], wk[q4], fmaf(f[q4 + 1], wk[q4 + 1], fmaf(f[q4 + 2], wk[q4 + 2], fmaf(f[q4 + 3], wk[q4 + 3], logit[k]))));
            }
    }
}
template <typename T, bool NORM>
__device__ __forceinline__ void head_dot(const T *feat, int64_t v, int64_t V, const float *__restrict__ w, const float *__restrict__ b,
                                         int C, int ncls, float *logit, const float *__restrict__ sc = nullptr,
                                         const float *__restrict__ sh = nullptr, float nslope = 1.0f) {
    if (C == 32) head_dot_impl<T, NORM, 32>(feat, v, V, w, b, C, ncls, logit, sc, sh, nslope);  // (wave-uniform)
    else head_dot_impl<T, NORM, 0>(feat, v, V, w, b, C, ncls, logit, sc, sh, nslope);
}

template <typename T, bool NORM>
__global__ void head_logits_kernel(const T *feat, const float *w, const float *b, int C, int ncls,
                                   int64_t V, float *logits, FeatNorm fn) {
    // (blockIdx.y = sample: the per-sample scale / shift rows stay wave-uniform)
    const int64_t n = blockIdx.y;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
        float lg[HEAD_MAX_CLS];
        head_dot<T, NORM>(feat + n * V * C, v, V, w, b, C, ncls, lg, NORM ? fn.scale + n * C : nullptr, NORM ? fn.shift + n * C : nullptr, fn.slope);
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k)
            if (k < ncls) logits[(n * ncls + k) * V + v] = lg[k];
    }
}

template <typename T>
static void launch_head_logits(const HeadWeights &w, const T *feat, int N, int64_t V, float *logits, const FeatNorm &fn, hipStream_t s) {
    int64_t blocks = (V + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (fn.scale)
        hipLaunchKernelGGL((head_logits_kernel<T, true>), dim3((unsigned)blocks, N), dim3(256), 0, s, feat, w.w_dev, w.b_dev, w.cin, w.ncls, V, logits, fn);
    else
        hipLaunchKernelGGL((head_logits_kernel<T, false>), dim3((unsigned)blocks, N), dim3(256), 0, s, feat, w.w_dev, w.b_dev, w.cin, w.ncls, V, logits, fn);
}

int head_logits(const HeadWeights &w, const void *feat, int dtype, int N, int64_t V, float *logits, hipStream_t s, const FeatNorm &fn) {
    MI355_REQUIRE(N >= 1 && N <= 65535, "head_logits: %d samples", N);
    if (dtype == MI355_F16) launch_head_logits<_Float16>(w, (const _Float16 *)feat, N, V, logits, fn, s);
    else launch_head_logits<float>(w, (const float *)feat, N, V, logits, fn, s);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// ------------------------------------------------------------------ aggregation
int make_mirrors(const char *what, const int *mirrors_host, int n, MirrorList *out) {
    MI355_REQUIRE(mirrors_host && n >= 1 && n <= 8, "%s: %d mirrors", what, n);
    out->n = n;
    for (int i = 0; i < 8; ++i) out->m[i] = i < n ? mirrors_host[i] : 0;
    return MI355_OK;
}

// Where the logits of one mirror of a tile come from: src(mi, sv, PV, ncls, lg) gives lg[k] = class k (0 for k >= ncls) of the tile's
// mirror sample mi at its voxel sv of PV.  LogitsSource: the last conv already applied the head - logits [n_mirrors][ncls][PV] of this tile.
struct LogitsSource {
    const float *logits;
    __device__ __forceinline__ void operator()(int mi, int64_t sv, int64_t PV, int ncls, float *lg) const {
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k) lg[k] = (k < ncls) ? logits[((int64_t)mi * ncls + k) * PV + sv] : 0.f;
    }
};
// HeadSource: the head applied here to the last decoder feature map [n_mirrors][PV][C] of this tile (fn: rows of its first sample).
template <typename T, bool NORM>
struct HeadSource {
    const T *feat;
    const float *w, *b;
    int C;
    FeatNorm fn;
    __device__ __forceinline__ void operator()(int mi, int64_t sv, int64_t PV, int ncls, float *lg) const {
        head_dot<T, NORM>(feat + (int64_t)mi * PV * C, sv, PV, w, b, C, ncls, lg, NORM ? fn.scale + mi * C : nullptr,
                          NORM ? fn.shift + mi * C : nullptr, fn.slope);
    }
};

// Replaces.  ONE tile's term of a voxel, the one expression of every aggregation kernel, so that they cannot
// drift by a rounding:
//   mirror_step: res += mult * flip_back(nonlin(logits_m))           mult = 1/n_mirrors, at the tile's voxel (pz, py, px); m in list order
//   grid_add:   acc[k] += res[k] * g ; c += g                        g = the voxel's Gaussian weight (or 1)
// M2 (compile time; false: res2 / acc2 are not touched): the second moment rides along - res2 = sum_m mult * p * p beside res,
// acc2[k] += res2[k] * g - so that var = agg2 / cnt - (agg / cnt)^2 is the spread of the samples whose mean the predictor keeps.  acc
// and c receive the same operations in the same order either way.
// grid_add's acc[k] is acc[k * stride]: the grid itself at the voxel (stride = the grid's voxels; the kernel that adds one term reads
// and writes one class at a time after the mirrors and carries nothing across them: the unrolled NM = 8 instantiations have no
// registers to spare) or the values a thread carries through several tiles (stride 1).  c may be null.
// NM: compile-time mirror count (8 = the reference's full TTA; 0 = run time, t.ml.n).  With the loop unrolled the feature loads of
// all mirrors are independent of the sigmoid / softmax arithmetic between them and go out together: from features this is a stream
// of 16-B loads (32 per voxel for 32 channels x 8 mirrors), and as a run-time loop it had one mirror's four in flight.
template <bool M2>
static __device__ __forceinline__ void grid_add(int ncls, const AggTile &t, int pz, int py, int px, const float res[HEAD_MAX_CLS], const float *res2,
                                                float *acc, float *c, float *acc2, int64_t stride) {
    const float g = t.gauss ? t.gauss[((int64_t)pz * t.P[1] + py) * t.P[2] + px] : 1.0f;
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k)
        if (k < ncls) acc[k * stride] += res[k] * g;
    if constexpr (M2) {
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k)
            if (k < ncls) acc2[k * stride] += res2[k] * g;
    }
    if (c) *c += g;
}
template <bool M2, typename Source>
static __device__ __forceinline__ void mirror_step(const Source &src, int ncls, const AggTile &t, int mi, int pz, int py, int px, float *res, float *res2) {
    const int P0 = t.P[0], P1 = t.P[1], P2 = t.P[2];
    const int64_t PV = (int64_t)P0 * P1 * P2;
    const float mult = 1.0f / (float)t.ml.n;
    const int m = t.ml.m[mi];
    const int sz = (m & 1) ? P0 - 1 - pz : pz;
    const int sy = (m & 2) ? P1 - 1 - py : py;
    const int sx = (m & 4) ? P2 - 1 - px : px;
    const int64_t sv = ((int64_t)sz * P1 + sy) * P2 + sx;
    float lg[HEAD_MAX_CLS];
    src(mi, sv, PV, ncls, lg);
    if (t.nonlin == MI355_NONLIN_SIGMOID) {
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) lg[k] = 1.0f / (1.0f + expf(-lg[k]));
    } else if (t.nonlin == MI355_NONLIN_SOFTMAX) {
        float mx = lg[0];
#pragma unroll
        for (int k = 1; k < HEAD_MAX_CLS; ++k) if (k < ncls) mx = fmaxf(mx, lg[k]);
        float den = 0.f;
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) { lg[k] = expf(lg[k] - mx); den += lg[k]; }
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) lg[k] = lg[k] / den;
    }
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) res[k] += mult * lg[k];
    if constexpr (M2) {
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k) if (k < ncls) res2[k] += mult * lg[k] * lg[k];
    }
}
template <bool M2>
static __device__ __forceinline__ void res_clear(float *res, float *res2) {
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) res[k] = 0.f;
    if constexpr (M2) {
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k) res2[k] = 0.f;
    }
}
template <bool M2, int NM, typename Source>
static __device__ __forceinline__ void tile_term(const Source &src, int ncls, const AggTile &t, int pz, int py, int px, float res[HEAD_MAX_CLS],
                                                 float *res2) {
    res_clear<M2>(res, res2);
    if constexpr (NM > 0) {
#pragma unroll
        for (int mi = 0; mi < NM; ++mi) mirror_step<M2>(src, ncls, t, mi, pz, py, px, res, res2);
    } else {
        for (int mi = 0; mi < t.ml.n; ++mi) mirror_step<M2>(src, ncls, t, mi, pz, py, px, res, res2);
    }
}
// The term added to values a thread carries (the tiles kernel), with res / res2 of its own: the same steps, but where the two arrays
// live decides the register allocation - 75 VGPRs and 6 waves per SIMD here against 83 and 5 with the caller's arrays, which costs
// that chain of dependent loads 15 % of its time, while the unrolled NM = 8 kernels spill unless the arrays are their caller's.
template <bool M2, typename Source>
static __device__ __forceinline__ void tile_term_add(const Source &src, int ncls, const AggTile &t, int pz, int py, int px, float *acc, float *c, float *acc2) {
    float res[HEAD_MAX_CLS];
    float res2[M2 ? HEAD_MAX_CLS : 1];
    res_clear<M2>(res, res2);
    for (int mi = 0; mi < t.ml.n; ++mi) mirror_step<M2>(src, ncls, t, mi, pz, py, px, res, res2);
    grid_add<M2>(ncls, t, pz, py, px, res, res2, acc, c, acc2, 1);
}

// what the grid holds at voxel gi, and back (the kernel that carries a voxel through several tiles)
template <bool M2>
static __device__ __forceinline__ void grid_load(const AggGrid &g, int ncls, int64_t gi, float acc[HEAD_MAX_CLS], float &c, float *acc2) {
    const int64_t ZYXp = (int64_t)g.Zp[0] * g.Zp[1] * g.Zp[2];
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k) acc[k] = (k < ncls) ? g.agg[k * ZYXp + gi] : 0.f;
    if constexpr (M2) {
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k) acc2[k] = (k < ncls) ? g.agg2[k * ZYXp + gi] : 0.f;
    }
    c = g.cnt ? g.cnt[gi] : 0.f;
}
template <bool M2>
static __device__ __forceinline__ void grid_store(const AggGrid &g, int ncls, int64_t gi, const float acc[HEAD_MAX_CLS], float c, const float *acc2) {
    const int64_t ZYXp = (int64_t)g.Zp[0] * g.Zp[1] * g.Zp[2];
#pragma unroll
    for (int k = 0; k < HEAD_MAX_CLS; ++k)
        if (k < ncls) g.agg[k * ZYXp + gi] = acc[k];
    if constexpr (M2) {
#pragma unroll
        for (int k = 0; k < HEAD_MAX_CLS; ++k)
            if (k < ncls) g.agg2[k * ZYXp + gi] = acc2[k];
    }
    if (g.cnt) g.cnt[gi] = c;
}

// One tile at (z0, y0, x0) of the grid: aggregated[:, tile] += term ; normaliser[tile] += gaussian.  One thread per voxel of the
// tile; the aggregate / normaliser read-modify-writes are coalesced along x.  From features (head_aggregate) or from logits
// (logits_aggregate); it keeps the name the profiles know it by.
template <bool M2, int NM, typename Source>
__global__ void head_aggregate_kernel(Source src, int ncls, AggTile t, AggGrid g, int z0, int y0, int x0) {
    const int64_t PV = (int64_t)t.P[0] * t.P[1] * t.P[2];
    const int64_t ZYXp = (int64_t)g.Zp[0] * g.Zp[1] * g.Zp[2];
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < PV; v += (int64_t)gridDim.x * blockDim.x) {
        const int px = (int)(v % t.P[2]);
        const int py = (int)((v / t.P[2]) % t.P[1]);
        const int pz = (int)(v / ((int64_t)t.P[2] * t.P[1]));
        float res[HEAD_MAX_CLS];
        float res2[M2 ? HEAD_MAX_CLS : 1];
        tile_term<M2, NM>(src, ncls, t, pz, py, px, res, res2);
        const int64_t gi = ((int64_t)(z0 + pz) * g.Zp[1] + (y0 + py)) * g.Zp[2] + (x0 + px);
        grid_add<M2>(ncls, t, pz, py, px, res, res2, g.agg + gi, g.cnt ? g.cnt + gi : nullptr, M2 ? g.agg2 + gi : nullptr, ZYXp);
    }
}

// The tiles of one forward in ONE launch: a launch per tile reads and rewrites agg / cnt once per tile, eight times for a voxel that
// eight tiles cover.  One thread = one voxel of the padded grid inside the bounding box [lo, lo + B) of the tiles; it loads agg / cnt
// once, walks the tiles in their order - tile i's logits are samples i * n_mirrors .. of `logits` - and adds, for each tile that
// holds the voxel, that tile's term (tile_term_add) to the value it carries: the same additions in the same order as the
// launches per tile, so the result is bit-identical.  A voxel that no tile holds is not written.
struct AggTileList {
    int n;
    int org[LOGITS_AGG_MAX_TILES][3];
    int lo[3], B[3];
};
static_assert(sizeof(AggTileList) + sizeof(AggTile) + sizeof(AggGrid) + sizeof(const float *) + sizeof(int) <= 4096,
              "the aggregation's arguments must fit the kernel-argument block");
template <bool M2>
__global__ __launch_bounds__(256) void logits_aggregate_tiles_kernel(const float *logits, int ncls, AggTile t, AggGrid g, AggTileList tl) {
    const int64_t PV = (int64_t)t.P[0] * t.P[1] * t.P[2];
    const int64_t BV = (int64_t)tl.B[0] * tl.B[1] * tl.B[2];
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < BV; v += (int64_t)gridDim.x * blockDim.x) {
        const int x = tl.lo[2] + (int)(v % tl.B[2]);
        const int y = tl.lo[1] + (int)((v / tl.B[2]) % tl.B[1]);
        const int z = tl.lo[0] + (int)(v / ((int64_t)tl.B[2] * tl.B[1]));
        const int64_t gi = ((int64_t)z * g.Zp[1] + y) * g.Zp[2] + x;
        float acc[HEAD_MAX_CLS];
        float acc2[M2 ? HEAD_MAX_CLS : 1];
        float c = 0.f;
        bool held = false;
        for (int i = 0; i < tl.n; ++i) {
            const int pz = z - tl.org[i][0], py = y - tl.org[i][1], px = x - tl.org[i][2];
            if ((unsigned)pz >= (unsigned)t.P[0] || (unsigned)py >= (unsigned)t.P[1] || (unsigned)px >= (unsigned)t.P[2]) continue;
            if (!held) {
                grid_load<M2>(g, ncls, gi, acc, c, acc2);
                held = true;
            }
            tile_term_add<M2>(LogitsSource{logits + (int64_t)i * t.ml.n * ncls * PV}, ncls, t, pz, py, px, acc, &c, acc2);
        }
        if (held) grid_store<M2>(g, ncls, gi, acc, c, acc2);
    }
}

// f(std::true_type or std::false_type): a run-time flag as a template argument
template <typename F>
static void dispatch(bool flag, F f) {
    if (flag) f(std::true_type());
    else f(std::false_type());
}

static int moments_check(const char *what, const AggTile &t, const AggGrid &g) {
    MI355_REQUIRE(!g.agg2 || t.nonlin != MI355_NONLIN_IDENTITY, "%s: the second moment needs probabilities (nonlin identity has none)", what);
    return MI355_OK;
}

template <int NM, typename Source>
static void launch_tile(const Source &src, int ncls, const AggTile &t, const AggGrid &g, const int org[3], hipStream_t s) {
    const int64_t PV = (int64_t)t.P[0] * t.P[1] * t.P[2];
    int64_t blocks = (PV + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    dispatch(g.agg2 != nullptr, [&](auto m2) {
        hipLaunchKernelGGL((head_aggregate_kernel<decltype(m2)::value, NM, Source>), dim3((unsigned)blocks), dim3(256), 0, s, src, ncls, t, g, org[0],
                           org[1], org[2]);
    });
}

int head_aggregate(const HeadWeights &w, const void *feat, int dtype, int first_sample, const AggTile &t, const AggGrid &g, const int org[3],
                   hipStream_t s, const FeatNorm &fn_all) {
    MI355_TRY(moments_check("head_aggregate", t, g));
    const size_t first = (size_t)first_sample * t.P[0] * t.P[1] * t.P[2] * w.cin;
    FeatNorm fn = fn_all;  // rows of this tile's first sample
    if (fn.scale) { fn.scale += (size_t)first_sample * w.cin; fn.shift += (size_t)first_sample * w.cin; }
    dispatch(dtype == MI355_F16, [&](auto f16) {
        typedef typename std::conditional<decltype(f16)::value, _Float16, float>::type T;
        dispatch(fn.scale != nullptr, [&](auto norm) {
            const HeadSource<T, decltype(norm)::value> src = {(const T *)feat + first, w.w_dev, w.b_dev, w.cin, fn};
            if (t.ml.n == 8) launch_tile<8>(src, w.ncls, t, g, org, s);
            else launch_tile<0>(src, w.ncls, t, g, org, s);
        });
    });
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// Same as head_aggregate when the last conv already applied the head (logits [n_samples][ncls][PV]).
int logits_aggregate(const float *logits, int ncls, int first_sample, const AggTile &t, const AggGrid &g, const int org[3], hipStream_t s) {
    MI355_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS, "logits_aggregate: bad arguments");
    MI355_TRY(moments_check("logits_aggregate", t, g));
    const int64_t PV = (int64_t)t.P[0] * t.P[1] * t.P[2];
    launch_tile<0>(LogitsSource{logits + (size_t)first_sample * ncls * PV}, ncls, t, g, org, s);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// origins_host: [n_tiles][3], inside the padded grid (the caller checks).  More than LOGITS_AGG_MAX_TILES tiles run as consecutive
// launches in order, each over the bounding box of its own tiles.
int logits_aggregate_tiles(const float *logits, int ncls, int first_sample, const AggTile &t, const AggGrid &g, const int *origins_host, int n_tiles,
                           hipStream_t s) {
    MI355_REQUIRE(ncls >= 1 && ncls <= HEAD_MAX_CLS && n_tiles >= 1, "logits_aggregate_tiles: bad arguments");
    MI355_TRY(moments_check("logits_aggregate_tiles", t, g));
    const int64_t PV = (int64_t)t.P[0] * t.P[1] * t.P[2];
    for (int t0 = 0; t0 < n_tiles; t0 += LOGITS_AGG_MAX_TILES) {
        AggTileList tl = {};
        tl.n = std::min(LOGITS_AGG_MAX_TILES, n_tiles - t0);
        int hi[3];
        for (int i = 0; i < tl.n; ++i)
            for (int a = 0; a < 3; ++a) {
                const int o = origins_host[(size_t)(t0 + i) * 3 + a];
                tl.org[i][a] = o;
                tl.lo[a] = i ? std::min(tl.lo[a], o) : o;
                hi[a] = i ? std::max(hi[a], o + t.P[a]) : o + t.P[a];
            }
        for (int a = 0; a < 3; ++a) tl.B[a] = hi[a] - tl.lo[a];
        const int64_t BV = (int64_t)tl.B[0] * tl.B[1] * tl.B[2];
        int64_t blocks = (BV + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        const float *first = logits + ((size_t)first_sample + (size_t)t0 * t.ml.n) * ncls * PV;
        dispatch(g.agg2 != nullptr, [&](auto m2) {
            hipLaunchKernelGGL(logits_aggregate_tiles_kernel<decltype(m2)::value>, dim3((unsigned)blocks), dim3(256), 0, s, first, ncls, t, g, tl);
        });
        MI355_HIP(hipGetLastError());
    }
    return MI355_OK;
}

__global__ void cnt_add_tile_kernel(AggTile t, AggGrid g, int z0, int y0, int x0) {
    const int64_t PV = (int64_t)t.P[0] * t.P[1] * t.P[2];
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < PV; v += (int64_t)gridDim.x * blockDim.x) {
        const int px = (int)(v % t.P[2]);
        const int py = (int)((v / t.P[2]) % t.P[1]);
        const int pz = (int)(v / ((int64_t)t.P[2] * t.P[1]));
        g.cnt[((int64_t)(z0 + pz) * g.Zp[1] + (y0 + py)) * g.Zp[2] + (x0 + px)] += t.gauss ? t.gauss[v] : 1.0f;
    }
}

int cnt_add_tile(const AggTile &t, const AggGrid &g, const int org[3], hipStream_t s) {
    const int64_t PV = (int64_t)t.P[0] * t.P[1] * t.P[2];
    int64_t blocks = (PV + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(cnt_add_tile_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t, g, org[0], org[1], org[2]);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// ------------------------------------------------------------------ finish
// The volume [Z][Y][X] sits at `pad` inside the padded grid.
struct CropBox {
    int Z, Y, X, pz, py, px;
};
static __device__ __forceinline__ int64_t crop_index(const CropBox &b, const AggGrid &g, int64_t v) {
    const int x = (int)(v % b.X);
    const int y = (int)((v / b.X) % b.Y);
    const int z = (int)(v / ((int64_t)b.X * b.Y));
    return ((int64_t)(z + b.pz) * g.Zp[1] + (y + b.py)) * g.Zp[2] + (x + b.px);
}

// class_probabilities = aggregated / normaliser, cropped back from the padded grid.
__global__ void finish_probs_kernel(AggGrid g, int C, CropBox b, float *probs, int accumulate) {
    const int64_t ZYX = (int64_t)b.Z * b.Y * b.X, ZYXp = (int64_t)g.Zp[0] * g.Zp[1] * g.Zp[2];
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < ZYX; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gi = crop_index(b, g, v);
        const float c = g.cnt[gi];
        for (int k = 0; k < C; ++k) {
            const float p = g.agg[k * ZYXp + gi] / c;
            if (accumulate)
                probs[k * ZYX + v] += p;
            else
                probs[k * ZYX + v] = p;
        }
    }
}

int finish_probs(const AggGrid &g, int C, const int vol[3], const int pad[3], float *probs, int accumulate, hipStream_t s) {
    const CropBox b = {vol[0], vol[1], vol[2], pad[0], pad[1], pad[2]};
    const int64_t ZYX = (int64_t)b.Z * b.Y * b.X;
    int64_t blocks = (ZYX + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(finish_probs_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g, C, b, probs, accumulate);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// Both moments of one ensemble member, cropped back from the padded grid: mean = agg / cnt / n_folds with the two divisions of
// finish_probs_kernel followed by scale_kernel (x / 1.0f is x: the same bits as without the second division), m2 likewise from agg2.
__global__ void finish_moments_kernel(AggGrid g, int C, CropBox b, float n_folds, float *mean, float *m2) {
    const int64_t ZYX = (int64_t)b.Z * b.Y * b.X, ZYXp = (int64_t)g.Zp[0] * g.Zp[1] * g.Zp[2];
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < ZYX; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gi = crop_index(b, g, v);
        const float c = g.cnt[gi];
        for (int k = 0; k < C; ++k) {
            const float p = g.agg[k * ZYXp + gi] / c;
            const float q = g.agg2[k * ZYXp + gi] / c;
            mean[k * ZYX + v] = p / n_folds;
            m2[k * ZYX + v] = q / n_folds;
        }
    }
}

int finish_moments(const AggGrid &g, int C, const int vol[3], const int pad[3], int n_folds, float *mean, float *m2, hipStream_t s) {
    const CropBox b = {vol[0], vol[1], vol[2], pad[0], pad[1], pad[2]};
    const int64_t ZYX = (int64_t)b.Z * b.Y * b.X;
    int64_t blocks = (ZYX + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(finish_moments_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g, C, b, (float)n_folds, mean, m2);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

__global__ void scale_kernel(float *x, int64_t n, float divisor) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        x[i] = x[i] / divisor;
}

int scale_inplace(float *x, int64_t n, float divisor, hipStream_t s) {
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, n, divisor);
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

}  // namespace mi355

