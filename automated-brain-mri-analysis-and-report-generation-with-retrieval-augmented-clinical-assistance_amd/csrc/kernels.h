// Host-side launchers of the gfx950 kernels (declarations).  All tensors are NDHWC.
#pragma once
#include <vector>

#include "common.h"

namespace mi355 {

enum { ACT_NONE = 0, ACT_LRELU = 1 };

// ---------------------------------------------------------------- conv 3x3x3 (implicit GEMM)
// Weights packed for the MFMA B operand; see pack_conv_weights_f32 in conv3d.hip.
struct ConvWeights {
    int cin = 0, cin_pad = 0, cout = 0, stride = 1;
    int cc = 0;               // channel chunk staged in LDS per pass
    int nf = 1;               // 32-wide cout fragments per workgroup
    bool pipe = false;        // pipelined (persistent, double-buffered) kernel; implies cc == 8
    float *wp_dev = nullptr;  // packed weights (device), chunk size cc
    float *wp16_dev = nullptr;  // second pack with 16-channel chunks for the 512-voxel-tile simple kernel (auto mode)
    float *wpw_dev = nullptr;   // Winograd pack F(2x2,3x3) over (z, y) (stride 1, 16-channel chunks, 32-cout blocks)
    float *wp3_dev = nullptr;   // 3-D Winograd pack F(2x2x2,3x3x3) (conv3d_wino3.hip; stride 1, 16-channel chunks, 32-cout blocks)
    uint16_t *wps_dev = nullptr;  // split-bf16 pack of the fp32 stride-2 LDS-DMA kernel (pack_conv_weights_s2split; stride 2, cc == 8, nf == 2), 1.5x wp_dev
    float *bias_dev = nullptr;
    float *w_plain_dev = nullptr;  // [cout][cin][27] PyTorch order (direct kernel / tests)
    size_t wp_bytes = 0;
};

// Which packs a layer gets, or why the layer is refused (pure: conv_weights_upload follows it; a plan can be computed from it
// without uploading anything).  Every *_weights_upload allocates in the DeviceAllocs it is given (common.h) and nowhere else: the
// weight structs are views of that owner's memory, and what a refused or failed upload had allocated goes with the owner.
struct ConvPackLayout {
    bool mfma = false;  // the MFMA pack exists (cout % 32 == 0, cin_pad % 8 == 0); otherwise the layer runs on the direct kernel
    int cc = 0, nf = 1;
    bool pipe = false;
    bool c16 = false, wino2 = false, wino3 = false;  // the second 16-channel-chunk pack, the F(2x2,3x3) and F(2x2x2,3x3x3) packs
};
int conv_pack_layout(int cin, int cin_pad, int cout, int stride, ConvPackLayout *out);
int conv_weights_upload(DeviceAllocs &mem, const float *w_host, const float *bias_host, int cin, int cin_pad, int cout,
                        int stride, bool keep_plain, ConvWeights *out);

// A per-sample view into a whole-volume tensor of the shared stage 0 (sw_share_plan.hip "stage-0 views"): the tile tensor [N][D][H][W][C] a
// conv reads is written only inside the shells - within `depth` voxels of a tile face whose bit is set - and every other voxel of
// sample n is read in place from `src` at smp[n].off + (z * sz + y * sy + x) voxels.  Voxel (z, y, x) of sample n comes from the tile
// tensor iff z < depth with face bit 0, z >= D - depth with bit 1, the same for y (bits 2, 3) and x (bits 4, 5); the reader's
// out-of-tile test comes first, so halo pieces beyond a tile face stay zero although the view has neighbours there.
// Passed by value inside the kernel arguments.  Built by stage0_view_make (below), which refuses a view that leaves its tensor.
constexpr int S0_VIEW_MAX_SAMPLES = 64;  // = S0_MAX_SAMPLES
struct S0ViewSample {
    unsigned off;    // voxel index of the tile's origin in src: (wv * Ve0 + org0) * Ve1 * Ve2 + org1 * Ve2 + org2
    unsigned faces;  // bit f = face f (z lo, z hi, y lo, y hi, x lo, x hi) lies inside the volume: its shell comes from the tile tensor
};
struct S0View {
    const float *src = nullptr;  // [n_wv][Ve0][Ve1][Ve2][C], C = the reader's channel count; null = no view
    int sy = 0, sz = 0;          // row and plane strides in voxels: Ve2, Ve1 * Ve2
    int depth = 0;               // shell depth
    S0ViewSample smp[S0_VIEW_MAX_SAMPLES];
};

// One 3x3x3 conv call; T = the element type of the activations (ConvCall = fp32 NDHWC, ConvCallH = fp16 channel-blocked).
template <typename T>
struct ConvCallT {
    const T *in0 = nullptr;  // [N,Di,Hi,Wi,C0]
    const T *in1 = nullptr;  // [N,Di,Hi,Wi,C1] second half of a virtual concat, or null
    int C0 = 0, C1 = 0;
    int N = 0, Di = 0, Hi = 0, Wi = 0;
    T *out = nullptr;         // [N,Do,Ho,Wo,Cout]
    double *stats = nullptr;  // [N][Cout][2] (sum, sum of squares) accumulated when non-null
    int act = ACT_NONE;
    float slope = 0.01f;
    // fused 1x1x1 segmentation head (last decoder conv, Cout = one workgroup's couts): when head_out is set the
    // feature map is NOT stored; logits [N][ncls][Vo] fp32 = head_w [ncls][Cout] . act(conv) + head_b are
    const float *head_w = nullptr, *head_b = nullptr;
    float *head_out = nullptr;
    int head_ncls = 0;
    // in0 is the RAW conv output of the previous block: apply x * in_scale[n][c] + in_shift[n][c] (+ LeakyReLU when in_act) while
    // staging it (only where conv3d_wino3_fuses_input_norm / conv3d_f16_fuses_input_norm says so: the F(2x2x2,3x3x3) kernel
    // normalises its brick in LDS, the fp16 kernels while staging)
    const float *in_scale = nullptr, *in_shift = nullptr;
    int in_act = ACT_NONE;
    // [N,Do,Ho,Wo,Cout] added to the conv sum in front of bias and activation: out = act(bias + conv(in) + addend).  The shared
    // skip half of a split concat conv (sw_share_plan.hip "shared skip half"); conv3_f32_wino3_kernel<3, false> only (the plain epilogue's twin), refused elsewhere.
    const T *addend = nullptr;
    // Stage-0 views (fp32): in0 / addend hold their shells only, the rest is read through the view.  The planner never looks at
    // them - a view must not change which kernel runs -; the launcher refuses a view on a kernel that cannot read through one
    // (in0_view: conv3_f32_s2dma_kernel_view, C1 == 0; addend_view: conv3_f32_wino3_kernel<3, false>).
    const S0View *in0_view = nullptr, *addend_view = nullptr;
    // Opt-in hint to the stride-2 LDS-DMA planner (plan_s2dma, fp32): take the tile shape, 2 x 2 x 32 or 2 x 4 x 16, whose padded
    // output columns times padded rows are fewer (ties: 2 x 2 x 32) instead of asking Wo >= 24.  Both shapes sum an output voxel
    // in the same order, so the hint changes which lanes are wasted, never a value.  Unset, every call plans as it always did.
    bool s2_least_padding = false;
};
typedef ConvCallT<float> ConvCall;
typedef ConvCallT<_Float16> ConvCallH;
int conv3d_mfma_f32(const ConvWeights &w, const ConvCall &c, hipStream_t s, const char **kernel_name = nullptr);
// conv3_f32_s2dma_kernel (or, with c.in0_view, its view instantiation) whatever the planner would pick; `force`: also below the
// fill-the-chip rule.  Test aid of the stage-0 views.
int conv3d_s2dma_f32(const ConvWeights &w, const ConvCall &c, bool force, hipStream_t s, const char **kernel_name = nullptr);
// F(2x2x2, 3x3x3) kernel (conv3d_wino3.hip)
void pack_conv_weights_s2split(const float *w, int cin, int cin_pad, int cout, std::vector<uint16_t> &out);  // conv3d.hip
void pack_conv_weights_wino3(const float *w, int cin, int cin_pad, int cout, std::vector<float> &out);
bool conv3d_wino3_enabled();
bool conv3d_wino3_fuses_input_norm(const ConvWeights &w, const ConvCall &c);
int plan_conv_direct(const ConvWeights &w, const ConvCall &c);  // the direct kernel's own refusals
int conv3d_direct_f32(const ConvWeights &w, const ConvCall &c, hipStream_t s);

// first conv of the network (Cin <= 4): x-taps folded into K, NDHW4 input (conv_stem.hip)
struct StemWeights {
    int cin = 0, cout = 0, dtype = 0;
    void *wp_dev = nullptr;
    float *bias_dev = nullptr;
};
int stem_weights_upload(DeviceAllocs &mem, const float *w_host, const float *bias_host, int cin, int cout, int dtype, StemWeights *out);
int conv3d_stem(const StemWeights &w, const void *in, int N, int D, int H, int W, void *out, double *stats, int act,
                float slope, hipStream_t s);

// fp16 storage / fp32 accumulate variants (conv3d_f16.hip)
struct ConvWeightsH {
    int cin = 0, cin_pad = 0, cout = 0, stride = 1, nf = 1;
    _Float16 *wp_dev = nullptr;
    float *bias_dev = nullptr;
};
int conv_pack_layout_f16(int cin, int cin_pad, int cout, int stride, int *nf);  // as conv_pack_layout: the refusals and nf
int conv_weights_upload_f16(DeviceAllocs &mem, const float *w_host, const float *bias_host, int cin, int cin_pad, int cout, int stride,
                            ConvWeightsH *out);
bool conv3d_f16_fuses_input_norm(const ConvWeightsH &w, const ConvCallH &c);
int conv3d_mfma_f16(const ConvWeightsH &w, const ConvCallH &c, hipStream_t s, const char **kernel_name = nullptr);

// ---------------------------------------------------------------- transposed conv k=2 s=2
struct TConvWeights {
    int cin = 0, cout = 0, dtype = 0;
    void *wp_dev = nullptr;  // packed float (MI355_F32) or _Float16 (MI355_F16)
};
int tconv_weights_upload(DeviceAllocs &mem, const float *w_host, int cin, int cout, int dtype, TConvWeights *out);
// in [N,D,H,W,Cin] -> out [N,2D,2H,2W,Cout], elements of w.dtype (fp16: channel-blocked)
int tconv2_mfma(const TConvWeights &w, const void *in, int N, int D, int H, int W, void *out, hipStream_t s,
                const char **kernel_name = nullptr);

// ---------------------------------------------------------------- elementwise.hip: normalisation, tile extraction, layouts
// stats [N][C][2] doubles -> scale/shift [N][C] so that y = x*scale + shift.
int norm_finalize(const double *stats, int N, int C, int64_t count, int kind, int groups, float eps,
                  const float *gamma, const float *beta, float *scale, float *shift, hipStream_t s);
// in place: x = act(x*scale[n][c] + shift[n][c]) over [N][V][C]
int norm_apply(void *x, int dtype, int N, int64_t V, int C, const float *scale, const float *shift, int act,
               float slope, hipStream_t s);

struct TileDesc {  // one forward sample = one (tile, mirror)
    int z0, y0, x0;  // origin in the padded volume
    int mirror;      // bit0 flip z, bit1 flip y, bit2 flip x
};
// vol [C][Z][Y][X] (unpadded; pad offsets give where it sits in the padded volume)
// -> x [n_samples][P0][P1][P2][Cpad] (channels >= C are zero)
int extract_tiles(const float *vol, int C, int Z, int Y, int X, int padz, int pady, int padx,
                  const TileDesc *tiles_host, int n_samples, int P0, int P1, int P2, int Cpad, void *x, int dtype,
                  hipStream_t s);
// plain NDHWC <-> channel-blocked [N][C / 8][V][8] fp16 (common.h)
int ndhwc_to_b8(const _Float16 *x, int N, int C, int64_t V, _Float16 *y, hipStream_t s);
int b8_to_ndhwc(const _Float16 *x, int N, int C, int64_t V, _Float16 *y, hipStream_t s);
// NCDHW -> NDHWC(Cpad) for the plain forward API
int nchw_to_ndhwc(const float *x, int N, int C, int64_t V, int Cpad, void *y, int dtype, hipStream_t s);

// ---------------------------------------------------------------- stage0_gather.hip: the shared stage 0's tile tensors
// Shared stage 0 of the sliding window (sw_share_plan.hip "shared stage 0"): encoder stage 0 runs once over the whole padded volume and
// over thin slabs at the tile faces that lie inside the volume; the tile tensor is then gathered from those results.
constexpr int S0_MAX_SAMPLES = 64;
struct S0Sample {   // one forward sample = one (tile, mirror), in the coordinates of its (mirrored) pass
    int wv;         // which whole-volume result (index of the mirror)
    int org[3];     // tile origin in that volume
    int slab[6];    // faces z lo, z hi, y lo, y hi, x lo, x hi: index into that axis's slab batch, or -1 (the face is a volume face)
};
struct S0GatherArgs {
    const float *wv;       // [n_mirrors][Ve0][Ve1][Ve2][C]
    const float *slab[3];  // per axis a: [n_slabs][S0][S1][S2][C], S[a] = t[a], S[k] = P[k] otherwise
    float *out;            // [n_samples][P0][P1][P2][C]
    int P[3], Ve[3], t[3];
    // Merged slabs (sw_share_plan.hip "merged slabs"): D[a] = extent of one slab of axis a - t[a] along a; along k != a either P[k] (the slab
    // carries the tile's own padding: the tile starts at 0 in it) or Ve[k] (the slab spans the volume: the tile starts at its origin,
    // so[a][k] = 1).  stage0_gather_dense() fills the per-tile form: D[a][k] = P[k], so = 0.
    int D[3][3], so[3][3];
    int r;                 // voxel layers taken from a slab at each of its faces
    int C4;                // C / 4
    // optional second tensor gathered for the same samples (out2 == nullptr: none): the shared skip half of the last decoder
    // stage's concat conv, C42 * 4 channels, taken r2 >= r layers deep from the slabs (t >= 2 r2)
    const float *wv2;
    const float *slab2[3];
    float *out2;
    int r2, C42;
    int n;                 // samples (set by stage0_gather)
    S0Sample smp[S0_MAX_SAMPLES];
    // Sub-boxes (sw_share_plan.hip "shared level 1"; T[0] > 0): sample i is the P-sized box at sub[i] of a tile of T voxels, org
    // its own origin in the volume; in a slab that carries the tile's own padding along k (so[a][k] = 0: D[a][k] = T[k]) it
    // starts at sub[i][k], not at 0.  T = 0 and sub = 0: the samples are the tiles.
    int T[3];
    int sub[S0_MAX_SAMPLES][3];
};
// the slabs of every axis have the tile's extent across their axis (the form before merged slabs)
inline void stage0_gather_dense(S0GatherArgs *a) {
    for (int ax = 0; ax < 3; ++ax)
        for (int k = 0; k < 3; ++k) { a->D[ax][k] = k == ax ? a->t[k] : a->P[k]; a->so[ax][k] = 0; }
}
// fp32 NDHWC, 16 bytes per lane.  Where the shells of two or three faces meet the first face in the order above wins.
// by_box: launched over the output boxes (stage0_gather_box_kernel: thin sub-boxes) instead of over the whole volume's rows; the
// same values.  A gather of two tensors, or of 2^31 quads and more, takes the row form whatever by_box says.
int stage0_gather(const S0GatherArgs &a, int n_samples, hipStream_t s, bool by_box = false);
// The same for a tensor whose reader takes a stage-0 view (S0View): only the voxels within r of a face that has a slab are written,
// from the sources and with the precedence of stage0_gather; the rest of the tile tensor is left as it is.  which = 0: the first
// tensor of `a` (out, depth r), 1: the second (out2, depth r2).
int stage0_gather_shells(const S0GatherArgs &a, int n_samples, int which, hipStream_t s);
// voxels of a P0 x P1 x P2 tile within r of a face f with faces[f] >= 0 (host; what stage0_gather_shells writes per sample)
int64_t stage0_shell_voxels(const int P[3], int r, const int faces[6]);
// The view of n samples (wv, org and faces as in S0Sample: slab[f] >= 0 sets face bit f) of P0 x P1 x P2 voxels into src
// [n_wv][Ve0][Ve1][Ve2][C], shell depth `depth`.  Pure host code.  Refused (MI355_ERR_INVALID, *out left without a source): a
// sample that leaves its tensor (wv >= n_wv, org + P > Ve), a shell deeper than half a tile, more than S0_VIEW_MAX_SAMPLES
// samples, or a tensor so large that an offset a kernel forms in 32 bits would not fit (n_wv * Ve0 * Ve1 * Ve2 * C >= 2^31).
int stage0_view_make(const float *src, int n_wv, const int Ve[3], const int P[3], int C, int depth, const S0Sample *smp, int n, S0View *out);
// x [N][Ve0][Ve1][Ve2][C] fp32: zero every voxel outside [0, Zp) (C % 4 == 0)
int stage0_mask(float *x, int N, const int Ve[3], const int Zp[3], int C, hipStream_t s);

// ---------------------------------------------------------------- aggregate.hip: segmentation head, sliding-window aggregation
struct HeadWeights {
    int cin = 0, ncls = 0;
    float *w_dev = nullptr;  // [ncls][cin]
    float *b_dev = nullptr;  // [ncls]
};
int head_weights_upload(DeviceAllocs &mem, const float *w_host, const float *b_host, int cin, int ncls, HeadWeights *out);
// The feature map handed to the head may be the RAW output of the last decoder conv: then scale / shift [N][C] (fp32) hold
// its Instance/GroupNorm affine and the head applies act(x * scale + shift) per channel while it reads the features
// (slope = 1: no activation).  scale == nullptr: the features are final.
struct FeatNorm {
    const float *scale = nullptr, *shift = nullptr;
    float slope = 1.0f;
};
// feat [N][V][C] -> logits [N][ncls][V]
int head_logits(const HeadWeights &w, const void *feat, int dtype, int N, int64_t V, float *logits, hipStream_t s,
                const FeatNorm &fn = FeatNorm());

// The operands of the aggregation by name; passed by value inside the kernel arguments.
struct MirrorList {  // the mirror masks of a tile's samples, in sample order (bit0 flip z, bit1 flip y, bit2 flip x)
    int n;
    int m[8];
};
int make_mirrors(const char *what, const int *mirrors_host, int n, MirrorList *out);  // refuses n outside 1 .. 8 ("<what>: n mirrors")
struct AggTile {         // what every tile of a forward shares
    int P[3];            // patch
    int nonlin;          // MI355_NONLIN_*
    const float *gauss;  // [P0][P1][P2] weights, or null: 1
    MirrorList ml;
};
struct AggGrid {  // the padded grid the tiles are added into
    float *agg;   // [ncls][Zp0][Zp1][Zp2]
    float *agg2;  // the same shape: the second moment, or null: not kept
    float *cnt;   // [Zp0][Zp1][Zp2] normaliser, or null (the aggregation kernels only)
    int Zp[3];
};
// One tile at org: result = sum_m (1/n_mirrors) * flip_back(nonlin(head(feat[first_sample+m])));
// agg[c][tile] += result * gauss ; cnt[tile] += gauss.
// agg2 (here and in the two below): agg2[c][tile] += (sum_m (1/n_mirrors) * p^2) * gauss, the second moment of the
// same samples; agg and cnt come out bit-identical with and without it.  nonlin identity is refused with agg2.
int head_aggregate(const HeadWeights &w, const void *feat, int dtype, int first_sample, const AggTile &t, const AggGrid &g, const int org[3],
                   hipStream_t s, const FeatNorm &fn = FeatNorm());
// same as head_aggregate for forwards whose last conv already produced logits [n_samples][ncls][PV]; bit-identical to
// head_aggregate of the features behind those logits
int logits_aggregate(const float *logits, int ncls, int first_sample, const AggTile &t, const AggGrid &g, const int org[3], hipStream_t s);
// The same for n_tiles tiles of one forward in one launch (per LOGITS_AGG_MAX_TILES tiles): tile i's logits are samples
// first_sample + i * n_mirrors .., its origin origins_host[3 i ..]; bit-identical to logits_aggregate called tile by tile in order.
constexpr int LOGITS_AGG_MAX_TILES = 64;
int logits_aggregate_tiles(const float *logits, int ncls, int first_sample, const AggTile &t, const AggGrid &g, const int *origins_host, int n_tiles,
                           hipStream_t s);
// cnt[tile] += gauss (or 1): the normaliser of a tile this rank does not evaluate itself
int cnt_add_tile(const AggTile &t, const AggGrid &g, const int org[3], hipStream_t s);
// probs[c][z][y][x] (+)= agg[c][z+pad0][y+pad1][x+pad2] / cnt[...] over the volume vol = (Z, Y, X); then optional scale (fold mean)
int finish_probs(const AggGrid &g, int C, const int vol[3], const int pad[3], float *probs, int accumulate, hipStream_t s);
int scale_inplace(float *x, int64_t n, float divisor, hipStream_t s);
// mean[c][z][y][x] = agg / cnt / n_folds (the bits of finish_probs then scale_inplace), m2 the same from agg2
int finish_moments(const AggGrid &g, int C, const int vol[3], const int pad[3], int n_folds, float *mean, float *m2, hipStream_t s);

}  // namespace mi355
