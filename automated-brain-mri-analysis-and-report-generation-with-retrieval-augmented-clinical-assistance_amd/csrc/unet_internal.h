// What the five host files behind include/mi355_nnunet.h share, and nobody else includes:
//   runtime.hip         last-error text, bind_device, the lanes and device_scratch, the scratch test aids, DeviceAllocs
//   unet.hip            the network object, the arena plan, run_block / forward_features, create / destroy / forward / profile
//   sw_share_plan.hip   pure: tile geometry, what overlapping tiles share as one plan per window, the geometry dry runs
//   sliding_window.hip  the device side of that plan: the shared stage 0 and level 1 passes, sw_accumulate, mi355_sw_*
//   single_op.hip       the single-op entry points the tests drive, mi355_conv3d_plan, the wrappers around the three files below
// and, behind kernels.h, the kernels around the convolutions by role:
//   elementwise.hip     norm finalise / apply, tile extraction, layout conversions, export / ensemble / z-score entry points
//   stage0_gather.hip   the shared stage 0's gathers (row, box, shells), stage0_view_make, stage0_mask
//   aggregate.hip       the segmentation head, the sliding-window aggregation over one tile term, the normaliser, the finish
// Types and the few functions that cross those files; a function used in one file is static there.
#pragma once
#include <array>
#include <string>
#include <vector>

#include "conv_plan.h"

namespace mi355 {

struct ConvLayer {
    ConvWeights w;     // MI355_F32
    ConvWeightsH wh;   // MI355_F16
    StemWeights stem;  // first conv of the net when Cin <= 4 (either dtype)
    bool is_stem = false;
    float *gamma_dev = nullptr, *beta_dev = nullptr;  // Instance/GroupNorm affine, or BN scale/shift (nonlin_first)
    bool runtime_norm = false;                        // statistics needed at run time (IN / GN)
    bool post_affine = false;                         // BN that could not be folded (nonlin_first)
    int cin = 0, cout = 0, stride = 1;
    // shared skip half (fp32, first block of the last decoder stage): the block's weights split at the concat boundary,
    // w_up = W[:, :split_c0] with the block's bias, w_skip = W[:, split_c0:] with zero bias; split_c0 = 0: not split
    ConvWeights w_up, w_skip;
    int split_c0 = 0;
};

}  // namespace mi355

struct mi355_unet {
    int in_channels = 0, cin_pad = 0, num_classes = 0, num_pool = 0;
    int norm = 0, num_groups = 0, nonlin_first = 0, dtype = 0;
    float eps = 1e-5f, slope = 0.01f;
    std::vector<std::vector<mi355::ConvLayer>> enc;  // num_pool + 1 stages
    std::vector<std::vector<mi355::ConvLayer>> dec;  // num_pool stages
    std::vector<mi355::TConvWeights> tu;
    mi355::HeadWeights head;
    mi355::DeviceAllocs mem;  // owns every weight above (the structs are views of it); freed with the handle
    // (the activation arena is not the handle's: one per LANE = per stream the caller launches on, shared by every handle that
    //  runs on that stream - device_scratch(SCR_ARENA, stream); a forward carries its pointer in its Plan)
    // gaussian importance map cache (an owner of its own: ensure_gaussian releases it when the patch changes)
    mi355::DeviceAllocs gauss_mem;
    float *gauss_dev = nullptr;
    int gauss_p[3] = {0, 0, 0};
    int max_channels = 0;
    // optional per-kernel HIP-event timing (bench.py roofline)
    bool prof_on = false;
    struct ProfRec { std::string name; double flops, bytes; hipEvent_t a, b; };
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> event_pool;  // events are recycled: nothing is created inside a timed region after warm-up
};

namespace mi355 {

inline int require_device() { return bind_device(); }

// ---- arena layout for one (N, D, H, W): per level four activation buffers + norm scratch
struct Plan {
    std::vector<int64_t> vox;          // voxels per sample at each level
    std::vector<int> maxc;             // widest tensor at each level
    std::vector<size_t> off[4];        // byte offsets of buffers A, B, U, T per level
    size_t stats_off = 0, scale_off = 0, shift_off = 0, x0_off = 0, total = 0;
    size_t scale2_off = 0, shift2_off = 0;  // second scale / shift pair: a block whose normalisation is applied by its consumer
    size_t stats_bytes = 0;
    char *arena = nullptr;             // the activation arena of the lane (stream) this forward runs on, set by ensure_arena
    // shared stage 0 (stage0_plan): whole-volume input / intermediate / result and the slab buffers, behind the tile plan
    struct { size_t wv_in = 0, wv_tmp[2] = {0, 0}, wv_out = 0, slab_in = 0, slab_tmp[2] = {0, 0}, slab_out[3] = {0, 0, 0};
             size_t wv_skip = 0, slab_skip[3] = {0, 0, 0}; } s0;  // (shared skip half: S over the whole volume and over the slabs)
    // shared level 1 (level1_plan): the regions' stage-0 slabs and level-0 shells, their level-1 tensors, and per forward the
    // level-0 sub-boxes of the tile slabs and their level-1 tensors
    struct { size_t rs_in = 0, rs_tmp[2] = {0, 0}, rs_out[3] = {0, 0, 0}, r_shell = 0, r_e[2] = {0, 0}, r_s = 0;
             size_t sub_in[3] = {0, 0, 0}, s_tmp = 0, s_e[3] = {0, 0, 0}, s_s[3] = {0, 0, 0}; } l1;
};
int make_plan(const mi355_unet &net, int N, int D, int H, int W, Plan *pl);
// appends 256-byte-aligned regions to an arena plan: starts at Plan::total, which receives `o` when the last one is taken
struct ArenaCursor { size_t o; size_t take(size_t bytes) { const size_t r = o; o += (bytes + 255) & ~size_t(255); return r; } };
int ensure_arena(Plan *pl, hipStream_t s);

struct ProfScope {
    mi355_unet *net; hipStream_t s; bool on; size_t idx;
    ProfScope(mi355_unet *n, hipStream_t st, const std::string &name, double flops, double bytes) : net(n), s(st), on(n->prof_on), idx(0) {
        if (!on) return;
        mi355_unet::ProfRec r; r.name = name; r.flops = flops; r.bytes = bytes;
        auto take = [&](hipEvent_t *e) {
            if (!net->event_pool.empty()) { *e = net->event_pool.back(); net->event_pool.pop_back(); return true; }
            return hipEventCreate(e) == hipSuccess;
        };
        if (!take(&r.a) || !take(&r.b)) { on = false; return; }
        (void)hipEventRecord(r.a, s);
        idx = net->prof.size();
        net->prof.push_back(r);
    }
    void rename(const char *name, const char *suffix = "") { if (on && name) net->prof[idx].name = std::string(name) + suffix; }
    ~ProfScope() { if (on) (void)hipEventRecord(net->prof[idx].b, s); }
};

// The fused operands a conv call may carry besides its first input (plain pointers; the single-op fp16 path converts x1 first).
struct FusedOps {
    const void *x1 = nullptr;  // [n,d,h,w,c1] plain NDHWC, or null
    int c1 = 0;
    const float *in_scale = nullptr, *in_shift = nullptr;  // [n][cin - c1] device fp32, or null
    int in_act = ACT_NONE;
    const float *head_w = nullptr, *head_b = nullptr;  // [ncls][cout], [ncls] device fp32
    float *head_out = nullptr;                         // [n][ncls][Vo] fp32 logits; the conv output is then not stored
    int head_ncls = 0;
    bool any() const { return x1 || c1 || in_scale || in_shift || head_w || head_b || head_out; }
};

// The call struct of one conv: x0 holds the first cin - f.c1 channels, f the fused operands.
template <typename T>
inline ConvCallT<T> make_call(const void *x0, int cin, int N, int Di, int Hi, int Wi, void *out, double *stats, int act, float slope,
                              const FusedOps &f = FusedOps()) {
    ConvCallT<T> c;
    c.in0 = (const T *)x0; c.C0 = cin - f.c1; c.in1 = (const T *)f.x1; c.C1 = f.c1;
    c.N = N; c.Di = Di; c.Hi = Hi; c.Wi = Wi; c.out = (T *)out; c.act = act; c.slope = slope;
    c.stats = stats;
    c.in_scale = f.in_scale; c.in_shift = f.in_shift; c.in_act = f.in_act;
    c.head_w = f.head_w; c.head_b = f.head_b; c.head_out = f.head_out; c.head_ncls = f.head_ncls;
    return c;
}

// The fp32 weights of a conv as conv_weights_upload would leave them, for a planner asked without a device: the fields of the pack
// layout, and a stand-in pointer for exactly the packs conv_weights_upload makes (the planners test them for null, nothing more).
inline ConvWeights stand_in_conv_weights(const ConvPackLayout &l, int cin, int cout, int stride, bool keep_plain = false) {
    static float stand_in[2];
    ConvWeights cw;
    cw.cin = cw.cin_pad = cin; cw.cout = cout; cw.stride = stride;
    cw.cc = l.cc; cw.nf = l.nf; cw.pipe = l.pipe;
    cw.bias_dev = stand_in;
    if (l.mfma) cw.wp_dev = stand_in;
    if (l.c16) cw.wp16_dev = stand_in;
    if (l.wino2) cw.wpw_dev = stand_in;
    if (l.wino3) cw.wp3_dev = stand_in;
    if (keep_plain || !l.mfma) cw.w_plain_dev = stand_in;
    return cw;
}

// The optional operands of run_block, by name.
struct BlockOpts {
    float *head_logits_out = nullptr;  // the fused 1x1x1 head writes fp32 logits here; the conv output is then not stored
    // defer_norm: the block's normalisation (+ activation) is NOT applied to `out`; its per-(sample, channel) scale / shift go to
    // the plan's second pair and the NEXT block applies them while staging its input (in_norm of that call)
    bool defer_norm = false, in_norm = false;
    // half (fp32, shared skip half): the launch runs with these weights instead of L's - one half of L's input channels, C0 + C1
    // of them - and addend [N][Vo][cout] is added in front of bias and activation; reported under the kernel's name + half_name
    const ConvWeights *half = nullptr;
    const float *addend = nullptr;
    const char *half_name = "";
    const S0View *in0_view = nullptr, *addend_view = nullptr;  // stage-0 views of in0 / of the addend (the caller asked the planner first)
    bool s2_least_padding = false;  // ConvCall::s2_least_padding of the launch (fp32; the shared level 1 sets it on enc[1][0])
};
int run_block(mi355_unet *net, const Plan &pl, const ConvLayer &L, const void *in0, int C0, const void *in1, int C1, int N, int Di, int Hi,
              int Wi, void *out, hipStream_t s, const BlockOpts &o = BlockOpts());

// The optional operands of forward_features, by name (unet.hip has what each means).
struct ForwardOpts {
    bool *is_logits = nullptr;
    float *logits_target = nullptr;
    FeatNorm *head_norm = nullptr;
    // What the sliding window computed of encoder level l = 0 (shared stage 0) or 1 (shared level 1) before the forward:
    struct Level {
        bool given = false;                // enc[l]'s output is already where its last block writes it; the pass starts at level l + 1
        const float *skip_half = nullptr;  // the skip half of the decoder conv that reads it, gathered into the level-l buffer that stage leaves free
        const S0View *feat_view = nullptr, *half_view = nullptr;  // views into the shared tensors: the tile tensors hold their shells only
    } lvl[2];
};
int forward_features(mi355_unet *net, const Plan &pl, int N, int D, int H, int W, const void **feat, int *feat_c, hipStream_t s,
                     const ForwardOpts &o = ForwardOpts());

// The volume a sliding window runs over: [C][Z][Y][X] fp32 on the device.
struct SwVolume { const float *vol; int Z, Y, X; };

// Where one run of enc[0] over a set of boxes (stage0_run) reads and writes, and in which launches.
struct S0Placement {
    const int *S = nullptr;        // extent of one box
    const int *mask_zp = nullptr;  // non-null: what lies outside this extent of a box is zeroed between the layers
    int group = 0;                 // > 0: the convs run as launches of exactly `group` boxes each
    size_t in_off = 0;
    const size_t *tmp_off = nullptr;  // [2]
    size_t out_off = 0;
    size_t skip_off = 0;           // != 0 (shared skip half): one more launch behind the last block writes S there
    const char *label = "";        // suffix of the gather's profile entry
};

// The network side of the shared skip half (sw_share_plan.hip "shared skip half"): what is known of the first block of the last
// decoder stage when the network is created, when a sliding window decides, and in the dry run - one description, one predicate.
struct SkipShareNet {
    int dtype = MI355_F32;
    int r = 0;                     // stage0_blocks
    int stride = 1;                // of the last decoder stage's first block
    bool runtime_norm = false, post_affine = false;
    bool skip_is_enc0 = true;      // its second input is enc[0]'s output
    int c_up = 0, c_skip = 0, cout = 0;
    int head_ncls = 0;             // > 0: the block is also the stage's only one, i.e. the net's last conv, which may carry the fused head
};
inline SkipShareNet skip_share_net_of(int dtype, int r, int stride, int norm, int nonlin_first, int c_up, int c_skip, int cout, int head_ncls) {
    SkipShareNet d;
    d.dtype = dtype; d.r = r; d.stride = stride;
    d.runtime_norm = norm == MI355_NORM_INSTANCE || norm == MI355_NORM_GROUP;
    d.post_affine = norm == MI355_NORM_BATCH && nonlin_first;
    d.c_up = c_up; d.c_skip = c_skip; d.cout = cout; d.head_ncls = head_ncls;
    return d;
}
bool skip_share_network_ok(const SkipShareNet &d);
int stage0_blocks(const mi355_unet &net);
int level1_share_mode();  // MI355_SHARE_LEVEL1: 0 off, 1 the default rule (unset), 2 wherever possible (sw_share_plan.hip "shared level 1")

// ---- what sw_share_plan.hip (pure) gives sliding_window.hip (the device side)
struct SwGeom {
    int P[3], Zp[3], pad_lo[3];
    std::vector<TileDesc> tiles;   // origin of every tile, loop order axis0 outer .. axis2 inner
    std::vector<int> mirrors;      // TileDesc-style masks in nnU-Net's evaluation order
};
int make_geom(const mi355_sw_opts &o, int Z, int Y, int X, SwGeom *g);
void gaussian_map(const int p[3], double sigma_scale, std::vector<float> &out);
int sw_batch_tiles(int dtype, int batch_tiles, int nm);

// The switches a window obeys, read once where a window (sw_accumulate) or a dry run begins: nothing below reads the environment.
struct SwSwitches {
    bool skip_conv, views, merge_slabs; int level1;  // MI355_SHARE_SKIP_CONV, MI355_STAGE0_VIEWS, MI355_MERGE_SLABS, level1_share_mode()
    // how two pieces of the shared level 1 are launched, never what they compute (0 = as before them):
    bool s2_least_padding;  // MI355_S2_LEAST_PADDING: enc[1][0] over the regions and sub-boxes plans with ConvCall::s2_least_padding
    bool subbox_gather;     // MI355_SUBBOX_GATHER: a dense gather of sub-boxes runs stage0_gather_box_kernel
};
SwSwitches sw_switches();
constexpr int CONV_TILE[3] = {4, 8, 8};  // the voxel tile of the conv kernels: volumes are extended, and slabs sized, in whole tiles
inline int whole_conv_tiles(int v, int a) { return ceil_div(v, CONV_TILE[a]) * CONV_TILE[a]; }

constexpr int S0_SLAB_GROUP = 8;  // (8 slabs of 4 x 128 x 128: 2048 tiles of the F(2x2x2,3x3x3) kernel, 8 per CU)
struct S0Merged { int wv, side, org[3]; };  // a merged slab: its (mirrored) pass, the side of the faces it serves, its origin in that pass
struct S0Geom {
    bool shared = false;
    int r = 0, rs = 0;             // rs = depth of the slab chain: r, or r + 1 with the shared skip half (one more conv behind stage 0)
    int Ve[3] = {0, 0, 0};         // padded volume extended to whole 4 x 8 x 8 conv tiles
    int t[3] = {0, 0, 0};          // slab thickness per axis: the smallest multiple of (4, 8, 8) that is >= 2 rs
    int max_faces[3] = {0, 0, 0};  // most interior faces any tile has on an axis
    std::vector<S0Sample> smp;     // [tile][mirror]; slab[f] = 0 where face f needs a slab, -1 where it is a volume face
    // merged slabs (stage0_merge_geometry): the y- and x-slabs of ALL tiles, one per key, sorted by key
    bool merge = false;
    std::vector<S0Merged> merged[3];         // [1] y-slabs, [2] x-slabs ([0] stays empty: z-slabs are per tile)
    int mdim[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // extent of one slab of each axis
    std::vector<std::array<int, 6>> mslab;   // per sample: index of face f (2 .. 5) in merged[f >> 1], or -1
};
inline void slab_dims(const SwGeom &g, const S0Geom &sg, int a, int S[3]) { for (int k = 0; k < 3; ++k) S[k] = k == a ? sg.t[k] : g.P[k]; }
// origin of the slab of face f (axis f >> 1, hi side if f & 1) of a box at org: thick[a] layers at that face, the box's extent on the other axes
inline void face_slab_origin(const int org[3], const int extent[3], const int thick[3], int f, int b[3]) {
    for (int k = 0; k < 3; ++k) b[k] = org[k] + (k == f >> 1 && (f & 1) ? extent[k] - thick[k] : 0);
}
struct L1Geom {
    bool possible = false;
    int r0 = 0, k1 = 0, d1 = 0, dS = 0;
    bool merged[3] = {false, false, false};
    int R[3] = {0, 0, 0};    // level-0 extent of a region
    int t1[3] = {0, 0, 0};   // level-1 slab thickness (0 on a per-origin axis)
    std::vector<S0Sample> regions;  // sorted by (mirror, origin); org in the (mirrored) pass; slab[f] = 0: face f needs stage-0 shells, -1: not
    std::vector<S0Sample> smp;      // [tile][mirror], as S0Geom::smp; wv = its region, org = its origin in it at level 1; slab[f] = 0: face f has a level-1 slab, else -1
};
constexpr int L1_SLAB_GROUP = 8;  // level-1 slabs run as launches of exactly this many (the last one filled up), as the stage-0 slabs do
inline int level1_slab_rows(int n_samples) { return ceil_div(2 * n_samples, L1_SLAB_GROUP) * L1_SLAB_GROUP; }

// The network side: the last decoder stage as the shared skip half sees it, and level 1.
struct L1ShareNet {
    SkipShareNet last;
    int num_pool = 0;
    int k1 = 0, c1 = 0;      // blocks of enc[1] (its first has stride 2, the others stride 1) and their output channels
    bool skip_is_enc1 = true;  // the second input of dec[np - 2][0] is enc[1]'s output
    int dec_blocks = 0;      // blocks of dec[np - 2]
    int c_up = 0, cout = 0;  // of dec[np - 2][0]: channels of the upsampled half, output channels
};
L1ShareNet level1_share_net(const mi355_unet &net);

// Everything one window decided from the network's description, the geometry of ALL tiles and the switches - never from rank, world,
// lane or batch size.  Built once per window by sw_share_plan, as the dry runs do; a local of the call (one handle may be driven from two lanes).
struct SwSharePlan {
    S0Geom sg;                // the shared stage 0, its merged slabs included
    bool share_skip = false;  // the shared skip half (sg.rs = sg.r + 1)
    L1Geom lg;
    bool share_l1 = false;    // the shared level 1; implies sg.shared and share_skip
};
SwSharePlan sw_share_plan(const L1ShareNet &d, const SwGeom &g, const SwSwitches &sw);

// Does the planner send this fp32 call (n boxes of S voxels, cin channels, run-time statistics or not) to the stride-2 kernel that takes a view (kernels.h S0View)?
// least_padding: the call carries ConvCall::s2_least_padding (the launch it is asked about must carry it too)
bool reader_takes_view(const ConvWeights &w, int cin, int n, const int S[3], bool stats, bool least_padding = false);
struct S0ViewChoice { bool enc0 = false, half = false; };
S0ViewChoice stage0_views_choose(bool views, const S0Geom &sg, bool share_skip, int n_samples, const int P[3], const ConvWeights *w1, int c0, bool w1_stats);

}  // namespace mi355
