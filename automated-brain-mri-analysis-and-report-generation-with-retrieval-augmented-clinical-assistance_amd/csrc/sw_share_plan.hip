// The pure part of the sliding-window predictor (no HIP runtime call, nothing launched): tile geometry, the Gaussian map, what
// overlapping tiles share as ONE plan per window (sw_share_plan), and the geometry dry runs through which the CPU tests see that
// plan.  sliding_window.hip runs what is decided here.
// Reference behaviour restated here:
//   * nnU-Net v1 SegmentationNetwork._internal_predict_3D_3Dconv_tiled / _compute_steps_for_
//     sliding_window / _get_gaussian / _internal_maybe_mirror_and_pred_3D (un-vendored upstream;
//     SURVEY.md 8a rows T1-T5) as driven by run_brats2021_inference_singlethread.py:97-128.
#include <cmath>
#include <cstring>
#include <map>

#include "unet_internal.h"

namespace mi355 {

// ---- sliding-window helpers (nnU-Net v1)
static std::vector<int> compute_steps(int patch, int image, double step_size) {
    // target = patch*step ; n = ceil((image-patch)/target)+1 ; actual = (image-patch)/(n-1)
    // The step is a double from the C ABI down, as nnU-Net's is a Python float: rounded to float32, 0.3, 0.6, 0.7 and 0.9 put the ceil
    // on the other side wherever image - patch is a multiple of the target (0.3, patch 96, image 240: 6 tiles for nnU-Net's 7).
    const double target = patch * step_size;
    const int n = (int)std::ceil((image - patch) / target) + 1;
    const int max_step = image - patch;
    const double actual = n > 1 ? (double)max_step / (n - 1) : 99999999999.0;
    std::vector<int> steps(n);
    for (int i = 0; i < n; ++i) steps[i] = (int)std::nearbyint(actual * i);  // np.round: half to even
    return steps;
}

// scipy.ndimage.gaussian_filter(delta at patch//2, sigma = patch*sigma_scale, mode='constant') is
// separable: the filtered delta is the outer product of the three normalised 1-D kernels
// (truncate=4.0 -> radius int(4*sigma+0.5)); then /max, fp32, zeros -> smallest non-zero.
void gaussian_map(const int p[3], double sigma_scale, std::vector<float> &out) {
    std::vector<double> ax[3];
    for (int a = 0; a < 3; ++a) {
        const double sigma = p[a] * sigma_scale;
        const int radius = (int)(4.0 * sigma + 0.5);
        double sum = 0.0;
        std::vector<double> k(2 * radius + 1);
        for (int i = -radius; i <= radius; ++i) { k[i + radius] = std::exp(-0.5 / (sigma * sigma) * (double)i * i); sum += k[i + radius]; }
        ax[a].assign(p[a], 0.0);
        const int c = p[a] / 2;
        for (int i = 0; i < p[a]; ++i) {
            const int o = i - c;
            if (o >= -radius && o <= radius) ax[a][i] = k[o + radius] / sum;
        }
    }
    const size_t n = (size_t)p[0] * p[1] * p[2];
    std::vector<double> g(n);
    double mx = 0.0;
    for (int z = 0; z < p[0]; ++z)
        for (int y = 0; y < p[1]; ++y)
            for (int x = 0; x < p[2]; ++x) {
                const double v = (ax[0][z] * ax[1][y]) * ax[2][x];
                g[((size_t)z * p[1] + y) * p[2] + x] = v;
                if (v > mx) mx = v;
            }
    out.resize(n);
    float mn = INFINITY;
    for (size_t i = 0; i < n; ++i) {
        out[i] = (float)(g[i] / mx * 1.0);
        if (out[i] != 0.f && out[i] < mn) mn = out[i];
    }
    for (size_t i = 0; i < n; ++i)
        if (out[i] == 0.f) out[i] = mn;
}

int make_geom(const mi355_sw_opts &o, int Z, int Y, int X, SwGeom *g) {
    const int dims[3] = {Z, Y, X};
    std::vector<int> steps[3];
    MI355_REQUIRE(o.step_size > 0.0 && o.step_size <= 1.0, "step_size must be in (0, 1]");  // (before compute_steps divides by it)
    for (int a = 0; a < 3; ++a) {
        g->P[a] = o.patch[a];
        MI355_REQUIRE(g->P[a] > 0 && dims[a] > 0, "bad patch / volume size");
        g->Zp[a] = std::max(dims[a], g->P[a]);       // pad_nd_image(..., "constant", 0)
        g->pad_lo[a] = (g->Zp[a] - dims[a]) / 2;     // pad_below = difference // 2
        steps[a] = compute_steps(g->P[a], g->Zp[a], o.step_size);
    }
    g->tiles.clear();
    for (int z : steps[0]) for (int y : steps[1]) for (int x : steps[2]) g->tiles.push_back(TileDesc{z, y, x, 0});
    // _internal_maybe_mirror_and_pred_3D: m = 0..7; bit0 of m flips the LAST axis (x), bit1 y, bit2 z
    g->mirrors.clear();
    for (int m = 0; m < 8; ++m) {
        const bool fx = m & 1, fy = m & 2, fz = m & 4;
        if ((fx && !(o.mirror_axes & 4)) || (fy && !(o.mirror_axes & 2)) || (fz && !(o.mirror_axes & 1))) continue;
        g->mirrors.push_back((fz ? 1 : 0) | (fy ? 2 : 0) | (fx ? 4 : 0));
    }
    return MI355_OK;
}

// the geometry of a dry run, which takes the three values of mi355_sw_opts that make_geom reads
static int sw_geom_from_abi(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes, SwGeom *g) {
    mi355_sw_opts o;
    memset(&o, 0, sizeof(o));
    for (int a = 0; a < 3; ++a) o.patch[a] = patch[a];
    o.step_size = step_size; o.mirror_axes = mirror_axes;
    return make_geom(o, z, y, x, g);
}

// tiles per forward (each with its nm mirrors): 16 samples (fp32) / 32 (fp16: half the bytes per sample; config 3 fp16 297 -> 293 ms
// per volume with 32, the deep levels' launches fill the chip better), 64 at the most - the arena is sized for 288 GB of HBM, not
// for a few GB.  One helper for sw_accumulate and the dry run mi355_stage0_view_plan, so that the two cannot drift.
int sw_batch_tiles(int dtype, int batch_tiles, int nm) {
    int bt = batch_tiles > 0 ? batch_tiles : std::max(1, (dtype == MI355_F16 ? 32 : 16) / nm);
    if (bt * nm > 64) bt = std::max(1, 64 / nm);
    return bt;
}

// ---- shared stage 0.  The tiles of a sliding window overlap (step 0.5: every voxel of a BraTS crop lies in up to 8 tiles), and
// encoder stage 0 - r stride-1 3x3x3 blocks without run-time statistics, in front of the first stride-2 conv - is translation-
// equivariant with a (2r + 1)^3 receptive field: a tile's stage-0 output equals the whole padded volume's except within r voxels
// of a tile face that lies INSIDE the volume, where the tile sees zero padding and the volume real neighbours.  So stage 0 runs
// once per (net, mirror) over the whole volume and, per batch of tiles, over one thin input slab per interior face (full tile
// extent on the other two axes, zero padding all around = the tile's own padding; its outer r layers are exact because their
// receptive field stays inside a slab of thickness >= 2r); stage0_gather_kernel then writes the tile tensor from the two.
// The decision depends on the network and the geometry of ALL tiles only - not on rank, world, lane or batch size - so that every
// rank and lane computes a tile's features the same way.
// For the same reason the slab convs run as launches of exactly S0_SLAB_GROUP slabs (the last one filled up): the kernel the
// planner picks, and with it the summation order, must not change with the number of tiles a rank or batch happens to hold.
// Coordinates: a mirrored pass works on the flipped padded volume, where a tile's origin along a flipped axis is Zp - P - origin.
// stage0_thickness: slab thickness t of a chain rs layers deep; r blocks can be shared with more than one tile and no patch thinner than a slab
static bool stage0_thickness(const SwGeom &g, int r, int rs, int t[3]) {
    bool fits = r >= 1 && g.tiles.size() > 1;
    for (int a = 0; a < 3; ++a) {
        t[a] = whole_conv_tiles(std::max(2 * rs, 1), a);
        fits = fits && g.P[a] >= t[a];
    }
    return fits;
}
static void stage0_geometry(const SwGeom &g, int r, S0Geom *o, int extra = 0) {
    *o = S0Geom();
    o->r = r; o->rs = r + extra;
    for (int a = 0; a < 3; ++a) o->Ve[a] = whole_conv_tiles(g.Zp[a], a);
    if (!stage0_thickness(g, r, o->rs, o->t)) return;
    o->shared = true;
    for (const TileDesc &td : g.tiles)
        for (size_t m = 0; m < g.mirrors.size(); ++m) {
            const int org[3] = {td.z0, td.y0, td.x0};
            S0Sample sm;
            sm.wv = (int)m;
            for (int a = 0; a < 3; ++a) {
                sm.org[a] = (g.mirrors[m] >> a) & 1 ? g.Zp[a] - g.P[a] - org[a] : org[a];
                sm.slab[2 * a] = sm.org[a] > 0 ? 0 : -1;
                sm.slab[2 * a + 1] = sm.org[a] + g.P[a] < g.Zp[a] ? 0 : -1;
                o->max_faces[a] = std::max(o->max_faces[a], (sm.slab[2 * a] >= 0) + (sm.slab[2 * a + 1] >= 0));
            }
            o->smp.push_back(sm);
        }
}

// ---- merged slabs (MI355_MERGE_SLABS).  Tiles that share a cut plane compute nearly the same y- and x-slabs.  The gather takes
// a voxel from the first shell that holds it, z before y before x, and that order decides which padding a slab must reproduce:
//   * a z-slab serves every voxel within the shell depth of an interior z face, the edges and corners it shares with y and x
//     faces included: it needs the tile's own y and x padding and stays per tile (stage0_tiles);
//   * a y-slab serves voxels within the depth of an interior y face and NOT within it of an interior z face: their receptive
//     field crosses a z face of the tile only where that is a volume face, so the slab may span the whole extended volume in z
//     (zeros outside [0, Zp0) restored between the layers as in the whole-volume pass).  It still carries the tile's x padding,
//     for the y-x edge.  Key (mirror, side, y of the slab, x origin of the tile), box Ve0 x t1 x P2;
//   * an x-slab serves voxels in neither other shell and needs no tile padding.  Key (mirror, side, x of the slab), box
//     Ve0 x Ve1 x t2.
// The keys are a function of the network and the geometry of all tiles; every rank computes all of them, once per volume, right
// behind the whole-volume pass, in one launch group per axis with N = number of keys - so the kernel the planner picks, and the
// summation order with it, cannot depend on who asks.  A rank of a tile-sharded run pays for slabs of tiles it does not hold.
static void stage0_merge_geometry(const SwGeom &g, S0Geom *o) {
    for (int a = 0; a < 3; ++a) o->merged[a].clear();
    o->mslab.clear();
    o->merge = false;
    if (!o->shared) return;
    const int dims[3][3] = {{o->t[0], g.P[1], g.P[2]}, {o->Ve[0], o->t[1], g.P[2]}, {o->Ve[0], o->Ve[1], o->t[2]}};
    memcpy(o->mdim, dims, sizeof(dims));
    typedef std::array<int, 5> Key;  // (wv, side, origin): sorted = the order of the slabs
    auto key_of = [&](const S0Sample &sm, int f) {
        Key k = {sm.wv, f & 1, 0, 0, 0};
        k[2 + (f >> 1)] = sm.org[f >> 1] + (f & 1 ? g.P[f >> 1] - o->t[f >> 1] : 0);
        if (f >> 1 == 1) k[4] = sm.org[2];
        return k;
    };
    std::map<Key, int> keys[3];
    for (const S0Sample &sm : o->smp)
        for (int f = 2; f < 6; ++f)
            if (sm.slab[f] >= 0) keys[f >> 1][key_of(sm, f)] = 0;
    for (int a = 1; a < 3; ++a)
        for (auto &kv : keys[a]) {
            kv.second = (int)o->merged[a].size();
            o->merged[a].push_back(S0Merged{kv.first[0], kv.first[1], {kv.first[2], kv.first[3], kv.first[4]}});
        }
    for (const S0Sample &sm : o->smp) {
        std::array<int, 6> idx = {-1, -1, -1, -1, -1, -1};
        for (int f = 2; f < 6; ++f)
            if (sm.slab[f] >= 0) idx[f] = keys[f >> 1][key_of(sm, f)];
        o->mslab.push_back(idx);
    }
    o->merge = !o->merged[1].empty() || !o->merged[2].empty();
}

// May a block of enc[0] be part of the shared stage 0?  fp32, stride 1, no run-time statistics (Instance/GroupNorm statistics are
// per tile), no BN left unfolded, and whole float4s of channels (the mask and gather kernels move 16 bytes per lane).  Over plain
// values: stage0_blocks asks it of every layer of a network, the dry runs (skip_share_net_from_abi) of a network's description.
static bool stage0_block_ok(int dtype, int stride, bool runtime_stats, bool post_affine, int cout) {
    return dtype == MI355_F32 && stride == 1 && !runtime_stats && !post_affine && cout % 4 == 0;
}
// blocks of enc[0] when the network allows the shared stage 0, else 0
int stage0_blocks(const mi355_unet &net) {
    if (!env_switch("MI355_SHARE_STAGE0")) return 0;
    for (const ConvLayer &L : net.enc[0])
        if (!stage0_block_ok(net.dtype, L.stride, L.runtime_norm, L.post_affine, L.cout)) return 0;
    return (int)net.enc[0].size();
}

SwSwitches sw_switches() {
    return SwSwitches{env_switch("MI355_SHARE_SKIP_CONV"), env_switch("MI355_STAGE0_VIEWS"), env_switch("MI355_MERGE_SLABS"), level1_share_mode(),
                      env_switch("MI355_S2_LEAST_PADDING"), env_switch("MI355_SUBBOX_GATHER")};
}

// ---- shared skip half.  The first block of the last decoder stage reads the virtual concat (upsampled, skip) and is linear in
// front of its bias and activation: out = act(bias + conv(W_up, up) + conv(W_skip, skip)).  Its skip is the output of the shared
// stage 0, so S = conv(W_skip, skip) is one more translation-equivariant layer behind it: computed once per (net, mirror) over the
// whole volume and over the slabs - whose chain is then r + 1 layers deep: thickness >= 2 (r + 1), shell r + 1 for S, r for the skip
// as before -, gathered per tile next to the skip, and added by the per-tile launch, which runs over the upsampled half alone
// (half the MFMAs of the largest launch of a forward), in its epilogue (Wino3Args::addend).
// What the decision may depend on is what stage 0's may: the network and the geometry of all tiles, never rank, lane or batch.
// halves_pack: a block of c_up + c_skip -> cout channels can be split at the concat boundary, both halves get the packs they need.
static bool halves_pack(int c_up, int c_skip, int cout) {
    if (c_up <= 0 || c_skip <= 0 || c_up % 4 || c_skip % 4 || cout % 4) return false;
    ConvPackLayout lu, ls;
    if (conv_pack_layout(c_up, c_up, cout, 1, &lu) != MI355_OK || conv_pack_layout(c_skip, c_skip, cout, 1, &ls) != MI355_OK) return false;
    return lu.wino3 && ls.mfma;
}
// The network's part: also what decides, at mi355_unet_create, whether the block gets the packs of its two halves.  A last stage
// of one block is left alone: its conv is the net's last and may carry the fused head, which has no addend.
static bool skip_share_network_rule(const SkipShareNet &d) {
    if (d.dtype != MI355_F32 || d.r < 1 || d.stride != 1 || d.runtime_norm || d.post_affine || !d.skip_is_enc0 || d.head_ncls > 0) return false;
    return halves_pack(d.c_up, d.c_skip, d.cout);
}
bool skip_share_network_ok(const SkipShareNet &d) { return env_switch("MI355_SHARE_SKIP_CONV") && skip_share_network_rule(d); }

// Is the launch over the upsampled half alone (halves_pack asked first) the kernel that has the addend epilogue?  Asked for ONE
// sample of S voxels: more samples never send a call away from that kernel, and the answer must not depend on the batch.  (plan_wino3
// is the first step of plan_conv_f32 and, unlike it, answers without leaving an error text behind)  and_plain: and the same call
// without the addend is a launch of the plain instantiation.
static bool up_half_has_addend(int c_up, int cout, const int S[3], bool and_plain) {
    ConvPackLayout lu;
    (void)conv_pack_layout(c_up, c_up, cout, 1, &lu);
    static float stand_in[2];
    const ConvWeights cw = stand_in_conv_weights(lu, c_up, cout, 1);  // (lu.wino3, which halves_pack asked for, implies every pack)
    ConvCall c = make_call<float>(stand_in, c_up, 1, S[0], S[1], S[2], stand_in, nullptr, ACT_LRELU, 0.01f);
    c.addend = stand_in;
    ConvPlan p;
    if (!plan_wino3(cw, c, &p) || strcmp(p.name, "conv3_f32_wino3_kernel<3, false>") != 0) return false;
    c.addend = nullptr;
    return !and_plain || (plan_wino3(cw, c, &p) && strcmp(p.name, "conv3_f32_wino3_kernel<0, false>") == 0);
}
static bool skip_share_decide(const SkipShareNet &d, const SwGeom &g, const SwSwitches &sw) {
    if (!sw.skip_conv || !skip_share_network_rule(d)) return false;
    int t[3];
    if (!stage0_thickness(g, d.r, d.r + 1, t)) return false;  // (one tile, or a patch thinner than a slab of the deeper chain)
    return up_half_has_addend(d.c_up, d.cout, g.P, true);
}
static SkipShareNet skip_share_net(const mi355_unet &net) {
    const std::vector<ConvLayer> &st = net.dec.back();
    const ConvLayer &L = st[0];
    const int c_skip = net.enc[0].back().cout;
    SkipShareNet d = skip_share_net_of(net.dtype, stage0_blocks(net), L.stride, net.norm, net.nonlin_first, L.cin - c_skip, c_skip, L.cout,
                                       st.size() == 1 ? net.head.ncls : 0);
    d.skip_is_enc0 = L.split_c0 == d.c_up;  // (Generic_UNet: the last stage's skip is enc[0]'s; the packs of the two halves were made)
    return d;
}

// The same description as a dry run is given it.  It states enc[0] in three values - the norm, the width of its last block and
// the number of blocks - so the rule of stage0_blocks is asked once, of a stride-1 block of that width, and never reads the
// MI355_SHARE_STAGE0 switch: a dry run answers for a process that has it on.
static SkipShareNet skip_share_net_from_abi(const mi355_skip_share_net *nd) {
    const bool runtime_stats = nd->norm != MI355_NORM_NONE && nd->norm != MI355_NORM_BATCH;
    const bool post_affine = nd->norm == MI355_NORM_BATCH && nd->nonlin_first;
    const int r0 = stage0_block_ok(nd->dtype, 1, runtime_stats, post_affine, nd->c_skip) ? nd->enc0_blocks : 0;
    SkipShareNet d = skip_share_net_of(nd->dtype, r0, nd->stride, nd->norm, nd->nonlin_first, nd->c_up, nd->c_skip, nd->cout, nd->head_ncls);
    d.skip_is_enc0 = nd->skip_is_enc0 != 0;
    return d;
}

// ---- stage-0 views (MI355_STAGE0_VIEWS).  The gather copies, per tile, mostly values that already lie in the whole-volume
// tensors: a tile's copy differs from them only inside the shells.  Each of the two tile tensors has one reader - the level-0
// features the first stride-2 conv (enc[1][0]), the skip half S the addend epilogue of the up-half launch -, so where that reader
// can take a per-sample view (kernels.h S0View) it reads the whole-volume tensor in place and only shell voxels from the tile
// tensor, and the gather writes the shells alone (stage0_gather_shells).  The tile tensors stay where they are, with their dense
// strides; outside the shells they then hold stale values nobody reads.
// Views change where bytes are read, never which kernel runs or in which order anything is summed: results are bit-identical, and
// unlike the plan of a window this decision may depend on the batch.  Per tensor and per forward:
//   * the level-0 features: the shared skip half is on (otherwise the concat conv reads them whole, as in1), and the planner - asked
//     first, for exactly this call - sends enc[1][0] to conv3_f32_s2dma_kernel; the launch then runs conv3_f32_s2dma_kernel_view;
//   * S: the shared skip half is on (its reader is then always conv3_f32_wino3_kernel<3, false>).
// A view that cannot be built (stage0_view_make: offsets beyond 32 bits) falls back to the full gather for that tensor.
bool reader_takes_view(const ConvWeights &w, int cin, int n, const int S[3], bool stats, bool least_padding) {
    static float stand_in[2];
    ConvCall c = make_call<float>(stand_in, cin, n, S[0], S[1], S[2], stand_in, stats ? (double *)stand_in : nullptr, ACT_LRELU, 0.01f);
    c.s2_least_padding = least_padding;
    ConvPlan p;
    return plan_conv_f32(w, c, &p) == MI355_OK && p.family == FAM_S2DMA;
}
// w1: the weights (or, for a dry run, the pack layout with stand-in pointers) of the first block of level 1, null = none that
// qualifies; c0 its input channels; w1_stats: it carries run-time statistics
S0ViewChoice stage0_views_choose(bool views, const S0Geom &sg, bool share_skip, int n_samples, const int P[3], const ConvWeights *w1, int c0, bool w1_stats) {
    S0ViewChoice v;
    if (!views || !sg.shared || !share_skip || n_samples < 1 || n_samples > S0_VIEW_MAX_SAMPLES) return v;
    v.half = true;
    v.enc0 = w1 && w1->wp_dev && w1->stride == 2 && reader_takes_view(*w1, c0, n_samples, P, w1_stats);
    return v;
}

// ---- shared level 1: the geometry (level1_geometry), the rule (level1_share_rule) and their dry run (mi355_level1_share_plan);
// the region pass and the per-forward slabs that run on them are sliding_window.hip's (MI355_SHARE_LEVEL1).
// A stride-2 conv commutes with shifts by an even number of voxels.  Along an axis on which every sample's origin is even, encoder
// level 1 (one stride-2 block, then stride-1 blocks) and the skip half of the conv that reads its output (dec[np - 2][0]) are
// therefore once more the same numbers computed once per tile: the shared stage 0, one level down.
//   * An axis is MERGED when it has more than one tile origin, every sample's origin on it (a mirrored origin is Zp - P - org) is
//     even and Zp is even; else it is PER-ORIGIN.
//   * A REGION is one box per (mirror, origin tuple on the per-origin axes): P[a] on a per-origin axis, at the tile's origin; the
//     whole extended volume Ve[a] on a merged one (the whole-volume stage-0 tensor is Ve wide, so a region reads it in place).  Its
//     level-0 input is enc[0]'s whole-volume result, with stage-0 shells (depth r0) at its faces on per-origin axes that lie inside
//     the volume - the region is a "tile" of the shared stage 0 there.  enc[1] and the skip half run over the regions once per
//     volume, zeros restored outside Zp / 2 between the layers.
//   * A tile's own level-1 values differ from its region's only near a tile face that lies inside the region on a merged axis:
//     within floor(r0 / 2) + 1 behind the stride-2 conv, one more per stride-1 block: d1 = floor(r0 / 2) + k1 for enc[1]'s output
//     (k1 blocks, the stride-2 one included), dS = d1 + 1 for the skip half.
//   * Those shells come from one level-1 SLAB per such face: the chain over the 2 t1 outermost level-0 layers of the tile (its own
//     padding and stage-0 shells on every other face, zero padding at the cut).  At the cut a hi slab loses one layer per conv
//     (k1 + 1 convs), so t1 - (k1 + 1) >= dS: t1 = the smallest multiple of (4, 8, 8) >= floor(r0 / 2) + 2 k1 + 2, and >= 2 dS as
//     the gather asks of every slab.
// Proved exactly, on an integer chain, in tests/test_level1_share_plan_cpu.py.
static void level1_geometry(const SwGeom &g, const S0Geom &sg, int k1, L1Geom *o) {
    *o = L1Geom();
    o->r0 = sg.r; o->k1 = k1;
    if (!sg.shared || k1 < 1) return;
    o->d1 = sg.r / 2 + k1; o->dS = o->d1 + 1;
    bool any = false, fits = true;
    for (int a = 0; a < 3; ++a) {
        bool even = g.Zp[a] % 2 == 0 && g.P[a] % 2 == 0, several = false;
        for (const S0Sample &sm : sg.smp) { even = even && sm.org[a] % 2 == 0; several = several || sm.org[a] != sg.smp[0].org[a]; }
        o->merged[a] = even && several;
        o->R[a] = o->merged[a] ? sg.Ve[a] : g.P[a];
        if (!o->merged[a]) continue;
        any = true;
        o->t1[a] = whole_conv_tiles(std::max(sg.r / 2 + 2 * k1 + 2, 2 * o->dS), a);
        // a tile with two faces inside the region has room for both slabs; the sub-box a slab is cut from holds its stage-0 shells
        fits = fits && g.P[a] / 2 >= 2 * o->t1[a] && 2 * o->t1[a] >= 2 * sg.r;
    }
    if (!any || !fits) return;
    o->possible = true;
    typedef std::array<int, 4> Key;  // (wv, origin): sorted = the order of the regions
    std::map<Key, int> keys;
    auto key_of = [&](const S0Sample &sm) {
        Key k = {sm.wv, 0, 0, 0};
        for (int a = 0; a < 3; ++a) k[1 + a] = o->merged[a] ? 0 : sm.org[a];
        return k;
    };
    for (const S0Sample &sm : sg.smp) keys[key_of(sm)] = 0;
    for (auto &kv : keys) {
        kv.second = (int)o->regions.size();
        S0Sample rg;
        rg.wv = kv.first[0];
        for (int a = 0; a < 3; ++a) {
            rg.org[a] = kv.first[1 + a];
            rg.slab[2 * a] = !o->merged[a] && rg.org[a] > 0 ? 0 : -1;
            rg.slab[2 * a + 1] = !o->merged[a] && rg.org[a] + g.P[a] < g.Zp[a] ? 0 : -1;
        }
        o->regions.push_back(rg);
    }
    for (const S0Sample &sm : sg.smp) {
        S0Sample ls;
        ls.wv = keys[key_of(sm)];
        for (int a = 0; a < 3; ++a) {
            ls.org[a] = o->merged[a] ? sm.org[a] / 2 : 0;
            ls.slab[2 * a] = o->merged[a] ? sm.slab[2 * a] : -1;  // (S0Sample::slab: 0 where the face lies inside the volume)
            ls.slab[2 * a + 1] = o->merged[a] ? sm.slab[2 * a + 1] : -1;
        }
        o->smp.push_back(ls);
    }
}

// sw.level1: 0 off, 1 the default rule, 2 wherever it is structurally possible.  Depends on the network and the geometry of all tiles
// only (through p).  The default rule asks P / 2 >= 8 t1 on every merged axis: a slab costs t1 / (P / 2) of a tile per face, so smaller
// patches lose, and it leaves the patch 64 and 32 paths that existing tests pin bit for bit alone.
static bool level1_share_rule(const L1ShareNet &d, const SwGeom &g, const SwSwitches &sw, const SwSharePlan &p) {
    const L1Geom &lg = p.lg;
    if (sw.level1 == 0 || !lg.possible) return false;
    // fp32 (skip_share_decide), the shared stage 0, the shared skip half and the stage-0 views all on
    if (!p.share_skip || !p.sg.shared || !sw.views) return false;
    // run-time statistics and an unfolded BatchNorm are the network's, not a block's: skip_share_decide has refused them
    if (d.num_pool < 2 || d.k1 < 1 || !d.skip_is_enc1 || d.dec_blocks < 2) return false;
    // dec[np - 2][0] over the upsampled half alone must be the kernel with the addend epilogue, its skip half a packed conv
    const int P1[3] = {g.P[0] / 2, g.P[1] / 2, g.P[2] / 2};
    if (!halves_pack(d.c_up, d.c1, d.cout) || !up_half_has_addend(d.c_up, d.cout, P1, false)) return false;
    // the regions read enc[0]'s whole-volume result in place: their first conv must be the stride-2 kernel that takes a view
    if ((int)lg.regions.size() > S0_VIEW_MAX_SAMPLES) return false;
    ConvPackLayout l1;
    if (conv_pack_layout(d.last.c_skip, d.last.c_skip, d.c1, 2, &l1) != MI355_OK || !l1.mfma) return false;
    if (!reader_takes_view(stand_in_conv_weights(l1, d.last.c_skip, d.c1, 2), d.last.c_skip, (int)lg.regions.size(), lg.R, false, sw.s2_least_padding)) return false;
    if (sw.level1 == 1)
        for (int a = 0; a < 3; ++a) {
            if (!lg.merged[a]) continue;
            if (g.P[a] / 2 < 8 * lg.t1[a]) return false;
            if (lg.R[a] / 2 % CONV_TILE[a]) return false;  // a region that is no whole number of conv tiles at level 1 leaves the F(2x2x2,3x3x3) kernel
        }
    return true;
}

L1ShareNet level1_share_net(const mi355_unet &net) {
    L1ShareNet d;
    d.last = skip_share_net(net);
    d.num_pool = net.num_pool;
    if (net.num_pool < 2 || net.dtype != MI355_F32) return d;
    const std::vector<ConvLayer> &e1 = net.enc[1], &st = net.dec[net.num_pool - 2];
    bool ok = !e1.empty() && e1[0].stride == 2 && !e1[0].is_stem;
    for (size_t i = 0; i < e1.size(); ++i) ok = ok && (i == 0 || e1[i].stride == 1) && !e1[i].runtime_norm && !e1[i].post_affine;
    d.k1 = ok ? (int)e1.size() : 0;
    d.c1 = e1.back().cout;
    d.dec_blocks = (int)st.size();
    d.c_up = st[0].cin - d.c1; d.cout = st[0].cout;
    d.skip_is_enc1 = d.c_up > 0 && st[0].split_c0 == d.c_up;  // (Generic_UNet: that stage's skip is enc[1]'s; the packs of the two halves were made)
    return d;
}
int level1_share_mode() {
    const char *e = getenv("MI355_SHARE_LEVEL1");
    return !e || !*e ? 1 : (e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1));
}
static L1ShareNet level1_share_net_from_abi(const mi355_level1_share_net *nd) {
    L1ShareNet d;
    d.last = skip_share_net_from_abi(&nd->last);
    d.num_pool = nd->num_pool; d.k1 = nd->enc1_blocks; d.c1 = nd->c_level1;
    d.skip_is_enc1 = nd->skip_is_enc1 != 0; d.dec_blocks = nd->dec1_blocks; d.c_up = nd->c_up1; d.cout = nd->cout1;
    return d;
}

// ---- the plan of one window: each layer decided once, on the layers below it (k1 = 0, the dry runs of stage 0 alone: an empty lg)
SwSharePlan sw_share_plan(const L1ShareNet &d, const SwGeom &g, const SwSwitches &sw) {
    SwSharePlan p;
    p.share_skip = skip_share_decide(d.last, g, sw);
    stage0_geometry(g, d.last.r, &p.sg, p.share_skip ? 1 : 0);
    if (sw.merge_slabs) stage0_merge_geometry(g, &p.sg);
    level1_geometry(g, p.sg, d.k1, &p.lg);
    p.share_l1 = level1_share_rule(d, g, sw, p);
    return p;
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_compute_steps(int patch, int image, double step_size, int32_t *steps, int max_steps) {
    MI355_REQUIRE(patch > 0 && image >= patch && step_size > 0.0 && step_size <= 1.0, "compute_steps: bad arguments");
    std::vector<int> st = compute_steps(patch, image, step_size);
    MI355_REQUIRE((int)st.size() <= max_steps, "compute_steps: %zu steps > buffer %d", st.size(), max_steps);
    for (size_t i = 0; i < st.size(); ++i) steps[i] = st[i];
    return (int)st.size();
}

// ---- the geometry dry runs.  The two that take a raw r / skip_half and no network ask the geometry layer directly.
extern "C" int mi355_stage0_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes, int r,
                                 mi355_stage0_geom *out, mi355_stage0_sample *samples, int max_samples) {
    MI355_REQUIRE(out && patch && r >= 0 && (samples || max_samples == 0), "mi355_stage0_plan: bad argument");
    SwGeom g;
    MI355_TRY(sw_geom_from_abi(z, y, x, patch, step_size, mirror_axes, &g));
    S0Geom sg;
    stage0_geometry(g, r, &sg);
    memset(out, 0, sizeof(*out));
    out->shared = sg.shared; out->r = r;
    out->n_tiles = (int32_t)g.tiles.size(); out->n_mirrors = (int32_t)g.mirrors.size();
    for (int a = 0; a < 3; ++a) { out->padded[a] = g.Zp[a]; out->volume[a] = sg.Ve[a]; out->slab_thickness[a] = sg.t[a]; }
    const int n = sg.shared ? (int)sg.smp.size() : 0;
    for (int i = 0; i < n && i < max_samples; ++i) {
        const S0Sample &sm = sg.smp[i];
        mi355_stage0_sample &d = samples[i];
        memset(&d, 0, sizeof(d));
        d.tile = i / (int)g.mirrors.size(); d.mirror = g.mirrors[sm.wv];
        for (int a = 0; a < 3; ++a) d.origin[a] = sm.org[a];
        for (int f = 0; f < 6; ++f) {
            if (sm.slab[f] < 0) continue;
            d.face[f] = 1;
            int S[3], b[3];
            slab_dims(g, sg, f >> 1, S);
            face_slab_origin(sm.org, g.P, sg.t, f, b);
            for (int a = 0; a < 3; ++a) { d.slab_origin[f][a] = b[a]; d.slab_shape[f][a] = S[a]; }
        }
    }
    return n;
}

extern "C" int mi355_stage0_merge_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes, int r, int skip_half,
                                       mi355_stage0_merge_geom *out, mi355_stage0_merge_slab *slabs, int max_slabs,
                                       mi355_stage0_merge_sample *samples, int max_samples) {
    MI355_REQUIRE(out && patch && r >= 0 && (slabs || max_slabs == 0) && (samples || max_samples == 0), "mi355_stage0_merge_plan: bad argument");
    SwGeom g;
    MI355_TRY(sw_geom_from_abi(z, y, x, patch, step_size, mirror_axes, &g));
    S0Geom sg;
    stage0_geometry(g, r, &sg, skip_half ? 1 : 0);
    stage0_merge_geometry(g, &sg);
    memset(out, 0, sizeof(*out));
    out->shared = sg.shared; out->r = sg.r; out->rs = sg.rs;
    out->n_tiles = (int32_t)g.tiles.size(); out->n_mirrors = (int32_t)g.mirrors.size();
    for (int a = 0; a < 3; ++a) { out->padded[a] = g.Zp[a]; out->volume[a] = sg.Ve[a]; out->slab_thickness[a] = sg.t[a]; }
    if (!sg.shared) return 0;
    for (int a = 0; a < 3; ++a) {
        int S[3];
        slab_dims(g, sg, a, S);
        int64_t faces = 0;
        for (const S0Sample &sm : sg.smp) faces += (sm.slab[2 * a] >= 0) + (sm.slab[2 * a + 1] >= 0);
        out->voxels_per_tile += faces * S[0] * S[1] * S[2];
        out->n_slabs[a] = a ? (int32_t)sg.merged[a].size() : (int32_t)faces;
        for (int k = 0; k < 3; ++k) out->slab_shape[a][k] = sg.mdim[a][k];
        out->voxels[a] = (int64_t)out->n_slabs[a] * sg.mdim[a][0] * sg.mdim[a][1] * sg.mdim[a][2];
    }
    int ns = 0;
    for (int a = 1; a < 3; ++a)
        for (const S0Merged &k : sg.merged[a]) {
            if (ns < max_slabs) {
                mi355_stage0_merge_slab &q = slabs[ns];
                q.axis = a; q.mirror = g.mirrors[k.wv]; q.side = k.side;
                for (int c = 0; c < 3; ++c) q.origin[c] = k.org[c];
            }
            ++ns;
        }
    const int n = (int)sg.smp.size();
    for (int i = 0; i < n && i < max_samples; ++i) {
        const S0Sample &sm = sg.smp[i];
        mi355_stage0_merge_sample &q = samples[i];
        memset(&q, 0, sizeof(q));
        q.tile = i / (int)g.mirrors.size(); q.mirror = g.mirrors[sm.wv];
        for (int a = 0; a < 3; ++a) q.origin[a] = sm.org[a];
        for (int f = 0; f < 6; ++f) {
            const int a = f >> 1;
            q.slab[f] = a == 0 ? sm.slab[f] : sg.mslab[i][f];
            if (q.slab[f] < 0 || a == 0) continue;
            for (int k = 0; k < 3; ++k) q.offset[f][k] = sm.org[k] + (k == a && (f & 1) ? g.P[a] - sg.t[a] : 0) - sg.merged[a][q.slab[f]].org[k];
        }
    }
    return n;
}

extern "C" int mi355_skip_share_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes,
                                     const mi355_skip_share_net *nd, int batch_tiles, int rank, int world, mi355_skip_share_geom *out) {
    MI355_REQUIRE(out && patch && nd && batch_tiles >= 0 && world >= 1 && rank >= 0 && rank < world, "mi355_skip_share_plan: bad argument");
    SwGeom g;
    MI355_TRY(sw_geom_from_abi(z, y, x, patch, step_size, mirror_axes, &g));
    // (rank, world, batch_tiles: taken so that a caller can see that nothing below reads them - the invariant of the shared stage 0)
    (void)batch_tiles; (void)rank; (void)world;
    L1ShareNet d; d.last = skip_share_net_from_abi(nd);
    const SwSharePlan p = sw_share_plan(d, g, sw_switches());
    const S0Geom &sg = p.sg;
    memset(out, 0, sizeof(*out));
    out->stage0_shared = sg.shared; out->skip_shared = p.share_skip;
    out->r = sg.r; out->skip_shell = p.share_skip ? sg.rs : 0;
    out->n_tiles = (int32_t)g.tiles.size(); out->n_mirrors = (int32_t)g.mirrors.size();
    for (int a = 0; a < 3; ++a) { out->volume[a] = sg.Ve[a]; out->slab_thickness[a] = sg.t[a]; }
    return MI355_OK;
}

extern "C" int mi355_stage0_view_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes,
                                      const mi355_skip_share_net *nd, int c_level1, int batch_samples, mi355_stage0_view_geom *out,
                                      mi355_stage0_view_sample *samples, int max_samples) {
    MI355_REQUIRE(out && patch && nd && c_level1 > 0 && batch_samples >= 0 && (samples || max_samples == 0), "mi355_stage0_view_plan: bad argument");
    SwGeom g;
    MI355_TRY(sw_geom_from_abi(z, y, x, patch, step_size, mirror_axes, &g));
    const SwSwitches sw = sw_switches();
    L1ShareNet d; d.last = skip_share_net_from_abi(nd);
    const SwSharePlan p = sw_share_plan(d, g, sw);
    const S0Geom &sg = p.sg;
    const bool on = p.share_skip;
    // the first block of level 1 as the network would hold it: c_skip -> c_level1, stride 2
    ConvPackLayout l;
    ConvWeights cw;
    const bool have_w1 = nd->dtype == MI355_F32 && conv_pack_layout(nd->c_skip, nd->c_skip, c_level1, 2, &l) == MI355_OK && l.mfma;
    if (have_w1) cw = stand_in_conv_weights(l, nd->c_skip, c_level1, 2);  // (a stride-2 layout has the MFMA pack alone)
    const int nm = (int)g.mirrors.size();
    // a full batch of one rank; a short last batch, or the tiles one rank of several gets, is asked for with batch_samples
    const int per_forward = batch_samples > 0 ? batch_samples : sw_batch_tiles(nd->dtype, 0, nm) * nm;
    const S0ViewChoice v = stage0_views_choose(sw.views, sg, on, std::min(per_forward, (int)g.tiles.size() * nm), g.P, have_w1 ? &cw : nullptr, nd->c_skip,
                                               d.last.runtime_norm);
    memset(out, 0, sizeof(*out));
    out->enc0_viewed = v.enc0; out->half_viewed = v.half;
    out->depth[0] = sg.r; out->depth[1] = on ? sg.rs : 0;
    out->n_tiles = (int32_t)g.tiles.size(); out->n_mirrors = nm;
    for (int a = 0; a < 3; ++a) out->volume[a] = sg.Ve[a];
    const int n = sg.shared ? (int)sg.smp.size() : 0;
    for (int i = 0; i < n && i < max_samples; ++i) {
        const S0Sample &sm = sg.smp[i];
        mi355_stage0_view_sample &q = samples[i];
        memset(&q, 0, sizeof(q));
        q.offset = (((int64_t)sm.wv * sg.Ve[0] + sm.org[0]) * sg.Ve[1] + sm.org[1]) * sg.Ve[2] + sm.org[2];
        for (int f = 0; f < 6; ++f) q.faces |= sm.slab[f] >= 0 ? 1 << f : 0;
        q.shell_voxels[0] = stage0_shell_voxels(g.P, sg.r, sm.slab);
        q.shell_voxels[1] = on ? stage0_shell_voxels(g.P, sg.rs, sm.slab) : 0;
    }
    return n;
}

extern "C" int mi355_level1_share_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes,
                                       const mi355_level1_share_net *nd, int mode, mi355_level1_share_geom *out,
                                       mi355_level1_share_region *regions, int max_regions, mi355_level1_share_sample *samples, int max_samples) {
    MI355_REQUIRE(out && patch && nd && mode >= 0 && mode <= 2 && (regions || max_regions == 0) && (samples || max_samples == 0),
                  "mi355_level1_share_plan: bad argument");
    SwGeom g;
    MI355_TRY(sw_geom_from_abi(z, y, x, patch, step_size, mirror_axes, &g));
    SwSwitches sw = sw_switches();
    sw.level1 = mode;  // (the dry run is told the mode; a window reads it)
    const SwSharePlan p = sw_share_plan(level1_share_net_from_abi(nd), g, sw);
    const S0Geom &sg = p.sg;
    const L1Geom &lg = p.lg;
    memset(out, 0, sizeof(*out));
    out->possible = lg.possible; out->on = p.share_l1;
    out->r0 = lg.r0; out->k1 = lg.k1; out->d1 = lg.d1; out->dS = lg.dS;
    out->n_tiles = (int32_t)g.tiles.size(); out->n_mirrors = (int32_t)g.mirrors.size();
    for (int a = 0; a < 3; ++a) { out->padded[a] = g.Zp[a]; out->volume[a] = sg.Ve[a]; out->stage0_slab_thickness[a] = sg.t[a]; }
    out->tile_voxels = (int64_t)sg.smp.size() * (g.P[0] / 2) * (g.P[1] / 2) * (g.P[2] / 2);
    if (!lg.possible) return 0;
    out->n_regions = (int32_t)lg.regions.size();
    for (int a = 0; a < 3; ++a) { out->merged[a] = lg.merged[a]; out->region[a] = lg.R[a]; out->slab_thickness[a] = lg.t1[a]; }
    out->region_voxels = (int64_t)lg.regions.size() * (lg.R[0] / 2) * (lg.R[1] / 2) * (lg.R[2] / 2);
    for (size_t i = 0; i < lg.regions.size() && (int)i < max_regions; ++i) {
        mi355_level1_share_region &q = regions[i];
        memset(&q, 0, sizeof(q));
        q.mirror = g.mirrors[lg.regions[i].wv];
        for (int a = 0; a < 3; ++a) q.origin[a] = lg.regions[i].org[a];
        for (int f = 0; f < 6; ++f) q.faces |= lg.regions[i].slab[f] >= 0 ? 1 << f : 0;
    }
    const int n = (int)lg.smp.size();
    for (int i = 0; i < n; ++i) {
        const S0Sample &ls = lg.smp[i], &sm = sg.smp[i];
        mi355_level1_share_sample q;
        memset(&q, 0, sizeof(q));
        q.tile = i / (int)g.mirrors.size(); q.mirror = g.mirrors[sm.wv]; q.region = ls.wv;
        for (int a = 0; a < 3; ++a) { q.origin[a] = sm.org[a]; q.origin1[a] = ls.org[a]; }
        for (int f = 0; f < 6; ++f) {
            q.faces |= sm.slab[f] >= 0 ? 1 << f : 0;
            if (ls.slab[f] < 0) continue;
            const int a = f >> 1;
            q.slab[f] = 1;
            out->n_slabs[a] += 1;
            int64_t v = lg.t1[a];
            for (int k = 0; k < 3; ++k) {
                q.slab_shape[f][k] = k == a ? 2 * lg.t1[a] : g.P[k];
                q.slab_offset[f][k] = k == a && (f & 1) ? g.P[a] - 2 * lg.t1[a] : 0;
                if (k != a) v *= g.P[k] / 2;
            }
            out->slab_voxels += v;
        }
        if (i < max_samples) samples[i] = q;
    }
    return n;
}
