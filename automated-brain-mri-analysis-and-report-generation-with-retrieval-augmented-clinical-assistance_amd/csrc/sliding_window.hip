// The sliding-window predictor (host side): tile geometry and the Gaussian map, the shared stage 0 and what is built on it (slabs,
// merged slabs, the shared skip half, stage-0 views, the shared level 1), sw_accumulate and the mi355_sw_* entry points declared in
// include/mi355_nnunet.h, and the geometry dry runs through which the CPU tests see the decisions taken here.
//
// Reference behaviour restated here:
//   * nnU-Net v1 SegmentationNetwork._internal_predict_3D_3Dconv_tiled / _compute_steps_for_
//     sliding_window / _get_gaussian / _internal_maybe_mirror_and_pred_3D (un-vendored upstream;
//     SURVEY.md 8a rows T1-T5) as driven by run_brats2021_inference_singlethread.py:97-128.
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "unet_internal.h"

namespace mi355 {

// ---- sliding-window helpers (nnU-Net v1)
static std::vector<int> compute_steps(int patch, int image, double step_size) {
    // target = patch*step ; n = ceil((image-patch)/target)+1 ; actual = (image-patch)/(n-1)
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
static void gaussian_map(const int p[3], double sigma_scale, std::vector<float> &out) {
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

static std::mutex g_gauss_mu;
static int ensure_gaussian(mi355_unet *net, const int p[3]) {
    std::lock_guard<std::mutex> lk(g_gauss_mu);  // (one handle may be driven from two lanes)
    if (net->gauss_dev && net->gauss_p[0] == p[0] && net->gauss_p[1] == p[1] && net->gauss_p[2] == p[2])
        return MI355_OK;
    if (net->gauss_dev) { MI355_HIP(hipDeviceSynchronize()); MI355_HIP(hipFree(net->gauss_dev)); net->gauss_dev = nullptr; }
    std::vector<float> g;
    gaussian_map(p, 1.0 / 8.0, g);
    MI355_TRY(upload(g.data(), g.size(), &net->gauss_dev));
    net->gauss_p[0] = p[0]; net->gauss_p[1] = p[1]; net->gauss_p[2] = p[2];
    return MI355_OK;
}

struct SwGeom {
    int P[3], Zp[3], pad_lo[3];
    std::vector<TileDesc> tiles;   // origin of every tile, loop order axis0 outer .. axis2 inner
    std::vector<int> mirrors;      // TileDesc-style masks in nnU-Net's evaluation order
};

static int make_geom(const mi355_sw_opts &o, int Z, int Y, int X, SwGeom *g) {
    const int dims[3] = {Z, Y, X};
    std::vector<int> steps[3];
    for (int a = 0; a < 3; ++a) {
        g->P[a] = o.patch[a];
        MI355_REQUIRE(g->P[a] > 0 && dims[a] > 0, "bad patch / volume size");
        g->Zp[a] = std::max(dims[a], g->P[a]);       // pad_nd_image(..., "constant", 0)
        g->pad_lo[a] = (g->Zp[a] - dims[a]) / 2;     // pad_below = difference // 2
        steps[a] = compute_steps(g->P[a], g->Zp[a], o.step_size);
    }
    MI355_REQUIRE(o.step_size > 0.f && o.step_size <= 1.f, "step_size must be in (0, 1]");
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
static int sw_geom_from_abi(int z, int y, int x, const int32_t patch[3], float step_size, int mirror_axes, SwGeom *g) {
    mi355_sw_opts o;
    memset(&o, 0, sizeof(o));
    for (int a = 0; a < 3; ++a) o.patch[a] = patch[a];
    o.step_size = step_size; o.mirror_axes = mirror_axes;
    return make_geom(o, z, y, x, g);
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
constexpr int S0_SLAB_GROUP = 8;  // (8 slabs of 4 x 128 x 128: 2048 tiles of the F(2x2x2,3x3x3) kernel, 8 per CU)
struct S0Merged { int wv, side, org[3]; };  // a merged slab: its (mirrored) pass, the side of the faces it serves, its origin in that pass
struct S0Geom {
    bool shared = false;
    int r = 0;
    int rs = 0;                    // depth of the slab chain: r, or r + 1 with the shared skip half (one more conv behind stage 0)
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

static void stage0_geometry(const SwGeom &g, int r, S0Geom *o, int extra = 0) {
    static const int unit[3] = {4, 8, 8};
    *o = S0Geom();
    o->r = r; o->rs = r + extra;
    bool fits = r >= 1 && g.tiles.size() > 1;
    for (int a = 0; a < 3; ++a) {
        o->Ve[a] = ceil_div(g.Zp[a], unit[a]) * unit[a];
        o->t[a] = ceil_div(std::max(2 * o->rs, 1), unit[a]) * unit[a];
        fits = fits && g.P[a] >= o->t[a];
    }
    if (!fits) return;
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
    auto key_of = [&](const S0Sample &sm, int a, int side) {
        Key k = {sm.wv, side, 0, 0, 0};
        k[2 + a] = sm.org[a] + (side ? g.P[a] - o->t[a] : 0);
        if (a == 1) k[4] = sm.org[2];
        return k;
    };
    std::map<Key, int> keys[3];
    for (const S0Sample &sm : o->smp)
        for (int f = 2; f < 6; ++f)
            if (sm.slab[f] >= 0) keys[f >> 1][key_of(sm, f >> 1, f & 1)] = 0;
    for (int a = 1; a < 3; ++a)
        for (auto &kv : keys[a]) {
            kv.second = (int)o->merged[a].size();
            o->merged[a].push_back(S0Merged{kv.first[0], kv.first[1], {kv.first[2], kv.first[3], kv.first[4]}});
        }
    for (const S0Sample &sm : o->smp) {
        std::array<int, 6> idx = {-1, -1, -1, -1, -1, -1};
        for (int f = 2; f < 6; ++f)
            if (sm.slab[f] >= 0) idx[f] = keys[f >> 1][key_of(sm, f >> 1, f & 1)];
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

// ---- shared skip half.  The first block of the last decoder stage reads the virtual concat (upsampled, skip) and is linear in
// front of its bias and activation: out = act(bias + conv(W_up, up) + conv(W_skip, skip)).  Its skip is the output of the shared
// stage 0, so S = conv(W_skip, skip) is one more translation-equivariant layer behind it: computed once per (net, mirror) over the
// whole volume and over the slabs - whose chain is then r + 1 layers deep: thickness >= 2 (r + 1), shell r + 1 for S, r for the skip
// as before -, gathered per tile next to the skip, and added by the per-tile launch, which runs over the upsampled half alone
// (half the MFMAs of the largest launch of a forward), in its epilogue (Wino3Args::addend).
// What the decision may depend on is what stage 0's may: the network and the geometry of all tiles, never rank, lane or batch.
// The network's part: also what decides, at mi355_unet_create, whether the block gets the packs of its two halves.  A last stage
// of one block is left alone: its conv is the net's last and may carry the fused head, which has no addend.
bool skip_share_network_ok(const SkipShareNet &d) {
    if (!env_switch("MI355_SHARE_SKIP_CONV")) return false;
    if (d.dtype != MI355_F32 || d.r < 1 || d.stride != 1 || d.runtime_norm || d.post_affine || !d.skip_is_enc0 || d.head_ncls > 0) return false;
    if (d.c_up <= 0 || d.c_skip <= 0 || d.c_up % 4 || d.c_skip % 4 || d.cout % 4) return false;
    ConvPackLayout lu, ls;
    if (conv_pack_layout(d.c_up, d.c_up, d.cout, 1, &lu) != MI355_OK || conv_pack_layout(d.c_skip, d.c_skip, d.cout, 1, &ls) != MI355_OK) return false;
    return lu.wino3 && ls.mfma;
}
static bool skip_share_decide(const SkipShareNet &d, const SwGeom &g) {
    if (!skip_share_network_ok(d)) return false;
    S0Geom sg;
    stage0_geometry(g, d.r, &sg, 1);
    if (!sg.shared) return false;  // (one tile, or a patch thinner than a slab of the deeper chain)
    // the per-tile launch over the upsampled half must be the kernel that has the addend epilogue.  Asked for ONE sample of the
    // tile shape: more samples never send a call away from that kernel, and the answer must not depend on the batch.
    // (plan_wino3 is the first step of plan_conv_f32 and, unlike it, answers without leaving an error text behind)
    ConvPackLayout lu;
    (void)conv_pack_layout(d.c_up, d.c_up, d.cout, 1, &lu);
    static float stand_in[2];
    const ConvWeights cw = stand_in_conv_weights(lu, d.c_up, d.cout, 1);  // (lu.wino3, which skip_share_network_ok asked for, implies every pack)
    ConvCall c = make_call<float>(stand_in, d.c_up, 1, g.P[0], g.P[1], g.P[2], stand_in, nullptr, ACT_LRELU, 0.01f);
    c.addend = stand_in;
    ConvPlan p;
    if (!plan_wino3(cw, c, &p) || strcmp(p.name, "conv3_f32_wino3_kernel<3, false>") != 0) return false;
    c.addend = nullptr;  // (and the same call without the addend is a launch of the plain instantiation)
    return plan_wino3(cw, c, &p) && strcmp(p.name, "conv3_f32_wino3_kernel<0, false>") == 0;
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

static void slab_dims(const SwGeom &g, const S0Geom &sg, int a, int S[3]) {
    for (int k = 0; k < 3; ++k) S[k] = k == a ? sg.t[k] : g.P[k];
}

// appends the stage-0 regions to the plan of `n_samples` (tile, mirror) samples per forward
static void stage0_plan(const mi355_unet &net, const SwGeom &g, const S0Geom &sg, int n_samples, Plan *pl) {
    size_t o = pl->total;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~size_t(255); return r; };
    int maxc = 0;
    for (auto &L : net.enc[0]) maxc = std::max(maxc, L.cout);
    const size_t wv = g.mirrors.size() * (size_t)sg.Ve[0] * sg.Ve[1] * sg.Ve[2];
    size_t sl = 0, sl_a[3];
    for (int a = 0; a < 3; ++a) {
        int S[3];
        slab_dims(g, sg, a, S);
        sl_a[a] = (size_t)ceil_div(n_samples * sg.max_faces[a], S0_SLAB_GROUP) * S0_SLAB_GROUP * S[0] * S[1] * S[2];
        if (sg.merge && a > 0)  // merged slabs: every key's slab, for all mirrors, lives from the whole-volume pass to the last forward
            sl_a[a] = sg.merged[a].size() * (size_t)sg.mdim[a][0] * sg.mdim[a][1] * sg.mdim[a][2];
        sl = std::max(sl, sl_a[a]);
    }
    pl->s0.wv_in = take(wv * net.cin_pad * 4);
    pl->s0.slab_in = take(sl * net.cin_pad * 4);
    for (int k = 0; k < 2 && k < sg.r - 1; ++k) {
        pl->s0.wv_tmp[k] = take(wv * maxc * 4);
        pl->s0.slab_tmp[k] = take(sl * maxc * 4);
    }
    pl->s0.wv_out = take(wv * net.enc[0].back().cout * 4);
    for (int a = 0; a < 3; ++a) pl->s0.slab_out[a] = take(sl_a[a] * net.enc[0].back().cout * 4);
    if (sg.rs > sg.r) {  // shared skip half: S for the whole volume per mirror and for the slabs (its tile tensor lives in the level-0 buffer the last decoder stage leaves free)
        pl->s0.wv_skip = take(wv * net.dec.back()[0].cout * 4);
        for (int a = 0; a < 3; ++a) pl->s0.slab_skip[a] = take(sl_a[a] * net.dec.back()[0].cout * 4);
    }
    pl->total = o;
}

// a box of the (mirrored) pass, origin b and size S, as the TileDesc extract_tiles takes: origin in the unflipped padded volume
static TileDesc pass_box(const SwGeom &g, int mirror, const int b[3], const int S[3]) {
    int o[3];
    for (int a = 0; a < 3; ++a) o[a] = (mirror >> a) & 1 ? g.Zp[a] - b[a] - S[a] : b[a];
    return TileDesc{o[0], o[1], o[2], mirror};
}

// enc[0] over n boxes of S voxels each, gathered from the volume, placed as `at` says (S0Placement, unet_internal.h): in_off receives
// the input, the last block writes out_off.
// group > 0: the convs run as launches of exactly `group` boxes each (n is a multiple of it).
// label: suffix of the gather's profile entry (the merged slabs name theirs).
// skip_off != 0 (shared skip half): one more launch behind the last block - the skip half of the last decoder stage's first conv,
// zero bias, no activation - writes S there.
static int stage0_run(mi355_unet *net, const Plan &pl, const SwVolume &v, const SwGeom &g, const std::vector<TileDesc> &boxes, const S0Placement &at,
                      hipStream_t s) {
    const int *const S = at.S;
    const int n = (int)boxes.size();
    const size_t vox = (size_t)S[0] * S[1] * S[2];
    for (int b0 = 0; b0 < n; b0 += S0_MAX_SAMPLES) {
        const int nb = std::min(S0_MAX_SAMPLES, n - b0);
        ProfScope ps(net, s, std::string("extract_tiles_kernel") + at.label, 0.0, (double)nb * vox * 4.0 * (net->in_channels + net->cin_pad));
        MI355_TRY(extract_tiles(v.vol, net->in_channels, v.Z, v.Y, v.X, g.pad_lo[0], g.pad_lo[1], g.pad_lo[2], boxes.data() + b0, nb, S[0], S[1], S[2],
                                net->cin_pad, (void *)(pl.arena + at.in_off + (size_t)b0 * vox * net->cin_pad * 4), net->dtype, s));
    }
    const int ng = at.group > 0 ? at.group : n;
    MI355_REQUIRE(n % ng == 0, "shared stage 0: %d boxes in launches of %d", n, ng);
    for (int g0 = 0; g0 < n; g0 += ng) {
        const void *cur = pl.arena + at.in_off + (size_t)g0 * vox * net->cin_pad * 4;
        int curC = net->cin_pad;
        for (size_t i = 0; i < net->enc[0].size(); ++i) {
            const ConvLayer &L = net->enc[0][i];
            const bool last = i + 1 == net->enc[0].size();
            void *out = pl.arena + (last ? at.out_off : at.tmp_off[i & 1]) + (size_t)g0 * vox * L.cout * 4;
            MI355_TRY(run_block(net, pl, L, cur, curC, nullptr, 0, ng, S[0], S[1], S[2], out, s));
            if ((!last || at.skip_off) && at.mask_zp) {
                // the next conv must see zero padding outside the padded volume, not act(bias)
                const double outside = (double)ng * (vox - (double)at.mask_zp[0] * at.mask_zp[1] * at.mask_zp[2]);
                ProfScope ps(net, s, "stage0_mask_kernel", 0.0, outside * L.cout * 4.0);
                MI355_TRY(stage0_mask((float *)out, ng, S, at.mask_zp, L.cout, s));
            }
            cur = out; curC = L.cout;
        }
        if (at.skip_off) {
            const ConvLayer &Ld = net->dec.back()[0];
            BlockOpts bo;
            bo.half = &Ld.w_skip; bo.half_name = " skip-half";
            MI355_TRY(run_block(net, pl, Ld, cur, curC, nullptr, 0, ng, S[0], S[1], S[2], pl.arena + at.skip_off + (size_t)g0 * vox * Ld.cout * 4, s, bo));
        }
    }
    return MI355_OK;
}

// whole-volume pass: one box per mirror
static int stage0_whole(mi355_unet *net, const Plan &pl, const SwVolume &v, const SwGeom &g, const S0Geom &sg, hipStream_t s) {
    std::vector<TileDesc> boxes;
    const int zero[3] = {0, 0, 0};
    // (a flipped axis: the flipped volume starts at 0 and its zero extension follows it, as on an unflipped axis)
    for (int m : g.mirrors) boxes.push_back(pass_box(g, m, zero, sg.Ve));
    const bool extended = sg.Ve[0] != g.Zp[0] || sg.Ve[1] != g.Zp[1] || sg.Ve[2] != g.Zp[2];
    S0Placement at;
    at.S = sg.Ve; at.mask_zp = extended ? g.Zp : nullptr;
    at.in_off = pl.s0.wv_in; at.tmp_off = pl.s0.wv_tmp; at.out_off = pl.s0.wv_out; at.skip_off = pl.s0.wv_skip;
    return stage0_run(net, pl, v, g, boxes, at, s);
}

// merged y- and x-slabs: every key, one launch group per axis (stage0_merge_geometry)
static int stage0_merged(mi355_unet *net, const Plan &pl, const SwVolume &v, const SwGeom &g, const S0Geom &sg, hipStream_t s) {
    for (int a = 1; a < 3; ++a) {
        if (sg.merged[a].empty()) continue;
        std::vector<TileDesc> boxes;
        for (const S0Merged &k : sg.merged[a]) boxes.push_back(pass_box(g, g.mirrors[k.wv], k.org, sg.mdim[a]));
        // along the axes a slab spans the extended volume it holds [Zp, Ve), which is zero in front of every conv
        const int keep[3] = {g.Zp[0], a == 1 ? sg.mdim[a][1] : g.Zp[1], sg.mdim[a][2]};
        const bool extended = keep[0] != sg.mdim[a][0] || keep[1] != sg.mdim[a][1];
        S0Placement at;
        at.S = sg.mdim[a]; at.mask_zp = extended ? keep : nullptr; at.label = " merged-slabs";
        at.in_off = pl.s0.slab_in; at.tmp_off = pl.s0.slab_tmp; at.out_off = pl.s0.slab_out[a]; at.skip_off = pl.s0.slab_skip[a];
        MI355_TRY(stage0_run(net, pl, v, g, boxes, at, s));
    }
    return MI355_OK;
}

// ---- stage-0 views (MI355_STAGE0_VIEWS).  The gather above copies, per tile, mostly values that already lie in the whole-volume
// tensors: a tile's copy differs from them only inside the shells.  Each of the two tile tensors has one reader - the level-0
// features the first stride-2 conv (enc[1][0]), the skip half S the addend epilogue of the up-half launch -, so where that reader
// can take a per-sample view (kernels.h S0View) it reads the whole-volume tensor in place and only shell voxels from the tile
// tensor, and the gather writes the shells alone (stage0_gather_shells).  The tile tensors stay where they are, with their dense
// strides; outside the shells they then hold stale values nobody reads.
// Views change where bytes are read, never which kernel runs or in which order anything is summed: results are bit-identical, and
// unlike stage0_plan this decision may depend on the batch.  Per tensor and per forward:
//   * the level-0 features: the shared skip half is on (otherwise the concat conv reads them whole, as in1), and the planner - asked
//     first, for exactly this call - sends enc[1][0] to conv3_f32_s2dma_kernel; the launch then runs conv3_f32_s2dma_kernel_view;
//   * S: the shared skip half is on (its reader is then always conv3_f32_wino3_kernel<3, false>).
// A view that cannot be built (stage0_view_make: offsets beyond 32 bits) falls back to the full gather for that tensor.
struct S0ViewChoice { bool enc0 = false, half = false; };
// w1: the weights (or, for a dry run, the pack layout with stand-in pointers) of the first block of level 1, null = none that
// qualifies; c0 its input channels; w1_stats: it carries run-time statistics
static S0ViewChoice stage0_views_choose(const S0Geom &sg, bool share_skip, int n_samples, const int P[3], const ConvWeights *w1, int c0, bool w1_stats) {
    S0ViewChoice v;
    if (!env_switch("MI355_STAGE0_VIEWS") || !sg.shared || !share_skip || n_samples < 1 || n_samples > S0_VIEW_MAX_SAMPLES) return v;
    v.half = true;
    if (!w1 || !w1->wp_dev || w1->stride != 2) return v;
    static float stand_in[2];
    ConvCall c = make_call<float>(stand_in, c0, n_samples, P[0], P[1], P[2], stand_in, w1_stats ? (double *)stand_in : nullptr, ACT_LRELU, 0.01f);
    ConvPlan p;
    v.enc0 = plan_conv_f32(*w1, c, &p) == MI355_OK && p.family == FAM_S2DMA;
    return v;
}
static S0ViewChoice stage0_views_decide(const mi355_unet &net, const S0Geom &sg, bool share_skip, int n_samples, const int P[3]) {
    if (net.dtype != MI355_F32 || net.num_pool < 1 || net.enc[1].empty()) return S0ViewChoice();
    const ConvLayer &L = net.enc[1][0];
    return stage0_views_choose(sg, share_skip, n_samples, P, L.is_stem ? nullptr : &L.w, net.enc[0].back().cout, L.runtime_norm);
}

// the slabs of one batch of samples (indices into sg.smp), then the gather of the batch's tile tensor.  want: which tensors'
// readers will take a view; *enc0_view / *half_view receive the views that were built (src = null: none, the tensor is dense).
static int stage0_tiles(mi355_unet *net, const Plan &pl, const SwVolume &v, const SwGeom &g, const S0Geom &sg, const std::vector<int> &samples,
                        hipStream_t s, S0ViewChoice want = S0ViewChoice(), S0View *enc0_view = nullptr, S0View *half_view = nullptr,
                        S0GatherArgs *ga_out = nullptr) {
    const int n = (int)samples.size();
    MI355_REQUIRE(n <= S0_MAX_SAMPLES, "shared stage 0: %d samples per forward (max %d)", n, S0_MAX_SAMPLES);
    const int C = net->enc[0].back().cout;
    S0GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    for (int i = 0; i < n; ++i) ga.smp[i] = sg.smp[samples[i]];
    for (int a = 0; a < 3; ++a) {
        int S[3];
        slab_dims(g, sg, a, S);
        if (sg.merge && a > 0) {  // merged slabs: computed behind the whole-volume pass, the sample's faces index them
            for (int i = 0; i < n; ++i)
                for (int side = 0; side < 2; ++side) ga.smp[i].slab[2 * a + side] = sg.mslab[samples[i]][2 * a + side];
            ga.slab[a] = (const float *)(pl.arena + pl.s0.slab_out[a]);
            ga.slab2[a] = (const float *)(pl.arena + pl.s0.slab_skip[a]);
            continue;
        }
        std::vector<TileDesc> boxes;
        for (int i = 0; i < n; ++i)
            for (int side = 0; side < 2; ++side) {
                S0Sample &sm = ga.smp[i];
                if (sm.slab[2 * a + side] < 0) continue;
                int b[3] = {sm.org[0], sm.org[1], sm.org[2]};
                if (side) b[a] += g.P[a] - sg.t[a];
                sm.slab[2 * a + side] = (int)boxes.size();
                boxes.push_back(pass_box(g, g.mirrors[sm.wv], b, S));
            }
        ga.slab[a] = (const float *)(pl.arena + pl.s0.slab_out[a]);
        if (boxes.empty()) continue;
        while (boxes.size() % S0_SLAB_GROUP) boxes.push_back(boxes.back());  // (a whole last launch: its spare results are not read)
        S0Placement at;
        at.S = S; at.group = S0_SLAB_GROUP;
        at.in_off = pl.s0.slab_in; at.tmp_off = pl.s0.slab_tmp; at.out_off = pl.s0.slab_out[a]; at.skip_off = pl.s0.slab_skip[a];
        MI355_TRY(stage0_run(net, pl, v, g, boxes, at, s));
        ga.slab2[a] = (const float *)(pl.arena + pl.s0.slab_skip[a]);
    }
    ga.wv = (const float *)(pl.arena + pl.s0.wv_out);
    ga.out = (float *)(pl.arena + pl.off[(net->enc[0].size() - 1) & 1][0]);
    for (int a = 0; a < 3; ++a) { ga.P[a] = g.P[a]; ga.Ve[a] = sg.Ve[a]; ga.t[a] = sg.t[a]; }
    stage0_gather_dense(&ga);
    if (sg.merge)
        for (int a = 1; a < 3; ++a)
            for (int k = 0; k < 3; ++k) { ga.D[a][k] = sg.mdim[a][k]; ga.so[a][k] = k < a && (k == 0 || a == 2); }
    ga.r = sg.r; ga.C4 = C / 4;
    int C2 = 0;
    if (sg.rs > sg.r) {  // shared skip half: S rides along, into the level-0 buffer that is not the skip's
        C2 = net->dec.back()[0].cout;
        ga.wv2 = (const float *)(pl.arena + pl.s0.wv_skip);
        ga.out2 = (float *)(pl.arena + pl.off[((net->enc[0].size() - 1) & 1) ^ 1][0]);
        ga.r2 = sg.rs; ga.C42 = C2 / 4;
    } else
        for (int a = 0; a < 3; ++a) ga.slab2[a] = nullptr;
    if (ga_out) *ga_out = ga;  // (shared level 1: the sources of the batch's sub-boxes)
    const double pv = (double)n * g.P[0] * g.P[1] * g.P[2];
    // stage-0 views: a view that cannot be built leaves its tensor to the full gather
    const int n_wv = (int)g.mirrors.size();
    bool v0 = want.enc0 && enc0_view && stage0_view_make(ga.wv, n_wv, ga.Ve, ga.P, C, ga.r, ga.smp, n, enc0_view) == MI355_OK;
    bool v1 = want.half && half_view && C2 && stage0_view_make(ga.wv2, n_wv, ga.Ve, ga.P, C2, ga.r2, ga.smp, n, half_view) == MI355_OK;
    double shell0 = 0.0, shell1 = 0.0;
    for (int i = 0; i < n; ++i) {
        shell0 += (double)stage0_shell_voxels(ga.P, ga.r, ga.smp[i].slab);
        if (C2) shell1 += (double)stage0_shell_voxels(ga.P, ga.r2, ga.smp[i].slab);
    }
    // (one profile entry, as before; its bytes are what is moved: read + written)
    ProfScope ps(net, s, "stage0_gather_kernel", 0.0, 2.0 * 4.0 * ((v0 ? shell0 : pv) * C + (v1 ? shell1 : pv) * C2));
    if (!v0 && !v1) return stage0_gather(ga, n, s);
    if (v0) MI355_TRY(stage0_gather_shells(ga, n, 0, s));
    else {  // the level-0 features whole, alone
        S0GatherArgs g0 = ga;
        g0.out2 = nullptr; g0.wv2 = nullptr;
        MI355_TRY(stage0_gather(g0, n, s));
    }
    if (!C2) return MI355_OK;
    if (v1) return stage0_gather_shells(ga, n, 1, s);
    S0GatherArgs g1 = ga;  // S whole, alone: as the first tensor of a gather
    g1.wv = ga.wv2; g1.out = ga.out2; g1.r = ga.r2; g1.C4 = ga.C42;
    for (int a = 0; a < 3; ++a) g1.slab[a] = ga.slab2[a];
    g1.out2 = nullptr; g1.wv2 = nullptr;
    return stage0_gather(g1, n, s);
}

// ---- shared level 1: the geometry (level1_geometry), the decision (level1_share_decide) and their dry run
// (mi355_level1_share_plan), then the region pass and the per-forward slabs that run on them (MI355_SHARE_LEVEL1).
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
struct L1Region { int wv; int org[3]; int face[6]; };  // org in the (mirrored) pass; face[f] = 0: face f needs stage-0 shells, -1: not
struct L1Sample { int region; int org1[3]; int slab[6]; };  // origin inside the region at level 1; slab[f] = 0: face f has a level-1 slab, else -1
struct L1Geom {
    bool possible = false;
    int r0 = 0, k1 = 0, d1 = 0, dS = 0;
    bool merged[3] = {false, false, false};
    int R[3] = {0, 0, 0};    // level-0 extent of a region
    int t1[3] = {0, 0, 0};   // level-1 slab thickness (0 on a per-origin axis)
    std::vector<L1Region> regions;  // sorted by (mirror, origin)
    std::vector<L1Sample> smp;      // [tile][mirror], as S0Geom::smp
};

static void level1_geometry(const SwGeom &g, const S0Geom &sg, int k1, L1Geom *o) {
    static const int unit[3] = {4, 8, 8};
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
        o->t1[a] = ceil_div(std::max(sg.r / 2 + 2 * k1 + 2, 2 * o->dS), unit[a]) * unit[a];
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
        L1Region rg;
        rg.wv = kv.first[0];
        for (int a = 0; a < 3; ++a) {
            rg.org[a] = kv.first[1 + a];
            rg.face[2 * a] = !o->merged[a] && rg.org[a] > 0 ? 0 : -1;
            rg.face[2 * a + 1] = !o->merged[a] && rg.org[a] + g.P[a] < g.Zp[a] ? 0 : -1;
        }
        o->regions.push_back(rg);
    }
    for (const S0Sample &sm : sg.smp) {
        L1Sample ls;
        ls.region = keys[key_of(sm)];
        for (int a = 0; a < 3; ++a) {
            ls.org1[a] = o->merged[a] ? sm.org[a] / 2 : 0;
            ls.slab[2 * a] = o->merged[a] ? sm.slab[2 * a] : -1;  // (S0Sample::slab: 0 where the face lies inside the volume)
            ls.slab[2 * a + 1] = o->merged[a] ? sm.slab[2 * a + 1] : -1;
        }
        o->smp.push_back(ls);
    }
}

// The network side: the last decoder stage as the shared skip half sees it, and level 1.
struct L1ShareNet {
    SkipShareNet last;
    int num_pool = 0;
    int k1 = 0;              // blocks of enc[1]; its first has stride 2, the others stride 1
    int c1 = 0;              // their output channels
    bool skip_is_enc1 = true;  // the second input of dec[np - 2][0] is enc[1]'s output
    int dec_blocks = 0;      // blocks of dec[np - 2]
    int c_up = 0, cout = 0;  // of dec[np - 2][0]: channels of the upsampled half, output channels
};
// mode: 0 off, 1 the default rule, 2 wherever it is structurally possible.  Depends on the network and the geometry of all tiles
// only.  The default rule asks P / 2 >= 8 t1 on every merged axis: a slab costs t1 / (P / 2) of a tile per face, so smaller patches
// lose, and it leaves the patch 64 and 32 paths that existing tests pin bit for bit alone.
static bool level1_share_decide(const L1ShareNet &d, const SwGeom &g, int mode, L1Geom *lg) {
    L1Geom local;
    if (!lg) lg = &local;
    *lg = L1Geom();
    const bool skip_on = skip_share_decide(d.last, g);
    S0Geom sg;
    stage0_geometry(g, d.last.r, &sg, skip_on ? 1 : 0);
    level1_geometry(g, sg, d.k1, lg);
    if (mode == 0 || !lg->possible) return false;
    // fp32 (skip_share_decide), the shared stage 0, the shared skip half and the stage-0 views all on
    if (!skip_on || !sg.shared || !env_switch("MI355_STAGE0_VIEWS")) return false;
    // run-time statistics and an unfolded BatchNorm are the network's, not a block's: skip_share_decide has refused them
    if (d.num_pool < 2 || d.k1 < 1 || !d.skip_is_enc1 || d.dec_blocks < 2) return false;
    if (d.c1 <= 0 || d.c1 % 4 || d.c_up <= 0 || d.c_up % 4 || d.cout % 4) return false;
    // dec[np - 2][0] over the upsampled half alone must be the kernel with the addend epilogue, its skip half a packed conv
    ConvPackLayout lu, ls;
    if (conv_pack_layout(d.c_up, d.c_up, d.cout, 1, &lu) != MI355_OK || conv_pack_layout(d.c1, d.c1, d.cout, 1, &ls) != MI355_OK) return false;
    if (!lu.wino3 || !ls.mfma) return false;
    static float stand_in[2];
    const ConvWeights cw = stand_in_conv_weights(lu, d.c_up, d.cout, 1);
    ConvCall c = make_call<float>(stand_in, d.c_up, 1, g.P[0] / 2, g.P[1] / 2, g.P[2] / 2, stand_in, nullptr, ACT_LRELU, 0.01f);
    c.addend = stand_in;
    ConvPlan p;
    if (!plan_wino3(cw, c, &p) || strcmp(p.name, "conv3_f32_wino3_kernel<3, false>") != 0) return false;
    // the regions read enc[0]'s whole-volume result in place: their first conv must be the stride-2 kernel that takes a view
    if ((int)lg->regions.size() > S0_VIEW_MAX_SAMPLES) return false;
    ConvPackLayout l1;
    if (conv_pack_layout(d.last.c_skip, d.last.c_skip, d.c1, 2, &l1) != MI355_OK || !l1.mfma) return false;
    const ConvWeights cw1 = stand_in_conv_weights(l1, d.last.c_skip, d.c1, 2);
    const ConvCall cr = make_call<float>(stand_in, d.last.c_skip, (int)lg->regions.size(), lg->R[0], lg->R[1], lg->R[2], stand_in, nullptr, ACT_LRELU, 0.01f);
    if (plan_conv_f32(cw1, cr, &p) != MI355_OK || p.family != FAM_S2DMA) return false;
    static const int unit[3] = {4, 8, 8};
    if (mode == 1)
        for (int a = 0; a < 3; ++a) {
            if (!lg->merged[a]) continue;
            if (g.P[a] / 2 < 8 * lg->t1[a]) return false;
            if (lg->R[a] / 2 % unit[a]) return false;  // a region that is no whole number of conv tiles at level 1 leaves the F(2x2x2,3x3x3) kernel
        }
    return true;
}

static L1ShareNet level1_share_net(const mi355_unet &net) {
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

constexpr int L1_SLAB_GROUP = 8;  // level-1 slabs run as launches of exactly this many (the last one filled up), as the stage-0 slabs do
static int level1_slab_rows(int n_samples) { return ceil_div(2 * n_samples, L1_SLAB_GROUP) * L1_SLAB_GROUP; }

// appends the level-1 regions to the plan of `n_samples` samples per forward
static void level1_plan(const mi355_unet &net, const SwGeom &g, const S0Geom &sg, const L1Geom &lg, int n_samples, Plan *pl) {
    size_t o = pl->total;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~size_t(255); return r; };
    int maxc0 = 0;
    for (auto &L : net.enc[0]) maxc0 = std::max(maxc0, L.cout);
    const size_t c0 = net.enc[0].back().cout, c1 = net.enc[1].back().cout, cS = net.dec[net.num_pool - 2][0].cout;
    size_t rs_a[3] = {0, 0, 0}, rs_max = 0;
    for (int a = 0; a < 3; ++a) {
        size_t box = sg.t[a];
        for (int k = 0; k < 3; ++k) if (k != a) box *= lg.R[k];
        for (const L1Region &rg : lg.regions) rs_a[a] += ((rg.face[2 * a] >= 0) + (rg.face[2 * a + 1] >= 0)) * box;
        rs_max = std::max(rs_max, rs_a[a]);
    }
    if (rs_max) {
        pl->l1.rs_in = take(rs_max * net.cin_pad * 4);
        for (int k = 0; k < 2 && k < sg.r - 1; ++k) pl->l1.rs_tmp[k] = take(rs_max * maxc0 * 4);
        for (int a = 0; a < 3; ++a) pl->l1.rs_out[a] = take(rs_a[a] * c0 * 4);
    }
    const size_t rv0 = lg.regions.size() * (size_t)lg.R[0] * lg.R[1] * lg.R[2], rv1 = rv0 / 8;
    pl->l1.r_shell = take(rv0 * c0 * 4);
    for (int k = 0; k < 2; ++k) pl->l1.r_e[k] = take(rv1 * c1 * 4);
    pl->l1.r_s = take(rv1 * cS * 4);
    size_t tmp = 0;
    for (int a = 0; a < 3; ++a) {
        if (!lg.merged[a]) continue;
        size_t sv0 = (size_t)level1_slab_rows(n_samples) * 2 * lg.t1[a];
        for (int k = 0; k < 3; ++k) if (k != a) sv0 *= g.P[k];
        pl->l1.sub_in[a] = take(sv0 * c0 * 4);
        pl->l1.s_e[a] = take(sv0 / 8 * c1 * 4);
        pl->l1.s_s[a] = take(sv0 / 8 * cS * 4);
        tmp = std::max(tmp, sv0 / 8 * c1 * 4);
    }
    pl->l1.s_tmp = take(tmp);
    pl->total = o;
}

// zero what lies outside `keep` of n boxes of S voxels each (nothing to do where keep == S)
static int level1_mask(mi355_unet *net, void *x, int n, const int S[3], const int keep[3], int C, hipStream_t s) {
    if (keep[0] == S[0] && keep[1] == S[1] && keep[2] == S[2]) return MI355_OK;
    ProfScope ps(net, s, "stage0_mask_kernel", 0.0, (double)n * ((double)S[0] * S[1] * S[2] - (double)keep[0] * keep[1] * keep[2]) * C * 4.0);
    return stage0_mask((float *)x, n, S, keep, C, s);
}

// enc[1] (its first block through in0_view when given) and the skip half of dec[np - 2][0] over n boxes of S level-0 voxels:
// x0 -> e_out (through tmp, and e_out itself, in turns) and s_out; keep1: zeros restored outside it behind every block
static int level1_chain(mi355_unet *net, const Plan &pl, const void *x0, const S0View *view, int n, const int S[3], const int *keep1, void *tmp,
                        void *e_out, void *s_out, hipStream_t s) {
    const std::vector<ConvLayer> &e1 = net->enc[1];
    const int S1[3] = {S[0] / 2, S[1] / 2, S[2] / 2};
    const void *cur = x0;
    int curC = net->enc[0].back().cout;
    for (size_t i = 0; i < e1.size(); ++i) {
        void *out = ((e1.size() - 1 - i) & 1) ? tmp : e_out;  // (the last block writes e_out)
        BlockOpts bo;
        if (i == 0) bo.in0_view = view;
        MI355_TRY(run_block(net, pl, e1[i], cur, curC, nullptr, 0, n, i ? S1[0] : S[0], i ? S1[1] : S[1], i ? S1[2] : S[2], out, s, bo));
        if (keep1) MI355_TRY(level1_mask(net, out, n, S1, keep1, e1[i].cout, s));
        cur = out; curC = e1[i].cout;
    }
    const ConvLayer &Ld = net->dec[net->num_pool - 2][0];
    BlockOpts bo;
    bo.half = &Ld.w_skip; bo.half_name = " skip-half";
    return run_block(net, pl, Ld, cur, curC, nullptr, 0, n, S1[0], S1[1], S1[2], s_out, s, bo);
}

// region pass, once per volume behind the whole-volume pass: the stage-0 slabs at the regions' faces on per-origin axes, the
// regions' level-0 shells, then enc[1] and the skip half over the regions, their level-0 input read in place through a view
static int level1_regions(mi355_unet *net, const Plan &pl, const SwVolume &v, const SwGeom &g, const S0Geom &sg, const L1Geom &lg, hipStream_t s) {
    const int nreg = (int)lg.regions.size();
    const int c0 = net->enc[0].back().cout;
    MI355_REQUIRE(nreg > 0 && nreg <= S0_VIEW_MAX_SAMPLES, "shared level 1: %d regions (max %d)", nreg, S0_VIEW_MAX_SAMPLES);
    S0GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    for (int i = 0; i < nreg; ++i) {
        ga.smp[i].wv = lg.regions[i].wv;
        for (int k = 0; k < 3; ++k) ga.smp[i].org[k] = lg.regions[i].org[k];
        for (int f = 0; f < 6; ++f) ga.smp[i].slab[f] = -1;
    }
    bool any = false;
    for (int a = 0; a < 3; ++a) {
        int S[3], keep[3];
        for (int k = 0; k < 3; ++k) { S[k] = k == a ? sg.t[k] : lg.R[k]; keep[k] = lg.merged[k] ? g.Zp[k] : S[k]; }
        std::vector<TileDesc> boxes;
        for (int i = 0; i < nreg; ++i)
            for (int side = 0; side < 2; ++side) {
                if (lg.regions[i].face[2 * a + side] < 0) continue;
                int b[3] = {lg.regions[i].org[0], lg.regions[i].org[1], lg.regions[i].org[2]};
                if (side) b[a] += lg.R[a] - sg.t[a];
                ga.smp[i].slab[2 * a + side] = (int)boxes.size();
                boxes.push_back(pass_box(g, g.mirrors[lg.regions[i].wv], b, S));
            }
        ga.slab[a] = (const float *)(pl.arena + pl.l1.rs_out[a]);
        if (boxes.empty()) continue;
        any = true;
        const bool extended = keep[0] != S[0] || keep[1] != S[1] || keep[2] != S[2];
        S0Placement at;
        at.S = S; at.mask_zp = extended ? keep : nullptr; at.label = " region-slabs";
        at.in_off = pl.l1.rs_in; at.tmp_off = pl.l1.rs_tmp; at.out_off = pl.l1.rs_out[a];
        MI355_TRY(stage0_run(net, pl, v, g, boxes, at, s));
        // (stage0_run leaves its last layer unmasked when no skip half follows; the regions read it)
        MI355_TRY(level1_mask(net, pl.arena + pl.l1.rs_out[a], (int)boxes.size(), S, keep, c0, s));
    }
    ga.wv = (const float *)(pl.arena + pl.s0.wv_out);
    ga.out = (float *)(pl.arena + pl.l1.r_shell);
    for (int k = 0; k < 3; ++k) { ga.P[k] = lg.R[k]; ga.Ve[k] = sg.Ve[k]; ga.t[k] = sg.t[k]; }
    stage0_gather_dense(&ga);
    ga.r = sg.r; ga.C4 = c0 / 4;
    if (any) {
        double shell = 0.0;
        for (int i = 0; i < nreg; ++i) shell += (double)stage0_shell_voxels(ga.P, ga.r, ga.smp[i].slab);
        ProfScope ps(net, s, "stage0_gather_kernel regions", 0.0, 2.0 * 4.0 * shell * c0);
        MI355_TRY(stage0_gather_shells(ga, nreg, 0, s));
    }
    S0View view;
    MI355_TRY(stage0_view_make(ga.wv, (int)g.mirrors.size(), ga.Ve, ga.P, c0, ga.r, ga.smp, nreg, &view));
    int keep1[3], R1[3];
    bool extended = false;
    for (int k = 0; k < 3; ++k) { R1[k] = lg.R[k] / 2; keep1[k] = lg.merged[k] ? g.Zp[k] / 2 : R1[k]; extended = extended || keep1[k] != R1[k]; }
    const int last = (int)((net->enc[1].size() - 1) & 1);
    return level1_chain(net, pl, ga.out, &view, nreg, lg.R, extended ? keep1 : nullptr, pl.arena + pl.l1.r_e[last ^ 1], pl.arena + pl.l1.r_e[last],
                        pl.arena + pl.l1.r_s, s);
}

// per forward: the level-1 slabs of the batch's samples (indices into sg.smp; ga0 = the stage-0 gather of the same batch, whose
// sources give a sub-box its level-0 features), then the gather of the two level-1 tile tensors from the regions and the slabs
static int level1_tiles(mi355_unet *net, const Plan &pl, const SwGeom &g, const S0Geom &sg, const L1Geom &lg, const S0GatherArgs &ga0,
                        const std::vector<int> &samples, hipStream_t s, S0View *e1_view = nullptr, S0View *s1_view = nullptr) {
    static const int unit[3] = {4, 8, 8};
    const bool views = env_switch("MI355_STAGE0_VIEWS");
    const int n = (int)samples.size();
    const int c0 = net->enc[0].back().cout, c1 = net->enc[1].back().cout, cS = net->dec[net->num_pool - 2][0].cout;
    MI355_REQUIRE(level1_slab_rows(n) <= S0_MAX_SAMPLES, "shared level 1: %d samples per forward", n);
    S0GatherArgs fin;
    memset(&fin, 0, sizeof(fin));
    for (int i = 0; i < n; ++i) {
        const L1Sample &ls = lg.smp[samples[i]];
        fin.smp[i].wv = ls.region;
        for (int k = 0; k < 3; ++k) fin.smp[i].org[k] = ls.org1[k];
        for (int f = 0; f < 6; ++f) fin.smp[i].slab[f] = -1;
    }
    for (int a = 0; a < 3; ++a) {
        fin.slab[a] = (const float *)(pl.arena + pl.l1.s_e[a]);
        fin.slab2[a] = (const float *)(pl.arena + pl.l1.s_s[a]);
        fin.t[a] = lg.merged[a] ? lg.t1[a] : ceil_div(2 * lg.dS, unit[a]) * unit[a];  // (a per-origin axis has no slab; the gather asks for a thickness all the same)
        if (!lg.merged[a]) continue;
        int Sb[3];
        for (int k = 0; k < 3; ++k) Sb[k] = k == a ? 2 * lg.t1[a] : g.P[k];
        // the sub-boxes' level-0 features, dense: the sources, slabs and precedence of the batch's stage-0 gather
        S0GatherArgs gs = ga0;
        gs.wv2 = nullptr; gs.out2 = nullptr; gs.r2 = 0; gs.C42 = 0;
        for (int k = 0; k < 3; ++k) { gs.slab2[k] = nullptr; gs.P[k] = Sb[k]; gs.T[k] = g.P[k]; }
        memset(gs.sub, 0, sizeof(gs.sub));
        int ns = 0;
        for (int i = 0; i < n; ++i)
            for (int side = 0; side < 2; ++side) {
                if (lg.smp[samples[i]].slab[2 * a + side] < 0) continue;
                const int off = side ? g.P[a] - Sb[a] : 0;
                S0Sample sb = ga0.smp[i];
                sb.org[a] += off;
                sb.slab[2 * a + (side ^ 1)] = -1;  // the cut: zero padding, no shell
                gs.smp[ns] = sb;
                gs.sub[ns][a] = off;
                fin.smp[i].slab[2 * a + side] = ns++;
            }
        if (!ns) continue;
        for (; ns % L1_SLAB_GROUP; ++ns) { gs.smp[ns] = gs.smp[ns - 1]; memcpy(gs.sub[ns], gs.sub[ns - 1], sizeof(gs.sub[0])); }  // (a whole last launch: its spare results are not read)
        gs.out = (float *)(pl.arena + pl.l1.sub_in[a]);
        const size_t sv0 = (size_t)Sb[0] * Sb[1] * Sb[2], sv1 = sv0 / 8;
        // where a launch of L1_SLAB_GROUP sub-boxes goes to the stride-2 kernel that takes a view, it reads enc[0]'s whole-volume
        // result in place and the gather writes the sub-boxes' shells alone (bit-identical: a view changes where bytes are read)
        bool viewed = false;
        if (views) {
            static float stand_in[2];
            const ConvCall c = make_call<float>(stand_in, c0, L1_SLAB_GROUP, Sb[0], Sb[1], Sb[2], stand_in, nullptr, ACT_LRELU, 0.01f);
            ConvPlan p;
            viewed = plan_conv_f32(net->enc[1][0].w, c, &p) == MI355_OK && p.family == FAM_S2DMA;
            S0View probe;
            viewed = viewed && stage0_view_make(gs.wv, (int)g.mirrors.size(), gs.Ve, gs.P, c0, gs.r, gs.smp, L1_SLAB_GROUP, &probe) == MI355_OK;
        }
        {
            double shell = 0.0;
            for (int i = 0; i < ns; ++i) shell += (double)stage0_shell_voxels(gs.P, gs.r, gs.smp[i].slab);
            ProfScope ps(net, s, "stage0_gather_kernel sub-boxes", 0.0, 2.0 * 4.0 * (viewed ? shell : (double)ns * sv0) * c0);
            if (viewed) MI355_TRY(stage0_gather_shells(gs, ns, 0, s));
            else MI355_TRY(stage0_gather(gs, ns, s));
        }
        for (int g0 = 0; g0 < ns; g0 += L1_SLAB_GROUP) {
            S0View view;
            if (viewed) MI355_TRY(stage0_view_make(gs.wv, (int)g.mirrors.size(), gs.Ve, gs.P, c0, gs.r, gs.smp + g0, L1_SLAB_GROUP, &view));
            MI355_TRY(level1_chain(net, pl, pl.arena + pl.l1.sub_in[a] + g0 * sv0 * c0 * 4, viewed ? &view : nullptr, L1_SLAB_GROUP, Sb, nullptr,
                                   pl.arena + pl.l1.s_tmp, pl.arena + pl.l1.s_e[a] + g0 * sv1 * c1 * 4, pl.arena + pl.l1.s_s[a] + g0 * sv1 * cS * 4, s));
        }
    }
    const int last = (int)((net->enc[1].size() - 1) & 1);
    fin.wv = (const float *)(pl.arena + pl.l1.r_e[last]);
    fin.wv2 = (const float *)(pl.arena + pl.l1.r_s);
    fin.out = (float *)(pl.arena + pl.off[last][1]);
    fin.out2 = (float *)(pl.arena + pl.off[last ^ 1][1]);
    for (int k = 0; k < 3; ++k) { fin.P[k] = g.P[k] / 2; fin.Ve[k] = lg.R[k] / 2; }
    stage0_gather_dense(&fin);
    fin.r = lg.d1; fin.C4 = c1 / 4; fin.r2 = lg.dS; fin.C42 = cS / 4;
    // the two readers take views where they can - enc[2][0] when the planner sends this forward's call to the stride-2 kernel that
    // has one, the addend epilogue always - and the gather then writes the shells alone
    const int nreg = (int)lg.regions.size();
    bool v0 = false, v1 = false;
    if (views && e1_view && s1_view && net->num_pool >= 2 && !net->enc[2].empty()) {
        const ConvLayer &L2 = net->enc[2][0];
        static float stand_in[2];
        const ConvCall c = make_call<float>(stand_in, c1, n, fin.P[0], fin.P[1], fin.P[2], stand_in, L2.runtime_norm ? (double *)stand_in : nullptr, ACT_LRELU, 0.01f);
        ConvPlan p;
        v0 = !L2.is_stem && L2.w.wp_dev && L2.stride == 2 && plan_conv_f32(L2.w, c, &p) == MI355_OK && p.family == FAM_S2DMA &&
             stage0_view_make(fin.wv, nreg, fin.Ve, fin.P, c1, fin.r, fin.smp, n, e1_view) == MI355_OK;
        v1 = stage0_view_make(fin.wv2, nreg, fin.Ve, fin.P, cS, fin.r2, fin.smp, n, s1_view) == MI355_OK;
    }
    const double pv = (double)n * fin.P[0] * fin.P[1] * fin.P[2];
    double shell0 = 0.0, shell1 = 0.0;
    for (int i = 0; i < n; ++i) { shell0 += (double)stage0_shell_voxels(fin.P, fin.r, fin.smp[i].slab); shell1 += (double)stage0_shell_voxels(fin.P, fin.r2, fin.smp[i].slab); }
    ProfScope ps(net, s, "stage0_gather_kernel level 1", 0.0, 2.0 * 4.0 * ((v0 ? shell0 : pv) * c1 + (v1 ? shell1 : pv) * cS));
    if (!v0 && !v1) return stage0_gather(fin, n, s);
    if (v0) MI355_TRY(stage0_gather_shells(fin, n, 0, s));
    else {
        S0GatherArgs f0 = fin;
        f0.out2 = nullptr; f0.wv2 = nullptr;
        MI355_TRY(stage0_gather(f0, n, s));
    }
    if (v1) return stage0_gather_shells(fin, n, 1, s);
    S0GatherArgs f1 = fin;  // the skip half whole, alone: as the first tensor of a gather
    f1.wv = fin.wv2; f1.out = fin.out2; f1.r = fin.r2; f1.C4 = fin.C42;
    for (int a = 0; a < 3; ++a) f1.slab[a] = fin.slab2[a];
    f1.out2 = nullptr; f1.wv2 = nullptr;
    return stage0_gather(f1, n, s);
}

static L1ShareNet level1_share_net_from_abi(const mi355_level1_share_net *nd) {
    L1ShareNet d;
    d.last = skip_share_net_from_abi(&nd->last);
    d.num_pool = nd->num_pool; d.k1 = nd->enc1_blocks; d.c1 = nd->c_level1;
    d.skip_is_enc1 = nd->skip_is_enc1 != 0; d.dec_blocks = nd->dec1_blocks; d.c_up = nd->c_up1; d.cout = nd->cout1;
    return d;
}

// Evaluates the tiles with (index % world) == rank of one net; adds into agg (and cnt if non-null,
// for ALL tiles so that every rank holds the full normaliser).
// `first_item`: index of this net's tile 0 in the caller's work list (fold f of a fold list: f * tiles): the work items
// (fold, tile) are dealt round-robin over the ranks as ONE list, so 5 folds x 8 tiles on 3 ranks still balance.
// tiles per forward (each with its nm mirrors): 16 samples (fp32) / 32 (fp16: half the bytes per sample; config 3 fp16 297 -> 293 ms
// per volume with 32, the deep levels' launches fill the chip better), 64 at the most - the arena is sized for 288 GB of HBM, not
// for a few GB.  One helper for sw_accumulate and the dry run mi355_stage0_view_plan, so that the two cannot drift.
static int sw_batch_tiles(int dtype, int batch_tiles, int nm) {
    int bt = batch_tiles > 0 ? batch_tiles : std::max(1, (dtype == MI355_F16 ? 32 : 16) / nm);
    if (bt * nm > 64) bt = std::max(1, 64 / nm);
    return bt;
}

static int sw_accumulate(mi355_unet *net, const SwVolume &v, const mi355_sw_opts &o, const SwGeom &g, int rank, int world, float *agg, float *cnt,
                         hipStream_t s, long first_item = 0) {
    const int nm = (int)g.mirrors.size();
    const bool use_gauss = o.use_gaussian && g.tiles.size() > 1;
    if (use_gauss) MI355_TRY(ensure_gaussian(net, g.P));
    std::vector<int> mine;
    for (size_t t = 0; t < g.tiles.size(); ++t) if ((int)((first_item + (long)t) % world) == rank) mine.push_back((int)t);
    int bt = sw_batch_tiles(net->dtype, o.batch_tiles, nm);
    MI355_REQUIRE(nm <= 64, "too many mirrors");
    // shared level 1: decided by the network and the geometry of all tiles alone; a forward then holds at most two slabs per sample
    // and axis in one gather, so a batch the caller asked to be larger than S0_MAX_SAMPLES / 2 samples is split (the default batch
    // of an fp32 net is 16; mi355_stage0_view_plan, asked for more samples than that, does not know of the cap)
    L1Geom lg;
    const bool share_l1 = level1_share_decide(level1_share_net(*net), g, level1_share_mode(), &lg);
    if (share_l1 && level1_slab_rows(bt * nm) > S0_MAX_SAMPLES) bt = std::max(1, S0_MAX_SAMPLES / 2 / nm);
    Plan pl;
    MI355_TRY(make_plan(*net, bt * nm, g.P[0], g.P[1], g.P[2], &pl));
    S0Geom sg;
    const bool share_skip = skip_share_decide(skip_share_net(*net), g);
    stage0_geometry(g, stage0_blocks(*net), &sg, share_skip ? 1 : 0);
    if (env_switch("MI355_MERGE_SLABS")) stage0_merge_geometry(g, &sg);
    if (sg.shared) stage0_plan(*net, g, sg, bt * nm, &pl);
    MI355_REQUIRE(!share_l1 || (sg.shared && share_skip), "shared level 1 without the shared stage 0 and the shared skip half");
    if (share_l1) level1_plan(*net, g, sg, lg, bt * nm, &pl);
    MI355_TRY(ensure_arena(&pl, s));
    if (mine.empty()) return MI355_OK;
    if (sg.shared) MI355_TRY(stage0_whole(net, pl, v, g, sg, s));
    if (sg.merge) MI355_TRY(stage0_merged(net, pl, v, g, sg, s));
    if (share_l1) MI355_TRY(level1_regions(net, pl, v, g, sg, lg, s));
    for (size_t b0 = 0; b0 < mine.size(); b0 += bt) {
        const int nb = (int)std::min<size_t>(bt, mine.size() - b0);
        std::vector<TileDesc> samples;
        std::vector<int> sample_ids;  // (tile, mirror) as indexed by S0Geom::smp
        for (int i = 0; i < nb; ++i)
            for (int m = 0; m < nm; ++m) {
                TileDesc td = g.tiles[mine[b0 + i]];
                td.mirror = g.mirrors[m];
                samples.push_back(td);
                sample_ids.push_back(mine[b0 + i] * nm + m);
            }
        S0View enc0_view, half_view, enc1_view, half1_view;
        if (sg.shared) {
            const S0ViewChoice want = stage0_views_decide(*net, sg, share_skip, (int)samples.size(), g.P);
            S0GatherArgs ga0;
            MI355_TRY(stage0_tiles(net, pl, v, g, sg, sample_ids, s, want, &enc0_view, &half_view, share_l1 ? &ga0 : nullptr));
            if (share_l1) MI355_TRY(level1_tiles(net, pl, g, sg, lg, ga0, sample_ids, s, &enc1_view, &half1_view));
        } else {
        const double pv = (double)samples.size() * g.P[0] * g.P[1] * g.P[2];
        ProfScope ps(net, s, "extract_tiles_kernel", 0.0, pv * (4.0 * net->in_channels + (net->dtype == MI355_F16 ? 2.0 : 4.0) * net->cin_pad));
        MI355_TRY(extract_tiles(v.vol, net->in_channels, v.Z, v.Y, v.X, g.pad_lo[0], g.pad_lo[1], g.pad_lo[2], samples.data(),
                                (int)samples.size(), g.P[0], g.P[1], g.P[2], net->cin_pad,
                                (void *)(pl.arena + pl.x0_off), net->dtype, s));
        }
        const void *feat; int fc; bool is_logits = false;
        FeatNorm head_norm;
        ForwardOpts fo;
        fo.is_logits = &is_logits; fo.head_norm = &head_norm; fo.after_enc0 = sg.shared;
        if (share_skip) fo.skip_half = (const float *)(pl.arena + pl.off[((net->enc[0].size() - 1) & 1) ^ 1][0]);
        if (enc0_view.src) fo.enc0_view = &enc0_view;
        if (half_view.src) fo.skip_half_view = &half_view;
        if (share_l1) {
            fo.after_enc1 = true;
            fo.skip_half1 = (const float *)(pl.arena + pl.off[((net->enc[1].size() - 1) & 1) ^ 1][1]);
            if (enc1_view.src) fo.enc1_view = &enc1_view;
            if (half1_view.src) fo.skip_half1_view = &half1_view;
        }
        MI355_TRY(forward_features(net, pl, (int)samples.size(), g.P[0], g.P[1], g.P[2], &feat, &fc, s, fo));
        MI355_REQUIRE(is_logits || fc == net->head.cin, "head expects %d channels, decoder gives %d", net->head.cin, fc);
        if (is_logits) {  // the forward's tiles in one launch: agg / cnt are read and written once per voxel, not once per tile
            std::vector<int> origins;
            int lo[3], hi[3];
            for (int i = 0; i < nb; ++i) {
                const TileDesc &td = g.tiles[mine[b0 + i]];
                const int org[3] = {td.z0, td.y0, td.x0};
                for (int a = 0; a < 3; ++a) {
                    origins.push_back(org[a]);
                    lo[a] = i ? std::min(lo[a], org[a]) : org[a];
                    hi[a] = i ? std::max(hi[a], org[a] + g.P[a]) : org[a] + g.P[a];
                }
            }
            const double pv = (double)g.P[0] * g.P[1] * g.P[2], box = (double)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
            ProfScope ps(net, s, "logits_aggregate_tiles_kernel", 0.0, 4.0 * (nb * pv * (nm * net->num_classes + 1.0) + box * (2.0 * net->num_classes + 2.0)));
            MI355_TRY(logits_aggregate_tiles((const float *)feat, net->num_classes, 0, g.mirrors.data(), nm, g.P[0], g.P[1], g.P[2], o.nonlin,
                                             use_gauss ? net->gauss_dev : nullptr, agg, (cnt && world == 1) ? cnt : nullptr, g.Zp[0], g.Zp[1],
                                             g.Zp[2], origins.data(), nb, s));
            continue;
        }
        for (int i = 0; i < nb; ++i) {
            const TileDesc &td = g.tiles[mine[b0 + i]];
            const double pv = (double)g.P[0] * g.P[1] * g.P[2];
            ProfScope ps(net, s, "head_aggregate_kernel", 2.0 * pv * nm * fc * net->num_classes,
                         pv * ((net->dtype == MI355_F16 ? 2.0 : 4.0) * nm * fc + 4.0 * (2.0 * net->num_classes + 3.0)));
            MI355_TRY(head_aggregate(net->head, feat, net->dtype, i * nm, g.mirrors.data(), nm, g.P[0], g.P[1], g.P[2], o.nonlin,
                                     use_gauss ? net->gauss_dev : nullptr, agg, (cnt && world == 1) ? cnt : nullptr,
                                     g.Zp[0], g.Zp[1], g.Zp[2], td.z0, td.y0, td.x0, s, head_norm));
        }
    }
    return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_compute_steps(int patch, int image, float step_size, int32_t *steps, int max_steps) {
    MI355_REQUIRE(patch > 0 && image >= patch && step_size > 0.f && step_size <= 1.f, "compute_steps: bad arguments");
    std::vector<int> st = compute_steps(patch, image, step_size);
    MI355_REQUIRE((int)st.size() <= max_steps, "compute_steps: %zu steps > buffer %d", st.size(), max_steps);
    for (size_t i = 0; i < st.size(); ++i) steps[i] = st[i];
    return (int)st.size();
}

// Partitioning B of SURVEY.md 8e with the reference's fold list (run_brats2021_inference_singlethread.py:161 folds=(0..4),
// :112-128): the work list is (fold, tile), item f * tiles + t, dealt round-robin over the ranks; agg_dev receives
// sum over this rank's items of the Gaussian-weighted, mirror-averaged probabilities - the fold mean is linear in the
// per-fold aggregates (mean_f(agg_f / cnt) = (sum_f agg_f) / cnt / n_folds), so ONE exchange per ensemble member suffices.
extern "C" int mi355_sw_partial_folds(const mi355_unet_t *nets, int n_nets, const float *vol_dev, int Z, int Y, int X,
                                      const mi355_sw_opts *opts, int rank, int world, float *agg_dev, float *cnt_dev, void *stream) {
    MI355_REQUIRE(nets && n_nets >= 1 && vol_dev && opts && agg_dev && world >= 1 && rank >= 0 && rank < world, "bad argument");
    for (int f = 0; f < n_nets; ++f) {
        MI355_REQUIRE(nets[f] != nullptr, "fold %d: null handle", f);
        MI355_REQUIRE(nets[f]->num_classes == nets[0]->num_classes, "fold %d has %d classes, fold 0 has %d", f, nets[f]->num_classes, nets[0]->num_classes);
    }
    MI355_TRY(bind_device());
    hipStream_t s = (hipStream_t)stream;
    SwGeom g;
    MI355_TRY(make_geom(*opts, Z, Y, X, &g));
    const size_t ZYXp = (size_t)g.Zp[0] * g.Zp[1] * g.Zp[2];
    MI355_HIP(hipMemsetAsync(agg_dev, 0, ZYXp * nets[0]->num_classes * sizeof(float), s));
    if (cnt_dev) MI355_HIP(hipMemsetAsync(cnt_dev, 0, ZYXp * sizeof(float), s));
    if (cnt_dev && world > 1) {
        // full normaliser of ONE fold on every rank: cnt[tile] += gaussian for ALL tiles, in tile order (no exchange needed)
        const bool use_gauss = opts->use_gaussian && g.tiles.size() > 1;
        if (use_gauss) MI355_TRY(ensure_gaussian(nets[0], g.P));
        for (const TileDesc &td : g.tiles)
            MI355_TRY(cnt_add_tile(use_gauss ? nets[0]->gauss_dev : nullptr, g.P[0], g.P[1], g.P[2], cnt_dev, g.Zp[1], g.Zp[2],
                                   td.z0, td.y0, td.x0, s));
    }
    // (world == 1: the first fold's aggregation kernels add the normaliser themselves, exactly as mi355_sw_predict does)
    for (int f = 0; f < n_nets; ++f)
        MI355_TRY(sw_accumulate(nets[f], SwVolume{vol_dev, Z, Y, X}, *opts, g, rank, world, agg_dev, f == 0 ? cnt_dev : nullptr, s,
                                (long)f * (long)g.tiles.size()));
    return MI355_OK;
}

extern "C" int mi355_sw_partial(mi355_unet_t net, const float *vol_dev, int Z, int Y, int X, const mi355_sw_opts *opts,
                                int rank, int world, float *agg_dev, float *cnt_dev, void *stream) {
    return mi355_sw_partial_folds(&net, 1, vol_dev, Z, Y, X, opts, rank, world, agg_dev, cnt_dev, stream);
}

extern "C" int mi355_sw_finish_folds(const float *agg_dev, const float *cnt_dev, int num_classes, int Z, int Y, int X,
                                     const int32_t patch[3], int n_folds, float *probs_dev, void *stream) {
    MI355_REQUIRE(agg_dev && cnt_dev && probs_dev && patch && n_folds >= 1, "bad argument");
    MI355_TRY(bind_device());
    const int Zp = std::max(Z, patch[0]), Yp = std::max(Y, patch[1]), Xp = std::max(X, patch[2]);
    MI355_TRY(finish_probs(agg_dev, cnt_dev, num_classes, Z, Y, X, Zp, Yp, Xp, (Zp - Z) / 2, (Yp - Y) / 2, (Xp - X) / 2,
                           probs_dev, 0, (hipStream_t)stream));
    if (n_folds > 1) MI355_TRY(scale_inplace(probs_dev, (int64_t)num_classes * Z * Y * X, (float)n_folds, (hipStream_t)stream));
    return MI355_OK;
}

extern "C" int mi355_sw_finish(const float *agg_dev, const float *cnt_dev, int num_classes, int Z, int Y, int X,
                               const int32_t patch[3], float *probs_dev, void *stream) {
    return mi355_sw_finish_folds(agg_dev, cnt_dev, num_classes, Z, Y, X, patch, 1, probs_dev, stream);
}

extern "C" int mi355_sw_predict(const mi355_unet_t *nets, int n_nets, const float *vol_dev, int Z, int Y, int X,
                                const mi355_sw_opts *opts, float *probs_dev, void *stream) {
    MI355_REQUIRE(nets && n_nets >= 1 && vol_dev && opts && probs_dev, "bad argument");
    MI355_TRY(bind_device());
    hipStream_t s = (hipStream_t)stream;
    SwGeom g;
    MI355_TRY(make_geom(*opts, Z, Y, X, &g));
    const int C = nets[0]->num_classes;
    const size_t ZYXp = (size_t)g.Zp[0] * g.Zp[1] * g.Zp[2];
    // aggregation scratch: process-wide like the activation arena, grown on demand, never freed per call - a
    // hipMalloc / synchronise / hipFree round trip per volume costs more than the small kernels of a step
    void *scratch = nullptr;
    MI355_TRY(device_scratch(SCR_SW_AGG, s, ZYXp * (size_t)(C + 1) * sizeof(float), &scratch));
    float *agg = (float *)scratch, *cnt = agg + ZYXp * C;
    int rc = MI355_OK;
    for (int f = 0; f < n_nets && rc == MI355_OK; ++f) {
        if (nets[f]->num_classes != C) { set_error("fold %d has %d classes, fold 0 has %d", f, nets[f]->num_classes, C); rc = MI355_ERR_INVALID; break; }
        if (hipMemsetAsync(agg, 0, ZYXp * C * sizeof(float), s) != hipSuccess ||
            hipMemsetAsync(cnt, 0, ZYXp * sizeof(float), s) != hipSuccess) { set_error("memset failed"); rc = MI355_ERR_HIP; break; }
        rc = sw_accumulate(nets[f], SwVolume{vol_dev, Z, Y, X}, *opts, g, 0, 1, agg, cnt, s);
        if (rc == MI355_OK)
            rc = finish_probs(agg, cnt, C, Z, Y, X, g.Zp[0], g.Zp[1], g.Zp[2], g.pad_lo[0], g.pad_lo[1], g.pad_lo[2],
                              probs_dev, f > 0, s);
    }
    // fold mean: np.mean(list_of_fp32_arrays, axis=0) = fp32 running sum in list order, one divide
    if (rc == MI355_OK && n_nets > 1) rc = scale_inplace(probs_dev, (int64_t)C * Z * Y * X, (float)n_nets, s);
    // asynchronous on `stream` like every other entry point that takes one: probs_dev is valid in stream order
    return rc;
}

extern "C" int mi355_stage0_plan(int z, int y, int x, const int32_t patch[3], float step_size, int mirror_axes, int r,
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
            int S[3];
            slab_dims(g, sg, f >> 1, S);
            for (int a = 0; a < 3; ++a) { d.slab_origin[f][a] = sm.org[a]; d.slab_shape[f][a] = S[a]; }
            if (f & 1) d.slab_origin[f][f >> 1] += g.P[f >> 1] - sg.t[f >> 1];
        }
    }
    return n;
}

extern "C" int mi355_stage0_merge_plan(int z, int y, int x, const int32_t patch[3], float step_size, int mirror_axes, int r, int skip_half,
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

extern "C" int mi355_skip_share_plan(int z, int y, int x, const int32_t patch[3], float step_size, int mirror_axes,
                                     const mi355_skip_share_net *nd, int batch_tiles, int rank, int world, mi355_skip_share_geom *out) {
    MI355_REQUIRE(out && patch && nd && batch_tiles >= 0 && world >= 1 && rank >= 0 && rank < world, "mi355_skip_share_plan: bad argument");
    SwGeom g;
    MI355_TRY(sw_geom_from_abi(z, y, x, patch, step_size, mirror_axes, &g));
    const SkipShareNet d = skip_share_net_from_abi(nd);
    // (rank, world, batch_tiles: taken so that a caller can see that nothing below reads them - the invariant of the shared stage 0)
    (void)batch_tiles; (void)rank; (void)world;
    const bool on = skip_share_decide(d, g);
    S0Geom sg;
    stage0_geometry(g, d.r, &sg, on ? 1 : 0);
    memset(out, 0, sizeof(*out));
    out->stage0_shared = sg.shared; out->skip_shared = on;
    out->r = sg.r; out->skip_shell = on ? sg.rs : 0;
    out->n_tiles = (int32_t)g.tiles.size(); out->n_mirrors = (int32_t)g.mirrors.size();
    for (int a = 0; a < 3; ++a) { out->volume[a] = sg.Ve[a]; out->slab_thickness[a] = sg.t[a]; }
    return MI355_OK;
}

// ---- stage-0 views: dry run and single-op entries
extern "C" int mi355_stage0_view_plan(int z, int y, int x, const int32_t patch[3], float step_size, int mirror_axes,
                                      const mi355_skip_share_net *nd, int c_level1, int batch_samples, mi355_stage0_view_geom *out,
                                      mi355_stage0_view_sample *samples, int max_samples) {
    MI355_REQUIRE(out && patch && nd && c_level1 > 0 && batch_samples >= 0 && (samples || max_samples == 0), "mi355_stage0_view_plan: bad argument");
    SwGeom g;
    MI355_TRY(sw_geom_from_abi(z, y, x, patch, step_size, mirror_axes, &g));
    const SkipShareNet d = skip_share_net_from_abi(nd);
    const bool on = skip_share_decide(d, g);
    S0Geom sg;
    stage0_geometry(g, d.r, &sg, on ? 1 : 0);
    // the first block of level 1 as the network would hold it: c_skip -> c_level1, stride 2
    ConvPackLayout l;
    ConvWeights cw;
    const bool have_w1 = nd->dtype == MI355_F32 && conv_pack_layout(nd->c_skip, nd->c_skip, c_level1, 2, &l) == MI355_OK && l.mfma;
    if (have_w1) cw = stand_in_conv_weights(l, nd->c_skip, c_level1, 2);  // (a stride-2 layout has the MFMA pack alone)
    const int nm = (int)g.mirrors.size();
    // a full batch of one rank; a short last batch, or the tiles one rank of several gets, is asked for with batch_samples
    const int per_forward = batch_samples > 0 ? batch_samples : sw_batch_tiles(nd->dtype, 0, nm) * nm;
    const S0ViewChoice v = stage0_views_choose(sg, on, std::min(per_forward, (int)g.tiles.size() * nm), g.P, have_w1 ? &cw : nullptr, nd->c_skip, d.runtime_norm);
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

// ---- shared level 1: dry run
extern "C" int mi355_level1_share_plan(int z, int y, int x, const int32_t patch[3], float step_size, int mirror_axes,
                                       const mi355_level1_share_net *nd, int mode, mi355_level1_share_geom *out,
                                       mi355_level1_share_region *regions, int max_regions, mi355_level1_share_sample *samples, int max_samples) {
    MI355_REQUIRE(out && patch && nd && mode >= 0 && mode <= 2 && (regions || max_regions == 0) && (samples || max_samples == 0),
                  "mi355_level1_share_plan: bad argument");
    SwGeom g;
    MI355_TRY(sw_geom_from_abi(z, y, x, patch, step_size, mirror_axes, &g));
    const L1ShareNet d = level1_share_net_from_abi(nd);
    L1Geom lg;
    const bool on = level1_share_decide(d, g, mode, &lg);
    S0Geom sg;
    stage0_geometry(g, d.last.r, &sg, skip_share_decide(d.last, g) ? 1 : 0);
    memset(out, 0, sizeof(*out));
    out->possible = lg.possible; out->on = on;
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
        for (int f = 0; f < 6; ++f) q.faces |= lg.regions[i].face[f] >= 0 ? 1 << f : 0;
    }
    const int n = (int)lg.smp.size();
    for (int i = 0; i < n; ++i) {
        const L1Sample &ls = lg.smp[i];
        const S0Sample &sm = sg.smp[i];
        mi355_level1_share_sample q;
        memset(&q, 0, sizeof(q));
        q.tile = i / (int)g.mirrors.size(); q.mirror = g.mirrors[sm.wv]; q.region = ls.region;
        for (int a = 0; a < 3; ++a) { q.origin[a] = sm.org[a]; q.origin1[a] = ls.org1[a]; }
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
