// The sliding-window predictor, device side: the Gaussian map on the device, the arena appendices and the passes of what a window's
// plan (sw_share_plan.hip: SwSharePlan, decided once per window) says overlapping tiles share - the shared stage 0, its slabs and merged
// slabs, the shared skip half, stage-0 views, the shared level 1 -, sw_accumulate and the mi355_sw_* entry points of include/mi355_nnunet.h.
#include <cstring>
#include <mutex>

#include "unet_internal.h"

namespace mi355 {

static std::mutex g_gauss_mu;
static int ensure_gaussian(mi355_unet *net, const int p[3]) {
    std::lock_guard<std::mutex> lk(g_gauss_mu);  // (one handle may be driven from two lanes)
    if (net->gauss_dev && net->gauss_p[0] == p[0] && net->gauss_p[1] == p[1] && net->gauss_p[2] == p[2])
        return MI355_OK;
    if (net->gauss_dev) { MI355_HIP(hipDeviceSynchronize()); net->gauss_mem.release(); net->gauss_dev = nullptr; }
    std::vector<float> g;
    gaussian_map(p, 1.0 / 8.0, g);
    const int rc = net->gauss_mem.upload(g.data(), g.size() * sizeof(float), &net->gauss_dev);
    if (rc != MI355_OK) { net->gauss_mem.release(); net->gauss_dev = nullptr; return rc; }  // (nothing has been launched on it)
    net->gauss_p[0] = p[0]; net->gauss_p[1] = p[1]; net->gauss_p[2] = p[2];
    return MI355_OK;
}

// ---- shared stage 0 (sw_share_plan.hip "shared stage 0")
// appends the stage-0 regions to the plan of `n_samples` (tile, mirror) samples per forward
static void stage0_plan(const mi355_unet &net, const SwGeom &g, const S0Geom &sg, int n_samples, Plan *pl) {
    ArenaCursor c{pl->total};
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
    pl->s0.wv_in = c.take(wv * net.cin_pad * 4);
    pl->s0.slab_in = c.take(sl * net.cin_pad * 4);
    for (int k = 0; k < 2 && k < sg.r - 1; ++k) {
        pl->s0.wv_tmp[k] = c.take(wv * maxc * 4);
        pl->s0.slab_tmp[k] = c.take(sl * maxc * 4);
    }
    pl->s0.wv_out = c.take(wv * net.enc[0].back().cout * 4);
    for (int a = 0; a < 3; ++a) pl->s0.slab_out[a] = c.take(sl_a[a] * net.enc[0].back().cout * 4);
    if (sg.rs > sg.r) {  // shared skip half: S for the whole volume per mirror and for the slabs (its tile tensor lives in the level-0 buffer the last decoder stage leaves free)
        pl->s0.wv_skip = c.take(wv * net.dec.back()[0].cout * 4);
        for (int a = 0; a < 3; ++a) pl->s0.slab_skip[a] = c.take(sl_a[a] * net.dec.back()[0].cout * 4);
    }
    pl->total = c.o;
}

// a box of the (mirrored) pass, origin b and size S, as the TileDesc extract_tiles takes: origin in the unflipped padded volume
static TileDesc pass_box(const SwGeom &g, int mirror, const int b[3], const int S[3]) {
    int o[3];
    for (int a = 0; a < 3; ++a) o[a] = (mirror >> a) & 1 ? g.Zp[a] - b[a] - S[a] : b[a];
    return TileDesc{o[0], o[1], o[2], mirror};
}
// one slab box of S voxels per face of axis a that needs one (smp[i].slab[f] >= 0, which receives the box's row) of n boxes of `extent`
static std::vector<TileDesc> face_slab_boxes(const SwGeom &g, S0Sample *smp, int n, int a, const int extent[3], const int thick[3], const int S[3]) {
    std::vector<TileDesc> boxes;
    for (int i = 0; i < n; ++i)
        for (int f = 2 * a; f < 2 * a + 2; ++f) {
            if (smp[i].slab[f] < 0) continue;
            int b[3];
            face_slab_origin(smp[i].org, extent, thick, f, b);
            smp[i].slab[f] = (int)boxes.size();
            boxes.push_back(pass_box(g, g.mirrors[smp[i].wv], b, S));
        }
    return boxes;
}

// zero what lies outside `keep` of n boxes of S voxels each (nothing to do where keep == S)
static int mask_outside(mi355_unet *net, void *x, int n, const int S[3], const int keep[3], int C, hipStream_t s) {
    if (keep[0] == S[0] && keep[1] == S[1] && keep[2] == S[2]) return MI355_OK;
    ProfScope ps(net, s, "stage0_mask_kernel", 0.0, (double)n * ((double)S[0] * S[1] * S[2] - (double)keep[0] * keep[1] * keep[2]) * C * 4.0);
    return stage0_mask((float *)x, n, S, keep, C, s);
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
            // the next conv must see zero padding outside the padded volume, not act(bias)
            if ((!last || at.skip_off) && at.mask_zp) MI355_TRY(mask_outside(net, out, ng, S, at.mask_zp, L.cout, s));
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
    S0Placement at;
    at.S = sg.Ve; at.mask_zp = g.Zp;
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
        S0Placement at;
        at.S = sg.mdim[a]; at.mask_zp = keep; at.label = " merged-slabs";
        at.in_off = pl.s0.slab_in; at.tmp_off = pl.s0.slab_tmp; at.out_off = pl.s0.slab_out[a]; at.skip_off = pl.s0.slab_skip[a];
        MI355_TRY(stage0_run(net, pl, v, g, boxes, at, s));
    }
    return MI355_OK;
}

// which readers of one forward's level-l tile tensors take a view (sw_share_plan.hip "stage-0 views"; may depend on the batch): the
// addend epilogue always, the first block of level l + 1 when the planner sends this forward's call to the stride-2 kernel that has one
static S0ViewChoice views_decide(const mi355_unet &net, int l, bool views, const SwSharePlan &p, int n_samples, const int P[3]) {
    if (net.dtype != MI355_F32 || net.num_pool < l + 1 || net.enc[l + 1].empty()) return S0ViewChoice();
    const ConvLayer &L = net.enc[l + 1][0];
    return stage0_views_choose(views, p.sg, p.share_skip, n_samples, P, L.is_stem ? nullptr : &L.w, net.enc[l].back().cout, L.runtime_norm);
}

// ---- the hand-off of one level to the forward: the features of n samples (C channels) and the skip half of the decoder conv that reads
// them (C2 channels, 0 = none), gathered from the n_wv shared tensors and the slabs `ga` names.  A tensor whose reader takes a view (want)
// is gathered in its shells alone and *out receives the view (src = null: none, the tensor is dense; so too where no view can be built).
// sw: how it is launched - a dense gather of sub-boxes runs over the boxes (subbox_gather).
struct LevelHandOff { S0View feat_view, half_view; };
static int handoff_gather(mi355_unet *net, const S0GatherArgs &ga, int n, int n_wv, int C, int C2, S0ViewChoice want, const SwSwitches &sw, const char *label,
                          LevelHandOff *out, hipStream_t s) {
    const bool v0 = want.enc0 && stage0_view_make(ga.wv, n_wv, ga.Ve, ga.P, C, ga.r, ga.smp, n, &out->feat_view) == MI355_OK;
    const bool v1 = want.half && C2 && stage0_view_make(ga.wv2, n_wv, ga.Ve, ga.P, C2, ga.r2, ga.smp, n, &out->half_view) == MI355_OK;
    const double pv = (double)n * ga.P[0] * ga.P[1] * ga.P[2];
    double shell0 = 0.0, shell1 = 0.0;
    for (int i = 0; i < n; ++i) {
        shell0 += (double)stage0_shell_voxels(ga.P, ga.r, ga.smp[i].slab);
        if (C2) shell1 += (double)stage0_shell_voxels(ga.P, ga.r2, ga.smp[i].slab);
    }
    // (one profile entry, as before the views; its bytes are what is moved: read + written)
    ProfScope ps(net, s, label, 0.0, 2.0 * 4.0 * ((v0 ? shell0 : pv) * C + (v1 ? shell1 : pv) * C2));
    const bool by_box = sw.subbox_gather && ga.T[0] > 0;
    if (!v0 && !v1) return stage0_gather(ga, n, s, by_box);
    if (v0) MI355_TRY(stage0_gather_shells(ga, n, 0, s));
    else {  // the features whole, alone
        S0GatherArgs g0 = ga;
        g0.out2 = nullptr; g0.wv2 = nullptr;
        MI355_TRY(stage0_gather(g0, n, s, by_box));
    }
    if (!C2) return MI355_OK;
    if (v1) return stage0_gather_shells(ga, n, 1, s);
    S0GatherArgs g1 = ga;  // the skip half whole, alone: as the first tensor of a gather
    g1.wv = ga.wv2; g1.out = ga.out2; g1.r = ga.r2; g1.C4 = ga.C42;
    for (int a = 0; a < 3; ++a) g1.slab[a] = ga.slab2[a];
    g1.out2 = nullptr; g1.wv2 = nullptr;
    return stage0_gather(g1, n, s, by_box);
}

// the slabs of one batch of samples (indices into sg.smp), then the hand-off of the batch's tile tensors.  want: which tensors'
// readers will take a view.  out->ga: the gather's arguments (shared level 1: the sources of the batch's sub-boxes).
struct S0TilesOut { LevelHandOff h; S0GatherArgs ga; };
static int stage0_tiles(mi355_unet *net, const Plan &pl, const SwVolume &v, const SwGeom &g, const S0Geom &sg, const std::vector<int> &samples,
                        S0ViewChoice want, const SwSwitches &sw, S0TilesOut *out, hipStream_t s) {
    const int n = (int)samples.size();
    MI355_REQUIRE(n <= S0_MAX_SAMPLES, "shared stage 0: %d samples per forward (max %d)", n, S0_MAX_SAMPLES);
    const int C = net->enc[0].back().cout;
    S0GatherArgs &ga = out->ga;
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
        std::vector<TileDesc> boxes = face_slab_boxes(g, ga.smp, n, a, g.P, sg.t, S);
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
    return handoff_gather(net, ga, n, (int)g.mirrors.size(), C, C2, want, sw, "stage0_gather_kernel", &out->h, s);
}

// ---- shared level 1 (sw_share_plan.hip "shared level 1"): the region pass and the per-forward slabs
// appends the level-1 regions to the plan of `n_samples` samples per forward
static void level1_plan(const mi355_unet &net, const SwGeom &g, const S0Geom &sg, const L1Geom &lg, int n_samples, Plan *pl) {
    ArenaCursor c{pl->total};
    int maxc0 = 0;
    for (auto &L : net.enc[0]) maxc0 = std::max(maxc0, L.cout);
    const size_t c0 = net.enc[0].back().cout, c1 = net.enc[1].back().cout, cS = net.dec[net.num_pool - 2][0].cout;
    size_t rs_a[3] = {0, 0, 0}, rs_max = 0;
    for (int a = 0; a < 3; ++a) {
        size_t box = sg.t[a];
        for (int k = 0; k < 3; ++k) if (k != a) box *= lg.R[k];
        for (const S0Sample &rg : lg.regions) rs_a[a] += ((rg.slab[2 * a] >= 0) + (rg.slab[2 * a + 1] >= 0)) * box;
        rs_max = std::max(rs_max, rs_a[a]);
    }
    if (rs_max) {
        pl->l1.rs_in = c.take(rs_max * net.cin_pad * 4);
        for (int k = 0; k < 2 && k < sg.r - 1; ++k) pl->l1.rs_tmp[k] = c.take(rs_max * maxc0 * 4);
        for (int a = 0; a < 3; ++a) pl->l1.rs_out[a] = c.take(rs_a[a] * c0 * 4);
    }
    const size_t rv0 = lg.regions.size() * (size_t)lg.R[0] * lg.R[1] * lg.R[2], rv1 = rv0 / 8;
    pl->l1.r_shell = c.take(rv0 * c0 * 4);
    for (int k = 0; k < 2; ++k) pl->l1.r_e[k] = c.take(rv1 * c1 * 4);
    pl->l1.r_s = c.take(rv1 * cS * 4);
    size_t tmp = 0;
    for (int a = 0; a < 3; ++a) {
        if (!lg.merged[a]) continue;
        size_t sv0 = (size_t)level1_slab_rows(n_samples) * 2 * lg.t1[a];
        for (int k = 0; k < 3; ++k) if (k != a) sv0 *= g.P[k];
        pl->l1.sub_in[a] = c.take(sv0 * c0 * 4);
        pl->l1.s_e[a] = c.take(sv0 / 8 * c1 * 4);
        pl->l1.s_s[a] = c.take(sv0 / 8 * cS * 4);
        tmp = std::max(tmp, sv0 / 8 * c1 * 4);
    }
    pl->l1.s_tmp = c.take(tmp);
    pl->total = c.o;
}

// enc[1] (its first block through in0_view when given) and the skip half of dec[np - 2][0] over n boxes of S level-0 voxels:
// x0 -> e_out (through tmp, and e_out itself, in turns) and s_out; keep1: zeros restored outside it behind every block;
// least_padding: the stride-2 block plans with ConvCall::s2_least_padding (whoever asked the planner about a view asked with it too)
static int level1_chain(mi355_unet *net, const Plan &pl, const void *x0, const S0View *view, bool least_padding, int n, const int S[3], const int *keep1,
                        void *tmp, void *e_out, void *s_out, hipStream_t s) {
    const std::vector<ConvLayer> &e1 = net->enc[1];
    const int S1[3] = {S[0] / 2, S[1] / 2, S[2] / 2};
    const void *cur = x0;
    int curC = net->enc[0].back().cout;
    for (size_t i = 0; i < e1.size(); ++i) {
        void *out = ((e1.size() - 1 - i) & 1) ? tmp : e_out;  // (the last block writes e_out)
        BlockOpts bo;
        if (i == 0) { bo.in0_view = view; bo.s2_least_padding = least_padding; }
        MI355_TRY(run_block(net, pl, e1[i], cur, curC, nullptr, 0, n, i ? S1[0] : S[0], i ? S1[1] : S[1], i ? S1[2] : S[2], out, s, bo));
        if (keep1) MI355_TRY(mask_outside(net, out, n, S1, keep1, e1[i].cout, s));
        cur = out; curC = e1[i].cout;
    }
    const ConvLayer &Ld = net->dec[net->num_pool - 2][0];
    BlockOpts bo;
    bo.half = &Ld.w_skip; bo.half_name = " skip-half";
    return run_block(net, pl, Ld, cur, curC, nullptr, 0, n, S1[0], S1[1], S1[2], s_out, s, bo);
}

// region pass, once per volume behind the whole-volume pass: the stage-0 slabs at the regions' faces on per-origin axes, the
// regions' level-0 shells, then enc[1] and the skip half over the regions, their level-0 input read in place through a view
static int level1_regions(mi355_unet *net, const Plan &pl, const SwVolume &v, const SwGeom &g, const S0Geom &sg, const L1Geom &lg, const SwSwitches &sw,
                          hipStream_t s) {
    const int nreg = (int)lg.regions.size();
    const int c0 = net->enc[0].back().cout;
    MI355_REQUIRE(nreg > 0 && nreg <= S0_VIEW_MAX_SAMPLES, "shared level 1: %d regions (max %d)", nreg, S0_VIEW_MAX_SAMPLES);
    S0GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    for (int i = 0; i < nreg; ++i) ga.smp[i] = lg.regions[i];
    bool any = false;
    for (int a = 0; a < 3; ++a) {
        int S[3], keep[3];
        for (int k = 0; k < 3; ++k) { S[k] = k == a ? sg.t[k] : lg.R[k]; keep[k] = lg.merged[k] ? g.Zp[k] : S[k]; }
        const std::vector<TileDesc> boxes = face_slab_boxes(g, ga.smp, nreg, a, lg.R, sg.t, S);
        ga.slab[a] = (const float *)(pl.arena + pl.l1.rs_out[a]);
        if (boxes.empty()) continue;
        any = true;
        S0Placement at;
        at.S = S; at.mask_zp = keep; at.label = " region-slabs";
        at.in_off = pl.l1.rs_in; at.tmp_off = pl.l1.rs_tmp; at.out_off = pl.l1.rs_out[a];
        MI355_TRY(stage0_run(net, pl, v, g, boxes, at, s));
        // (stage0_run leaves its last layer unmasked when no skip half follows; the regions read it)
        MI355_TRY(mask_outside(net, pl.arena + pl.l1.rs_out[a], (int)boxes.size(), S, keep, c0, s));
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
    int keep1[3];
    for (int k = 0; k < 3; ++k) keep1[k] = lg.merged[k] ? g.Zp[k] / 2 : lg.R[k] / 2;
    const int last = (int)((net->enc[1].size() - 1) & 1);
    return level1_chain(net, pl, ga.out, &view, sw.s2_least_padding, nreg, lg.R, keep1, pl.arena + pl.l1.r_e[last ^ 1], pl.arena + pl.l1.r_e[last],
                        pl.arena + pl.l1.r_s, s);
}

// The level-1 slabs of one batch on merged axis a, step 1: the sub-boxes they are cut from (2 t1 level-0 layers at each tile face
// inside the region) and their level-0 features, from the sources, slabs and precedence of the batch's stage-0 gather ga0.
// fin->smp[i].slab (0 where face f of sample i has a level-1 slab) receives the row of that slab.  Out: gs, the gather of the sub-boxes
// (gs.smp[0 .. *n_out), a multiple of L1_SLAB_GROUP; gs.P their extent); *viewed: the chain's first conv reads enc[0]'s whole-volume
// result through a view, gs.out holds the shells alone.
static int level1_sub_boxes(mi355_unet *net, const Plan &pl, const SwGeom &g, const L1Geom &lg, const S0GatherArgs &ga0, int n, int a, const SwSwitches &sw,
                            S0GatherArgs *fin, S0GatherArgs &gs, int *n_out, bool *viewed, hipStream_t s) {
    const int c0 = net->enc[0].back().cout;
    gs = ga0;
    gs.wv2 = nullptr; gs.out2 = nullptr; gs.r2 = 0; gs.C42 = 0;
    for (int k = 0; k < 3; ++k) { gs.slab2[k] = nullptr; gs.P[k] = k == a ? 2 * lg.t1[a] : g.P[k]; gs.T[k] = g.P[k]; }
    memset(gs.sub, 0, sizeof(gs.sub));
    int ns = 0;
    for (int i = 0; i < n; ++i)
        for (int side = 0; side < 2; ++side) {
            if (fin->smp[i].slab[2 * a + side] < 0) continue;
            const int off = side ? g.P[a] - gs.P[a] : 0;
            S0Sample sm = ga0.smp[i];
            sm.org[a] += off;
            sm.slab[2 * a + (side ^ 1)] = -1;  // the cut: zero padding, no shell
            gs.smp[ns] = sm;
            gs.sub[ns][a] = off;
            fin->smp[i].slab[2 * a + side] = ns++;
        }
    *n_out = 0; *viewed = false;
    if (!ns) return MI355_OK;
    for (; ns % L1_SLAB_GROUP; ++ns) { gs.smp[ns] = gs.smp[ns - 1]; memcpy(gs.sub[ns], gs.sub[ns - 1], sizeof(gs.sub[0])); }  // (a whole last launch: its spare results are not read)
    *n_out = ns;
    gs.out = (float *)(pl.arena + pl.l1.sub_in[a]);
    // where a launch of L1_SLAB_GROUP sub-boxes goes to the stride-2 kernel that takes a view, it reads enc[0]'s whole-volume
    // result in place and the gather writes the sub-boxes' shells alone (bit-identical: a view changes where bytes are read)
    S0ViewChoice want;
    want.enc0 = sw.views && reader_takes_view(net->enc[1][0].w, c0, L1_SLAB_GROUP, gs.P, false, sw.s2_least_padding);
    LevelHandOff probe;  // (of all ns: step 2 builds a view per launch; where none can be built the gather is dense)
    const int rc = handoff_gather(net, gs, ns, (int)g.mirrors.size(), c0, 0, want, sw, "stage0_gather_kernel sub-boxes", &probe, s);
    *viewed = probe.feat_view.src != nullptr;
    return rc;
}

// step 2: enc[1] and the skip half over the sub-boxes, in launches of exactly L1_SLAB_GROUP
static int level1_slabs(mi355_unet *net, const Plan &pl, const SwGeom &g, const S0GatherArgs &gs, int n, bool viewed, bool least_padding, int a, hipStream_t s) {
    const size_t c0 = net->enc[0].back().cout, c1 = net->enc[1].back().cout, cS = net->dec[net->num_pool - 2][0].cout;
    const size_t sv0 = (size_t)gs.P[0] * gs.P[1] * gs.P[2], sv1 = sv0 / 8;
    for (int g0 = 0; g0 < n; g0 += L1_SLAB_GROUP) {
        S0View view;
        if (viewed) MI355_TRY(stage0_view_make(gs.wv, (int)g.mirrors.size(), gs.Ve, gs.P, (int)c0, gs.r, gs.smp + g0, L1_SLAB_GROUP, &view));
        MI355_TRY(level1_chain(net, pl, pl.arena + pl.l1.sub_in[a] + g0 * sv0 * c0 * 4, viewed ? &view : nullptr, least_padding, L1_SLAB_GROUP, gs.P, nullptr,
                               pl.arena + pl.l1.s_tmp, pl.arena + pl.l1.s_e[a] + g0 * sv1 * c1 * 4, pl.arena + pl.l1.s_s[a] + g0 * sv1 * cS * 4, s));
    }
    return MI355_OK;
}

// per forward: the level-1 slabs of the batch's samples (indices into lg.smp; ga0 = the stage-0 gather of the same batch), then
// step 3, the hand-off of the two level-1 tile tensors from the regions and the slabs
static int level1_tiles(mi355_unet *net, const Plan &pl, const SwGeom &g, const SwSharePlan &p, const SwSwitches &sw, const S0GatherArgs &ga0,
                        const std::vector<int> &samples, LevelHandOff *out, hipStream_t s) {
    const L1Geom &lg = p.lg;
    const int n = (int)samples.size();
    const int c1 = net->enc[1].back().cout, cS = net->dec[net->num_pool - 2][0].cout;
    MI355_REQUIRE(level1_slab_rows(n) <= S0_MAX_SAMPLES, "shared level 1: %d samples per forward", n);
    S0GatherArgs fin;
    memset(&fin, 0, sizeof(fin));
    for (int i = 0; i < n; ++i) fin.smp[i] = lg.smp[samples[i]];
    for (int a = 0; a < 3; ++a) {
        fin.slab[a] = (const float *)(pl.arena + pl.l1.s_e[a]);
        fin.slab2[a] = (const float *)(pl.arena + pl.l1.s_s[a]);
        fin.t[a] = lg.merged[a] ? lg.t1[a] : whole_conv_tiles(2 * lg.dS, a);  // (a per-origin axis has no slab; the gather asks for a thickness all the same)
        if (!lg.merged[a]) continue;
        S0GatherArgs gs; int ns; bool viewed;
        MI355_TRY(level1_sub_boxes(net, pl, g, lg, ga0, n, a, sw, &fin, gs, &ns, &viewed, s));
        MI355_TRY(level1_slabs(net, pl, g, gs, ns, viewed, sw.s2_least_padding, a, s));
    }
    const int last = (int)((net->enc[1].size() - 1) & 1);
    fin.wv = (const float *)(pl.arena + pl.l1.r_e[last]);
    fin.wv2 = (const float *)(pl.arena + pl.l1.r_s);
    fin.out = (float *)(pl.arena + pl.off[last][1]);
    fin.out2 = (float *)(pl.arena + pl.off[last ^ 1][1]);
    for (int k = 0; k < 3; ++k) { fin.P[k] = g.P[k] / 2; fin.Ve[k] = lg.R[k] / 2; }
    stage0_gather_dense(&fin);
    fin.r = lg.d1; fin.C4 = c1 / 4; fin.r2 = lg.dS; fin.C42 = cS / 4;
    // the two readers take views where they can, and the gather then writes the shells alone
    return handoff_gather(net, fin, n, (int)lg.regions.size(), c1, cS, views_decide(*net, 1, sw.views, p, n, fin.P), sw, "stage0_gather_kernel level 1", out, s);
}

// Evaluates the tiles with (index % world) == rank of one net; adds into agg (and cnt if non-null,
// for ALL tiles so that every rank holds the full normaliser).
// `first_item`: index of this net's tile 0 in the caller's work list (fold f of a fold list: f * tiles): the work items
// (fold, tile) are dealt round-robin over the ranks as ONE list, so 5 folds x 8 tiles on 3 ranks still balance.
// agg2 (null: not kept): the second moment of the same samples, handed to whichever aggregation the forward ends in; agg and cnt
// are the same bits with and without it.
static int sw_accumulate(mi355_unet *net, const SwVolume &v, const mi355_sw_opts &o, const SwGeom &g, int rank, int world, float *agg, float *cnt,
                         hipStream_t s, long first_item = 0, float *agg2 = nullptr) {
    const int nm = (int)g.mirrors.size();
    const bool use_gauss = o.use_gaussian && g.tiles.size() > 1;
    if (use_gauss) MI355_TRY(ensure_gaussian(net, g.P));
    // the aggregation's operands, the same for every tile (cnt: for ALL tiles when every rank adds its own, else cnt_add_tile has)
    AggTile tile = {{g.P[0], g.P[1], g.P[2]}, o.nonlin, use_gauss ? net->gauss_dev : nullptr, {}};
    MI355_TRY(make_mirrors("sliding window", g.mirrors.data(), nm, &tile.ml));
    const AggGrid grid = {agg, agg2, (cnt && world == 1) ? cnt : nullptr, {g.Zp[0], g.Zp[1], g.Zp[2]}};
    std::vector<int> mine;
    for (size_t t = 0; t < g.tiles.size(); ++t) if ((int)((first_item + (long)t) % world) == rank) mine.push_back((int)t);
    int bt = sw_batch_tiles(net->dtype, o.batch_tiles, nm);
    MI355_REQUIRE(nm <= 64, "too many mirrors");
    // what the tiles share: decided here, once, by the network, the geometry of all tiles and the switches alone
    const SwSwitches sw = sw_switches();
    const SwSharePlan p = sw_share_plan(level1_share_net(*net), g, sw);
    const S0Geom &sg = p.sg;
    // shared level 1: a forward then holds at most two slabs per sample and axis in one gather, so a batch the caller asked to be
    // larger than S0_MAX_SAMPLES / 2 samples is split (the default batch of an fp32 net is 16; mi355_stage0_view_plan, asked for
    // more samples than that, does not know of the cap).  The batch is not the plan's: it never changes what a tile's launch computes
    if (p.share_l1 && level1_slab_rows(bt * nm) > S0_MAX_SAMPLES) bt = std::max(1, S0_MAX_SAMPLES / 2 / nm);
    Plan pl;
    MI355_TRY(make_plan(*net, bt * nm, g.P[0], g.P[1], g.P[2], &pl));
    if (sg.shared) stage0_plan(*net, g, sg, bt * nm, &pl);
    MI355_REQUIRE(!p.share_l1 || (sg.shared && p.share_skip), "shared level 1 without the shared stage 0 and the shared skip half");
    if (p.share_l1) level1_plan(*net, g, sg, p.lg, bt * nm, &pl);
    MI355_TRY(ensure_arena(&pl, s));
    if (mine.empty()) return MI355_OK;
    if (sg.shared) MI355_TRY(stage0_whole(net, pl, v, g, sg, s));
    if (sg.merge) MI355_TRY(stage0_merged(net, pl, v, g, sg, s));
    if (p.share_l1) MI355_TRY(level1_regions(net, pl, v, g, sg, p.lg, sw, s));
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
        const void *feat; int fc; bool is_logits = false;
        FeatNorm head_norm;
        ForwardOpts fo;
        fo.is_logits = &is_logits; fo.head_norm = &head_norm;
        // level l is the forward's: its output and, where shared, its skip half lie where the forward expects them
        auto give = [&](int l, const LevelHandOff &h, bool half) {
            ForwardOpts::Level &gl = fo.lvl[l];
            gl.given = true;
            if (half) gl.skip_half = (const float *)(pl.arena + pl.off[((net->enc[l].size() - 1) & 1) ^ 1][l]);
            if (h.feat_view.src) gl.feat_view = &h.feat_view;
            if (h.half_view.src) gl.half_view = &h.half_view;
        };
        S0TilesOut t0; LevelHandOff h1;
        if (sg.shared) {
            MI355_TRY(stage0_tiles(net, pl, v, g, sg, sample_ids, views_decide(*net, 0, sw.views, p, (int)samples.size(), g.P), sw, &t0, s));
            give(0, t0.h, p.share_skip);
            if (p.share_l1) {
                MI355_TRY(level1_tiles(net, pl, g, p, sw, t0.ga, sample_ids, &h1, s));
                give(1, h1, true);
            }
        } else {
        const double pv = (double)samples.size() * g.P[0] * g.P[1] * g.P[2];
        ProfScope ps(net, s, "extract_tiles_kernel", 0.0, pv * (4.0 * net->in_channels + (net->dtype == MI355_F16 ? 2.0 : 4.0) * net->cin_pad));
        MI355_TRY(extract_tiles(v.vol, net->in_channels, v.Z, v.Y, v.X, g.pad_lo[0], g.pad_lo[1], g.pad_lo[2], samples.data(),
                                (int)samples.size(), g.P[0], g.P[1], g.P[2], net->cin_pad,
                                (void *)(pl.arena + pl.x0_off), net->dtype, s));
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
            ProfScope ps(net, s, agg2 ? "logits_aggregate_tiles_kernel m2" : "logits_aggregate_tiles_kernel", 0.0,
                         4.0 * (nb * pv * (nm * net->num_classes + 1.0) + box * (2.0 * net->num_classes + 2.0) + (agg2 ? box * 2.0 * net->num_classes : 0.0)));
            MI355_TRY(logits_aggregate_tiles((const float *)feat, net->num_classes, 0, tile, grid, origins.data(), nb, s));
            continue;
        }
        for (int i = 0; i < nb; ++i) {
            const TileDesc &td = g.tiles[mine[b0 + i]];
            const double pv = (double)g.P[0] * g.P[1] * g.P[2];
            ProfScope ps(net, s, agg2 ? "head_aggregate_kernel m2" : "head_aggregate_kernel", 2.0 * pv * nm * fc * net->num_classes,
                         pv * ((net->dtype == MI355_F16 ? 2.0 : 4.0) * nm * fc + 4.0 * (2.0 * net->num_classes + 3.0 + (agg2 ? 2.0 * net->num_classes : 0.0))));
            const int org[3] = {td.z0, td.y0, td.x0};
            MI355_TRY(head_aggregate(net->head, feat, net->dtype, i * nm, tile, grid, org, s, head_norm));
        }
    }
    return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

// Partitioning B of SURVEY.md 8e with the reference's fold list (run_brats2021_inference_singlethread.py:161 folds=(0..4),
// :112-128): the work list is (fold, tile), item f * tiles + t, dealt round-robin over the ranks; agg_dev receives
// sum over this rank's items of the Gaussian-weighted, mirror-averaged probabilities - the fold mean is linear in the
// per-fold aggregates (mean_f(agg_f / cnt) = (sum_f agg_f) / cnt / n_folds), so ONE exchange per ensemble member suffices.
static int sw_partial_folds(const mi355_unet_t *nets, int n_nets, const float *vol_dev, int Z, int Y, int X, const mi355_sw_opts *opts, int rank, int world,
                            float *agg_dev, float *agg2_dev, float *cnt_dev, void *stream) {
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
    if (agg2_dev) MI355_HIP(hipMemsetAsync(agg2_dev, 0, ZYXp * nets[0]->num_classes * sizeof(float), s));
    if (cnt_dev) MI355_HIP(hipMemsetAsync(cnt_dev, 0, ZYXp * sizeof(float), s));
    if (cnt_dev && world > 1) {
        // full normaliser of ONE fold on every rank: cnt[tile] += gaussian for ALL tiles, in tile order (no exchange needed)
        const bool use_gauss = opts->use_gaussian && g.tiles.size() > 1;
        if (use_gauss) MI355_TRY(ensure_gaussian(nets[0], g.P));
        const AggTile tile = {{g.P[0], g.P[1], g.P[2]}, opts->nonlin, use_gauss ? nets[0]->gauss_dev : nullptr, {}};
        const AggGrid grid = {agg_dev, agg2_dev, cnt_dev, {g.Zp[0], g.Zp[1], g.Zp[2]}};
        for (const TileDesc &td : g.tiles) {
            const int org[3] = {td.z0, td.y0, td.x0};
            MI355_TRY(cnt_add_tile(tile, grid, org, s));
        }
    }
    // (world == 1: the first fold's aggregation kernels add the normaliser themselves, exactly as mi355_sw_predict does)
    for (int f = 0; f < n_nets; ++f)
        MI355_TRY(sw_accumulate(nets[f], SwVolume{vol_dev, Z, Y, X}, *opts, g, rank, world, agg_dev, f == 0 ? cnt_dev : nullptr, s,
                                (long)f * (long)g.tiles.size(), agg2_dev));
    return MI355_OK;
}

extern "C" int mi355_sw_partial_folds(const mi355_unet_t *nets, int n_nets, const float *vol_dev, int Z, int Y, int X,
                                      const mi355_sw_opts *opts, int rank, int world, float *agg_dev, float *cnt_dev, void *stream) {
    return sw_partial_folds(nets, n_nets, vol_dev, Z, Y, X, opts, rank, world, agg_dev, nullptr, cnt_dev, stream);
}

// The same with the second moment kept: agg2_dev receives sum over this rank's items of gaussian * mean over mirrors of p^2, linear in
// the per-tile terms exactly as agg_dev is, so it splits over ranks and sums in rank order the same way.  Extends the fold mean of
// run_brats2021_inference_singlethread.py:97-128, which keeps the first moment alone.
extern "C" int mi355_sw_partial_folds_moments(const mi355_unet_t *nets, int n_nets, const float *vol_dev, int Z, int Y, int X,
                                              const mi355_sw_opts *opts, int rank, int world, float *agg_dev, float *agg2_dev, float *cnt_dev,
                                              void *stream) {
    MI355_REQUIRE(agg2_dev && opts, "mi355_sw_partial_folds_moments: bad argument");
    MI355_REQUIRE(opts->nonlin != MI355_NONLIN_IDENTITY, "mi355_sw_partial_folds_moments: nonlin identity has no probabilities to take moments of");
    return sw_partial_folds(nets, n_nets, vol_dev, Z, Y, X, opts, rank, world, agg_dev, agg2_dev, cnt_dev, stream);
}

extern "C" int mi355_sw_partial(mi355_unet_t net, const float *vol_dev, int Z, int Y, int X, const mi355_sw_opts *opts,
                                int rank, int world, float *agg_dev, float *cnt_dev, void *stream) {
    return mi355_sw_partial_folds(&net, 1, vol_dev, Z, Y, X, opts, rank, world, agg_dev, cnt_dev, stream);
}

// The grid a finish call reads (nothing here writes it), laid out as make_geom does: max(volume, patch) voxels, the volume centred.
static AggGrid finished_grid(const float *agg, const float *agg2, const float *cnt, const int vol[3], const int32_t patch[3], int pad[3]) {
    AggGrid grid = {(float *)agg, (float *)agg2, (float *)cnt, {}};
    for (int k = 0; k < 3; ++k) { grid.Zp[k] = std::max(vol[k], (int)patch[k]); pad[k] = (grid.Zp[k] - vol[k]) / 2; }
    return grid;
}

extern "C" int mi355_sw_finish_folds(const float *agg_dev, const float *cnt_dev, int num_classes, int Z, int Y, int X,
                                     const int32_t patch[3], int n_folds, float *probs_dev, void *stream) {
    MI355_REQUIRE(agg_dev && cnt_dev && probs_dev && patch && n_folds >= 1, "bad argument");
    MI355_TRY(bind_device());
    const int vol[3] = {Z, Y, X};
    int pad[3];
    const AggGrid grid = finished_grid(agg_dev, nullptr, cnt_dev, vol, patch, pad);
    MI355_TRY(finish_probs(grid, num_classes, vol, pad, probs_dev, 0, (hipStream_t)stream));
    if (n_folds > 1) MI355_TRY(scale_inplace(probs_dev, (int64_t)num_classes * Z * Y * X, (float)n_folds, (hipStream_t)stream));
    return MI355_OK;
}

extern "C" int mi355_sw_finish_moments(const float *agg_dev, const float *agg2_dev, const float *cnt_dev, int num_classes, int Z, int Y, int X,
                                       const int32_t patch[3], int n_folds, float *mean_dev, float *m2_dev, void *stream) {
    MI355_REQUIRE(agg_dev && agg2_dev && cnt_dev && mean_dev && m2_dev && patch && n_folds >= 1 && num_classes >= 1 && Z >= 1 && Y >= 1 && X >= 1,
                  "mi355_sw_finish_moments: bad argument");
    MI355_TRY(bind_device());
    const int vol[3] = {Z, Y, X};
    int pad[3];
    const AggGrid grid = finished_grid(agg_dev, agg2_dev, cnt_dev, vol, patch, pad);
    return finish_moments(grid, num_classes, vol, pad, n_folds, mean_dev, m2_dev, (hipStream_t)stream);
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
    // allocate / synchronise / free round trip per volume costs more than the small kernels of a step
    void *scratch = nullptr;
    MI355_TRY(device_scratch(SCR_SW_AGG, s, ZYXp * (size_t)(C + 1) * sizeof(float), &scratch));
    float *agg = (float *)scratch, *cnt = agg + ZYXp * C;
    const AggGrid grid = {agg, nullptr, cnt, {g.Zp[0], g.Zp[1], g.Zp[2]}};
    const int vol[3] = {Z, Y, X};
    int rc = MI355_OK;
    for (int f = 0; f < n_nets && rc == MI355_OK; ++f) {
        if (nets[f]->num_classes != C) { set_error("fold %d has %d classes, fold 0 has %d", f, nets[f]->num_classes, C); rc = MI355_ERR_INVALID; break; }
        if (hipMemsetAsync(agg, 0, ZYXp * C * sizeof(float), s) != hipSuccess ||
            hipMemsetAsync(cnt, 0, ZYXp * sizeof(float), s) != hipSuccess) { set_error("memset failed"); rc = MI355_ERR_HIP; break; }
        rc = sw_accumulate(nets[f], SwVolume{vol_dev, Z, Y, X}, *opts, g, 0, 1, agg, cnt, s);
        if (rc == MI355_OK)
            rc = finish_probs(grid, C, vol, g.pad_lo, probs_dev, f > 0, s);
    }
    // fold mean: np.mean(list_of_fp32_arrays, axis=0) = fp32 running sum in list order, one divide
    if (rc == MI355_OK && n_nets > 1) rc = scale_inplace(probs_dev, (int64_t)C * Z * Y * X, (float)n_nets, s);
    // asynchronous on `stream` like every other entry point that takes one: probs_dev is valid in stream order
    return rc;
}
