// Network object, activation arena and forward pass (host side), plus the create / destroy / forward / profile entry points
// declared in include/mi355_nnunet.h.  The sliding-window predictor that drives it is sliding_window.hip.
//
// Reference behaviour restated here:
//   * Generic_UNet.forward                 model_architecture/generic_UNet.py:423-446
//   * eval-mode BatchNorm folded into the preceding conv (ConvDropoutNormNonlin :68-72)
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "unet_internal.h"

namespace mi355 {

// half != nullptr (the first block of the last decoder stage, which reads the virtual concat (upsampled, skip)): when the network
// qualifies for the shared skip half (skip_share_network_ok, the predicate the sliding window decides by) the block also gets the
// packs of its two halves, each through conv_weights_upload and so through conv_pack_layout like any layer: the same fp64
// Winograd transform, rounded once.  Everything is uploaded straight into net.mem: a refusal part-way through a layer leaves
// nothing behind once the handle goes.
static int build_conv(mi355_unet &net, const mi355_conv_desc &d, int cin_phys, ConvLayer *out, bool stem = false, const SkipShareNet *half = nullptr) {
    MI355_REQUIRE(d.weight != nullptr, "conv %d->%d: null weight", d.cin, d.cout);
    MI355_REQUIRE(d.cin > 0 && d.cout > 0 && cin_phys >= d.cin, "conv: bad channel counts %d->%d (phys %d)", d.cin, d.cout, cin_phys);
    ConvLayer L;
    L.cin = d.cin; L.cout = d.cout; L.stride = d.stride;
    const size_t wn = (size_t)d.cout * d.cin * 27;
    std::vector<float> w(d.weight, d.weight + wn);
    std::vector<float> b(d.cout, 0.f);
    if (d.bias) b.assign(d.bias, d.bias + d.cout);
    if (net.norm == MI355_NORM_BATCH) {
        MI355_REQUIRE(d.running_mean && d.running_var, "BatchNorm conv %d->%d: running stats missing", d.cin, d.cout);
        std::vector<float> sc(d.cout), sh(d.cout);
        for (int co = 0; co < d.cout; ++co) {
            const double g = d.gamma ? d.gamma[co] : 1.0, be = d.beta ? d.beta[co] : 0.0;
            const double s = g / std::sqrt((double)d.running_var[co] + (double)net.eps);
            sc[co] = (float)s;
            sh[co] = (float)(be - (double)d.running_mean[co] * s);
        }
        if (!net.nonlin_first) {
            // y = lrelu(BN(conv(x)+b)) = lrelu(conv'(x) + b')  with w' = w*s, b' = b*s + shift
            for (int co = 0; co < d.cout; ++co) {
                const double s = sc[co];
                for (size_t k = 0; k < (size_t)d.cin * 27; ++k)
                    w[(size_t)co * d.cin * 27 + k] = (float)((double)w[(size_t)co * d.cin * 27 + k] * s);
                b[co] = (float)((double)b[co] * s + (double)sh[co]);
            }
        } else {
            L.post_affine = true;
            MI355_TRY(net.mem.upload(sc.data(), d.cout * sizeof(float), &L.gamma_dev));
            MI355_TRY(net.mem.upload(sh.data(), d.cout * sizeof(float), &L.beta_dev));
        }
    } else if (net.norm == MI355_NORM_INSTANCE || net.norm == MI355_NORM_GROUP) {
        L.runtime_norm = true;
        std::vector<float> g(d.cout, 1.f), be(d.cout, 0.f);
        if (d.gamma) g.assign(d.gamma, d.gamma + d.cout);
        if (d.beta) be.assign(d.beta, d.beta + d.cout);
        MI355_TRY(net.mem.upload(g.data(), d.cout * sizeof(float), &L.gamma_dev));
        MI355_TRY(net.mem.upload(be.data(), d.cout * sizeof(float), &L.beta_dev));
    }
    if (stem) { L.is_stem = true; MI355_TRY(stem_weights_upload(net.mem, w.data(), b.data(), d.cin, d.cout, net.dtype, &L.stem)); }
    else if (net.dtype == MI355_F16) MI355_TRY(conv_weights_upload_f16(net.mem, w.data(), b.data(), d.cin, cin_phys, d.cout, d.stride, &L.wh));
    else MI355_TRY(conv_weights_upload(net.mem, w.data(), b.data(), d.cin, cin_phys, d.cout, d.stride, false, &L.w));
    if (half && !stem && cin_phys == d.cin && half->c_up + half->c_skip == d.cin && skip_share_network_ok(*half)) {
        const int split_c0 = half->c_up, c_skip = half->c_skip;
        {
            std::vector<float> wu((size_t)d.cout * split_c0 * 27), ws((size_t)d.cout * c_skip * 27);
            for (int co = 0; co < d.cout; ++co) {
                const float *src = &w[(size_t)co * d.cin * 27];
                std::copy(src, src + (size_t)split_c0 * 27, &wu[(size_t)co * split_c0 * 27]);
                std::copy(src + (size_t)split_c0 * 27, src + (size_t)d.cin * 27, &ws[(size_t)co * c_skip * 27]);
            }
            MI355_TRY(conv_weights_upload(net.mem, wu.data(), b.data(), split_c0, split_c0, d.cout, 1, false, &L.w_up));
            MI355_TRY(conv_weights_upload(net.mem, ws.data(), nullptr, c_skip, c_skip, d.cout, 1, false, &L.w_skip));
            L.split_c0 = split_c0;
        }
    }
    *out = L;
    return MI355_OK;
}

static void destroy(mi355_unet *net) {  // (device memory goes with net->mem and net->gauss_mem)
    if (!net) return;
    for (auto &r : net->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (hipEvent_t e : net->event_pool) (void)hipEventDestroy(e);
    delete net;
}

int make_plan(const mi355_unet &net, int N, int D, int H, int W, Plan *pl) {
    const int np = net.num_pool;
    MI355_REQUIRE(D % (1 << np) == 0 && H % (1 << np) == 0 && W % (1 << np) == 0,
                  "patch %dx%dx%d must be divisible by %d (generic_UNet.py:256)", D, H, W, 1 << np);
    pl->vox.resize(np + 1);
    pl->maxc.assign(np + 1, 0);
    for (int l = 0; l <= np; ++l) {
        pl->vox[l] = (int64_t)(D >> l) * (H >> l) * (W >> l);
        for (auto &L : net.enc[l]) pl->maxc[l] = std::max(pl->maxc[l], L.cout);
    }
    for (int u = 0; u < np; ++u) {
        const int l = np - 1 - u;
        pl->maxc[l] = std::max(pl->maxc[l], net.tu[u].cout);
        for (auto &L : net.dec[u]) pl->maxc[l] = std::max(pl->maxc[l], L.cout);
    }
    ArenaCursor c{0};
    const size_t es = net.dtype == MI355_F16 ? 2 : 4;
    pl->x0_off = c.take((size_t)N * pl->vox[0] * net.cin_pad * es);
    for (int k = 0; k < 4; ++k) pl->off[k].resize(np + 1);
    for (int l = 0; l <= np; ++l)
        for (int k = 0; k < 4; ++k)
            pl->off[k][l] = c.take((size_t)N * pl->vox[l] * pl->maxc[l] * es);
    pl->stats_bytes = (size_t)N * net.max_channels * 2 * sizeof(double);
    pl->stats_off = c.take(pl->stats_bytes);
    pl->scale_off = c.take((size_t)N * net.max_channels * sizeof(float));
    pl->shift_off = c.take((size_t)N * net.max_channels * sizeof(float));
    pl->scale2_off = c.take((size_t)N * net.max_channels * sizeof(float));
    pl->shift2_off = c.take((size_t)N * net.max_channels * sizeof(float));
    pl->total = c.o;
    return MI355_OK;
}

int ensure_arena(Plan *pl, hipStream_t s) {
    void *p = nullptr;
    MI355_TRY(device_scratch(SCR_ARENA, s, pl->total, &p));
    pl->arena = (char *)p;
    return MI355_OK;
}

// One ConvDropoutNormNonlin / ConvDropoutNonlinNorm block; `o`: its optional operands (BlockOpts, unet_internal.h).
int run_block(mi355_unet *net, const Plan &pl, const ConvLayer &L, const void *in0, int C0, const void *in1, int C1, int N, int Di, int Hi,
              int Wi, void *out, hipStream_t s, const BlockOpts &o) {
    const bool f16 = net->dtype == MI355_F16;
    MI355_REQUIRE(!o.half || (!f16 && !L.is_stem && !L.runtime_norm && !L.post_affine && o.half->cin == C0 + C1), "conv %d->%d: bad half launch", L.cin, L.cout);
    MI355_REQUIRE((!o.in0_view && !o.addend_view) || (!f16 && !L.is_stem), "conv %d->%d: a stage-0 view on a launch that cannot take one", L.cin, L.cout);
    double *stats = (double *)(pl.arena + pl.stats_off);
    float *scale = (float *)(pl.arena + (o.defer_norm ? pl.scale2_off : pl.scale_off)), *shift = (float *)(pl.arena + (o.defer_norm ? pl.shift2_off : pl.shift_off));
    int act = ACT_LRELU;
    double *stats_arg = nullptr;
    if (L.runtime_norm) {
        act = net->nonlin_first ? ACT_LRELU : ACT_NONE;
        stats_arg = stats;
        MI355_HIP(hipMemsetAsync(stats, 0, (size_t)N * L.cout * 2 * sizeof(double), s));
    }
    const int st = L.stride;
    const int64_t Vo = (int64_t)((Di - 1) / st + 1) * ((Hi - 1) / st + 1) * ((Wi - 1) / st + 1);
    {
        // algorithmic work of this launch: 2*MAC over the LOGICAL cin; input read once + output written once + weights
        const double es = f16 ? 2.0 : 4.0;
        const int cin = o.half ? o.half->cin : L.cin;
        const double flops = 2.0 * N * Vo * L.cout * (double)cin * 27.0;
        const double bytes = es * ((double)N * Di * Hi * Wi * (C0 + C1) + (o.addend ? 2.0 : 1.0) * N * Vo * L.cout + (double)L.cout * cin * 27.0);
        FusedOps f;
        f.x1 = in1; f.c1 = C1;
        if (o.head_logits_out) { f.head_w = net->head.w_dev; f.head_b = net->head.b_dev; f.head_ncls = net->head.ncls; f.head_out = o.head_logits_out; }
        if (o.in_norm) {  // in0 is the previous block's raw conv output: normalise (+ LeakyReLU) while staging (fp32: the F(2x2x2,3x3x3) kernel, in LDS)
            f.in_scale = (const float *)(pl.arena + pl.scale2_off); f.in_shift = (const float *)(pl.arena + pl.shift2_off);
            f.in_act = net->nonlin_first ? ACT_NONE : ACT_LRELU;
        }
        const char *kname = nullptr;
        if (L.is_stem) {
            ProfScope ps(net, s, f16 ? "conv3_stem_f16_kernel" : "conv3_stem_f32_kernel", flops, bytes);
            MI355_TRY(conv3d_stem(L.stem, in0, N, Di, Hi, Wi, out, stats_arg, act, net->slope, s));
        } else if (f16) {
            ProfScope ps(net, s, "conv3_f16", flops, bytes);
            MI355_TRY(conv3d_mfma_f16(L.wh, make_call<_Float16>(in0, C0 + C1, N, Di, Hi, Wi, out, stats_arg, act, net->slope, f), s, &kname));
            ps.rename(kname);
        } else {
            ConvCall c = make_call<float>(in0, C0 + C1, N, Di, Hi, Wi, out, stats_arg, o.half && !o.addend ? ACT_NONE : act, net->slope, f);
            c.addend = o.addend;
            c.in0_view = o.in0_view; c.addend_view = o.addend_view;  // (stage-0 views: the caller asked the planner first)
            c.s2_least_padding = o.s2_least_padding;
            const ConvWeights &W = o.half ? *o.half : L.w;
            ProfScope ps(net, s, "conv3_direct_kernel", flops, bytes);  // (renamed to the instantiation the MFMA dispatch picks)
            if (W.wp_dev) MI355_TRY(conv3d_mfma_f32(W, c, s, &kname));
            else MI355_TRY(conv3d_direct_f32(W, c, s));
            ps.rename(kname, o.half_name);
        }
    }
    if (o.half) return MI355_OK;
    const double es = f16 ? 2.0 : 4.0;
    if (L.runtime_norm) {
        MI355_TRY(norm_finalize(stats, N, L.cout, Vo, net->norm, net->num_groups, net->eps, L.gamma_dev, L.beta_dev,
                                scale, shift, s));
        if (o.defer_norm) return MI355_OK;  // the consumer applies scale / shift (and the activation) in its staging
        ProfScope ps(net, s, f16 ? "norm_apply_kernel<f16>" : "norm_apply_kernel<f32>", 2.0 * N * Vo * L.cout, 2.0 * es * N * Vo * L.cout);
        MI355_TRY(norm_apply(out, net->dtype, N, Vo, L.cout, scale, shift, net->nonlin_first ? ACT_NONE : ACT_LRELU, net->slope, s));
    } else if (L.post_affine) {
        // BN after the nonlinearity: per-channel affine, identical for every sample
        for (int n = 0; n < N; ++n)
            MI355_TRY(norm_apply((char *)out + (size_t)n * Vo * L.cout * (size_t)es, net->dtype, 1, Vo, L.cout, L.gamma_dev, L.beta_dev,
                                 ACT_NONE, net->slope, s));
    }
    return MI355_OK;
}

// Can block `L` (run-time Instance/GroupNorm) leave its normalisation to the next block `Ln` of the same stage?
// generic_UNet.py:62-72 is one expression, lrelu(instnorm(conv(x))).  fp16: the consumer must be a kernel that normalises while
// staging (conv3d_f16_fuses_input_norm: register-staged pipelined kernel or the LDS-DMA kernel).  fp32 (round 4): the consumer
// must be a launch of the F(2x2x2,3x3x3) kernel, which normalises its brick in LDS (conv3d_wino3_fuses_input_norm).
static bool can_defer_norm(const mi355_unet *net, const ConvLayer &L, const ConvLayer &Ln, int N, int Dl, int Hl, int Wl) {
    if (!L.runtime_norm || Ln.stride != 1 || Ln.is_stem || Ln.cin != L.cout) return false;
    double *const stats = Ln.runtime_norm ? (double *)1 : nullptr;  // (only tested for null)
    if (net->dtype == MI355_F16) {
        if ((!L.is_stem && !L.wh.wp_dev) || !Ln.wh.wp_dev) return false;
        return conv3d_f16_fuses_input_norm(Ln.wh, make_call<_Float16>(nullptr, L.cout, N, Dl, Hl, Wl, nullptr, stats, ACT_NONE, 0.f));
    }
    if (!Ln.w.wp3_dev) return false;
    return conv3d_wino3_fuses_input_norm(Ln.w, make_call<float>(nullptr, L.cout, N, Dl, Hl, Wl, nullptr, stats, ACT_NONE, 0.f));
}

// x0: [N,D,H,W,cin_pad] already in the arena at pl.x0_off.  Returns the last decoder feature map.
// If the last decoder block has no run-time normalisation (BN folded / no norm) and its Cout fits one workgroup, the
// 1x1x1 head is fused into its epilogue: *is_logits = true and *feat points at fp32 logits [N][ncls][V] (written to
// logits_target when given, else into the arena); the 32-channel feature map is then never written nor re-read.
// head_norm (round 3): when non-null and the last decoder block carries a run-time Instance/GroupNorm, that block's
// normalisation (+ activation) is NOT applied to the returned feature map: *head_norm receives its scale / shift and the
// caller's head kernel applies them while reading the features (head_logits / head_aggregate take a FeatNorm).
// lvl[l] (ForwardOpts::Level; l = 0: shared stage 0, l = 1: shared level 1, which asks for level 0 and both skip halves):
// given: the level-l features are already where enc[l]'s last block writes them; the pass starts at level l + 1.
// skip_half: [N][V][cout] = the skip half of the first conv of the decoder stage that reads them (the last stage; dec[np - 2]), already
// gathered into the level-l buffer that stage leaves free; that block then runs over the upsampled tensor alone and adds it in its epilogue.
// feat_view / half_view (stage-0 views): the level-l features / the skip half hold their shells only; their one reader - the
// first block of level l + 1 / that epilogue - takes the rest through the view.
int forward_features(mi355_unet *net, const Plan &pl, int N, int D, int H, int W, const void **feat, int *feat_c, hipStream_t s,
                     const ForwardOpts &o) {
    const int np = net->num_pool;
    const bool f16 = net->dtype == MI355_F16;
    auto buf = [&](int k, int l) { return (void *)(pl.arena + pl.off[k][l]); };
    const void *cur = (const void *)(pl.arena + pl.x0_off);
    int curC = net->cin_pad;
    std::vector<const void *> skip(np);
    std::vector<int> skipC(np);
    // encoder + bottleneck
    for (int l = 0; l <= np; ++l) {
        int Di = D >> l, Hi = H >> l, Wi = W >> l;
        bool pending = false;  // cur holds a raw conv output whose normalisation the next block applies
        const bool given = l < 2 && o.lvl[l].given;
        if (given) { cur = buf((int)((net->enc[l].size() - 1) & 1), l); curC = net->enc[l].back().cout; }
        for (size_t i = 0; i < net->enc[l].size() && !given; ++i) {
            const ConvLayer &L = net->enc[l][i];
            int inD = Di, inH = Hi, inW = Wi;
            if (L.stride == 2) { inD = Di * 2; inH = Hi * 2; inW = Wi * 2; }
            void *out = buf((int)(i & 1), l);
            const bool defer = i + 1 < net->enc[l].size() && can_defer_norm(net, L, net->enc[l][i + 1], N, Di, Hi, Wi);
            BlockOpts bo;
            bo.defer_norm = defer; bo.in_norm = pending;
            if (i == 0 && (l == 1 || l == 2) && o.lvl[l - 1].given) bo.in0_view = o.lvl[l - 1].feat_view;
            MI355_TRY(run_block(net, pl, L, cur, curC, nullptr, 0, N, inD, inH, inW, out, s, bo));
            pending = defer;
            cur = out; curC = L.cout;
        }
        if (l < np) { skip[l] = cur; skipC[l] = curC; }
    }
    MI355_REQUIRE(!o.lvl[0].feat_view || (o.lvl[0].skip_half && np >= 1), "stage-0 view of the level-0 features while the decoder reads them whole");
    MI355_REQUIRE(!o.lvl[1].given || (o.lvl[0].given && o.lvl[0].skip_half && o.lvl[1].skip_half && np >= 2), "shared level 1 without the shared stage 0 and both skip halves");
    // decoder
    for (int u = 0; u < np; ++u) {
        const int l = np - 1 - u;
        const int Dl = D >> l, Hl = H >> l, Wl = W >> l;
        void *up = buf(2, l);
        const int tcin = net->tu[u].cin, tcout = net->tu[u].cout;
        MI355_REQUIRE(tcin == curC, "tu.%d expects %d channels, got %d", u, tcin, curC);
        {
            const double es = f16 ? 2.0 : 4.0;
            const double vin = (double)N * (Dl / 2) * (Hl / 2) * (Wl / 2);
            TconvPlan tp;
            MI355_TRY(plan_tconv(net->tu[u].dtype, tcin, tcout, (long)N * (Dl / 2) * (Hl / 2) * (Wl / 2), &tp));
            ProfScope ps(net, s, tp.row->name, 2.0 * vin * tcin * tcout * 8.0, es * (vin * tcin + 8.0 * vin * tcout + 8.0 * tcin * tcout));
            MI355_TRY(launch_tconv(net->tu[u], tp, cur, N, Dl / 2, Hl / 2, Wl / 2, up, s));
        }
        // concat order (upsampled, skip): generic_UNet.py:438 - never materialised
        const void *in0 = up, *in1 = skip[l];
        int C0 = tcout, C1 = skipC[l];
        // outputs alternate between T and whichever of A/B is not the skip
        void *freeAB = (skip[l] == buf(0, l)) ? buf(1, l) : buf(0, l);
        bool pending_d = false;
        for (size_t i = 0; i < net->dec[u].size(); ++i) {
            const ConvLayer &L = net->dec[u][i];
            void *out = (i & 1) ? freeAB : buf(3, l);
            const bool fuse = env_switch("MI355_FUSE_HEAD") && !(f16 && conv_impl() == 0);  // the fp16 fused epilogue exists in the pipelined kernel only
            const bool last = o.is_logits && (u == np - 1) && (i + 1 == net->dec[u].size());
            const int lnf = f16 ? L.wh.nf : L.w.nf;
            const bool has_pack = f16 ? (L.wh.wp_dev != nullptr) : (L.w.wp_dev != nullptr);
            if (last && fuse && !L.runtime_norm && !L.post_affine && has_pack && L.cout == 32 * lnf && net->head.ncls <= 4 &&
                net->head.cin == L.cout && (!f16 || lnf == 1)) {
                float *lg = o.logits_target ? o.logits_target : (float *)out;
                BlockOpts bo;
                bo.head_logits_out = lg; bo.in_norm = pending_d;  // (a pending norm is refused loudly by the fused-head conv: ADVICE r2)
                MI355_TRY(run_block(net, pl, L, in0, C0, in1, C1, N, Dl, Hl, Wl, nullptr, s, bo));
                *o.is_logits = true;
                *feat = lg; *feat_c = net->head.ncls;
                return MI355_OK;
            }
            if (i == 0 && l < 2 && o.lvl[l].skip_half) {  // the block runs over the upsampled half alone; the gathered skip half is its addend
                const ForwardOpts::Level &gl = o.lvl[l];
                MI355_REQUIRE(l != 1 || (L.split_c0 == C0 && (const void *)gl.skip_half == freeAB && net->dec[u].size() > 1), "shared level 1: the block was not split at %d channels", C0);
                MI355_REQUIRE(l != 0 || (L.split_c0 == C0 && (const void *)gl.skip_half == freeAB), "shared skip half: the block was not split at %d channels", C0);
                BlockOpts bo;
                bo.half = &L.w_up; bo.addend = gl.skip_half; bo.half_name = " up-half"; bo.addend_view = gl.half_view;
                MI355_TRY(run_block(net, pl, L, in0, C0, nullptr, 0, N, Dl, Hl, Wl, out, s, bo));
                in0 = out; C0 = L.cout; in1 = nullptr; C1 = 0;
                continue;
            }
            const bool to_head = env_switch("MI355_FUSE_NORM") && o.head_norm && L.runtime_norm && (u == np - 1) && (i + 1 == net->dec[u].size());
            const bool defer = to_head || (i + 1 < net->dec[u].size() && can_defer_norm(net, L, net->dec[u][i + 1], N, Dl, Hl, Wl));
            BlockOpts bo;
            bo.defer_norm = defer; bo.in_norm = pending_d;
            MI355_TRY(run_block(net, pl, L, in0, C0, in1, C1, N, Dl, Hl, Wl, out, s, bo));
            if (to_head) {
                o.head_norm->scale = (const float *)(pl.arena + pl.scale2_off);
                o.head_norm->shift = (const float *)(pl.arena + pl.shift2_off);
                o.head_norm->slope = net->nonlin_first ? 1.0f : net->slope;  // ConvDropoutNonlinNorm: the activation came before the norm
            }
            pending_d = defer;
            in0 = out; C0 = L.cout; in1 = nullptr; C1 = 0;
        }
        cur = in0; curC = C0;
    }
    if (o.is_logits) *o.is_logits = false;
    *feat = cur; *feat_c = curC;
    return MI355_OK;
}

}  // namespace mi355

using namespace mi355;

// =============================================================================== C ABI
extern "C" int mi355_unet_create(const mi355_unet_desc *d, mi355_unet_t *out) {
    MI355_REQUIRE(d && out, "null argument");
    MI355_TRY(require_device());
    MI355_REQUIRE(d->dtype == MI355_F32 || d->dtype == MI355_F16, "dtype %d unknown", d->dtype);
    MI355_REQUIRE(d->num_pool >= 1 && d->num_pool <= 7, "num_pool %d out of range", d->num_pool);
    MI355_REQUIRE(d->in_channels >= 1 && d->in_channels <= 8, "in_channels %d unsupported (1..8)", d->in_channels);
    MI355_REQUIRE(d->norm >= MI355_NORM_NONE && d->norm <= MI355_NORM_GROUP, "norm kind %d", d->norm);
    // every kernel computes LeakyReLU as max(x, slope * x), which is LeakyReLU for 0 <= slope <= 1 only; the
    // reference's is 0.01 (generic_UNet.py:39)
    MI355_REQUIRE(d->lrelu_slope >= 0.f && d->lrelu_slope <= 1.f, "lrelu_slope %g outside [0, 1]: the kernels evaluate LeakyReLU as max(x, slope x)", (double)d->lrelu_slope);
    mi355_unet *net = new mi355_unet();
    net->in_channels = d->in_channels; net->cin_pad = d->dtype == MI355_F16 ? 16 : 8; net->num_classes = d->num_classes;
    const bool use_stem = d->in_channels <= 4 && d->n_convs > 0 && d->convs[0].cout % 32 == 0 && d->convs[0].stride == 1 &&
                          !(getenv("MI355_NO_STEM") && getenv("MI355_NO_STEM")[0] == '1');
    if (use_stem) net->cin_pad = 4;  // NDHW4 input, x-taps folded into K (conv_stem.hip)
    net->num_pool = d->num_pool; net->norm = d->norm; net->num_groups = d->num_groups;
    net->nonlin_first = d->nonlin_first; net->dtype = d->dtype; net->eps = d->eps; net->slope = d->lrelu_slope;
    int rc = MI355_OK;
    int ci = 0;
    int prevC = net->cin_pad;
    net->enc.resize(d->num_pool + 1);
    net->dec.resize(d->num_pool);
    net->tu.resize(d->num_pool);
    std::vector<int> skipC(d->num_pool, 0);
    auto fail = [&](int code) { destroy(net); return code; };
    for (int l = 0; l <= d->num_pool && rc == MI355_OK; ++l) {
        if (d->enc_convs[l] < 1) { set_error("encoder stage %d has no convs", l); return fail(MI355_ERR_INVALID); }
        for (int i = 0; i < d->enc_convs[l]; ++i) {
            if (ci >= d->n_convs) { set_error("conv list too short"); return fail(MI355_ERR_INVALID); }
            const mi355_conv_desc &cd = d->convs[ci++];
            const int want_stride = (l > 0 && i == 0) ? 2 : 1;
            if (cd.stride != want_stride) { set_error("encoder conv %d.%d: stride %d, expected %d", l, i, cd.stride, want_stride); return fail(MI355_ERR_INVALID); }
            const int logical_in = (l == 0 && i == 0) ? d->in_channels : prevC;
            if (cd.cin != logical_in) { set_error("encoder conv %d.%d: cin %d, expected %d", l, i, cd.cin, logical_in); return fail(MI355_ERR_INVALID); }
            ConvLayer L;
            rc = build_conv(*net, cd, prevC, &L, use_stem && l == 0 && i == 0);
            if (rc != MI355_OK) return fail(rc);
            net->enc[l].push_back(L);
            prevC = cd.cout;
            net->max_channels = std::max(net->max_channels, cd.cout);
        }
        if (l < d->num_pool) skipC[l] = prevC;
    }
    for (int u = 0; u < d->num_pool; ++u) {
        const int l = d->num_pool - 1 - u;
        const mi355_tconv_desc &td = d->tconvs[u];
        if (td.cin != prevC) { set_error("tu.%d: cin %d, expected %d", u, td.cin, prevC); return fail(MI355_ERR_INVALID); }
        rc = tconv_weights_upload(net->mem, td.weight, td.cin, td.cout, d->dtype, &net->tu[u]);
        if (rc != MI355_OK) return fail(rc);
        net->max_channels = std::max(net->max_channels, td.cout);
        int inC = td.cout + skipC[l];
        if (d->dec_convs[u] < 1) { set_error("decoder stage %d has no convs", u); return fail(MI355_ERR_INVALID); }
        for (int i = 0; i < d->dec_convs[u]; ++i) {
            if (ci >= d->n_convs) { set_error("conv list too short"); return fail(MI355_ERR_INVALID); }
            const mi355_conv_desc &cd = d->convs[ci++];
            if (cd.stride != 1 || cd.cin != inC) { set_error("decoder conv %d.%d: cin %d stride %d, expected %d / 1", u, i, cd.cin, cd.stride, inC); return fail(MI355_ERR_INVALID); }
            ConvLayer L;
            // (the stage that reads enc[0]'s output - shared skip half - and, unless MI355_SHARE_LEVEL1 is 0 now, the one that reads
            //  enc[1]'s - shared level 1; the latter is never the net's last conv.  A net made with the switch at 0 has no such packs
            //  and never takes that path)
            const SkipShareNet half = skip_share_net_of(d->dtype, stage0_blocks(*net), cd.stride, d->norm, d->nonlin_first, td.cout, skipC[l], cd.cout,
                                                         d->dec_convs[u] == 1 ? d->num_classes : 0);
            const bool split = i == 0 && (l == 0 || (l == 1 && d->dec_convs[u] > 1 && level1_share_mode() != 0));
            rc = build_conv(*net, cd, inC, &L, false, split ? &half : nullptr);
            if (rc != MI355_OK) return fail(rc);
            net->dec[u].push_back(L);
            inC = cd.cout;
            net->max_channels = std::max(net->max_channels, cd.cout);
        }
        prevC = inC;
    }
    if (ci != d->n_convs) { set_error("%d convs given, topology uses %d", d->n_convs, ci); return fail(MI355_ERR_INVALID); }
    if (d->head.cin != prevC || d->head.num_classes != d->num_classes) { set_error("head: cin %d classes %d, expected %d / %d", d->head.cin, d->head.num_classes, prevC, d->num_classes); return fail(MI355_ERR_INVALID); }
    rc = head_weights_upload(net->mem, d->head.weight, d->head.bias, d->head.cin, d->head.num_classes, &net->head);
    if (rc != MI355_OK) return fail(rc);
    *out = net;
    return MI355_OK;
}

extern "C" int mi355_unet_destroy(mi355_unet_t net) {
    destroy(net);
    return MI355_OK;
}

extern "C" int64_t mi355_unet_flops(mi355_unet_t net, int d, int h, int w) {
    if (!net) return -1;
    const int np = net->num_pool;
    int64_t total = 0;
    auto vox = [&](int l) { return (int64_t)(d >> l) * (h >> l) * (w >> l); };
    for (int l = 0; l <= np; ++l)
        for (auto &L : net->enc[l]) total += 2 * vox(l) * L.cout * L.cin * 27;
    for (int u = 0; u < np; ++u) {
        const int l = np - 1 - u;
        total += 2 * vox(l + 1) * ((int64_t)net->tu[u].cin * net->tu[u].cout) * 8;
        for (auto &L : net->dec[u]) total += 2 * vox(l) * L.cout * L.cin * 27;
    }
    total += 2 * vox(0) * net->head.cin * net->head.ncls;
    return total;
}

extern "C" int mi355_unet_forward(mi355_unet_t net, const float *x_dev, int n, int d, int h, int w, float *logits_dev,
                                  void *stream) {
    MI355_REQUIRE(net && x_dev && logits_dev && n > 0, "bad argument");
    MI355_TRY(bind_device());
    hipStream_t s = (hipStream_t)stream;
    Plan pl;
    MI355_TRY(make_plan(*net, n, d, h, w, &pl));
    MI355_TRY(ensure_arena(&pl, s));
    const int64_t V = (int64_t)d * h * w;
    MI355_TRY(nchw_to_ndhwc(x_dev, n, net->in_channels, V, net->cin_pad, (void *)(pl.arena + pl.x0_off), net->dtype, s));
    const void *feat; int fc; bool is_logits = false;
    FeatNorm head_norm;
    ForwardOpts fo;
    fo.is_logits = &is_logits; fo.logits_target = logits_dev; fo.head_norm = &head_norm;
    MI355_TRY(forward_features(net, pl, n, d, h, w, &feat, &fc, s, fo));
    if (is_logits) return MI355_OK;  // the last conv wrote [n][ncls][V] straight into logits_dev
    MI355_REQUIRE(fc == net->head.cin, "head expects %d channels, decoder gives %d", net->head.cin, fc);
    MI355_TRY(head_logits(net->head, feat, net->dtype, n, V, logits_dev, s, head_norm));
    return MI355_OK;
}

extern "C" int mi355_profile_enable(mi355_unet_t net, int on) {
    MI355_REQUIRE(net, "null handle");
    net->prof_on = on != 0;
    if (net->prof_on) {
        // pre-create the events here, outside any timed region (a bench run records ~120 per step)
        while (net->event_pool.size() < 4096) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) break;
            net->event_pool.push_back(e);
        }
    }
    return MI355_OK;
}

// Synchronises the device, folds the recorded launches per kernel name, clears the log.
extern "C" int mi355_profile_read(mi355_unet_t net, mi355_prof_entry *out, int max_entries) {
    MI355_REQUIRE(net && out && max_entries > 0, "bad argument");
    MI355_HIP(hipDeviceSynchronize());
    int n = 0;
    for (auto &r : net->prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) ms = 0.f;
        net->event_pool.push_back(r.a);
        net->event_pool.push_back(r.b);
        int k = 0;
        for (; k < n; ++k) if (r.name == out[k].name) break;
        if (k == n) {
            if (n == max_entries) continue;
            memset(&out[n], 0, sizeof(out[n]));
            snprintf(out[n].name, sizeof(out[n].name), "%s", r.name.c_str());
            ++n;
        }
        out[k].launches += 1; out[k].ms += ms; out[k].flops += r.flops; out[k].bytes += r.bytes;
    }
    net->prof.clear();
    return n;
}
