// Network object, activation arena, forward pass and the sliding-window predictor (host side),
// plus the extern "C" entry points declared in include/mi355_nnunet.h.
//
// Reference behaviour restated here:
//   * Generic_UNet.forward                 model_architecture/generic_UNet.py:423-446
//   * eval-mode BatchNorm folded into the preceding conv (ConvDropoutNormNonlin :68-72)
//   * nnU-Net v1 SegmentationNetwork._internal_predict_3D_3Dconv_tiled / _compute_steps_for_
//     sliding_window / _get_gaussian / _internal_maybe_mirror_and_pred_3D (un-vendored upstream;
//     SURVEY.md 8a rows T1-T5) as driven by run_brats2021_inference_singlethread.py:97-128.
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "conv_plan.h"

namespace mi355 {

static thread_local std::string g_last_error;
static thread_local std::string g_last_conv_kernel;  // mi355_last_conv_kernel(): which instantiation a single-op conv call ran

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

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

using namespace mi355;

struct mi355_unet {
    int in_channels = 0, cin_pad = 0, num_classes = 0, num_pool = 0;
    int norm = 0, num_groups = 0, nonlin_first = 0, dtype = 0;
    float eps = 1e-5f, slope = 0.01f;
    std::vector<std::vector<ConvLayer>> enc;  // num_pool + 1 stages
    std::vector<std::vector<ConvLayer>> dec;  // num_pool stages
    std::vector<TConvWeights> tu;
    std::vector<TConvWeightsH> tuh;
    HeadWeights head;
    // (the activation arena is not the handle's: one per LANE = per stream the caller launches on, shared by every handle that
    //  runs on that stream - device_scratch(SCR_ARENA, stream); a forward carries its pointer in its Plan)
    // gaussian importance map cache
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

static std::mutex g_mu;
static int g_bound_device = -1;
static bool is_gfx950(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

int bind_device() {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0) {
        set_error("no HIP device visible (%s); this library has no CPU fallback", e == hipSuccess ? "none current" : hipGetErrorString(e));
        return MI355_ERR_NO_DEVICE;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_bound_device < 0) {
        if (!is_gfx950(dev)) {
            set_error("HIP device %d is not gfx950 (MI355X); this library has no other code path", dev);
            return MI355_ERR_NO_DEVICE;
        }
        g_bound_device = dev;
    } else if (g_bound_device != dev) {
        set_error("this process is bound to HIP device %d but device %d is current: one process per GPU (weights, arena and "
                  "scratch live on the bound device)", g_bound_device, dev);
        return MI355_ERR_INVALID;
    }
    return MI355_OK;
}

// Lanes (round 5).  Scratch is per STREAM: the first MAX_LANES distinct streams the caller launches on get a lane of their own -
// activation arena, aggregation buffers, split-K partials, small reduction scratch - so that independent pieces of the work (the two
// ensemble members, or two halves of one member's (fold, tile) list: predictor.predict_folds(lanes = 2)) can be in flight on two
// streams at once: the HBM-bound kernels of one lane (norm passes, transposed convs, first layer, aggregation: a sixth of a
// config-3 step) then run beside the matrix-bound kernels of the other instead of in front of them.  Work on ONE stream is ordered
// by that stream, as before.  A stream beyond the table takes over the least recently used lane after a device synchronise.
// SCR_ZEROS / SCR_ZERO_BIAS are read-only once cleared and shared by all lanes.
constexpr int MAX_LANES = MI355_SCRATCH_LANES;
static struct { void *p; size_t bytes; } g_scratch[MAX_LANES][SCR_COUNT];
static struct { hipStream_t s; bool used; unsigned long tick; } g_lane[MAX_LANES];
static unsigned long g_lane_tick = 0;

static int lane_of_locked(hipStream_t s, int *lane) {
    int free_lane = -1, lru = 0;
    for (int i = 0; i < MAX_LANES; ++i) {
        if (g_lane[i].used && g_lane[i].s == s) { g_lane[i].tick = ++g_lane_tick; *lane = i; return MI355_OK; }
        if (!g_lane[i].used && free_lane < 0) free_lane = i;
        if (g_lane[i].used && g_lane[i].tick < g_lane[lru].tick) lru = i;
    }
    if (free_lane < 0) {
        MI355_HIP(hipDeviceSynchronize());  // whatever still runs on the evicted stream's scratch
        free_lane = lru;
    }
    g_lane[free_lane].s = s; g_lane[free_lane].used = true; g_lane[free_lane].tick = ++g_lane_tick;
    *lane = free_lane;
    return MI355_OK;
}

int device_scratch(int slot, hipStream_t stream, size_t bytes, void **out, bool zeroed) {
    MI355_REQUIRE(slot >= 0 && slot < SCR_COUNT && out, "bad scratch slot %d", slot);
    MI355_TRY(bind_device());
    std::lock_guard<std::mutex> lk(g_mu);
    int lane = 0;
    if (slot != SCR_ZEROS && slot != SCR_ZERO_BIAS) MI355_TRY(lane_of_locked(stream, &lane));
    auto &b = g_scratch[lane][slot];
    if (b.bytes < bytes) {
        if (b.p) {
            MI355_HIP(hipDeviceSynchronize());  // work in flight may still use the old buffer
            MI355_HIP(hipFree(b.p));
            b.p = nullptr; b.bytes = 0;
        }
        MI355_HIP(hipMalloc(&b.p, bytes));
        b.bytes = bytes;
        if (zeroed) MI355_HIP(hipMemset(b.p, 0, bytes));
    }
    *out = b.p;
    return MI355_OK;
}

// Test aids (mi355_nnunet.h, "Device scratch, for tests"): look at, overwrite and drop what device_scratch hands out.  Host code.
static bool scratch_slot_shared(int slot) { return slot == SCR_ZEROS || slot == SCR_ZERO_BIAS; }
static int lane_peek_locked(hipStream_t s) {  // the lane of a stream, or -1: claims nothing, touches no tick
    for (int i = 0; i < MAX_LANES; ++i)
        if (g_lane[i].used && g_lane[i].s == s) return i;
    return -1;
}

extern "C" int mi355_scratch_sizes(void *stream, int64_t *bytes, int n) {
    MI355_REQUIRE(n >= 0 && (bytes || n == 0), "mi355_scratch_sizes: bad arguments");
    std::lock_guard<std::mutex> lk(g_mu);
    const int lane = lane_peek_locked((hipStream_t)stream);
    for (int slot = 0; slot < SCR_COUNT && slot < n; ++slot) {
        if (scratch_slot_shared(slot)) bytes[slot] = (int64_t)g_scratch[0][slot].bytes;
        else bytes[slot] = lane < 0 ? 0 : (int64_t)g_scratch[lane][slot].bytes;
    }
    return SCR_COUNT;
}

extern "C" int64_t mi355_scratch_fill(void *stream, int slot, uint32_t word) {
    MI355_REQUIRE(slot >= -1 && slot < SCR_COUNT, "mi355_scratch_fill: bad scratch slot %d", slot);
    MI355_REQUIRE(slot < 0 || !scratch_slot_shared(slot), "mi355_scratch_fill: slot %d is a shared zero page", slot);
    MI355_TRY(bind_device());
    std::lock_guard<std::mutex> lk(g_mu);
    const int lane = lane_peek_locked((hipStream_t)stream);
    if (lane < 0) return 0;
    int64_t filled = 0;
    for (int i = 0; i < SCR_COUNT; ++i) {
        if (scratch_slot_shared(i) || (slot >= 0 && i != slot)) continue;
        auto &b = g_scratch[lane][i];
        if (!b.p || b.bytes < 4) continue;
        MI355_HIP(hipMemsetD32Async((hipDeviceptr_t)b.p, (int)word, b.bytes / 4, (hipStream_t)stream));
        filled += (int64_t)(b.bytes / 4 * 4);
    }
    return filled;
}

extern "C" int mi355_scratch_release(void *stream) {
    MI355_TRY(bind_device());
    std::lock_guard<std::mutex> lk(g_mu);
    const int lane = lane_peek_locked((hipStream_t)stream);
    if (lane < 0) return MI355_OK;
    MI355_HIP(hipDeviceSynchronize());  // work in flight may still use the buffers
    for (int i = 0; i < SCR_COUNT; ++i) {
        if (scratch_slot_shared(i)) continue;  // (lane 0 also holds the zero pages of every lane)
        auto &b = g_scratch[lane][i];
        if (b.p) MI355_HIP(hipFree(b.p));
        b.p = nullptr; b.bytes = 0;
    }
    g_lane[lane].used = false; g_lane[lane].s = nullptr; g_lane[lane].tick = 0;
    return MI355_OK;
}

extern "C" int mi355_scratch_zero_pages(int64_t *nonzero_bytes) {
    MI355_REQUIRE(nonzero_bytes, "mi355_scratch_zero_pages: null output");
    const int slots[2] = {SCR_ZEROS, SCR_ZERO_BIAS};
    nonzero_bytes[0] = nonzero_bytes[1] = 0;
    std::lock_guard<std::mutex> lk(g_mu);
    for (int k = 0; k < 2; ++k) {
        auto &b = g_scratch[0][slots[k]];
        if (!b.p) continue;
        MI355_HIP(hipDeviceSynchronize());
        std::vector<unsigned char> host(b.bytes);
        MI355_HIP(hipMemcpy(host.data(), b.p, b.bytes, hipMemcpyDeviceToHost));
        for (unsigned char v : host) nonzero_bytes[k] += v != 0;
    }
    return MI355_OK;
}

static int require_device() { return bind_device(); }

static int upload(const float *host, size_t n, float **dev) {
    MI355_HIP(hipMalloc(dev, n * sizeof(float)));
    MI355_HIP(hipMemcpy(*dev, host, n * sizeof(float), hipMemcpyHostToDevice));
    return MI355_OK;
}

// The network side of the shared skip half ("shared skip half" below): what is known of the first block of the last decoder stage
// when the network is created, when a sliding window decides, and in the dry run - one description, one predicate.
struct SkipShareNet {
    int dtype = MI355_F32;
    int r = 0;                     // stage0_blocks
    int stride = 1;                // of the last decoder stage's first block
    bool runtime_norm = false, post_affine = false;
    bool skip_is_enc0 = true;      // its second input is enc[0]'s output
    int c_up = 0, c_skip = 0, cout = 0;
    int head_ncls = 0;             // > 0: the block is also the stage's only one, i.e. the net's last conv, which may carry the fused head
};
static SkipShareNet skip_share_net_of(int dtype, int r, int stride, int norm, int nonlin_first, int c_up, int c_skip, int cout, int head_ncls) {
    SkipShareNet d;
    d.dtype = dtype; d.r = r; d.stride = stride;
    d.runtime_norm = norm == MI355_NORM_INSTANCE || norm == MI355_NORM_GROUP;
    d.post_affine = norm == MI355_NORM_BATCH && nonlin_first;
    d.c_up = c_up; d.c_skip = c_skip; d.cout = cout; d.head_ncls = head_ncls;
    return d;
}
static bool skip_share_network_ok(const SkipShareNet &d);
static int stage0_blocks(const mi355_unet &net);

// half != nullptr (the first block of the last decoder stage, which reads the virtual concat (upsampled, skip)): when the network
// qualifies for the shared skip half (skip_share_network_ok, the predicate the sliding window decides by) the block also gets the
// packs of its two halves, each through conv_weights_upload and so through conv_pack_layout like any layer: the same fp64
// Winograd transform, rounded once.
static int build_conv(const mi355_unet &net, const mi355_conv_desc &d, int cin_phys, ConvLayer *out, bool stem = false, const SkipShareNet *half = nullptr) {
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
            MI355_TRY(upload(sc.data(), d.cout, &L.gamma_dev));
            MI355_TRY(upload(sh.data(), d.cout, &L.beta_dev));
        }
    } else if (net.norm == MI355_NORM_INSTANCE || net.norm == MI355_NORM_GROUP) {
        L.runtime_norm = true;
        std::vector<float> g(d.cout, 1.f), be(d.cout, 0.f);
        if (d.gamma) g.assign(d.gamma, d.gamma + d.cout);
        if (d.beta) be.assign(d.beta, d.beta + d.cout);
        MI355_TRY(upload(g.data(), d.cout, &L.gamma_dev));
        MI355_TRY(upload(be.data(), d.cout, &L.beta_dev));
    }
    if (stem) { L.is_stem = true; MI355_TRY(stem_weights_upload(w.data(), b.data(), d.cin, d.cout, net.dtype, &L.stem)); }
    else if (net.dtype == MI355_F16) MI355_TRY(conv_weights_upload_f16(w.data(), b.data(), d.cin, cin_phys, d.cout, d.stride, &L.wh));
    else MI355_TRY(conv_weights_upload(w.data(), b.data(), d.cin, cin_phys, d.cout, d.stride, false, &L.w));
    if (half && !stem && cin_phys == d.cin && half->c_up + half->c_skip == d.cin && skip_share_network_ok(*half)) {
        const int split_c0 = half->c_up, c_skip = half->c_skip;
        {
            std::vector<float> wu((size_t)d.cout * split_c0 * 27), ws((size_t)d.cout * c_skip * 27);
            for (int co = 0; co < d.cout; ++co) {
                const float *src = &w[(size_t)co * d.cin * 27];
                std::copy(src, src + (size_t)split_c0 * 27, &wu[(size_t)co * split_c0 * 27]);
                std::copy(src + (size_t)split_c0 * 27, src + (size_t)d.cin * 27, &ws[(size_t)co * c_skip * 27]);
            }
            MI355_TRY(conv_weights_upload(wu.data(), b.data(), split_c0, split_c0, d.cout, 1, false, &L.w_up));
            MI355_TRY(conv_weights_upload(ws.data(), nullptr, c_skip, c_skip, d.cout, 1, false, &L.w_skip));
            L.split_c0 = split_c0;
        }
    }
    *out = L;
    return MI355_OK;
}

static void free_conv(ConvLayer *L) {
    conv_weights_free(&L->w);
    conv_weights_free(&L->w_up);
    conv_weights_free(&L->w_skip);
    conv_weights_free_f16(&L->wh);
    stem_weights_free(&L->stem);
    if (L->gamma_dev) (void)hipFree(L->gamma_dev);
    if (L->beta_dev) (void)hipFree(L->beta_dev);
}

static void destroy(mi355_unet *net) {
    if (!net) return;
    for (auto &st : net->enc) for (auto &L : st) free_conv(&L);
    for (auto &st : net->dec) for (auto &L : st) free_conv(&L);
    for (auto &t : net->tu) tconv_weights_free(&t);
    for (auto &t : net->tuh) tconv_weights_free_f16(&t);
    head_weights_free(&net->head);
    if (net->gauss_dev) (void)hipFree(net->gauss_dev);
    for (auto &r : net->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (hipEvent_t e : net->event_pool) (void)hipEventDestroy(e);
    delete net;
}

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
};

static int make_plan(const mi355_unet &net, int N, int D, int H, int W, Plan *pl) {
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
        pl->maxc[l] = std::max(pl->maxc[l], net.dtype == MI355_F16 ? net.tuh[u].cout : net.tu[u].cout);
        for (auto &L : net.dec[u]) pl->maxc[l] = std::max(pl->maxc[l], L.cout);
    }
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~size_t(255); return r; };
    const size_t es = net.dtype == MI355_F16 ? 2 : 4;
    pl->x0_off = take((size_t)N * pl->vox[0] * net.cin_pad * es);
    for (int k = 0; k < 4; ++k) pl->off[k].resize(np + 1);
    for (int l = 0; l <= np; ++l)
        for (int k = 0; k < 4; ++k)
            pl->off[k][l] = take((size_t)N * pl->vox[l] * pl->maxc[l] * es);
    pl->stats_bytes = (size_t)N * net.max_channels * 2 * sizeof(double);
    pl->stats_off = take(pl->stats_bytes);
    pl->scale_off = take((size_t)N * net.max_channels * sizeof(float));
    pl->shift_off = take((size_t)N * net.max_channels * sizeof(float));
    pl->scale2_off = take((size_t)N * net.max_channels * sizeof(float));
    pl->shift2_off = take((size_t)N * net.max_channels * sizeof(float));
    pl->total = o;
    return MI355_OK;
}

static int ensure_arena(Plan *pl, hipStream_t s) {
    void *p = nullptr;
    MI355_TRY(device_scratch(SCR_ARENA, s, pl->total, &p));
    pl->arena = (char *)p;
    return MI355_OK;
}

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
namespace {
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
}  // namespace

// The call struct of one conv: x0 holds the first cin - f.c1 channels, f the fused operands.
template <typename T>
static ConvCallT<T> make_call(const void *x0, int cin, int N, int Di, int Hi, int Wi, void *out, double *stats, int act, float slope,
                              const FusedOps &f = FusedOps()) {
    ConvCallT<T> c;
    c.in0 = (const T *)x0; c.C0 = cin - f.c1; c.in1 = (const T *)f.x1; c.C1 = f.c1;
    c.N = N; c.Di = Di; c.Hi = Hi; c.Wi = Wi; c.out = (T *)out; c.act = act; c.slope = slope;
    c.stats = stats;
    c.in_scale = f.in_scale; c.in_shift = f.in_shift; c.in_act = f.in_act;
    c.head_w = f.head_w; c.head_b = f.head_b; c.head_out = f.head_out; c.head_ncls = f.head_ncls;
    return c;
}

// One ConvDropoutNormNonlin / ConvDropoutNonlinNorm block.
// `defer_norm`: the block's normalisation (+ activation) is NOT applied to `out`; its per-(sample, channel) scale / shift go
// to the plan's second pair and the NEXT block applies them while staging its input (`in_norm` of that call).
static int run_block(mi355_unet *net, const Plan &pl, const ConvLayer &L, const void *in0, int C0,
                     const void *in1, int C1, int N, int Di, int Hi, int Wi, void *out, hipStream_t s,
                     float *head_logits_out = nullptr, bool defer_norm = false, bool in_norm = false,
                     const ConvWeights *half = nullptr, const float *addend = nullptr, const char *half_name = "",
                     const S0View *in0_view = nullptr, const S0View *addend_view = nullptr) {
    // `half` (fp32, shared skip half): the launch runs with these weights instead of L's - one half of L's input channels, C0 + C1
    // of them - and `addend` [N][Vo][cout] is added in front of bias and activation; reported under the kernel's name + half_name
    const bool f16 = net->dtype == MI355_F16;
    MI355_REQUIRE(!half || (!f16 && !L.is_stem && !L.runtime_norm && !L.post_affine && half->cin == C0 + C1), "conv %d->%d: bad half launch", L.cin, L.cout);
    MI355_REQUIRE((!in0_view && !addend_view) || (!f16 && !L.is_stem), "conv %d->%d: a stage-0 view on a launch that cannot take one", L.cin, L.cout);
    double *stats = (double *)(pl.arena + pl.stats_off);
    float *scale = (float *)(pl.arena + (defer_norm ? pl.scale2_off : pl.scale_off)), *shift = (float *)(pl.arena + (defer_norm ? pl.shift2_off : pl.shift_off));
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
        const int cin = half ? half->cin : L.cin;
        const double flops = 2.0 * N * Vo * L.cout * (double)cin * 27.0;
        const double bytes = es * ((double)N * Di * Hi * Wi * (C0 + C1) + (addend ? 2.0 : 1.0) * N * Vo * L.cout + (double)L.cout * cin * 27.0);
        FusedOps f;
        f.x1 = in1; f.c1 = C1;
        if (head_logits_out) { f.head_w = net->head.w_dev; f.head_b = net->head.b_dev; f.head_ncls = net->head.ncls; f.head_out = head_logits_out; }
        if (in_norm) {  // in0 is the previous block's raw conv output: normalise (+ LeakyReLU) while staging (fp32: the F(2x2x2,3x3x3) kernel, in LDS)
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
            ConvCall c = make_call<float>(in0, C0 + C1, N, Di, Hi, Wi, out, stats_arg, half && !addend ? ACT_NONE : act, net->slope, f);
            c.addend = addend;
            c.in0_view = in0_view; c.addend_view = addend_view;  // (stage-0 views: the caller asked the planner first)
            const ConvWeights &W = half ? *half : L.w;
            ProfScope ps(net, s, "conv3_direct_kernel", flops, bytes);  // (renamed to the instantiation the MFMA dispatch picks)
            if (W.wp_dev) MI355_TRY(conv3d_mfma_f32(W, c, s, &kname));
            else MI355_TRY(conv3d_direct_f32(W, c, s));
            ps.rename(kname, half_name);
        }
    }
    if (half) return MI355_OK;
    const double es = f16 ? 2.0 : 4.0;
    if (L.runtime_norm) {
        MI355_TRY(norm_finalize(stats, N, L.cout, Vo, net->norm, net->num_groups, net->eps, L.gamma_dev, L.beta_dev,
                                scale, shift, s));
        if (defer_norm) return MI355_OK;  // the consumer applies scale / shift (and the activation) in its staging
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
// after_enc0 (shared stage 0): the level-0 features are already where enc[0]'s last block writes them; the pass starts at level 1.
// skip_half (shared skip half): [N][V][cout] = the skip half of the last decoder stage's first conv, already gathered into the
// level-0 buffer that stage leaves free; that block then runs over the upsampled tensor alone and adds it in its epilogue.
// enc0_view / skip_half_view (stage-0 views): the level-0 features / the skip half hold their shells only; their one reader - the
// first block of level 1 / that epilogue - takes the rest through the view.
static int forward_features(mi355_unet *net, const Plan &pl, int N, int D, int H, int W, const void **feat,
                            int *feat_c, hipStream_t s, bool *is_logits = nullptr, float *logits_target = nullptr,
                            FeatNorm *head_norm = nullptr, bool after_enc0 = false, const float *skip_half = nullptr,
                            const S0View *enc0_view = nullptr, const S0View *skip_half_view = nullptr) {
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
        if (l == 0 && after_enc0) { cur = buf((int)((net->enc[0].size() - 1) & 1), 0); curC = net->enc[0].back().cout; }
        for (size_t i = 0; i < net->enc[l].size() && !(l == 0 && after_enc0); ++i) {
            const ConvLayer &L = net->enc[l][i];
            int inD = Di, inH = Hi, inW = Wi;
            if (L.stride == 2) { inD = Di * 2; inH = Hi * 2; inW = Wi * 2; }
            void *out = buf((int)(i & 1), l);
            const bool defer = i + 1 < net->enc[l].size() && can_defer_norm(net, L, net->enc[l][i + 1], N, Di, Hi, Wi);
            const S0View *view = (l == 1 && i == 0 && after_enc0) ? enc0_view : nullptr;
            MI355_TRY(run_block(net, pl, L, cur, curC, nullptr, 0, N, inD, inH, inW, out, s, nullptr, defer, pending, nullptr, nullptr, "", view));
            pending = defer;
            cur = out; curC = L.cout;
        }
        if (l < np) { skip[l] = cur; skipC[l] = curC; }
    }
    MI355_REQUIRE(!enc0_view || (skip_half && np >= 1), "stage-0 view of the level-0 features while the decoder reads them whole");
    // decoder
    for (int u = 0; u < np; ++u) {
        const int l = np - 1 - u;
        const int Dl = D >> l, Hl = H >> l, Wl = W >> l;
        void *up = buf(2, l);
        const int tcin = f16 ? net->tuh[u].cin : net->tu[u].cin, tcout = f16 ? net->tuh[u].cout : net->tu[u].cout;
        MI355_REQUIRE(tcin == curC, "tu.%d expects %d channels, got %d", u, tcin, curC);
        {
            const double es = f16 ? 2.0 : 4.0;
            const double vin = (double)N * (Dl / 2) * (Hl / 2) * (Wl / 2);
            ProfScope ps(net, s, f16 ? "tconv2_f16_mfma_v2_kernel" : "tconv2_f32_mfma_v2_kernel", 2.0 * vin * tcin * tcout * 8.0,
                         es * (vin * tcin + 8.0 * vin * tcout + 8.0 * tcin * tcout));
            const char *tname = nullptr;
            if (f16) { MI355_TRY(tconv2_mfma_f16(net->tuh[u], (const _Float16 *)cur, N, Dl / 2, Hl / 2, Wl / 2, (_Float16 *)up, s, &tname)); ps.rename(tname); }
            else { MI355_TRY(tconv2_mfma_f32(net->tu[u], (const float *)cur, N, Dl / 2, Hl / 2, Wl / 2, (float *)up, s, &tname)); ps.rename(tname); }
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
            const bool last = is_logits && (u == np - 1) && (i + 1 == net->dec[u].size());
            const int lnf = f16 ? L.wh.nf : L.w.nf;
            const bool has_pack = f16 ? (L.wh.wp_dev != nullptr) : (L.w.wp_dev != nullptr);
            if (last && fuse && !L.runtime_norm && !L.post_affine && has_pack && L.cout == 32 * lnf && net->head.ncls <= 4 &&
                net->head.cin == L.cout && (!f16 || lnf == 1)) {
                float *lg = logits_target ? logits_target : (float *)out;
                MI355_TRY(run_block(net, pl, L, in0, C0, in1, C1, N, Dl, Hl, Wl, nullptr, s, lg, false, pending_d));  // (a pending norm is refused loudly by the fused-head conv: ADVICE r2)
                *is_logits = true;
                *feat = lg; *feat_c = net->head.ncls;
                return MI355_OK;
            }
            if (skip_half && u == np - 1 && i == 0) {
                MI355_REQUIRE(L.split_c0 == C0 && (const void *)skip_half == freeAB, "shared skip half: the block was not split at %d channels", C0);
                MI355_TRY(run_block(net, pl, L, in0, C0, nullptr, 0, N, Dl, Hl, Wl, out, s, nullptr, false, false, &L.w_up, skip_half, " up-half", nullptr, skip_half_view));
                in0 = out; C0 = L.cout; in1 = nullptr; C1 = 0;
                continue;
            }
            const bool to_head = env_switch("MI355_FUSE_NORM") && head_norm && L.runtime_norm && (u == np - 1) && (i + 1 == net->dec[u].size());
            const bool defer = to_head || (i + 1 < net->dec[u].size() && can_defer_norm(net, L, net->dec[u][i + 1], N, Dl, Hl, Wl));
            MI355_TRY(run_block(net, pl, L, in0, C0, in1, C1, N, Dl, Hl, Wl, out, s, nullptr, defer, pending_d));
            if (to_head) {
                head_norm->scale = (const float *)(pl.arena + pl.scale2_off);
                head_norm->shift = (const float *)(pl.arena + pl.shift2_off);
                head_norm->slope = net->nonlin_first ? 1.0f : net->slope;  // ConvDropoutNonlinNorm: the activation came before the norm
            }
            pending_d = defer;
            in0 = out; C0 = L.cout; in1 = nullptr; C1 = 0;
        }
        cur = in0; curC = C0;
    }
    if (is_logits) *is_logits = false;
    *feat = cur; *feat_c = curC;
    return MI355_OK;
}

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

static int ensure_gaussian(mi355_unet *net, const int p[3]) {
    std::lock_guard<std::mutex> lk(g_mu);  // (one handle may be driven from two lanes)
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

// blocks of enc[0] when the network allows the shared stage 0, else 0
static int stage0_blocks(const mi355_unet &net) {
    if (!env_switch("MI355_SHARE_STAGE0") || net.dtype != MI355_F32) return 0;
    for (const ConvLayer &L : net.enc[0])
        if (L.stride != 1 || L.runtime_norm || L.post_affine || L.cout % 4) return 0;  // (Instance/GroupNorm statistics are per tile; the mask and gather kernels move 16 bytes per lane)
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
static bool skip_share_network_ok(const SkipShareNet &d) {
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
    ConvWeights cw;
    cw.cin = cw.cin_pad = d.c_up; cw.cout = d.cout; cw.stride = 1;
    cw.cc = lu.cc; cw.nf = lu.nf; cw.pipe = lu.pipe;
    cw.bias_dev = cw.wp_dev = cw.wp16_dev = cw.wpw_dev = cw.wp3_dev = stand_in;  // (lu.wino3 implies the other packs)
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

// enc[0] over n boxes of S voxels each, gathered from the volume: `in` receives the input, the last block writes `out`.
// group > 0: the convs run as launches of exactly `group` boxes each (n is a multiple of it).
// label: suffix of the gather's profile entry (the merged slabs name theirs).
// skip_off != 0 (shared skip half): one more launch behind the last block - the skip half of the last decoder stage's first conv,
// zero bias, no activation - writes S there.
static int stage0_run(mi355_unet *net, const Plan &pl, const float *vol, int Z, int Y, int X, const SwGeom &g, const std::vector<TileDesc> &boxes,
                      const int S[3], const int *mask_zp, int group, size_t in_off, const size_t tmp_off[2], size_t out_off, size_t skip_off, hipStream_t s,
                      const char *label = "") {
    const int n = (int)boxes.size();
    const size_t vox = (size_t)S[0] * S[1] * S[2];
    for (int b0 = 0; b0 < n; b0 += S0_MAX_SAMPLES) {
        const int nb = std::min(S0_MAX_SAMPLES, n - b0);
        ProfScope ps(net, s, std::string("extract_tiles_kernel") + label, 0.0, (double)nb * vox * 4.0 * (net->in_channels + net->cin_pad));
        MI355_TRY(extract_tiles(vol, net->in_channels, Z, Y, X, g.pad_lo[0], g.pad_lo[1], g.pad_lo[2], boxes.data() + b0, nb, S[0], S[1], S[2],
                                net->cin_pad, (void *)(pl.arena + in_off + (size_t)b0 * vox * net->cin_pad * 4), net->dtype, s));
    }
    const int ng = group > 0 ? group : n;
    MI355_REQUIRE(n % ng == 0, "shared stage 0: %d boxes in launches of %d", n, ng);
    for (int g0 = 0; g0 < n; g0 += ng) {
        const void *cur = pl.arena + in_off + (size_t)g0 * vox * net->cin_pad * 4;
        int curC = net->cin_pad;
        for (size_t i = 0; i < net->enc[0].size(); ++i) {
            const ConvLayer &L = net->enc[0][i];
            const bool last = i + 1 == net->enc[0].size();
            void *out = pl.arena + (last ? out_off : tmp_off[i & 1]) + (size_t)g0 * vox * L.cout * 4;
            MI355_TRY(run_block(net, pl, L, cur, curC, nullptr, 0, ng, S[0], S[1], S[2], out, s));
            if ((!last || skip_off) && mask_zp) {
                // the next conv must see zero padding outside the padded volume, not act(bias)
                const double outside = (double)ng * (vox - (double)mask_zp[0] * mask_zp[1] * mask_zp[2]);
                ProfScope ps(net, s, "stage0_mask_kernel", 0.0, outside * L.cout * 4.0);
                MI355_TRY(stage0_mask((float *)out, ng, S, mask_zp, L.cout, s));
            }
            cur = out; curC = L.cout;
        }
        if (skip_off) {
            const ConvLayer &Ld = net->dec.back()[0];
            MI355_TRY(run_block(net, pl, Ld, cur, curC, nullptr, 0, ng, S[0], S[1], S[2], pl.arena + skip_off + (size_t)g0 * vox * Ld.cout * 4, s,
                                nullptr, false, false, &Ld.w_skip, nullptr, " skip-half"));
        }
    }
    return MI355_OK;
}

// whole-volume pass: one box per mirror
static int stage0_whole(mi355_unet *net, const Plan &pl, const float *vol, int Z, int Y, int X, const SwGeom &g, const S0Geom &sg, hipStream_t s) {
    std::vector<TileDesc> boxes;
    const int zero[3] = {0, 0, 0};
    // (a flipped axis: the flipped volume starts at 0 and its zero extension follows it, as on an unflipped axis)
    for (int m : g.mirrors) boxes.push_back(pass_box(g, m, zero, sg.Ve));
    const bool extended = sg.Ve[0] != g.Zp[0] || sg.Ve[1] != g.Zp[1] || sg.Ve[2] != g.Zp[2];
    return stage0_run(net, pl, vol, Z, Y, X, g, boxes, sg.Ve, extended ? g.Zp : nullptr, 0, pl.s0.wv_in, pl.s0.wv_tmp, pl.s0.wv_out, pl.s0.wv_skip, s);
}

// merged y- and x-slabs: every key, one launch group per axis (stage0_merge_geometry)
static int stage0_merged(mi355_unet *net, const Plan &pl, const float *vol, int Z, int Y, int X, const SwGeom &g, const S0Geom &sg, hipStream_t s) {
    for (int a = 1; a < 3; ++a) {
        if (sg.merged[a].empty()) continue;
        std::vector<TileDesc> boxes;
        for (const S0Merged &k : sg.merged[a]) boxes.push_back(pass_box(g, g.mirrors[k.wv], k.org, sg.mdim[a]));
        // along the axes a slab spans the extended volume it holds [Zp, Ve), which is zero in front of every conv
        const int keep[3] = {g.Zp[0], a == 1 ? sg.mdim[a][1] : g.Zp[1], sg.mdim[a][2]};
        const bool extended = keep[0] != sg.mdim[a][0] || keep[1] != sg.mdim[a][1];
        MI355_TRY(stage0_run(net, pl, vol, Z, Y, X, g, boxes, sg.mdim[a], extended ? keep : nullptr, 0, pl.s0.slab_in, pl.s0.slab_tmp, pl.s0.slab_out[a],
                             pl.s0.slab_skip[a], s, " merged-slabs"));
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
static int stage0_tiles(mi355_unet *net, const Plan &pl, const float *vol, int Z, int Y, int X, const SwGeom &g, const S0Geom &sg,
                        const std::vector<int> &samples, hipStream_t s, S0ViewChoice want = S0ViewChoice(), S0View *enc0_view = nullptr,
                        S0View *half_view = nullptr) {
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
        MI355_TRY(stage0_run(net, pl, vol, Z, Y, X, g, boxes, S, nullptr, S0_SLAB_GROUP, pl.s0.slab_in, pl.s0.slab_tmp, pl.s0.slab_out[a], pl.s0.slab_skip[a], s));
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

static int sw_accumulate(mi355_unet *net, const float *vol, int Z, int Y, int X, const mi355_sw_opts &o,
                         const SwGeom &g, int rank, int world, float *agg, float *cnt, hipStream_t s, long first_item = 0) {
    const int nm = (int)g.mirrors.size();
    const bool use_gauss = o.use_gaussian && g.tiles.size() > 1;
    if (use_gauss) MI355_TRY(ensure_gaussian(net, g.P));
    std::vector<int> mine;
    for (size_t t = 0; t < g.tiles.size(); ++t) if ((int)((first_item + (long)t) % world) == rank) mine.push_back((int)t);
    const int bt = sw_batch_tiles(net->dtype, o.batch_tiles, nm);
    MI355_REQUIRE(nm <= 64, "too many mirrors");
    Plan pl;
    MI355_TRY(make_plan(*net, bt * nm, g.P[0], g.P[1], g.P[2], &pl));
    S0Geom sg;
    const bool share_skip = skip_share_decide(skip_share_net(*net), g);
    stage0_geometry(g, stage0_blocks(*net), &sg, share_skip ? 1 : 0);
    if (env_switch("MI355_MERGE_SLABS")) stage0_merge_geometry(g, &sg);
    if (sg.shared) stage0_plan(*net, g, sg, bt * nm, &pl);
    MI355_TRY(ensure_arena(&pl, s));
    if (mine.empty()) return MI355_OK;
    if (sg.shared) MI355_TRY(stage0_whole(net, pl, vol, Z, Y, X, g, sg, s));
    if (sg.merge) MI355_TRY(stage0_merged(net, pl, vol, Z, Y, X, g, sg, s));
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
        S0View enc0_view, half_view;
        if (sg.shared) {
            const S0ViewChoice want = stage0_views_decide(*net, sg, share_skip, (int)samples.size(), g.P);
            MI355_TRY(stage0_tiles(net, pl, vol, Z, Y, X, g, sg, sample_ids, s, want, &enc0_view, &half_view));
        } else {
        const double pv = (double)samples.size() * g.P[0] * g.P[1] * g.P[2];
        ProfScope ps(net, s, "extract_tiles_kernel", 0.0, pv * (4.0 * net->in_channels + (net->dtype == MI355_F16 ? 2.0 : 4.0) * net->cin_pad));
        MI355_TRY(extract_tiles(vol, net->in_channels, Z, Y, X, g.pad_lo[0], g.pad_lo[1], g.pad_lo[2], samples.data(),
                                (int)samples.size(), g.P[0], g.P[1], g.P[2], net->cin_pad,
                                (void *)(pl.arena + pl.x0_off), net->dtype, s));
        }
        const void *feat; int fc; bool is_logits = false;
        FeatNorm head_norm;
        MI355_TRY(forward_features(net, pl, (int)samples.size(), g.P[0], g.P[1], g.P[2], &feat, &fc, s, &is_logits, nullptr, &head_norm, sg.shared,
                                   share_skip ? (const float *)(pl.arena + pl.off[((net->enc[0].size() - 1) & 1) ^ 1][0]) : nullptr,
                                   enc0_view.src ? &enc0_view : nullptr, half_view.src ? &half_view : nullptr));
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

// =============================================================================== C ABI
extern "C" const char *mi355_last_error(void) { return g_last_error.c_str(); }
extern "C" const char *mi355_last_conv_kernel(void) { return g_last_conv_kernel.c_str(); }
extern "C" int mi355_version(void) { return 102; }
extern "C" int mi355_device_count(void) {
    int n = 0, good = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    for (int d = 0; d < n; ++d) good += is_gfx950(d) ? 1 : 0;
    return good;
}

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
    if (d->dtype == MI355_F16) net->tuh.resize(d->num_pool); else net->tu.resize(d->num_pool);
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
        rc = d->dtype == MI355_F16 ? tconv_weights_upload_f16(td.weight, td.cin, td.cout, &net->tuh[u])
                                   : tconv_weights_upload(td.weight, td.cin, td.cout, &net->tu[u]);
        if (rc != MI355_OK) return fail(rc);
        net->max_channels = std::max(net->max_channels, td.cout);
        int inC = td.cout + skipC[l];
        if (d->dec_convs[u] < 1) { set_error("decoder stage %d has no convs", u); return fail(MI355_ERR_INVALID); }
        for (int i = 0; i < d->dec_convs[u]; ++i) {
            if (ci >= d->n_convs) { set_error("conv list too short"); return fail(MI355_ERR_INVALID); }
            const mi355_conv_desc &cd = d->convs[ci++];
            if (cd.stride != 1 || cd.cin != inC) { set_error("decoder conv %d.%d: cin %d stride %d, expected %d / 1", u, i, cd.cin, cd.stride, inC); return fail(MI355_ERR_INVALID); }
            ConvLayer L;
            const SkipShareNet half = skip_share_net_of(d->dtype, stage0_blocks(*net), cd.stride, d->norm, d->nonlin_first, td.cout, skipC[l], cd.cout,
                                                         d->dec_convs[u] == 1 ? d->num_classes : 0);
            rc = build_conv(*net, cd, inC, &L, false, (u == d->num_pool - 1 && i == 0) ? &half : nullptr);
            if (rc != MI355_OK) return fail(rc);
            net->dec[u].push_back(L);
            inC = cd.cout;
            net->max_channels = std::max(net->max_channels, cd.cout);
        }
        prevC = inC;
    }
    if (ci != d->n_convs) { set_error("%d convs given, topology uses %d", d->n_convs, ci); return fail(MI355_ERR_INVALID); }
    if (d->head.cin != prevC || d->head.num_classes != d->num_classes) { set_error("head: cin %d classes %d, expected %d / %d", d->head.cin, d->head.num_classes, prevC, d->num_classes); return fail(MI355_ERR_INVALID); }
    rc = head_weights_upload(d->head.weight, d->head.bias, d->head.cin, d->head.num_classes, &net->head);
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
        total += 2 * vox(l + 1) * (net->dtype == MI355_F16 ? (int64_t)net->tuh[u].cin * net->tuh[u].cout : (int64_t)net->tu[u].cin * net->tu[u].cout) * 8;
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
    MI355_TRY(forward_features(net, pl, n, d, h, w, &feat, &fc, s, &is_logits, logits_dev, &head_norm));
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
        MI355_TRY(sw_accumulate(nets[f], vol_dev, Z, Y, X, *opts, g, rank, world, agg_dev, f == 0 ? cnt_dev : nullptr, s,
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
        rc = sw_accumulate(nets[f], vol_dev, Z, Y, X, *opts, g, 0, 1, agg, cnt, s);
        if (rc == MI355_OK)
            rc = finish_probs(agg, cnt, C, Z, Y, X, g.Zp[0], g.Zp[1], g.Zp[2], g.pad_lo[0], g.pad_lo[1], g.pad_lo[2],
                              probs_dev, f > 0, s);
    }
    // fold mean: np.mean(list_of_fp32_arrays, axis=0) = fp32 running sum in list order, one divide
    if (rc == MI355_OK && n_nets > 1) rc = scale_inplace(probs_dev, (int64_t)C * Z * Y * X, (float)n_nets, s);
    // asynchronous on `stream` like every other entry point that takes one: probs_dev is valid in stream order
    return rc;
}

// The single-op fp16 entry points take and return PLAIN NDHWC tensors (include/mi355_nnunet.h); the kernels work on
// channel-blocked ones (common.h), so the operands pass through ndhwc_to_b8 / b8_to_ndhwc here.
namespace {
struct TmpBuf {
    void *p = nullptr;
    ~TmpBuf() { if (p) (void)hipFree(p); }
};
// the uploaded weights of a single-op call, freed on every exit
template <typename W, void (*FREE)(W *)>
struct TmpWeights {
    W w;
    ~TmpWeights() { FREE(&w); }
};
}  // namespace

// the network's first-layer kernel instead of the generic dispatch (plain NDHW4 input)
static bool single_op_stem(int cin, int stride, int impl, int cout, const FusedOps &f) {
    return cin == 4 && stride == 1 && impl == 0 && cout % 32 == 0 && !f.any();
}
// end of a single-op call: wait for the stream and report a kernel that failed asynchronously
static int synced(int rc, hipStream_t s, const char *what) {
    hipError_t e = hipStreamSynchronize(s);
    if (rc == MI355_OK && e != hipSuccess) { set_error("%s kernel failed: %s", what, hipGetErrorString(e)); rc = MI355_ERR_HIP; }
    return rc;
}

// Guard bands of the single-op fp16 entry points.  The fp16 kernels store into a channel-blocked buffer these entry points own,
// not into the caller's tensor, so a caller cannot see a store that misses it.  The buffer therefore sits between two bands of
// GUARD_BYTE - a sample's worth each, at most 4 MiB - that are read back after the launch: a byte changed there fails the call.
constexpr unsigned char GUARD_BYTE = 0xA5;
static size_t guard_bytes(size_t sample_bytes) {
    const size_t g = sample_bytes < 4096 ? 4096 : (sample_bytes > (4u << 20) ? (4u << 20) : sample_bytes);
    return (g + 255) / 256 * 256;  // (the buffer between the bands keeps hipMalloc's alignment to 256 B)
}
static int guards_intact(const void *buf, size_t guard, size_t bytes, const char *kernel) {
    std::vector<unsigned char> host(2 * guard);
    MI355_HIP(hipMemcpy(host.data(), buf, guard, hipMemcpyDeviceToHost));
    MI355_HIP(hipMemcpy(host.data() + guard, (const char *)buf + guard + bytes, guard, hipMemcpyDeviceToHost));
    size_t front = 0, behind = 0, first_behind = 0;
    for (size_t i = 0; i < guard; ++i) front += host[i] != GUARD_BYTE;
    for (size_t i = guard; i-- > 0;)
        if (host[guard + i] != GUARD_BYTE) { ++behind; first_behind = i; }
    if (front || behind) {
        set_error("%s stored outside its %zu-byte output: %zu bytes changed in front of it, %zu behind (first at +%zu)", kernel, bytes, front,
                  behind, first_behind);
        return MI355_ERR_HIP;
    }
    return MI355_OK;
}

// `sums` (device, [n][cout][2] doubles, zeroed here) != nullptr: the launch also carries the Instance/GroupNorm statistics
// epilogue (sum x, sum x^2 of its output per sample and channel) exactly as a run-time-norm block of the network does.
// `f` (optional): the fused operands of a network conv (ConvCall): the second half of a virtual concat, the producer's
// normalisation applied while staging, the 1x1x1 head.  They go to the dispatchers unchanged (mi355_conv3d_fused_ndhwc).
static int conv3d_ndhwc_f32_impl(const float *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                                 const float *bias_host, int cout, int stride, int act, float slope, int impl, float *y_dev,
                                 double *sums, void *stream, const FusedOps &f = FusedOps()) {
    MI355_TRY(require_device());
    MI355_REQUIRE(act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    MI355_REQUIRE(f.c1 >= 0 && f.c1 < cin && (f.c1 == 0) == (f.x1 == nullptr), "bad concat split %d of %d channels", f.c1, cin);
    hipStream_t s = (hipStream_t)stream;
    if (sums) MI355_HIP(hipMemsetAsync(sums, 0, (size_t)n * cout * 2 * sizeof(double), s));
    if (single_op_stem(cin, stride, impl, cout, f)) {
        TmpWeights<StemWeights, stem_weights_free> sw;
        MI355_TRY(stem_weights_upload(weight_host, bias_host, cin, cout, MI355_F32, &sw.w));
        g_last_conv_kernel = "conv3_stem_f32_kernel";
        return synced(conv3d_stem(sw.w, x_dev, n, d, h, w, y_dev, sums, act, slope, s), s, "stem conv");
    }
    TmpWeights<ConvWeights, conv_weights_free> cw;
    MI355_TRY(conv_weights_upload(weight_host, bias_host, cin, cin, cout, stride, impl == 1, &cw.w));
    const ConvCall c = make_call<float>(x_dev, cin, n, d, h, w, y_dev, sums, act, slope, f);
    MI355_REQUIRE(!sums || impl != 1, "the direct cross-check kernel carries no statistics epilogue");
    const char *kname = "conv3_direct_kernel";
    const int rc = (impl == 1) ? conv3d_direct_f32(cw.w, c, s) : conv3d_mfma_f32(cw.w, c, s, &kname);
    g_last_conv_kernel = kname ? kname : "";
    return synced(rc, s, "conv");
}

extern "C" int mi355_conv3d_ndhwc(const float *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                                  const float *bias_host, int cout, int stride, int act, float slope, int impl, float *y_dev,
                                  void *stream) {
    return conv3d_ndhwc_f32_impl(x_dev, n, d, h, w, cin, weight_host, bias_host, cout, stride, act, slope, impl, y_dev, nullptr, stream);
}

extern "C" int mi355_tconv3d_ndhwc(const float *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                                   int cout, float *y_dev, void *stream) {
    MI355_TRY(require_device());
    TmpWeights<TConvWeights, tconv_weights_free> tw;
    MI355_TRY(tconv_weights_upload(weight_host, cin, cout, &tw.w));
    const char *tname = "tconv2_f32_mfma_v2_kernel";
    const int rc = tconv2_mfma_f32(tw.w, x_dev, n, d, h, w, y_dev, (hipStream_t)stream, &tname);
    g_last_conv_kernel = tname;
    return synced(rc, (hipStream_t)stream, "tconv");
}

static int conv3d_ndhwc_f16_impl(const void *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                                 const float *bias_host, int cout, int stride, int act, float slope, void *y_dev,
                                 double *sums, void *stream, const FusedOps &f = FusedOps()) {
    MI355_TRY(require_device());
    MI355_REQUIRE(stride == 1 || stride == 2, "conv stride %d unsupported", stride);
    MI355_REQUIRE(act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    MI355_REQUIRE(f.c1 >= 0 && f.c1 < cin && (f.c1 == 0) == (f.x1 == nullptr), "bad concat split %d of %d channels", f.c1, cin);
    hipStream_t s = (hipStream_t)stream;
    if (sums) MI355_HIP(hipMemsetAsync(sums, 0, (size_t)n * cout * 2 * sizeof(double), s));
    const int64_t Vi = (int64_t)d * h * w;
    const int64_t Vo = (int64_t)((d - 1) / stride + 1) * ((h - 1) / stride + 1) * ((w - 1) / stride + 1);
    MI355_REQUIRE(cout % 8 == 0, "fp16 conv needs cout %% 8 == 0 (got %d)", cout);
    const size_t ybytes = (size_t)n * Vo * cout * 2, guard = guard_bytes((size_t)Vo * cout * 2);
    TmpBuf ybuf;  // guard band, the kernel's output, guard band (guards_intact)
    MI355_HIP(hipMalloc(&ybuf.p, ybytes + 2 * guard));
    struct { void *p; } yb = {(char *)ybuf.p + guard};
    MI355_HIP(hipMemsetAsync(ybuf.p, GUARD_BYTE, ybytes + 2 * guard, s));
    // all-NaN (0xFFFF) before the launch: a voxel the kernel fails to store cannot pass for a result
    MI355_HIP(hipMemsetAsync(yb.p, 0xFF, ybytes, s));
    int rc;
    if (single_op_stem(cin, stride, 0, cout, f)) {
        TmpWeights<StemWeights, stem_weights_free> sw;
        MI355_TRY(stem_weights_upload(weight_host, bias_host, cin, cout, MI355_F16, &sw.w));
        rc = conv3d_stem(sw.w, x_dev, n, d, h, w, yb.p, sums, act, slope, s);
        g_last_conv_kernel = "conv3_stem_f16_kernel";
        if (rc == MI355_OK) rc = b8_to_ndhwc((const _Float16 *)yb.p, n, cout, Vo, (_Float16 *)y_dev, s);
        rc = synced(rc, s, "stem conv");
        return rc == MI355_OK ? guards_intact(ybuf.p, guard, ybytes, g_last_conv_kernel.c_str()) : rc;
    }
    MI355_REQUIRE(cin % 8 == 0 && f.c1 % 8 == 0, "fp16 conv needs cin %% 8 == 0 on both inputs (got %d, %d)", cin - f.c1, f.c1);
    const int c0 = cin - f.c1;
    TmpBuf xb, x1b;
    MI355_HIP(hipMalloc(&xb.p, (size_t)n * Vi * c0 * 2));
    MI355_TRY(ndhwc_to_b8((const _Float16 *)x_dev, n, c0, Vi, (_Float16 *)xb.p, s));
    if (f.x1) {
        MI355_HIP(hipMalloc(&x1b.p, (size_t)n * Vi * f.c1 * 2));
        MI355_TRY(ndhwc_to_b8((const _Float16 *)f.x1, n, f.c1, Vi, (_Float16 *)x1b.p, s));
    }
    TmpWeights<ConvWeightsH, conv_weights_free_f16> cw;
    MI355_TRY(conv_weights_upload_f16(weight_host, bias_host, cin, cin, cout, stride, &cw.w));
    FusedOps fb = f;  // (the channel-blocked copy of x1)
    fb.x1 = x1b.p;
    const char *kname = nullptr;
    // head mode stores logits only (run_block)
    rc = conv3d_mfma_f16(cw.w, make_call<_Float16>(xb.p, cin, n, d, h, w, f.head_out ? nullptr : yb.p, sums, act, slope, fb), s, &kname);
    g_last_conv_kernel = kname ? kname : "";
    if (rc == MI355_OK && !f.head_out) rc = b8_to_ndhwc((const _Float16 *)yb.p, n, cout, Vo, (_Float16 *)y_dev, s);
    rc = synced(rc, s, "conv");
    return rc == MI355_OK ? guards_intact(ybuf.p, guard, ybytes, g_last_conv_kernel.c_str()) : rc;
}

extern "C" int mi355_conv3d_ndhwc_f16(const void *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                                      const float *bias_host, int cout, int stride, int act, float slope, void *y_dev,
                                      void *stream) {
    return conv3d_ndhwc_f16_impl(x_dev, n, d, h, w, cin, weight_host, bias_host, cout, stride, act, slope, y_dev, nullptr, stream);
}

extern "C" int mi355_conv3d_sums_ndhwc(const void *x_dev, int dtype, int n, int d, int h, int w, int cin, const float *weight_host,
                                       const float *bias_host, int cout, int stride, int act, float slope, void *y_dev,
                                       double *sums_dev, void *stream) {
    MI355_REQUIRE(sums_dev != nullptr, "mi355_conv3d_sums_ndhwc: sums_dev is null");
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    if (dtype == MI355_F16)
        return conv3d_ndhwc_f16_impl(x_dev, n, d, h, w, cin, weight_host, bias_host, cout, stride, act, slope, y_dev, sums_dev, stream);
    return conv3d_ndhwc_f32_impl((const float *)x_dev, n, d, h, w, cin, weight_host, bias_host, cout, stride, act, slope, 0, (float *)y_dev,
                                 sums_dev, stream);
}

extern "C" int mi355_conv3d_fused_ndhwc(const void *x0_dev, const void *x1_dev, int dtype, int n, int d, int h, int w, int c0,
                                        int c1, const float *weight_host, const float *bias_host, int cout, int stride, int act,
                                        float slope, int impl, const float *in_scale_dev, const float *in_shift_dev, int in_act,
                                        const float *head_w_dev, const float *head_b_dev, int head_ncls, float *head_out_dev,
                                        void *y_dev, double *sums_dev, void *stream) {
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    MI355_REQUIRE(x0_dev && c0 > 0 && c1 >= 0 && (c1 == 0) == (x1_dev == nullptr), "bad conv inputs (c0 %d, c1 %d)", c0, c1);
    MI355_REQUIRE((y_dev == nullptr) == (head_out_dev != nullptr), "give exactly one of y (feature map) and head_out (logits)");
    MI355_REQUIRE(!in_scale_dev == !in_shift_dev, "in_scale and in_shift come together");
    MI355_REQUIRE(in_act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    FusedOps f;
    f.x1 = x1_dev; f.c1 = c1;
    f.in_scale = in_scale_dev; f.in_shift = in_shift_dev; f.in_act = in_act;
    f.head_w = head_w_dev; f.head_b = head_b_dev; f.head_out = head_out_dev; f.head_ncls = head_out_dev ? head_ncls : 0;
    if (dtype == MI355_F16) {
        MI355_REQUIRE(impl == 0, "the fp16 path has no direct kernel");
        return conv3d_ndhwc_f16_impl(x0_dev, n, d, h, w, c0 + c1, weight_host, bias_host, cout, stride, act, slope, y_dev, sums_dev,
                                     stream, f);
    }
    return conv3d_ndhwc_f32_impl((const float *)x0_dev, n, d, h, w, c0 + c1, weight_host, bias_host, cout, stride, act, slope, impl,
                                 (float *)y_dev, sums_dev, stream, f);
}

// What mi355_conv3d_fused_ndhwc would do with a call of this shape, without a device: the same route through the stem
// shortcut, the pack layout and the planner, with stand-in pointers where the planners test for null.
static int conv3d_plan_impl(int dtype, int n, int d, int h, int w, int c0, int c1, int cout, int stride, int impl, bool stats,
                            bool in_norm, int head_ncls, mi355_conv_plan *out) {
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    MI355_REQUIRE(n > 0 && d > 0 && h > 0 && w > 0 && c0 > 0 && c1 >= 0 && cout > 0 && head_ncls >= 0, "bad conv shape");
    static float stand_in[2];
    static _Float16 stand_in_h[2];
    FusedOps f;
    f.c1 = c1;
    if (c1) f.x1 = stand_in;
    if (in_norm) f.in_scale = f.in_shift = stand_in;
    if (head_ncls) { f.head_w = f.head_b = stand_in; f.head_out = stand_in; f.head_ncls = head_ncls; }
    double *const sums = stats ? (double *)stand_in : nullptr;
    void *const y = head_ncls ? nullptr : (void *)stand_in;
    const int cin = c0 + c1;
    const char *name = nullptr;
    ConvPlan p;
    FusedOps plain = f;  // the call as can_defer_norm asks about it: without the norm operands
    plain.in_scale = plain.in_shift = nullptr;
    if (dtype == MI355_F16) {
        MI355_REQUIRE(impl == 0, "the fp16 path has no direct kernel");
        if (single_op_stem(cin, stride, 0, cout, f)) name = "conv3_stem_f16_kernel";
        else {
            ConvWeightsH cw;
            cw.cin = cw.cin_pad = cin; cw.cout = cout; cw.stride = stride;
            MI355_TRY(conv_pack_layout_f16(cin, cin, cout, stride, &cw.nf));
            cw.wp_dev = stand_in_h; cw.bias_dev = stand_in;
            out->fuses_in_norm = conv3d_f16_fuses_input_norm(cw, make_call<_Float16>(stand_in_h, cin, n, d, h, w, y, sums, ACT_NONE, 0.f, plain));
            MI355_TRY(plan_conv_f16(cw, make_call<_Float16>(stand_in_h, cin, n, d, h, w, y, sums, ACT_NONE, 0.f, f), &p));
        }
    } else if (single_op_stem(cin, stride, impl, cout, f)) name = "conv3_stem_f32_kernel";
    else {
        ConvPackLayout l;
        MI355_TRY(conv_pack_layout(cin, cin, cout, stride, &l));
        ConvWeights cw;
        cw.cin = cw.cin_pad = cin; cw.cout = cout; cw.stride = stride;
        cw.cc = l.cc; cw.nf = l.nf; cw.pipe = l.pipe;
        cw.bias_dev = stand_in;
        if (l.mfma) cw.wp_dev = stand_in;
        if (l.c16) cw.wp16_dev = stand_in;
        if (l.wino2) cw.wpw_dev = stand_in;
        if (l.wino3) cw.wp3_dev = stand_in;
        if (impl == 1 || !l.mfma) cw.w_plain_dev = stand_in;
        const ConvCall c = make_call<float>(stand_in, cin, n, d, h, w, y, sums, ACT_NONE, 0.f, f);
        out->fuses_in_norm = impl == 0 && cw.wp3_dev && conv3d_wino3_fuses_input_norm(cw, make_call<float>(stand_in, cin, n, d, h, w, y, sums, ACT_NONE, 0.f, plain));
        MI355_REQUIRE(!sums || impl != 1, "the direct cross-check kernel carries no statistics epilogue");
        if (impl == 1) { MI355_TRY(plan_conv_direct(cw, c)); name = "conv3_direct_kernel"; }
        else MI355_TRY(plan_conv_f32(cw, c, &p));
    }
    if (p.row) {  // (the stem and direct kernels size their own grids: only the name is reported)
        name = p.name;
        out->grid[0] = (int32_t)p.gx; out->grid[1] = (int32_t)p.gy; out->grid[2] = (int32_t)p.gz;
        out->lds_bytes = (int64_t)p.lds_bytes;
        out->splitk = p.ksplit;
        out->tile[0] = 1 << p.g.lz; out->tile[1] = 1 << p.g.ly; out->tile[2] = 1 << p.g.lx;
    }
    snprintf(out->kernel, sizeof(out->kernel), "%s", name);
    return MI355_OK;
}

extern "C" int mi355_conv3d_plan(int dtype, int n, int d, int h, int w, int c0, int c1, int cout, int stride, int impl, int has_stats,
                                 int has_in_norm, int head_ncls, mi355_conv_plan *out) {
    MI355_REQUIRE(out != nullptr, "mi355_conv3d_plan: out is null");
    memset(out, 0, sizeof(*out));
    out->splitk = 1;
    out->rc = conv3d_plan_impl(dtype, n, d, h, w, c0, c1, cout, stride, impl, has_stats != 0, has_in_norm != 0, head_ncls, out);
    return out->rc;
}

extern "C" int64_t mi355_conv_kernel_names(char *buf, int64_t buf_bytes) {
    MI355_REQUIRE(buf != nullptr || buf_bytes == 0, "mi355_conv_kernel_names: buf is null");
    std::string s;
    list_f32_rows(&s); list_wino3_rows(&s); list_f16_rows(&s); list_s2h_rows(&s);
    if (buf_bytes > 0) snprintf(buf, (size_t)buf_bytes, "%s", s.c_str());
    return (int64_t)s.size() + 1;
}

extern "C" int mi355_stage0_plan(int z, int y, int x, const int32_t patch[3], float step_size, int mirror_axes, int r,
                                 mi355_stage0_geom *out, mi355_stage0_sample *samples, int max_samples) {
    MI355_REQUIRE(out && patch && r >= 0 && (samples || max_samples == 0), "mi355_stage0_plan: bad argument");
    mi355_sw_opts o;
    memset(&o, 0, sizeof(o));
    for (int a = 0; a < 3; ++a) o.patch[a] = patch[a];
    o.step_size = step_size; o.mirror_axes = mirror_axes;
    SwGeom g;
    MI355_TRY(make_geom(o, z, y, x, &g));
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
    mi355_sw_opts o;
    memset(&o, 0, sizeof(o));
    for (int a = 0; a < 3; ++a) o.patch[a] = patch[a];
    o.step_size = step_size; o.mirror_axes = mirror_axes;
    SwGeom g;
    MI355_TRY(make_geom(o, z, y, x, &g));
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
    mi355_sw_opts o;
    memset(&o, 0, sizeof(o));
    for (int a = 0; a < 3; ++a) o.patch[a] = patch[a];
    o.step_size = step_size; o.mirror_axes = mirror_axes;
    SwGeom g;
    MI355_TRY(make_geom(o, z, y, x, &g));
    // stage0_blocks' rule, from the description: fp32, enc[0] = stride-1 blocks without run-time statistics or a BN left unfolded
    const bool folded = nd->norm == MI355_NORM_NONE || (nd->norm == MI355_NORM_BATCH && !nd->nonlin_first);
    const int r0 = (nd->dtype == MI355_F32 && folded && nd->c_skip % 4 == 0) ? nd->enc0_blocks : 0;
    SkipShareNet d = skip_share_net_of(nd->dtype, r0, nd->stride, nd->norm, nd->nonlin_first, nd->c_up, nd->c_skip, nd->cout, nd->head_ncls);
    d.skip_is_enc0 = nd->skip_is_enc0 != 0;
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

extern "C" int mi355_conv3d_wino3_ndhwc(const float *x0_dev, const float *x1_dev, int n, int d, int h, int w, int c0, int c1,
                                        const float *weight_host, const float *bias_host, int cout, int act, float slope,
                                        const float *addend_dev, float *y_dev, void *stream) {
    MI355_REQUIRE(x0_dev && y_dev && weight_host && c0 > 0 && c1 >= 0 && (c1 == 0) == (x1_dev == nullptr), "mi355_conv3d_wino3_ndhwc: bad argument");
    MI355_REQUIRE(act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    TmpWeights<ConvWeights, conv_weights_free> cw;
    MI355_TRY(conv_weights_upload(weight_host, bias_host, c0 + c1, c0 + c1, cout, 1, false, &cw.w));
    FusedOps f;
    f.x1 = x1_dev; f.c1 = c1;
    ConvCall c = make_call<float>(x0_dev, c0 + c1, n, d, h, w, y_dev, nullptr, act, slope, f);
    c.addend = addend_dev;
    ConvPlan p;
    if (!plan_wino3(cw.w, c, &p, true)) {
        set_error("mi355_conv3d_wino3_ndhwc: %dx%dx%dx%d, %d+%d -> %d is not a call of the F(2x2x2,3x3x3) kernel", n, d, h, w, c0, c1, cout);
        return MI355_ERR_UNSUPPORTED;
    }
    g_last_conv_kernel = p.name;
    return synced(launch_wino3(cw.w, c, p, s), s, "conv");
}

// ---- stage-0 views: dry run and single-op entries
extern "C" int mi355_stage0_view_plan(int z, int y, int x, const int32_t patch[3], float step_size, int mirror_axes,
                                      const mi355_skip_share_net *nd, int c_level1, int batch_samples, mi355_stage0_view_geom *out,
                                      mi355_stage0_view_sample *samples, int max_samples) {
    MI355_REQUIRE(out && patch && nd && c_level1 > 0 && batch_samples >= 0 && (samples || max_samples == 0), "mi355_stage0_view_plan: bad argument");
    mi355_sw_opts o;
    memset(&o, 0, sizeof(o));
    for (int a = 0; a < 3; ++a) o.patch[a] = patch[a];
    o.step_size = step_size; o.mirror_axes = mirror_axes;
    SwGeom g;
    MI355_TRY(make_geom(o, z, y, x, &g));
    const bool folded = nd->norm == MI355_NORM_NONE || (nd->norm == MI355_NORM_BATCH && !nd->nonlin_first);
    const int r0 = (nd->dtype == MI355_F32 && folded && nd->c_skip % 4 == 0) ? nd->enc0_blocks : 0;
    SkipShareNet d = skip_share_net_of(nd->dtype, r0, nd->stride, nd->norm, nd->nonlin_first, nd->c_up, nd->c_skip, nd->cout, nd->head_ncls);
    d.skip_is_enc0 = nd->skip_is_enc0 != 0;
    const bool on = skip_share_decide(d, g);
    S0Geom sg;
    stage0_geometry(g, d.r, &sg, on ? 1 : 0);
    // the first block of level 1 as the network would hold it: c_skip -> c_level1, stride 2
    static float stand_in[2];
    ConvPackLayout l;
    ConvWeights cw;
    const bool have_w1 = nd->dtype == MI355_F32 && conv_pack_layout(nd->c_skip, nd->c_skip, c_level1, 2, &l) == MI355_OK && l.mfma;
    if (have_w1) {
        cw.cin = cw.cin_pad = nd->c_skip; cw.cout = c_level1; cw.stride = 2;
        cw.cc = l.cc; cw.nf = l.nf; cw.pipe = l.pipe;
        cw.bias_dev = cw.wp_dev = stand_in;
    }
    const int nm = (int)g.mirrors.size();
    // a full batch of one rank; a short last batch, or the tiles one rank of several gets, is asked for with batch_samples
    const int per_forward = batch_samples > 0 ? batch_samples : sw_batch_tiles(nd->dtype, 0, nm) * nm;
    const S0ViewChoice v = stage0_views_choose(sg, on, std::min(per_forward, (int)g.tiles.size() * nm), g.P, have_w1 ? &cw : nullptr, nd->c_skip, !folded);
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

// the C-ABI description of a view -> S0View (refused where stage0_view_make refuses)
static int view_from_abi(const mi355_stage0_view *v, int n, int d, int h, int w, int c, S0View *out) {
    MI355_REQUIRE(v->src_dev && v->n_samples == n, "stage-0 view: %d samples for a call of %d", v->n_samples, n);
    MI355_REQUIRE(n > 0 && n <= S0_VIEW_MAX_SAMPLES, "stage-0 view: %d samples (max %d)", n, S0_VIEW_MAX_SAMPLES);
    std::vector<S0Sample> smp(n);
    for (int i = 0; i < n; ++i) {
        smp[i].wv = v->samples[i].wv;
        for (int k = 0; k < 3; ++k) smp[i].org[k] = v->samples[i].origin[k];
        for (int f = 0; f < 6; ++f) smp[i].slab[f] = (v->samples[i].faces >> f) & 1 ? 0 : -1;
    }
    const int Ve[3] = {v->volume[0], v->volume[1], v->volume[2]}, P[3] = {d, h, w};
    return stage0_view_make(v->src_dev, v->n_wv, Ve, P, c, v->depth, smp.data(), n, out);
}

extern "C" int mi355_conv3d_s2dma_view_ndhwc(const float *x_dev, const mi355_stage0_view *view, int n, int d, int h, int w, int cin,
                                             const float *weight_host, const float *bias_host, int cout, int act, float slope, int force,
                                             float *y_dev, void *stream) {
    MI355_REQUIRE(x_dev && y_dev && weight_host && cin > 0 && cout > 0, "mi355_conv3d_s2dma_view_ndhwc: bad argument");
    MI355_REQUIRE(act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    S0View sv;
    if (view) MI355_TRY(view_from_abi(view, n, d, h, w, cin, &sv));  // (before anything touches the device: a bad view launches nothing)
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    TmpWeights<ConvWeights, conv_weights_free> cw;
    MI355_TRY(conv_weights_upload(weight_host, bias_host, cin, cin, cout, 2, false, &cw.w));
    ConvCall c = make_call<float>(x_dev, cin, n, d, h, w, y_dev, nullptr, act, slope);
    if (view) c.in0_view = &sv;
    const char *kname = nullptr;
    const int rc = conv3d_s2dma_f32(cw.w, c, force != 0, s, &kname);
    g_last_conv_kernel = kname ? kname : "";
    return synced(rc, s, "conv");
}

extern "C" int mi355_conv3d_wino3_view_ndhwc(const float *x0_dev, int n, int d, int h, int w, int c0, const float *weight_host,
                                             const float *bias_host, int cout, int act, float slope, const float *addend_dev,
                                             const mi355_stage0_view *view, float *y_dev, void *stream) {
    MI355_REQUIRE(x0_dev && y_dev && weight_host && addend_dev && c0 > 0 && cout > 0, "mi355_conv3d_wino3_view_ndhwc: bad argument");
    MI355_REQUIRE(act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    S0View sv;
    if (view) MI355_TRY(view_from_abi(view, n, d, h, w, cout, &sv));
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    TmpWeights<ConvWeights, conv_weights_free> cw;
    MI355_TRY(conv_weights_upload(weight_host, bias_host, c0, c0, cout, 1, false, &cw.w));
    ConvCall c = make_call<float>(x0_dev, c0, n, d, h, w, y_dev, nullptr, act, slope);
    c.addend = addend_dev;
    if (view) c.addend_view = &sv;
    ConvPlan p;
    if (!plan_wino3(cw.w, c, &p, true)) {
        set_error("mi355_conv3d_wino3_view_ndhwc: %dx%dx%dx%d, %d -> %d is not a call of the F(2x2x2,3x3x3) kernel", n, d, h, w, c0, cout);
        return MI355_ERR_UNSUPPORTED;
    }
    g_last_conv_kernel = p.name;
    return synced(launch_wino3(cw.w, c, p, s), s, "conv");
}

extern "C" int mi355_tconv3d_ndhwc_f16(const void *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                                       int cout, void *y_dev, void *stream) {
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t Vi = (int64_t)d * h * w;
    TmpBuf xb, yb;
    MI355_HIP(hipMalloc(&xb.p, (size_t)n * Vi * cin * 2));
    MI355_HIP(hipMalloc(&yb.p, (size_t)n * Vi * 8 * cout * 2));
    MI355_HIP(hipMemsetAsync(yb.p, 0xFF, (size_t)n * Vi * 8 * cout * 2, s));  // all-NaN: an unstored voxel cannot pass for a result
    TmpWeights<TConvWeightsH, tconv_weights_free_f16> tw;
    MI355_TRY(tconv_weights_upload_f16(weight_host, cin, cout, &tw.w));
    int rc = ndhwc_to_b8((const _Float16 *)x_dev, n, cin, Vi, (_Float16 *)xb.p, s);
    const char *tname = nullptr;
    if (rc == MI355_OK) rc = tconv2_mfma_f16(tw.w, (const _Float16 *)xb.p, n, d, h, w, (_Float16 *)yb.p, s, &tname);
    g_last_conv_kernel = tname ? tname : "";
    if (rc == MI355_OK) rc = b8_to_ndhwc((const _Float16 *)yb.p, n, cout, Vi * 8, (_Float16 *)y_dev, s);
    return synced(rc, s, "tconv");
}

// ---- single-op entry points of the kernels around the convolutions (csrc/elementwise.hip): each binds the device, calls the
// launcher the network calls and waits for the stream.  Test aids; tensors are taken in the layout the launcher takes.
static bool tile_in_grid(const int32_t patch[3], const int32_t padded[3], const int32_t origin[3]) {
    for (int a = 0; a < 3; ++a)
        if (patch[a] <= 0 || origin[a] < 0 || origin[a] + patch[a] > padded[a]) return false;
    return true;
}

extern "C" int mi355_norm_finalize(const double *stats_dev, int n, int c, int64_t count, int kind, int groups, float eps,
                                   const float *gamma_dev, const float *beta_dev, float *scale_dev, float *shift_dev, void *stream) {
    MI355_REQUIRE(stats_dev && scale_dev && shift_dev && n > 0 && c > 0 && count > 0, "mi355_norm_finalize: bad argument");
    MI355_REQUIRE(kind == MI355_NORM_INSTANCE || kind == MI355_NORM_GROUP, "mi355_norm_finalize: norm kind %d has no run-time statistics", kind);
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    return synced(norm_finalize(stats_dev, n, c, count, kind, groups, eps, gamma_dev, beta_dev, scale_dev, shift_dev, s), s, "norm_finalize");
}

extern "C" int mi355_norm_apply(void *x_dev, int dtype, int n, int64_t v, int c, const float *scale_dev, const float *shift_dev, int act,
                                float slope, void *stream) {
    MI355_REQUIRE(x_dev && scale_dev && shift_dev && n > 0 && v > 0 && c > 0, "mi355_norm_apply: bad argument");
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    return synced(norm_apply(x_dev, dtype, n, v, c, scale_dev, shift_dev, act, slope, s), s, "norm_apply");
}

extern "C" int mi355_extract_tiles(const float *vol_dev, int c, int z, int y, int x, const int32_t pad[3], const int32_t *tiles_host,
                                   int n_samples, const int32_t patch[3], int cpad, void *x_dev, int dtype, void *stream) {
    MI355_REQUIRE(vol_dev && pad && tiles_host && patch && x_dev && c > 0 && z > 0 && y > 0 && x > 0, "mi355_extract_tiles: bad argument");
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    MI355_REQUIRE(patch[0] > 0 && patch[1] > 0 && patch[2] > 0 && cpad >= c, "mi355_extract_tiles: patch %d x %d x %d, %d of %d channels", patch[0],
                  patch[1], patch[2], c, cpad);
    MI355_REQUIRE(n_samples > 0 && n_samples <= S0_MAX_SAMPLES, "mi355_extract_tiles: %d samples", n_samples);
    MI355_TRY(require_device());
    std::vector<TileDesc> tiles(n_samples);
    for (int i = 0; i < n_samples; ++i) tiles[i] = TileDesc{tiles_host[4 * i], tiles_host[4 * i + 1], tiles_host[4 * i + 2], tiles_host[4 * i + 3]};
    hipStream_t s = (hipStream_t)stream;
    return synced(extract_tiles(vol_dev, c, z, y, x, pad[0], pad[1], pad[2], tiles.data(), n_samples, patch[0], patch[1], patch[2], cpad, x_dev, dtype, s),
                  s, "extract_tiles");
}

static FeatNorm feat_norm(const float *scale_dev, const float *shift_dev, float slope) {
    FeatNorm fn;
    fn.scale = scale_dev; fn.shift = shift_dev; fn.slope = slope;
    return fn;
}

extern "C" int mi355_head_logits(const void *feat_dev, int dtype, int n, int64_t v, int cin, const float *weight_host, const float *bias_host,
                                 int ncls, const float *scale_dev, const float *shift_dev, float slope, float *logits_dev, void *stream) {
    MI355_REQUIRE(feat_dev && weight_host && logits_dev && v > 0, "mi355_head_logits: bad argument");
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    MI355_REQUIRE(!scale_dev == !shift_dev, "scale and shift come together");
    MI355_TRY(require_device());
    TmpWeights<HeadWeights, head_weights_free> hw;
    MI355_TRY(head_weights_upload(weight_host, bias_host, cin, ncls, &hw.w));
    hipStream_t s = (hipStream_t)stream;
    return synced(head_logits(hw.w, feat_dev, dtype, n, v, logits_dev, s, feat_norm(scale_dev, shift_dev, slope)), s, "head_logits");
}

extern "C" int mi355_head_aggregate(const void *feat_dev, int dtype, int cin, const float *weight_host, const float *bias_host, int ncls,
                                    const float *scale_dev, const float *shift_dev, float slope, int first_sample, const int32_t *mirrors_host,
                                    int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                                    const int32_t padded[3], const int32_t origin[3], void *stream) {
    MI355_REQUIRE(feat_dev && weight_host && mirrors_host && patch && agg_dev && padded && origin && first_sample >= 0, "mi355_head_aggregate: bad argument");
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    MI355_REQUIRE(!scale_dev == !shift_dev, "scale and shift come together");
    MI355_REQUIRE(tile_in_grid(patch, padded, origin), "mi355_head_aggregate: the tile leaves the padded grid");
    MI355_TRY(require_device());
    TmpWeights<HeadWeights, head_weights_free> hw;
    MI355_TRY(head_weights_upload(weight_host, bias_host, cin, ncls, &hw.w));
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> mirrors(mirrors_host, mirrors_host + std::max(n_mirrors, 0));
    return synced(head_aggregate(hw.w, feat_dev, dtype, first_sample, mirrors.data(), n_mirrors, patch[0], patch[1], patch[2], nonlin, gauss_dev, agg_dev,
                                 cnt_dev, padded[0], padded[1], padded[2], origin[0], origin[1], origin[2], s, feat_norm(scale_dev, shift_dev, slope)),
                  s, "head_aggregate");
}

extern "C" int mi355_logits_aggregate(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                                      const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                                      const int32_t padded[3], const int32_t origin[3], void *stream) {
    MI355_REQUIRE(logits_dev && mirrors_host && patch && agg_dev && padded && origin && first_sample >= 0, "mi355_logits_aggregate: bad argument");
    MI355_REQUIRE(tile_in_grid(patch, padded, origin), "mi355_logits_aggregate: the tile leaves the padded grid");
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> mirrors(mirrors_host, mirrors_host + std::max(n_mirrors, 0));
    return synced(logits_aggregate(logits_dev, ncls, first_sample, mirrors.data(), n_mirrors, patch[0], patch[1], patch[2], nonlin, gauss_dev, agg_dev,
                                   cnt_dev, padded[0], padded[1], padded[2], origin[0], origin[1], origin[2], s),
                  s, "logits_aggregate");
}

extern "C" int mi355_logits_aggregate_tiles(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                                            const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                                            const int32_t padded[3], const int32_t *origins, int n_tiles, void *stream) {
    MI355_REQUIRE(logits_dev && mirrors_host && patch && agg_dev && padded && origins && first_sample >= 0 && n_tiles >= 1,
                  "mi355_logits_aggregate_tiles: bad argument");
    for (int i = 0; i < n_tiles; ++i)
        MI355_REQUIRE(tile_in_grid(patch, padded, origins + 3 * (size_t)i), "mi355_logits_aggregate_tiles: tile %d leaves the padded grid", i);
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> mirrors(mirrors_host, mirrors_host + std::max(n_mirrors, 0));
    std::vector<int> org(origins, origins + 3 * (size_t)n_tiles);
    return synced(logits_aggregate_tiles(logits_dev, ncls, first_sample, mirrors.data(), n_mirrors, patch[0], patch[1], patch[2], nonlin, gauss_dev,
                                         agg_dev, cnt_dev, padded[0], padded[1], padded[2], org.data(), n_tiles, s),
                  s, "logits_aggregate_tiles");
}

extern "C" int mi355_cnt_add_tile(const float *gauss_dev, const int32_t patch[3], float *cnt_dev, const int32_t padded[3],
                                  const int32_t origin[3], void *stream) {
    MI355_REQUIRE(patch && cnt_dev && padded && origin, "mi355_cnt_add_tile: bad argument");
    MI355_REQUIRE(tile_in_grid(patch, padded, origin), "mi355_cnt_add_tile: the tile leaves the padded grid");
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    return synced(cnt_add_tile(gauss_dev, patch[0], patch[1], patch[2], cnt_dev, padded[1], padded[2], origin[0], origin[1], origin[2], s), s,
                  "cnt_add_tile");
}

static int stage0_gather_abi(const mi355_stage0_gather_args *a, void *stream, bool shells_only) {
    MI355_REQUIRE(a && a->wv_dev && a->out_dev && a->channels > 0 && a->channels % 4 == 0, "mi355_stage0_gather: bad argument");
    MI355_REQUIRE(a->n_samples > 0 && a->n_samples <= S0_MAX_SAMPLES, "mi355_stage0_gather: %d samples (max %d)", a->n_samples, S0_MAX_SAMPLES);
    MI355_TRY(require_device());
    S0GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.wv = a->wv_dev; ga.out = a->out_dev;
    for (int k = 0; k < 3; ++k) { ga.slab[k] = a->slab_dev[k]; ga.P[k] = a->patch[k]; ga.Ve[k] = a->volume[k]; ga.t[k] = a->slab_thickness[k]; }
    ga.r = a->r; ga.C4 = a->channels / 4;
    stage0_gather_dense(&ga);
    for (int i = 0; i < a->n_samples; ++i) {
        S0Sample &sm = ga.smp[i];
        sm.wv = a->samples[i].wv;
        MI355_REQUIRE(sm.wv >= 0, "mi355_stage0_gather: sample %d: whole-volume index %d", i, sm.wv);
        for (int k = 0; k < 3; ++k) sm.org[k] = a->samples[i].origin[k];
        for (int f = 0; f < 6; ++f) {
            sm.slab[f] = a->samples[i].slab[f];
            MI355_REQUIRE(sm.slab[f] < 0 || a->slab_dev[f >> 1], "mi355_stage0_gather: sample %d: face %d without a slab tensor", i, f);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (shells_only) return synced(stage0_gather_shells(ga, a->n_samples, 0, s), s, "stage0_gather_shells");
    return synced(stage0_gather(ga, a->n_samples, s), s, "stage0_gather");
}
extern "C" int mi355_stage0_gather(const mi355_stage0_gather_args *a, void *stream) { return stage0_gather_abi(a, stream, false); }
extern "C" int mi355_stage0_gather_shells(const mi355_stage0_gather_args *a, void *stream) { return stage0_gather_abi(a, stream, true); }

extern "C" int mi355_stage0_gather_merged(const mi355_stage0_gather_merged_args *m, int shells_only, void *stream) {
    MI355_REQUIRE(m, "mi355_stage0_gather_merged: bad argument");
    const mi355_stage0_gather_args *a = &m->base;
    MI355_REQUIRE(a->wv_dev && a->out_dev && a->channels > 0 && a->channels % 4 == 0, "mi355_stage0_gather_merged: bad argument");
    MI355_REQUIRE(a->n_samples > 0 && a->n_samples <= S0_MAX_SAMPLES, "mi355_stage0_gather_merged: %d samples (max %d)", a->n_samples, S0_MAX_SAMPLES);
    MI355_REQUIRE(!m->out2_dev || (m->wv2_dev && m->channels2 > 0 && m->channels2 % 4 == 0), "mi355_stage0_gather_merged: bad second tensor");
    MI355_TRY(require_device());
    S0GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.wv = a->wv_dev; ga.out = a->out_dev;
    for (int k = 0; k < 3; ++k) { ga.slab[k] = a->slab_dev[k]; ga.P[k] = a->patch[k]; ga.Ve[k] = a->volume[k]; ga.t[k] = a->slab_thickness[k]; }
    ga.r = a->r; ga.C4 = a->channels / 4;
    if (m->out2_dev) {
        ga.wv2 = m->wv2_dev; ga.out2 = m->out2_dev; ga.r2 = m->r2; ga.C42 = m->channels2 / 4;
        for (int k = 0; k < 3; ++k) ga.slab2[k] = m->slab2_dev[k];
    }
    for (int ax = 0; ax < 3; ++ax)
        for (int k = 0; k < 3; ++k) {
            ga.D[ax][k] = m->slab_shape[ax][k];
            MI355_REQUIRE(m->spans_volume[ax][k] == 0 || m->spans_volume[ax][k] == 1, "mi355_stage0_gather_merged: spans_volume[%d][%d]", ax, k);
            ga.so[ax][k] = m->spans_volume[ax][k];
        }
    for (int i = 0; i < a->n_samples; ++i) {
        S0Sample &sm = ga.smp[i];
        sm.wv = a->samples[i].wv;
        MI355_REQUIRE(sm.wv >= 0, "mi355_stage0_gather_merged: sample %d: whole-volume index %d", i, sm.wv);
        for (int k = 0; k < 3; ++k) sm.org[k] = a->samples[i].origin[k];
        for (int f = 0; f < 6; ++f) {
            sm.slab[f] = a->samples[i].slab[f];
            MI355_REQUIRE(sm.slab[f] < 0 || (a->slab_dev[f >> 1] && (!m->out2_dev || m->slab2_dev[f >> 1])),
                          "mi355_stage0_gather_merged: sample %d: face %d without a slab tensor", i, f);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (!shells_only) return synced(stage0_gather(ga, a->n_samples, s), s, "stage0_gather");
    MI355_TRY(stage0_gather_shells(ga, a->n_samples, 0, s));
    if (ga.out2) MI355_TRY(stage0_gather_shells(ga, a->n_samples, 1, s));
    return synced(MI355_OK, s, "stage0_gather_shells");
}

extern "C" int mi355_stage0_mask(float *x_dev, int n, const int32_t volume[3], const int32_t keep[3], int c, void *stream) {
    MI355_REQUIRE(x_dev && volume && keep, "mi355_stage0_mask: bad argument");
    MI355_TRY(require_device());
    const int ve[3] = {volume[0], volume[1], volume[2]}, zp[3] = {keep[0], keep[1], keep[2]};
    hipStream_t s = (hipStream_t)stream;
    return synced(stage0_mask(x_dev, n, ve, zp, c, s), s, "stage0_mask");
}
