// Single-op entry points (host side; include/mi355_nnunet.h): one kernel family per call, driven by the tests and by nothing in
// the product - convs and transposed convs in both dtypes with their guard bands, the F(2x2x2,3x3x3) and stride-2 view entries,
// mi355_conv3d_plan (what a conv call would launch, without a device) and the wrappers around the launchers of elementwise.hip,
// stage0_gather.hip and aggregate.hip.
#include <cstring>
#include <string>
#include <vector>

#include "unet_internal.h"

using namespace mi355;

static thread_local std::string g_last_conv_kernel;  // mi355_last_conv_kernel(): which instantiation a single-op conv call ran
extern "C" const char *mi355_last_conv_kernel(void) { return g_last_conv_kernel.c_str(); }

// The single-op fp16 entry points take and return PLAIN NDHWC tensors (include/mi355_nnunet.h); the kernels work on
// channel-blocked ones (common.h), so the operands pass through ndhwc_to_b8 / b8_to_ndhwc here.  Every entry point that uploads
// weights or needs such a copy has one DeviceAllocs `mem` on its stack: freed on every exit, after the call has synchronised.

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
    return (g + 255) / 256 * 256;  // (the buffer between the bands keeps the allocation's alignment to 256 B)
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
    DeviceAllocs mem;
    if (single_op_stem(cin, stride, impl, cout, f)) {
        StemWeights sw;
        MI355_TRY(stem_weights_upload(mem, weight_host, bias_host, cin, cout, MI355_F32, &sw));
        g_last_conv_kernel = "conv3_stem_f32_kernel";
        return synced(conv3d_stem(sw, x_dev, n, d, h, w, y_dev, sums, act, slope, s), s, "stem conv");
    }
    ConvWeights cw;
    MI355_TRY(conv_weights_upload(mem, weight_host, bias_host, cin, cin, cout, stride, impl == 1, &cw));
    const ConvCall c = make_call<float>(x_dev, cin, n, d, h, w, y_dev, sums, act, slope, f);
    MI355_REQUIRE(!sums || impl != 1, "the direct cross-check kernel carries no statistics epilogue");
    const char *kname = "conv3_direct_kernel";
    const int rc = (impl == 1) ? conv3d_direct_f32(cw, c, s) : conv3d_mfma_f32(cw, c, s, &kname);
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
    DeviceAllocs mem;
    TConvWeights tw;
    MI355_TRY(tconv_weights_upload(mem, weight_host, cin, cout, MI355_F32, &tw));
    const char *tname = nullptr;
    const int rc = tconv2_mfma(tw, x_dev, n, d, h, w, y_dev, (hipStream_t)stream, &tname);
    g_last_conv_kernel = tname ? tname : "";
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
    DeviceAllocs mem;
    void *ybuf = nullptr;  // guard band, the kernel's output, guard band (guards_intact)
    MI355_TRY(mem.alloc(ybytes + 2 * guard, &ybuf));
    void *const yb = (char *)ybuf + guard;
    MI355_HIP(hipMemsetAsync(ybuf, GUARD_BYTE, ybytes + 2 * guard, s));
    // all-NaN (0xFFFF) before the launch: a voxel the kernel fails to store cannot pass for a result
    MI355_HIP(hipMemsetAsync(yb, 0xFF, ybytes, s));
    int rc;
    if (single_op_stem(cin, stride, 0, cout, f)) {
        StemWeights sw;
        MI355_TRY(stem_weights_upload(mem, weight_host, bias_host, cin, cout, MI355_F16, &sw));
        rc = conv3d_stem(sw, x_dev, n, d, h, w, yb, sums, act, slope, s);
        g_last_conv_kernel = "conv3_stem_f16_kernel";
        if (rc == MI355_OK) rc = b8_to_ndhwc((const _Float16 *)yb, n, cout, Vo, (_Float16 *)y_dev, s);
        rc = synced(rc, s, "stem conv");
        return rc == MI355_OK ? guards_intact(ybuf, guard, ybytes, g_last_conv_kernel.c_str()) : rc;
    }
    MI355_REQUIRE(cin % 8 == 0 && f.c1 % 8 == 0, "fp16 conv needs cin %% 8 == 0 on both inputs (got %d, %d)", cin - f.c1, f.c1);
    const int c0 = cin - f.c1;
    void *xb = nullptr, *x1b = nullptr;  // the channel-blocked copies of x0 and x1
    MI355_TRY(mem.alloc((size_t)n * Vi * c0 * 2, &xb));
    MI355_TRY(ndhwc_to_b8((const _Float16 *)x_dev, n, c0, Vi, (_Float16 *)xb, s));
    if (f.x1) {
        MI355_TRY(mem.alloc((size_t)n * Vi * f.c1 * 2, &x1b));
        MI355_TRY(ndhwc_to_b8((const _Float16 *)f.x1, n, f.c1, Vi, (_Float16 *)x1b, s));
    }
    ConvWeightsH cw;
    MI355_TRY(conv_weights_upload_f16(mem, weight_host, bias_host, cin, cin, cout, stride, &cw));
    FusedOps fb = f;
    fb.x1 = x1b;
    const char *kname = nullptr;
    // head mode stores logits only (run_block)
    rc = conv3d_mfma_f16(cw, make_call<_Float16>(xb, cin, n, d, h, w, f.head_out ? nullptr : yb, sums, act, slope, fb), s, &kname);
    g_last_conv_kernel = kname ? kname : "";
    if (rc == MI355_OK && !f.head_out) rc = b8_to_ndhwc((const _Float16 *)yb, n, cout, Vo, (_Float16 *)y_dev, s);
    rc = synced(rc, s, "conv");
    return rc == MI355_OK ? guards_intact(ybuf, guard, ybytes, g_last_conv_kernel.c_str()) : rc;
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
                            bool in_norm, int head_ncls, bool s2_least_padding, mi355_conv_plan *out) {
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
        const ConvWeights cw = stand_in_conv_weights(l, cin, cout, stride, impl == 1);
        ConvCall c = make_call<float>(stand_in, cin, n, d, h, w, y, sums, ACT_NONE, 0.f, f);
        c.s2_least_padding = s2_least_padding;
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

extern "C" int mi355_conv3d_plan_hinted(int dtype, int n, int d, int h, int w, int c0, int c1, int cout, int stride, int impl, int has_stats,
                                        int has_in_norm, int head_ncls, int s2_least_padding, mi355_conv_plan *out) {
    MI355_REQUIRE(out != nullptr, "mi355_conv3d_plan: out is null");
    memset(out, 0, sizeof(*out));
    out->splitk = 1;
    out->rc = conv3d_plan_impl(dtype, n, d, h, w, c0, c1, cout, stride, impl, has_stats != 0, has_in_norm != 0, head_ncls, s2_least_padding != 0, out);
    return out->rc;
}
extern "C" int mi355_conv3d_plan(int dtype, int n, int d, int h, int w, int c0, int c1, int cout, int stride, int impl, int has_stats,
                                 int has_in_norm, int head_ncls, mi355_conv_plan *out) {
    return mi355_conv3d_plan_hinted(dtype, n, d, h, w, c0, c1, cout, stride, impl, has_stats, has_in_norm, head_ncls, 0, out);
}

static int tconv3d_plan_impl(int dtype, int n, int d, int h, int w, int cin, int cout, mi355_conv_plan *out) {
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    MI355_REQUIRE(n > 0 && d > 0 && h > 0 && w > 0, "bad tconv shape");
    TconvPlan p;
    MI355_TRY(plan_tconv(dtype, cin, cout, (long)n * d * h * w, &p));
    out->grid[0] = (int32_t)p.gx; out->grid[1] = (int32_t)p.gy; out->grid[2] = 1;
    out->lds_bytes = (int64_t)p.lds_bytes;
    snprintf(out->kernel, sizeof(out->kernel), "%s", p.row->name);
    return MI355_OK;
}
extern "C" int mi355_tconv3d_plan(int dtype, int n, int d, int h, int w, int cin, int cout, mi355_conv_plan *out) {
    MI355_REQUIRE(out != nullptr, "mi355_tconv3d_plan: out is null");
    memset(out, 0, sizeof(*out));
    out->splitk = 1;
    out->rc = tconv3d_plan_impl(dtype, n, d, h, w, cin, cout, out);
    return out->rc;
}

extern "C" int64_t mi355_conv_kernel_names(char *buf, int64_t buf_bytes) {
    MI355_REQUIRE(buf != nullptr || buf_bytes == 0, "mi355_conv_kernel_names: buf is null");
    std::string s;
    list_f32_rows(&s); list_wino3_rows(&s); list_f16_rows(&s); list_s2h_rows(&s);
    if (buf_bytes > 0) snprintf(buf, (size_t)buf_bytes, "%s", s.c_str());
    return (int64_t)s.size() + 1;
}

extern "C" int mi355_conv3d_wino3_ndhwc(const float *x0_dev, const float *x1_dev, int n, int d, int h, int w, int c0, int c1,
                                        const float *weight_host, const float *bias_host, int cout, int act, float slope,
                                        const float *addend_dev, float *y_dev, void *stream) {
    MI355_REQUIRE(x0_dev && y_dev && weight_host && c0 > 0 && c1 >= 0 && (c1 == 0) == (x1_dev == nullptr), "mi355_conv3d_wino3_ndhwc: bad argument");
    MI355_REQUIRE(act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    DeviceAllocs mem;
    ConvWeights cw;
    MI355_TRY(conv_weights_upload(mem, weight_host, bias_host, c0 + c1, c0 + c1, cout, 1, false, &cw));
    FusedOps f;
    f.x1 = x1_dev; f.c1 = c1;
    ConvCall c = make_call<float>(x0_dev, c0 + c1, n, d, h, w, y_dev, nullptr, act, slope, f);
    c.addend = addend_dev;
    ConvPlan p;
    if (!plan_wino3(cw, c, &p, true)) {
        set_error("mi355_conv3d_wino3_ndhwc: %dx%dx%dx%d, %d+%d -> %d is not a call of the F(2x2x2,3x3x3) kernel", n, d, h, w, c0, c1, cout);
        return MI355_ERR_UNSUPPORTED;
    }
    g_last_conv_kernel = p.name;
    return synced(launch_wino3(cw, c, p, s), s, "conv");
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

extern "C" int mi355_conv3d_s2dma_hinted_ndhwc(const float *x_dev, const mi355_stage0_view *view, int n, int d, int h, int w, int cin,
                                               const float *weight_host, const float *bias_host, int cout, int act, float slope, int force,
                                               int s2_least_padding, float *y_dev, void *stream) {
    MI355_REQUIRE(x_dev && y_dev && weight_host && cin > 0 && cout > 0, "mi355_conv3d_s2dma_view_ndhwc: bad argument");
    MI355_REQUIRE(act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    S0View sv;
    if (view) MI355_TRY(view_from_abi(view, n, d, h, w, cin, &sv));  // (before anything touches the device: a bad view launches nothing)
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    DeviceAllocs mem;
    ConvWeights cw;
    MI355_TRY(conv_weights_upload(mem, weight_host, bias_host, cin, cin, cout, 2, false, &cw));
    ConvCall c = make_call<float>(x_dev, cin, n, d, h, w, y_dev, nullptr, act, slope);
    if (view) c.in0_view = &sv;
    c.s2_least_padding = s2_least_padding != 0;
    const char *kname = nullptr;
    const int rc = conv3d_s2dma_f32(cw, c, force != 0, s, &kname);
    g_last_conv_kernel = kname ? kname : "";
    return synced(rc, s, "conv");
}
// The plain kernel over a virtual concat [x0 | x1] (c0 and c1 multiples of 8): the chunks that come from the second tensor.
extern "C" int mi355_conv3d_s2dma_concat_ndhwc(const float *x0_dev, const float *x1_dev, int n, int d, int h, int w, int c0, int c1,
                                               const float *weight_host, const float *bias_host, int cout, int act, float slope, int force,
                                               int s2_least_padding, float *y_dev, void *stream) {
    MI355_REQUIRE(x0_dev && x1_dev && y_dev && weight_host && c0 > 0 && c1 > 0 && cout > 0, "mi355_conv3d_s2dma_concat_ndhwc: bad argument");
    MI355_REQUIRE(act != ACT_LRELU || (slope >= 0.f && slope <= 1.f), "LeakyReLU slope %g outside [0, 1]", (double)slope);
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    DeviceAllocs mem;
    ConvWeights cw;
    MI355_TRY(conv_weights_upload(mem, weight_host, bias_host, c0 + c1, c0 + c1, cout, 2, false, &cw));
    FusedOps f;
    f.x1 = x1_dev; f.c1 = c1;
    ConvCall c = make_call<float>(x0_dev, c0 + c1, n, d, h, w, y_dev, nullptr, act, slope, f);
    c.s2_least_padding = s2_least_padding != 0;
    const char *kname = nullptr;
    const int rc = conv3d_s2dma_f32(cw, c, force != 0, s, &kname);
    g_last_conv_kernel = kname ? kname : "";
    return synced(rc, s, "conv");
}

// The split pack conv_weights_upload builds for a stride-2 layer, on the host (test aid of pack_conv_weights_s2split; no device).
extern "C" int64_t mi355_conv_s2_split_pack(const float *weight_host, int cin, int cin_pad, int cout, uint16_t *out, int64_t out_elems) {
    MI355_REQUIRE(weight_host && cin > 0 && cin_pad >= cin && cin_pad % 8 == 0 && cout > 0 && cout % 64 == 0 && (out || out_elems == 0),
                  "mi355_conv_s2_split_pack: bad argument (cin_pad a multiple of 8, cout of 64)");
    std::vector<uint16_t> pack;
    pack_conv_weights_s2split(weight_host, cin, cin_pad, cout, pack);
    if (out_elems >= (int64_t)pack.size()) memcpy(out, pack.data(), pack.size() * sizeof(uint16_t));
    return (int64_t)pack.size();
}

extern "C" int mi355_conv3d_s2dma_view_ndhwc(const float *x_dev, const mi355_stage0_view *view, int n, int d, int h, int w, int cin,
                                             const float *weight_host, const float *bias_host, int cout, int act, float slope, int force,
                                             float *y_dev, void *stream) {
    return mi355_conv3d_s2dma_hinted_ndhwc(x_dev, view, n, d, h, w, cin, weight_host, bias_host, cout, act, slope, force, 0, y_dev, stream);
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
    DeviceAllocs mem;
    ConvWeights cw;
    MI355_TRY(conv_weights_upload(mem, weight_host, bias_host, c0, c0, cout, 1, false, &cw));
    ConvCall c = make_call<float>(x0_dev, c0, n, d, h, w, y_dev, nullptr, act, slope);
    c.addend = addend_dev;
    if (view) c.addend_view = &sv;
    ConvPlan p;
    if (!plan_wino3(cw, c, &p, true)) {
        set_error("mi355_conv3d_wino3_view_ndhwc: %dx%dx%dx%d, %d -> %d is not a call of the F(2x2x2,3x3x3) kernel", n, d, h, w, c0, cout);
        return MI355_ERR_UNSUPPORTED;
    }
    g_last_conv_kernel = p.name;
    return synced(launch_wino3(cw, c, p, s), s, "conv");
}

extern "C" int mi355_tconv3d_ndhwc_f16(const void *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                                       int cout, void *y_dev, void *stream) {
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const int64_t Vi = (int64_t)d * h * w;
    const size_t ybytes = (size_t)n * Vi * 8 * cout * 2, guard = guard_bytes((size_t)Vi * 8 * cout * 2);
    DeviceAllocs mem;
    void *xb = nullptr, *ybuf = nullptr;  // ybuf: guard band, the kernel's output, guard band (guards_intact)
    MI355_TRY(mem.alloc((size_t)n * Vi * cin * 2, &xb));
    MI355_TRY(mem.alloc(ybytes + 2 * guard, &ybuf));
    void *const yb = (char *)ybuf + guard;
    MI355_HIP(hipMemsetAsync(ybuf, GUARD_BYTE, ybytes + 2 * guard, s));
    MI355_HIP(hipMemsetAsync(yb, 0xFF, ybytes, s));  // all-NaN: an unstored voxel cannot pass for a result
    TConvWeights tw;
    MI355_TRY(tconv_weights_upload(mem, weight_host, cin, cout, MI355_F16, &tw));
    int rc = ndhwc_to_b8((const _Float16 *)x_dev, n, cin, Vi, (_Float16 *)xb, s);
    const char *tname = nullptr;
    if (rc == MI355_OK) rc = tconv2_mfma(tw, xb, n, d, h, w, yb, s, &tname);
    g_last_conv_kernel = tname ? tname : "";
    if (rc == MI355_OK) rc = b8_to_ndhwc((const _Float16 *)yb, n, cout, Vi * 8, (_Float16 *)y_dev, s);
    rc = synced(rc, s, "tconv");
    return rc == MI355_OK ? guards_intact(ybuf, guard, ybytes, g_last_conv_kernel.c_str()) : rc;
}

// ---- single-op entry points of the kernels around the convolutions (csrc/elementwise.hip, stage0_gather.hip, aggregate.hip): each binds the device, calls the
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
    DeviceAllocs mem;
    HeadWeights hw;
    MI355_TRY(head_weights_upload(mem, weight_host, bias_host, cin, ncls, &hw));
    hipStream_t s = (hipStream_t)stream;
    return synced(head_logits(hw, feat_dev, dtype, n, v, logits_dev, s, feat_norm(scale_dev, shift_dev, slope)), s, "head_logits");
}

// ---- the aggregation entry points and their _m2 twins, which keep the second moment (agg2_dev, laid out as agg_dev; agg_dev / cnt_dev
// come out as from the plain calls): one implementation per pair.  m2: the call is the twin - agg2_dev is required and nonlin identity
// refused here; name: the entry point, for its messages.
static int agg_operands(const char *what, const int32_t *mirrors_host, int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev,
                        float *agg2_dev, float *cnt_dev, const int32_t padded[3], AggTile *t, AggGrid *g) {
    *t = AggTile{{patch[0], patch[1], patch[2]}, nonlin, gauss_dev, {}};
    *g = AggGrid{agg_dev, agg2_dev, cnt_dev, {padded[0], padded[1], padded[2]}};
    return make_mirrors(what, mirrors_host, n_mirrors, &t->ml);
}

static int head_aggregate_abi(const char *name, bool m2, const void *feat_dev, int dtype, int cin, const float *weight_host, const float *bias_host,
                              int ncls, const float *scale_dev, const float *shift_dev, float slope, int first_sample, const int32_t *mirrors_host,
                              int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev,
                              float *cnt_dev, const int32_t padded[3], const int32_t origin[3], void *stream) {
    MI355_REQUIRE(feat_dev && weight_host && mirrors_host && patch && agg_dev && (agg2_dev || !m2) && padded && origin && first_sample >= 0,
                  "%s: bad argument", name);
    MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_F16, "unknown dtype %d", dtype);
    MI355_REQUIRE(!scale_dev == !shift_dev, "scale and shift come together");
    MI355_REQUIRE(!m2 || nonlin != MI355_NONLIN_IDENTITY, "%s: nonlin identity has no probabilities to take moments of", name);
    MI355_REQUIRE(tile_in_grid(patch, padded, origin), "%s: the tile leaves the padded grid", name);
    MI355_TRY(require_device());
    DeviceAllocs mem;
    HeadWeights hw;
    MI355_TRY(head_weights_upload(mem, weight_host, bias_host, cin, ncls, &hw));
    hipStream_t s = (hipStream_t)stream;
    AggTile t;
    AggGrid g;
    MI355_TRY(agg_operands("head_aggregate", mirrors_host, n_mirrors, patch, nonlin, gauss_dev, agg_dev, agg2_dev, cnt_dev, padded, &t, &g));
    return synced(head_aggregate(hw, feat_dev, dtype, first_sample, t, g, origin, s, feat_norm(scale_dev, shift_dev, slope)), s,
                  m2 ? "head_aggregate m2" : "head_aggregate");
}

static int logits_aggregate_abi(const char *name, bool m2, const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host,
                                int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev,
                                float *cnt_dev, const int32_t padded[3], const int32_t origin[3], void *stream) {
    MI355_REQUIRE(logits_dev && mirrors_host && patch && agg_dev && (agg2_dev || !m2) && padded && origin && first_sample >= 0, "%s: bad argument",
                  name);
    MI355_REQUIRE(!m2 || nonlin != MI355_NONLIN_IDENTITY, "%s: nonlin identity has no probabilities to take moments of", name);
    MI355_REQUIRE(tile_in_grid(patch, padded, origin), "%s: the tile leaves the padded grid", name);
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    AggTile t;
    AggGrid g;
    MI355_TRY(agg_operands("logits_aggregate", mirrors_host, n_mirrors, patch, nonlin, gauss_dev, agg_dev, agg2_dev, cnt_dev, padded, &t, &g));
    return synced(logits_aggregate(logits_dev, ncls, first_sample, t, g, origin, s), s, m2 ? "logits_aggregate m2" : "logits_aggregate");
}

static int logits_aggregate_tiles_abi(const char *name, bool m2, const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host,
                                      int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev,
                                      float *cnt_dev, const int32_t padded[3], const int32_t *origins, int n_tiles, void *stream) {
    MI355_REQUIRE(logits_dev && mirrors_host && patch && agg_dev && (agg2_dev || !m2) && padded && origins && first_sample >= 0 && n_tiles >= 1,
                  "%s: bad argument", name);
    MI355_REQUIRE(!m2 || nonlin != MI355_NONLIN_IDENTITY, "%s: nonlin identity has no probabilities to take moments of", name);
    for (int i = 0; i < n_tiles; ++i)
        MI355_REQUIRE(tile_in_grid(patch, padded, origins + 3 * (size_t)i), "%s: tile %d leaves the padded grid", name, i);
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    AggTile t;
    AggGrid g;
    MI355_TRY(agg_operands("logits_aggregate_tiles", mirrors_host, n_mirrors, patch, nonlin, gauss_dev, agg_dev, agg2_dev, cnt_dev, padded, &t, &g));
    return synced(logits_aggregate_tiles(logits_dev, ncls, first_sample, t, g, origins, n_tiles, s), s,
                  m2 ? "logits_aggregate_tiles m2" : "logits_aggregate_tiles");
}

extern "C" int mi355_head_aggregate(const void *feat_dev, int dtype, int cin, const float *weight_host, const float *bias_host, int ncls,
                                    const float *scale_dev, const float *shift_dev, float slope, int first_sample, const int32_t *mirrors_host,
                                    int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                                    const int32_t padded[3], const int32_t origin[3], void *stream) {
    return head_aggregate_abi("mi355_head_aggregate", false, feat_dev, dtype, cin, weight_host, bias_host, ncls, scale_dev, shift_dev, slope, first_sample,
                              mirrors_host, n_mirrors, patch, nonlin, gauss_dev, agg_dev, nullptr, cnt_dev, padded, origin, stream);
}
extern "C" int mi355_head_aggregate_m2(const void *feat_dev, int dtype, int cin, const float *weight_host, const float *bias_host, int ncls,
                                       const float *scale_dev, const float *shift_dev, float slope, int first_sample, const int32_t *mirrors_host,
                                       int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev,
                                       float *cnt_dev, const int32_t padded[3], const int32_t origin[3], void *stream) {
    return head_aggregate_abi("mi355_head_aggregate_m2", true, feat_dev, dtype, cin, weight_host, bias_host, ncls, scale_dev, shift_dev, slope,
                              first_sample, mirrors_host, n_mirrors, patch, nonlin, gauss_dev, agg_dev, agg2_dev, cnt_dev, padded, origin, stream);
}
extern "C" int mi355_logits_aggregate(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                                      const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                                      const int32_t padded[3], const int32_t origin[3], void *stream) {
    return logits_aggregate_abi("mi355_logits_aggregate", false, logits_dev, ncls, first_sample, mirrors_host, n_mirrors, patch, nonlin, gauss_dev, agg_dev,
                                nullptr, cnt_dev, padded, origin, stream);
}
extern "C" int mi355_logits_aggregate_m2(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                                         const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev, float *cnt_dev,
                                         const int32_t padded[3], const int32_t origin[3], void *stream) {
    return logits_aggregate_abi("mi355_logits_aggregate_m2", true, logits_dev, ncls, first_sample, mirrors_host, n_mirrors, patch, nonlin, gauss_dev,
                                agg_dev, agg2_dev, cnt_dev, padded, origin, stream);
}
extern "C" int mi355_logits_aggregate_tiles(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                                            const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                                            const int32_t padded[3], const int32_t *origins, int n_tiles, void *stream) {
    return logits_aggregate_tiles_abi("mi355_logits_aggregate_tiles", false, logits_dev, ncls, first_sample, mirrors_host, n_mirrors, patch, nonlin,
                                      gauss_dev, agg_dev, nullptr, cnt_dev, padded, origins, n_tiles, stream);
}
extern "C" int mi355_logits_aggregate_tiles_m2(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                                               const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev,
                                               float *cnt_dev, const int32_t padded[3], const int32_t *origins, int n_tiles, void *stream) {
    return logits_aggregate_tiles_abi("mi355_logits_aggregate_tiles_m2", true, logits_dev, ncls, first_sample, mirrors_host, n_mirrors, patch, nonlin,
                                      gauss_dev, agg_dev, agg2_dev, cnt_dev, padded, origins, n_tiles, stream);
}

extern "C" int mi355_cnt_add_tile(const float *gauss_dev, const int32_t patch[3], float *cnt_dev, const int32_t padded[3],
                                  const int32_t origin[3], void *stream) {
    MI355_REQUIRE(patch && cnt_dev && padded && origin, "mi355_cnt_add_tile: bad argument");
    MI355_REQUIRE(tile_in_grid(patch, padded, origin), "mi355_cnt_add_tile: the tile leaves the padded grid");
    MI355_TRY(require_device());
    hipStream_t s = (hipStream_t)stream;
    const AggTile t = {{patch[0], patch[1], patch[2]}, MI355_NONLIN_IDENTITY, gauss_dev, {}};
    const AggGrid g = {nullptr, nullptr, cnt_dev, {padded[0], padded[1], padded[2]}};
    return synced(cnt_add_tile(t, g, origin, s), s, "cnt_add_tile");
}

// The four stage-0 gather entry points.  a: the samples and the first tensor; m (null: the slabs have the tile's extent across their
// axis, stage0_gather_dense, and there is one tensor): the merged-slab geometry and the second tensor; boxes (null: the samples are the
// tiles): the sub-box form; by_box: the dense gather runs over the boxes; name: the entry point, for its messages.
static int stage0_gather_general(const char *name, const mi355_stage0_gather_args *a, const mi355_stage0_gather_merged_args *m,
                                 const mi355_stage0_gather_boxes_args *boxes, int shells_only, bool by_box, void *stream) {
    MI355_REQUIRE(a && a->wv_dev && a->out_dev && a->channels > 0 && a->channels % 4 == 0, "%s: bad argument", name);
    MI355_REQUIRE(a->n_samples > 0 && a->n_samples <= S0_MAX_SAMPLES, "%s: %d samples (max %d)", name, a->n_samples, S0_MAX_SAMPLES);
    const bool second = m && m->out2_dev;
    MI355_REQUIRE(!second || (m->wv2_dev && m->channels2 > 0 && m->channels2 % 4 == 0), "%s: bad second tensor", name);
    MI355_TRY(require_device());
    S0GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.wv = a->wv_dev; ga.out = a->out_dev;
    for (int k = 0; k < 3; ++k) { ga.slab[k] = a->slab_dev[k]; ga.P[k] = a->patch[k]; ga.Ve[k] = a->volume[k]; ga.t[k] = a->slab_thickness[k]; }
    ga.r = a->r; ga.C4 = a->channels / 4;
    if (second) {
        ga.wv2 = m->wv2_dev; ga.out2 = m->out2_dev; ga.r2 = m->r2; ga.C42 = m->channels2 / 4;
        for (int k = 0; k < 3; ++k) ga.slab2[k] = m->slab2_dev[k];
    }
    if (!m) stage0_gather_dense(&ga);
    for (int ax = 0; m && ax < 3; ++ax)
        for (int k = 0; k < 3; ++k) {
            ga.D[ax][k] = m->slab_shape[ax][k];
            MI355_REQUIRE(m->spans_volume[ax][k] == 0 || m->spans_volume[ax][k] == 1, "%s: spans_volume[%d][%d]", name, ax, k);
            ga.so[ax][k] = m->spans_volume[ax][k];
        }
    for (int i = 0; i < a->n_samples; ++i) {
        S0Sample &sm = ga.smp[i];
        sm.wv = a->samples[i].wv;
        MI355_REQUIRE(sm.wv >= 0, "%s: sample %d: whole-volume index %d", name, i, sm.wv);
        for (int k = 0; k < 3; ++k) sm.org[k] = a->samples[i].origin[k];
        for (int f = 0; f < 6; ++f) {
            sm.slab[f] = a->samples[i].slab[f];
            MI355_REQUIRE(sm.slab[f] < 0 || (a->slab_dev[f >> 1] && (!second || m->slab2_dev[f >> 1])), "%s: sample %d: face %d without a slab tensor",
                          name, i, f);
        }
    }
    if (boxes)
        for (int k = 0; k < 3; ++k) {
            ga.T[k] = boxes->tile[k];
            for (int i = 0; i < a->n_samples; ++i) ga.sub[i][k] = boxes->sub[i][k];
        }
    hipStream_t s = (hipStream_t)stream;
    if (!shells_only) return synced(stage0_gather(ga, a->n_samples, s, by_box), s, "stage0_gather");
    MI355_TRY(stage0_gather_shells(ga, a->n_samples, 0, s));
    if (ga.out2) MI355_TRY(stage0_gather_shells(ga, a->n_samples, 1, s));
    return synced(MI355_OK, s, "stage0_gather_shells");
}
extern "C" int mi355_stage0_gather(const mi355_stage0_gather_args *a, void *stream) {
    return stage0_gather_general("mi355_stage0_gather", a, nullptr, nullptr, 0, false, stream);
}
extern "C" int mi355_stage0_gather_shells(const mi355_stage0_gather_args *a, void *stream) {
    return stage0_gather_general("mi355_stage0_gather", a, nullptr, nullptr, 1, false, stream);
}
extern "C" int mi355_stage0_gather_merged(const mi355_stage0_gather_merged_args *m, int shells_only, void *stream) {
    MI355_REQUIRE(m, "mi355_stage0_gather_merged: bad argument");
    return stage0_gather_general("mi355_stage0_gather_merged", &m->base, m, nullptr, shells_only, false, stream);
}
extern "C" int mi355_stage0_gather_boxes(const mi355_stage0_gather_boxes_args *b, int shells_only, int by_box, void *stream) {
    MI355_REQUIRE(b && b->tile[0] > 0 && b->tile[1] > 0 && b->tile[2] > 0, "mi355_stage0_gather_boxes: bad argument");
    return stage0_gather_general("mi355_stage0_gather_merged", &b->merged.base, &b->merged, b, shells_only, by_box != 0, stream);
}

extern "C" int mi355_stage0_mask(float *x_dev, int n, const int32_t volume[3], const int32_t keep[3], int c, void *stream) {
    MI355_REQUIRE(x_dev && volume && keep, "mi355_stage0_mask: bad argument");
    MI355_TRY(require_device());
    const int ve[3] = {volume[0], volume[1], volume[2]}, zp[3] = {keep[0], keep[1], keep[2]};
    hipStream_t s = (hipStream_t)stream;
    return synced(stage0_mask(x_dev, n, ve, zp, c, s), s, "stage0_mask");
}
