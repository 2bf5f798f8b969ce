"""Single-op parity of the fused operand paths of the conv kernels, through mi355_conv3d_fused_ndhwc: the virtual concat
(ConvCall::in1, the first conv of every decoder stage), the producer's normalisation applied while staging (in_scale /
in_shift / in_act, the second conv of an Instance/GroupNorm stage) and the fused 1x1x1 segmentation head (head_w / head_b /
head_out, the last decoder conv).  The network runs all three on every forward; test_gpu_ops.py reaches none of them.

The reference is the composition of reference ops the network computes, in torch.float64 on the CPU: producer norm (zero
padding AFTER it), concat (upsampled half first, unet.hip forward_features), conv3d(padding=1) + bias + LeakyReLU,
statistics of that output, head.  On the fp16 path it models the staging arithmetic of conv3d_f16.hip (scale and shift
rounded to fp16, x * s + h one fp16 fma, the LeakyReLU product rounded to fp16) and the fp16 rounding of the activation the
head reads; the conv itself runs on exactly the operands the kernel stages, so what remains is summation order and the
rounding of the output - the error budget of the plain-input gates of test_gpu_ops.py, which are reused unchanged:
  conv output   |y - y_ref| <= G * max(1, max|y_ref|), G = 2e-5 (fp32), 2e-3 (fp16);
  statistics    the two 1e-4 gates of test_conv3d_norm_sums_match_reference;
  head logits   |l - l_ref| <= sum_c |hw[k,c]| * (G * max(1, max|a_ref|) + eps * |a_ref[n,c,v]|), eps = 2^-11 on fp16 (the
                kernel rounds the activation to fp16 before the head), 0 on fp32: the conv gate carried through the head's
                linear map plus one fp16 ulp per activation.
The fp16 cases without a head add the rounding gate of f16_rounding_util.py on y: the stored bits are RNE16 of the fp64
reference except at a rate of at most max(0.5 %, 4 x the rate of the same composition in torch float32), no element off by
more than one fp16 ulp.  That needs the staging model to be bit-faithful, not merely close: _f16 rounds a double ONCE, as
v_pk_fma_f16 / v_pk_mul_f16 round their exact result (torch's double -> half conversion goes through float32 and rounds
twice), and the output slope is the float32 the kernel is handed.
LeakyReLU slopes: the 2e-3-of-range gate cannot tell a slope of 0.01 - the network's own - from a zero slope, so the fp16
cases written for it run at 0.2.  The rounding gate can: the cases with the suffix _s01 repeat four of them at 0.01, and
their zero-slope mutants (M4in, M4out) are judged by it.
The CPU tests (no gpu mark) check that these gates can see the defects they are for: every mutated reference that applies
to a case (padding before the norm, one sample's scale for all, in_act toggled, negative slope 0, a channel taking its
neighbour's scale, concat halves swapped or straddled, head bias / activation / class order, statistics before the
activation) must miss the gate by at least 4x at some element, at the case's own inputs."""
import os
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_rounding_util as ru

G32, G16 = 2e-5, 2e-3           # conv output gates (test_gpu_ops.py)
SUMS_GATE = 1e-4                # statistics gates (test_conv3d_norm_sums_match_reference)
EPS16 = 2.0 ** -11              # one fp16 ulp (relative) per activation the fp16 head reads
MUTANT_MARGIN = 4.0             # a mutated reference must miss the gate by this factor
CROP = 8                        # mutants are evaluated on the 8^3 output corner (exact there; see _reference)

F32_SWITCHES = ("MI355_CONV_IMPL", "MI355_WINOGRAD", "MI355_WINO3", "MI355_S2_DMA", "MI355_SPLITK", "MI355_FUSE_NORM")
F16_SWITCHES = ("MI355_CONV_IMPL", "MI355_F16_DMA", "MI355_F16_C32", "MI355_F16_S2", "MI355_S2_DMA", "MI355_SPLITK", "MI355_FUSE_NORM")

# norm: None = no producer norm, else its in_act (0 none: ConvDropoutNonlinNorm, 1 LeakyReLU); head: classes (0 = no head);
# kernel: the instantiation the case is written for (None: whichever runs)
Case = namedtuple("Case", "name dtype shape c0 c1 cout act slope norm head stats impl kernel")


def _c(name, dtype, shape, c0, c1, cout, act=1, slope=None, norm=None, head=0, stats=False, impl="mfma", kernel=None):
    if slope is None:
        slope = 0.2 if dtype == "f16" else 0.01  # fp16: G16 cannot see a zero slope at 0.01; the _s01 cases can (module docstring)
    return Case(name, dtype, shape, c0, c1, cout, act, slope, norm, head, stats, impl, kernel)


CASES = [
    # ---- fp32.  F(2x2x2,3x3x3): whole 4 x 8 x 8 tiles, 16-channel chunks on both halves (conv3d_wino3.hip wino3_fits)
    _c("w3_cat", "f32", (2, 32, 64, 64), 32, 32, 32, kernel="conv3_f32_wino3_kernel<0, false>"),
    _c("w3_cat_uneven", "f32", (2, 32, 64, 64), 48, 16, 64, act=0, kernel="conv3_f32_wino3_kernel<0, false>"),
    _c("w3_cat_head", "f32", (2, 32, 64, 64), 32, 32, 32, head=3, kernel="conv3_f32_wino3_kernel<1, false>"),
    _c("w3_cat_stats", "f32", (2, 32, 64, 64), 32, 32, 32, stats=True, kernel="conv3_f32_wino3_kernel<2, false>"),
    _c("w3_norm_lrelu", "f32", (2, 32, 64, 64), 32, 0, 32, act=0, norm=1, stats=True, kernel="conv3_f32_wino3_kernel<2, true>"),
    _c("w3_norm_none", "f32", (2, 32, 64, 64), 32, 0, 32, act=1, norm=0, stats=True, kernel="conv3_f32_wino3_kernel<2, true>"),
    # deep-level rule (160 units of 20 chunks): one z tile, every brick on all six faces; slope 0.2
    _c("w3_norm_deep", "f32", (8, 8, 8, 8), 320, 0, 320, act=0, slope=0.2, norm=1, stats=True, kernel="conv3_f32_wino3_kernel<2, true>"),
    # F(2x2,3x3): z not a multiple of 4
    _c("w2_cat", "f32", (2, 30, 64, 128), 16, 16, 32, kernel="conv3_f32_wino2_kernel<0>"),
    _c("w2_cat_head", "f32", (2, 30, 64, 128), 16, 16, 32, head=4, kernel="conv3_f32_wino2_kernel<1>"),
    _c("w2_cat_stats", "f32", (2, 30, 64, 128), 16, 16, 32, stats=True, kernel="conv3_f32_wino2_kernel<2>"),
    # pipelined kernel (small launches): head at Cout 32 and 64; at (1,16,16,32) the 64-cout head used to be split over two
    # 32-cout workgroups that overwrote each other's partial logits
    _c("pipe_cat_head32_small", "f32", (1, 16, 16, 32), 32, 32, 32, head=3, kernel="conv3_f32_mfma_pipe_kernel<1, 1>"),
    _c("pipe_cat_head64_small", "f32", (1, 16, 16, 32), 32, 32, 64, head=3, kernel="conv3_f32_mfma_pipe_kernel<2, 2>"),
    _c("pipe_cat_head64", "f32", (2, 32, 32, 64), 32, 32, 64, head=3, slope=0.2, kernel="conv3_f32_mfma_pipe_kernel<2, 2>"),
    _c("pipe_cat_head32", "f32", (2, 32, 32, 64), 32, 32, 32, head=2, kernel="conv3_f32_mfma_pipe_kernel<2, 1>"),
    _c("pipe_cat_stats_small", "f32", (1, 16, 16, 32), 32, 32, 32, stats=True, kernel="conv3_f32_mfma_pipe_kernel<1, 1>"),
    _c("pipe_cat_stats", "f32", (2, 32, 32, 64), 32, 32, 32, stats=True, kernel="conv3_f32_mfma_pipe_kernel<2, 1>"),
    _c("splitk_cat", "f32", (2, 4, 4, 4), 160, 160, 320, kernel="conv3_f32_mfma_kernel<1, 8, 2, 2> split-K"),
    _c("direct_cat", "f32", (1, 6, 5, 7), 8, 16, 32, impl="direct", kernel="conv3_direct_kernel"),
    # a concat split that is a multiple of 8 only, on a volume the 16-channel-chunk kernels would take: correct on whichever
    # kernel runs, or refused
    _c("straddle_cat", "f32", (2, 30, 64, 128), 24, 40, 32),
    # ---- fp16.  LDS-DMA kernels: 8 x 8 x 8 tiles
    _c("c32_cat", "f16", (8, 32, 32, 32), 16, 16, 32, kernel="conv3_f16_c32_kernel<false, false, false>"),
    _c("c32_cat_stats", "f16", (8, 32, 32, 32), 16, 16, 32, stats=True, kernel="conv3_f16_c32_kernel<true, false, false>"),
    _c("c32_cat_head", "f16", (8, 32, 32, 32), 16, 16, 32, head=3, kernel="conv3_f16_c32_kernel<false, false, true>"),
    _c("c32_norm_lrelu_stats", "f16", (8, 32, 32, 32), 32, 0, 32, act=0, norm=1, stats=True, kernel="conv3_f16_c32_kernel<true, true, false>"),
    _c("c32_norm_none_stats", "f16", (8, 32, 32, 32), 32, 0, 32, act=1, norm=0, stats=True, kernel="conv3_f16_c32_kernel<true, true, false>"),
    _c("c32_norm_lrelu", "f16", (8, 32, 32, 32), 32, 0, 32, act=1, norm=1, kernel="conv3_f16_c32_kernel<false, true, false>"),
    _c("c32_norm_none", "f16", (8, 32, 32, 32), 32, 0, 32, act=1, norm=0, kernel="conv3_f16_c32_kernel<false, true, false>"),
    _c("dma_cat", "f16", (8, 32, 32, 32), 32, 32, 64, kernel="conv3_f16_dma_kernel<false, false>"),
    _c("dma_cat_stats", "f16", (8, 32, 32, 32), 32, 32, 64, stats=True, kernel="conv3_f16_dma_kernel<true, false>"),
    _c("dma_norm_lrelu_stats", "f16", (8, 32, 32, 32), 64, 0, 64, act=0, norm=1, stats=True, kernel="conv3_f16_dma_kernel<true, true>"),
    _c("dma_norm_none", "f16", (8, 32, 32, 32), 64, 0, 64, act=1, norm=0, kernel="conv3_f16_dma_kernel<false, true>"),
    # register-staged pipelined kernel (too few 8^3 tiles for the LDS-DMA kernels)
    _c("pipe2_norm32", "f16", (2, 16, 16, 32), 32, 0, 32, act=1, norm=1, kernel="conv3_f16_mfma_pipe_kernel<2, 1, false, true, 1, true>"),
    _c("pipe2_norm32_none_stats", "f16", (2, 16, 16, 32), 32, 0, 32, act=1, norm=0, stats=True, kernel="conv3_f16_mfma_pipe_kernel<2, 1, false, true, 1, true>"),
    _c("pipe2_norm64_stats", "f16", (2, 16, 16, 32), 64, 0, 64, act=0, norm=1, stats=True, kernel="conv3_f16_mfma_pipe_kernel<2, 2, false, true, 1, true>"),
    _c("pipe2_norm_cat", "f16", (2, 16, 16, 32), 32, 32, 32, act=1, norm=1, kernel="conv3_f16_mfma_pipe_kernel<2, 1, false, true, 1, true>"),
    # 640 tiles of 4 x 4 x 32 voxels; d = 20 is not a multiple of 8, so the LDS-DMA kernels decline
    _c("pipe4_norm_stats", "f16", (2, 20, 64, 128), 32, 0, 32, act=0, norm=1, stats=True, kernel="conv3_f16_mfma_pipe_kernel<4, 1, false, true, 1, true>"),
    _c("pipe2_cat_head", "f16", (1, 16, 16, 32), 32, 32, 32, head=3, kernel="conv3_f16_mfma_pipe_kernel<2, 1, true, false, 1, false>"),
    _c("pipe4_head", "f16", (2, 20, 64, 128), 32, 0, 32, head=4, kernel="conv3_f16_mfma_pipe_kernel<4, 1, true, false, 1, true>"),
    _c("pipe4_head_ragged", "f16", (2, 19, 64, 120), 32, 0, 32, head=2, kernel="conv3_f16_mfma_pipe_kernel<4, 1, true, false, 1, false>"),
    _c("splitk_cat_f16", "f16", (2, 4, 4, 4), 160, 160, 320, kernel="conv3_f16_mfma_kernel<1, 2, 2> split-K"),
    # ---- fp16 at the network's own slope 0.01 (output activation; producer activation on the three staging paths)
    _c("c32_cat_s01", "f16", (8, 32, 32, 32), 16, 16, 32, slope=0.01, kernel="conv3_f16_c32_kernel<false, false, false>"),
    _c("c32_norm_lrelu_s01", "f16", (8, 32, 32, 32), 32, 0, 32, act=1, slope=0.01, norm=1, kernel="conv3_f16_c32_kernel<false, true, false>"),
    _c("dma_norm_lrelu_stats_s01", "f16", (8, 32, 32, 32), 64, 0, 64, act=0, slope=0.01, norm=1, stats=True, kernel="conv3_f16_dma_kernel<true, true>"),
    _c("pipe2_norm32_s01", "f16", (2, 16, 16, 32), 32, 0, 32, act=1, slope=0.01, norm=1, kernel="conv3_f16_mfma_pipe_kernel<2, 1, false, true, 1, true>"),
]
EXPECT_KERNEL = {c.name: c.kernel for c in CASES if c.kernel}

#: every fused instantiation (and fp32 kernel family) that must be asserted by at least one case
REQUIRED_KERNELS = [
    "conv3_f32_wino3_kernel<0, false>", "conv3_f32_wino3_kernel<1, false>", "conv3_f32_wino3_kernel<2, false>",
    "conv3_f32_wino3_kernel<2, true>",
    "conv3_f32_wino2_kernel<0>", "conv3_f32_wino2_kernel<1>", "conv3_f32_wino2_kernel<2>",
    "conv3_f32_mfma_pipe_kernel<1, 1>", "conv3_f32_mfma_pipe_kernel<2, 1>", "conv3_f32_mfma_pipe_kernel<2, 2>",
    "conv3_f32_mfma_kernel<1, 8, 2, 2> split-K", "conv3_direct_kernel",
    "conv3_f16_c32_kernel<false, false, false>", "conv3_f16_c32_kernel<true, false, false>",
    "conv3_f16_c32_kernel<false, false, true>", "conv3_f16_c32_kernel<true, true, false>",
    "conv3_f16_c32_kernel<false, true, false>",
    "conv3_f16_dma_kernel<false, false>", "conv3_f16_dma_kernel<true, false>", "conv3_f16_dma_kernel<true, true>",
    "conv3_f16_dma_kernel<false, true>",
    "conv3_f16_mfma_pipe_kernel<2, 1, false, true, 1, true>", "conv3_f16_mfma_pipe_kernel<2, 2, false, true, 1, true>",
    "conv3_f16_mfma_pipe_kernel<4, 1, false, true, 1, true>",
    "conv3_f16_mfma_pipe_kernel<2, 1, true, false, 1, false>", "conv3_f16_mfma_pipe_kernel<4, 1, true, false, 1, true>",
    "conv3_f16_mfma_pipe_kernel<4, 1, true, false, 1, false>",
    "conv3_f16_mfma_kernel<1, 2, 2> split-K",
]


def _inputs(case):
    """Inputs of a case, deterministic per case name.  x0 = mu + sigma z per (n, c) when a producer norm applies, with
    scale = gamma / sigma and shift = beta - mu gamma / sigma (all different per sample); otherwise x0 ~ N(0, 1).  x1 ~ N(0, 1)
    (a skip tensor normalised when it was written).  Weights N(0,1)/sqrt(27 Cin), bias N(0,1), head_w N(0,1)/sqrt(Cout),
    |head_b| in [0.5, 1.5].  fp16 cases: x0, x1 and the weights are rounded to fp16 here, so the reference and the kernel see
    the same operands."""
    rs = np.random.RandomState(zlib.crc32(case.name.encode()))
    n, d, h, w = case.shape
    cin = case.c0 + case.c1
    z = rs.standard_normal((n, d, h, w, case.c0))
    inp = {}
    if case.norm is not None:
        mu, sigma = rs.uniform(-2, 2, (n, case.c0)), rs.uniform(0.5, 2, (n, case.c0))
        gamma, beta = rs.uniform(0.5, 1.5, (n, case.c0)), rs.uniform(-1, 1, (n, case.c0))
        x0 = mu[:, None, None, None, :] + sigma[:, None, None, None, :] * z
        inp["s"] = (gamma / sigma).astype(np.float32)
        inp["h"] = (beta - mu * gamma / sigma).astype(np.float32)
    else:
        x0 = z
    x1 = rs.standard_normal((n, d, h, w, case.c1)) if case.c1 else None
    wt = rs.standard_normal((case.cout, cin, 3, 3, 3)) / np.sqrt(27 * cin)
    dt = np.float16 if case.dtype == "f16" else np.float32
    inp["x0"] = x0.astype(dt)
    inp["x1"] = None if x1 is None else x1.astype(dt)
    inp["w"] = wt.astype(dt).astype(np.float32)
    inp["b"] = rs.standard_normal(case.cout).astype(np.float32)
    if case.head:
        inp["hw"] = (rs.standard_normal((case.head, case.cout)) / np.sqrt(case.cout)).astype(np.float32)
        inp["hb"] = (rs.choice([-1.0, 1.0], case.head) * rs.uniform(0.5, 1.5, case.head)).astype(np.float32)
    return inp


def _t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _f16(t):
    """a double rounded to fp16 ONCE (numpy; t.to(torch.float16) goes through float32 and rounds twice)"""
    return torch.from_numpy(t.contiguous().numpy().astype(np.float16).astype(np.float64))


def _lrelu(t, slope):
    return torch.maximum(t, t * slope)  # slope in [0, 1]


def _in_norm(x, s, h, in_act, slope, f16):
    """the producer's normalisation + activation as the kernels stage it; x [N,C,D,H,W], s / h [N,C] fp64"""
    s, h = s[:, :, None, None, None], h[:, :, None, None, None]
    if f16:  # conv3d_f16.hip in_affine: fp16 scale / shift, one fp16 fma, LeakyReLU product rounded to fp16
        t = _f16(x * _f16(s) + _f16(h))  # (exact in fp64 before the rounding: fp16 x fp16 + fp16)
        return torch.maximum(t, _f16(t * float(np.float16(slope)))) if in_act else t
    t = x * s + h
    return _lrelu(t, slope) if in_act else t


def _straddled(x0, x1):
    """cat(x0, x1) as a kernel reads it that picks in0 or in1 once per 16-channel chunk and indexes the chosen tensor
    with its own channel count: a chunk that starts in x0 runs on into the next voxel's channels (x0 [N,D,H,W,C0], NDHWC)"""
    n, d, h, w, c0 = x0.shape
    c1 = x1.shape[4]
    V = d * h * w
    f0 = np.concatenate([x0.reshape(n, -1), np.zeros((n, 16), x0.dtype)], 1)
    f1 = np.concatenate([x1.reshape(n, -1), np.zeros((n, 16), x1.dtype)], 1)
    out = np.zeros((n, V, c0 + c1), x0.dtype)
    v = np.arange(V)[:, None]
    for cg in range(0, c0 + c1, 16):
        if cg < c0:
            out[:, :, cg:cg + 16] = f0[:, v * c0 + cg + np.arange(16)]
        else:
            out[:, :, cg:cg + 16] = f1[:, v * c1 + cg - c0 + np.arange(16)]
    return out.reshape(n, d, h, w, c0 + c1)


def _reference(case, inp, mut=(), crop=None, dtype=torch.float64):
    """fp64 reference of one case, optionally with one mutation (see _mutations).  Returns y = act(conv) [N,Cout,D,H,W],
    z (the conv + bias before the activation), sums [N,Cout,2] when the case has statistics, and logits [N,K,D,H,W] plus the
    activation `a` the head reads when it has a head.  crop = k: only the outputs [:k, :k, :k] of the corner, computed
    exactly from the (padded) inputs they depend on.  dtype = torch.float32: the same staged operands (exact in fp16, so in
    float32), conv + bias + LeakyReLU in torch's float32 - the independent fp32 implementation of the rounding gate."""
    f16 = case.dtype == "f16"
    pad = lambda t: F.pad(t, (1, 1, 1, 1, 1, 1))  # noqa: E731
    ncdhw = lambda a: _t64(a).permute(0, 4, 1, 2, 3)  # noqa: E731
    if "M6straddle" in mut:
        xin = pad(ncdhw(_straddled(inp["x0"], inp["x1"])))
    else:
        x0 = ncdhw(inp["x0"])
        if case.norm is not None:
            s, h = _t64(inp["s"]), _t64(inp["h"])
            in_act = case.norm ^ ("M3" in mut)
            in_slope = 0.0 if "M4in" in mut else case.slope
            if "M2" in mut:
                s, h = s[:1].expand_as(s), h[:1].expand_as(h)
            if "M5" in mut:  # channel 17 (second 16-channel chunk) takes channel 16's scale and shift
                s, h = s.clone(), h.clone()
                s[:, 17], h[:, 17] = s[:, 16], h[:, 16]
            if "M1" in mut:  # padding before the norm: border taps see A_in(shift)
                x0p = _in_norm(pad(x0), s, h, in_act, in_slope, f16)
            else:
                x0p = pad(_in_norm(x0, s, h, in_act, in_slope, f16))
        else:
            x0p = pad(x0)
        parts = [x0p] + ([pad(ncdhw(inp["x1"]))] if case.c1 else [])
        if "M6swap" in mut:
            parts = parts[::-1]
        xin = torch.cat(parts, 1)
    if crop is not None:
        xin = xin[:, :, :crop + 2, :crop + 2, :crop + 2]
    z = F.conv3d(xin.to(dtype), _t64(inp["w"]).to(dtype), _t64(inp["b"]).to(dtype))
    slope = 0.0 if ("M4out" in mut or "M4head" in mut) else float(np.float32(case.slope))  # (the C ABI takes a float)
    y = _lrelu(z, slope) if case.act and "M7act" not in mut else z
    res = {"y": y, "z": z}
    if case.stats:
        res["sums"] = _sums(y)
    if case.head:
        a = _f16(y) if f16 else y  # the fp16 kernel rounds the activation before the head (conv3d_f16.hip HEAD)
        hw, hb = _t64(inp["hw"]), _t64(inp["hb"])
        if "M7bias" in mut:
            hb = torch.zeros_like(hb)
        if "M7rot" in mut:
            hw, hb = torch.roll(hw, 1, 0), torch.roll(hb, 1, 0)
        res["a"], res["abs_hw"] = a, _t64(np.abs(inp["hw"]))
        res["logits"] = torch.einsum("kc,ncdhw->nkdhw", hw, a) + hb[None, :, None, None, None]
    return res


def _sums(y):
    return torch.stack([y.sum(dim=(2, 3, 4)), (y * y).sum(dim=(2, 3, 4))], -1)


def _mutations(case):
    """the mutated references that apply to a case"""
    m = []
    if case.norm is not None:
        m += ["M1", "M3"]
        if case.shape[0] > 1:
            m.append("M2")
        if case.norm == 1:
            m.append("M4in")
        if case.c0 >= 32:
            m.append("M5")
    if case.c1:
        m.append("M6swap")
        if (case.c0 % 16 or case.c1 % 16) and (case.c0 + case.c1) % 16 == 0:
            m.append("M6straddle")
    if case.act and not case.head:
        m.append("M4out")
    if case.head:
        m.append("M7bias")
        if case.head >= 2:
            m.append("M7rot")
        if case.act:
            m += ["M4head", "M7act"]
    if case.stats and case.act:
        m.append("M8")
    return m


def _gate(case):
    return G16 if case.dtype == "f16" else G32


def _rounding_gated(case):
    """fp16 cases whose output is the fp16 y (the head cases store fp32 logits)"""
    return case.dtype == "f16" and not case.head


def _by_rounding_gate(case, m):
    """the zero-slope mutants of the slope-0.01 cases: below G16 (module docstring), judged by the rounding gate"""
    return case.name.endswith("_s01") and m in ("M4in", "M4out")


def _nchw16(t):
    return t.contiguous().numpy().astype(np.float16)


def _out_ratio(case, ref, got, crop=None):
    """max over elements of |got - ref| / gate; `got` is y [N,Cout,...] or logits [N,K,...] (fp64, NCDHW), compared with the
    [:crop]^3 corner of the full reference `ref` (whose maximum sets the gate)"""
    g = _gate(case)
    sl = (slice(None), slice(None)) + (slice(None, crop),) * 3
    if case.head:
        M = max(1.0, float(ref["a"].abs().max()))
        eps = EPS16 if case.dtype == "f16" else 0.0
        bound = torch.einsum("kc,ncdhw->nkdhw", ref["abs_hw"], g * M + eps * ref["a"][sl].abs())
        return float(((got - ref["logits"][sl]).abs() / bound).max())
    M = max(1.0, float(ref["y"].abs().max()))
    return float((got - ref["y"][sl]).abs().max()) / (g * M)


def _sums_ratio(ref_y, sums):
    """max of the two statistics errors of test_conv3d_norm_sums_match_reference, divided by their gate"""
    ref = _sums(ref_y)
    V = ref_y.shape[2] * ref_y.shape[3] * ref_y.shape[4]
    mean_ref, msq_ref = ref[..., 0] / V, ref[..., 1] / V
    mean_err = ((sums[..., 0] / V - mean_ref).abs() / msq_ref.sqrt()).max()
    msq_err = ((sums[..., 1] / V - msq_ref).abs() / msq_ref).max()
    return float(max(mean_err, msq_err)) / SUMS_GATE


_INPUTS = {}


def _inputs_cache(case):
    if case.name not in _INPUTS:
        _INPUTS.clear()  # one case at a time: the large ones are ~100 MB
        _INPUTS[case.name] = _inputs(case)
    return _INPUTS[case.name]


# ------------------------------------------------------------------ CPU: the case table and the power of the gates
def test_required_kernels_are_in_the_expectation_table():
    expected = set(EXPECT_KERNEL.values())
    missing = [k for k in REQUIRED_KERNELS if k not in expected]
    assert not missing, missing
    assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reference_mutations_exceed_the_gates(case):
    """Every mutated reference that applies to the case misses the case's gate by >= 4x at some element.  Mutants of the
    output are evaluated on the 8^3 corner (which holds three of the six borders): an element there that misses the gate
    is one of the full output.  M4in and M4out of the _s01 cases are judged by the rounding gate instead: the mutant's y,
    rounded to fp16 once, mismatches the reference's bits on that corner at >= 3x the cap the corner's references set."""
    inp = _inputs_cache(case)
    ref = _reference(case, inp)
    ratios, rates = {}, {}
    for m in _mutations(case):
        if m == "M8":  # statistics of the conv before its activation: the sums gate
            ratios[m] = _sums_ratio(ref["y"], _sums(ref["z"]))
            continue
        mut = _reference(case, inp, (m,), crop=CROP)
        if _by_rounding_gate(case, m):
            ref64 = _reference(case, inp, crop=CROP)["y"].numpy()
            cap, _ = ru.gate(_reference(case, inp, crop=CROP, dtype=torch.float32)["y"].numpy(), ref64)
            rates[m] = ru.rounding_report(_nchw16(mut["y"]), ref64)[0] / cap
            continue
        ratios[m] = _out_ratio(case, ref, mut["logits"] if case.head else mut["y"], crop=CROP)
    print(f"MUTANTS {case.name}: " + " ".join(f"{m}={r:.3g}" for m, r in ratios.items())
          + "".join(f" {m}={r:.3g} x the mismatch cap" for m, r in rates.items()))
    assert ratios or rates, "no mutation applies"
    weak = {m: r for m, r in ratios.items() if not r >= MUTANT_MARGIN}
    assert not weak, f"mutants within {MUTANT_MARGIN}x of the gate: {weak}"
    weak = {m: r for m, r in rates.items() if not r >= ru.MUTANT_FACTOR}
    assert not weak, f"mutants within {ru.MUTANT_FACTOR}x of the mismatch cap: {weak}"
    if case.name.endswith("_s01"):
        assert rates, "a slope-0.01 case without a zero-slope mutant"


# ------------------------------------------------------------------ GPU: every fused instantiation against the reference
def _switched(case):
    return any(k in os.environ for k in (F16_SWITCHES if case.dtype == "f16" else F32_SWITCHES))


def _run(amd, gpu, case, inp):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    return amd.ops.conv3d_fused_ndhwc(
        dev(inp["x0"]), inp["w"], inp["b"], x1=dev(inp["x1"]),
        in_scale=dev(inp.get("s")), in_shift=dev(inp.get("h")), in_act=case.norm or 0,
        head_w=dev(inp.get("hw")), head_b=dev(inp.get("hb")), stats=case.stats, act=case.act, slope=case.slope, impl=case.impl)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_fused_conv_matches_reference(amd, gpu, case):
    inp = _inputs_cache(case)
    ref = _reference(case, inp)
    try:
        out, sums = _run(amd, gpu, case, inp)
    except amd._lib.Mi355Error as e:
        if case.kernel is None:  # (the straddle case: a refusal is an acceptable outcome, wrong numbers are not)
            assert str(e).strip(), "refusal without a message"
            print(f"PARITY {case.name} refused: {e}")
            return
        raise
    ran = amd.ops.last_conv_kernel()
    torch.cuda.synchronize()
    tail = torch.as_strided(out, (amd.ops.FUSED_GUARD,), (1,), out.numel()).float().cpu().numpy()
    got = out.double().cpu()
    if not case.head:
        got = got.permute(0, 4, 1, 2, 3)
    bad = int((~torch.isfinite(got)).sum())
    assert bad == 0, f"{bad} non-finite outputs of {got.numel()} ({ran}): voxels left unstored or overflow"
    assert np.isnan(tail).all(), f"{int((~np.isnan(tail)).sum())} guard elements behind the output were written ({ran})"
    r_out = _out_ratio(case, ref, got)
    line = f"PARITY {case.name} [{ran}] out={r_out:.3g}"
    r_sums = None
    if case.stats:
        r_sums = _sums_ratio(ref["y"], sums.cpu())
        line += f" sums={r_sums:.3g}"
    print(line)
    assert r_out <= 1.0, f"output error {r_out:.3g} x the gate ({ran})"
    if case.stats:
        assert r_sums <= 1.0, f"statistics error {r_sums:.3g} x the gate ({ran})"
    if case.kernel and not _switched(case):
        assert ran == case.kernel, ran
    if _rounding_gated(case):
        ref32 = _reference(case, inp, dtype=torch.float32)["y"].numpy()
        mismatch, cap, worst, worst_cap = ru.check(f"{case.name} [{ran}]", out.cpu().permute(0, 4, 1, 2, 3).contiguous().numpy(), ref32, ref["y"].numpy())
        assert mismatch <= cap, f"{mismatch:.3e} of the outputs are not RNE16 of the fp64 reference, cap {cap:.3e} ({ran})"
        assert worst <= worst_cap, f"an output is {worst:.3f} fp16 ulps from the fp64 reference ({ran})"


# ------------------------------------------------------------------ GPU: refused combinations
def _plain_conv_still_works(amd, gpu, dtype):
    """a plain conv on the same thread after a refusal"""
    rs = np.random.RandomState(5)
    x = rs.standard_normal((1, 8, 8, 16, 32)).astype(np.float16 if dtype == "f16" else np.float32)
    wt = (rs.standard_normal((32, 32, 3, 3, 3)) / np.sqrt(27 * 32)).astype(np.float32)
    if dtype == "f16":
        wt = wt.astype(np.float16).astype(np.float32)
    b = rs.standard_normal(32).astype(np.float32)
    y = amd.ops.conv3d_ndhwc(torch.from_numpy(x).to(gpu), wt, b, act=1, slope=0.01).double().cpu().permute(0, 4, 1, 2, 3)
    ref = _lrelu(F.conv3d(_t64(x).permute(0, 4, 1, 2, 3), _t64(wt), _t64(b), padding=1), 0.01)
    g = G16 if dtype == "f16" else G32
    assert float((y - ref).abs().max()) <= g * max(1.0, float(ref.abs().max()))


REFUSALS = [
    # (id, dtype, (n, d, h, w), c0, c1, cout, stride, norm, head classes, stats, impl)
    ("f32_norm_wino3_declines", "f32", (1, 16, 16, 32), 32, 0, 32, 1, 1, 0, True, "mfma"),
    ("f32_norm_without_stats", "f32", (2, 32, 64, 64), 32, 0, 32, 1, 1, 0, False, "mfma"),
    ("f32_norm_with_concat", "f32", (2, 32, 64, 64), 32, 32, 32, 1, 1, 0, True, "mfma"),
    ("f32_norm_with_head", "f32", (2, 32, 64, 64), 32, 0, 32, 1, 1, 3, False, "mfma"),
    ("f32_head_5_classes", "f32", (2, 32, 64, 64), 32, 32, 32, 1, None, 5, False, "mfma"),
    ("f32_head_with_stats", "f32", (2, 32, 64, 64), 32, 32, 32, 1, None, 3, True, "mfma"),
    ("f32_direct_head", "f32", (1, 6, 5, 7), 8, 16, 32, 1, None, 3, False, "direct"),
    ("f32_direct_norm", "f32", (1, 6, 5, 8), 16, 0, 32, 1, 1, 0, False, "direct"),
    ("f32_direct_stats", "f32", (1, 6, 5, 7), 8, 16, 32, 1, None, 0, True, "direct"),
    ("f16_norm_stride2", "f16", (2, 16, 16, 32), 32, 0, 64, 2, 1, 0, True, "mfma"),
    ("f16_norm_ragged", "f16", (2, 15, 16, 32), 32, 0, 32, 1, 1, 0, True, "mfma"),
    ("f16_head_cout64", "f16", (1, 16, 16, 32), 32, 32, 64, 1, None, 3, False, "mfma"),
    ("f16_head_stride2", "f16", (1, 16, 16, 32), 32, 0, 32, 2, None, 3, False, "mfma"),
    ("f16_head_with_norm", "f16", (1, 16, 16, 32), 32, 0, 32, 1, 1, 3, False, "mfma"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("spec", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_fused_conv_refusals(amd, gpu, spec):
    name, dtype, (n, d, h, w), c0, c1, cout, stride, norm, head, stats, impl = spec
    rs = np.random.RandomState(zlib.crc32(name.encode()))
    dt = torch.float16 if dtype == "f16" else torch.float32
    x0 = torch.randn((n, d, h, w, c0), dtype=dt, device=gpu)
    x1 = torch.randn((n, d, h, w, c1), dtype=dt, device=gpu) if c1 else None
    wt = (rs.standard_normal((cout, c0 + c1, 3, 3, 3)) / np.sqrt(27 * (c0 + c1))).astype(np.float32)
    kw = {}
    if norm is not None:
        kw.update(in_scale=torch.ones((n, c0), device=gpu), in_shift=torch.zeros((n, c0), device=gpu), in_act=norm)
    if head:
        kw.update(head_w=torch.randn((head, cout), device=gpu), head_b=torch.randn((head,), device=gpu))
    with pytest.raises(amd._lib.Mi355Error) as e:
        amd.ops.conv3d_fused_ndhwc(x0, wt, None, x1=x1, stats=stats, stride=stride, act=1, slope=0.01, impl=impl, **kw)
    msg = str(e.value).split(":", 1)[-1].strip()
    print(f"REFUSED {name}: {msg}")
    assert msg and msg != "?", str(e.value)
    _plain_conv_still_works(amd, gpu, dtype)
