"""One GPU case per 3x3x3 conv kernel instantiation that the planner selects and no older test runs (plain data: no GPU import).

tests/test_gpu_ops.py and tests/test_gpu_conv_fused.py judge a conv kernel on random data (2e-5 / 2e-3 of the range) once a case
reaches it; neither asks whether every row of the four row tables (f32_rows, wino3_rows, f16_rows, s2h_rows) is reached.  (The
Winograd rows, which those modules declare and CASES therefore leaves out, have their exact-integer runs and guard bands in a
table of their own: tests/wino_exact_util.py GPU_CASES, run by tests/test_gpu_wino_exact.py.)  CASES below are written for the rows
that a sweep of the dry-run planner selects and that no case of those modules declares; tests/test_conv_rows_cpu.py keeps that
set closed (a row the planner can select needs a GPU case; a row nothing selects needs an entry in UNPLANNED with its reason) and
tests/test_gpu_conv_rows.py runs every case.

A NEW ROW IN A TABLE NEEDS A CASE HERE (or, if only a test entry point launches it, a line in UNPLANNED): shrink a call that
reaches it with ``brats_amd.ops.conv3d_plan`` until the fp64 CPU reference takes a second or two, and add a ragged and a
whole-tile shape, with and without statistics where the kernel takes them as a run-time argument."""
import itertools
import os
import zlib
from collections import namedtuple

import numpy as np

#: the A/B switches of the conv dispatch (conv_plan.h env_switch / conv_impl), read once per process
SWITCHES = ("MI355_CONV_IMPL", "MI355_WINOGRAD", "MI355_WINO3", "MI355_S2_DMA", "MI355_SPLITK", "MI355_FUSE_NORM", "MI355_F16_DMA",
            "MI355_F16_C32", "MI355_F16_S2")

# env: the switches the case needs ({} = defaults); shape = (N, D, H, W); kernel: the planner's name, " split-K" included;
# ragged: the output volume is not a whole number of the plan's tiles (what the sentinel check is about; asserted on the CPU)
Case = namedtuple("Case", "name env dtype shape cin cout stride act slope stats kernel ragged")

IMPL0 = {"MI355_CONV_IMPL": "0"}
WINOGRAD0 = {"MI355_WINOGRAD": "0"}


def _c(name, env, dtype, shape, cin, cout, kernel, ragged, stats=False, act=1, slope=0.01, stride=1):
    return Case(name, dict(env), dtype, tuple(shape), cin, cout, stride, act, slope, stats, kernel, ragged)


def _trio(prefix, env, dtype, cin, cout, kernel, **kw):
    """the three small shapes of a one-tile-per-workgroup row: one ragged tile; several tiles, ragged in z, y and x, with
    statistics; one whole 8 x 8 x 4 tile"""
    return [_c(prefix + "_ragged", env, dtype, (1, 5, 6, 7), cin, cout, kernel, True, **kw),
            _c(prefix + "_tiles_stats", env, dtype, (2, 9, 12, 20), cin, cout, kernel, True, stats=True, act=0, **kw),
            _c(prefix + "_whole", env, dtype, (1, 8, 8, 4), cin, cout, kernel, False, **kw)]


F32_THIN_1, F32_THIN_2 = "conv3_f32_mfma_kernel<1, 16, 4, 1>", "conv3_f32_mfma_kernel<1, 16, 4, 2>"
F16_PIPE2_RAGGED = "conv3_f16_mfma_pipe_kernel<2, 1, false, false, 1, false>"
F16_PIPE4_RAGGED = "conv3_f16_mfma_pipe_kernel<4, 1, false, false, 1, false>"
F16_PIPE4_WHOLE = "conv3_f16_mfma_pipe_kernel<4, 1, false, false, 1, true>"

CASES = [
    # ---- default switches
    # 512-voxel tiles on 16-channel chunks: a stride-1 launch of >= 512 (tile, cout block) units whose x extent is below 16 (the
    # Winograd kernels decline it).  x = 12 leaves a quarter of every tile's lanes past the edge
    _c("f32_thin_nf1", {}, "f32", (16, 32, 32, 12), 16, 32, F32_THIN_1, True),
    _c("f32_thin_nf1_cout96_stats", {}, "f32", (30, 9, 14, 12), 16, 96, F32_THIN_1, True, stats=True, act=0),   # ragged in z, y, x; 3 cout blocks
    _c("f32_thin_nf2", {}, "f32", (64, 9, 14, 12), 16, 64, F32_THIN_2, True, act=0),
    _c("f32_thin_nf2_stats", {}, "f32", (43, 10, 21, 12), 16, 64, F32_THIN_2, True, stats=True),
    # the fp16 register-staged pipelined kernels off whole tiles (WHOLE = false): every ragged fp16 launch with Cout = 32 or 96
    _c("f16_pipe2_ragged", {}, "f16", (1, 5, 6, 7), 16, 32, F16_PIPE2_RAGGED, True),
    _c("f16_pipe2_ragged_tiles_stats", {}, "f16", (2, 9, 12, 20), 16, 32, F16_PIPE2_RAGGED, True, stats=True, act=0),
    _c("f16_pipe4_ragged_cout96", {}, "f16", (16, 9, 7, 35), 16, 96, F16_PIPE4_RAGGED, True),
    _c("f16_pipe4_ragged_cout32_stats", {}, "f16", (52, 9, 7, 35), 16, 32, F16_PIPE4_RAGGED, True, stats=True, act=0),
    # ... and the 512-voxel one on whole tiles with three cout blocks (Cout = 32 goes to the LDS-DMA kernel, Cout = 64 to NF = 2)
    _c("f16_pipe4_whole_cout96", {}, "f16", (3, 32, 32, 32), 16, 96, F16_PIPE4_WHOLE, False),
    _c("f16_pipe4_whole_cout96_stats", {}, "f16", (11, 8, 32, 32), 16, 96, F16_PIPE4_WHOLE, False, stats=True, act=0),
    # fp16 split-K with one 32-cout fragment per workgroup (Cin >= 128 into Cout = 32 on a small volume), both strides
    _c("f16_splitk_nf1_2x2x2", {}, "f16", (1, 2, 2, 2), 128, 32, "conv3_f16_mfma_kernel<1, 2, 1> split-K", True),
    _c("f16_splitk_nf1_tiles_cin320", {}, "f16", (2, 5, 6, 7), 320, 32, "conv3_f16_mfma_kernel<1, 2, 1> split-K", True, act=0),
    _c("f16_splitk_nf1_whole", {}, "f16", (1, 8, 8, 4), 128, 32, "conv3_f16_mfma_kernel<1, 2, 1> split-K", False),
    _c("f16_s2_splitk_nf1_tiles", {}, "f16", (2, 9, 10, 11), 128, 32, "conv3_f16_mfma_kernel<2, 1, 1> split-K", True, stride=2),
    _c("f16_s2_splitk_nf1_whole", {}, "f16", (1, 8, 16, 16), 128, 32, "conv3_f16_mfma_kernel<2, 1, 1> split-K", False, act=0, stride=2),
    # ---- MI355_WINOGRAD=0: the thin-volume kernel takes the large ragged launches too (two x tiles of 32)
    _c("f32_c16_mf4_nowino_cout96", WINOGRAD0, "f32", (16, 9, 7, 35), 16, 96, F32_THIN_1, True),
    # ---- MI355_CONV_IMPL=0: the one-tile-per-workgroup kernels behind every stride-1 call
    *_trio("f16_simple_nf1", IMPL0, "f16", 16, 32, "conv3_f16_mfma_kernel<1, 2, 1>"),
    *_trio("f16_simple_nf2", IMPL0, "f16", 16, 64, "conv3_f16_mfma_kernel<1, 2, 2>"),
    *_trio("f32_c16_mf2_nf1", IMPL0, "f32", 16, 32, "conv3_f32_mfma_kernel<1, 16, 2, 1>"),
    *_trio("f32_c16_mf2_nf2", IMPL0, "f32", 16, 64, "conv3_f32_mfma_kernel<1, 16, 2, 2>"),
    *_trio("f32_c8_mf2_nf1", IMPL0, "f32", 8, 32, "conv3_f32_mfma_kernel<1, 8, 2, 1>"),
    *_trio("f32_c8_mf2_nf2", IMPL0, "f32", 8, 64, "conv3_f32_mfma_kernel<1, 8, 2, 2>"),
    _c("f32_c8_mf4_ragged", IMPL0, "f32", (16, 9, 7, 35), 8, 96, "conv3_f32_mfma_kernel<1, 8, 4, 1>", True),
    _c("f32_c8_mf4_whole_stats", IMPL0, "f32", (3, 32, 32, 32), 8, 96, "conv3_f32_mfma_kernel<1, 8, 4, 1>", False, stats=True, act=0),
    # whole 4 x 4 x 32 tiles of the 16-channel 512-voxel kernels (under the defaults the Winograd kernels take such volumes)
    _c("f32_c16_mf4_nf1_whole_stats", IMPL0, "f32", (8, 32, 32, 32), 16, 32, F32_THIN_1, False, stats=True, act=0),
    _c("f32_c16_mf4_nf2_whole", IMPL0, "f32", (8, 32, 32, 32), 16, 64, F32_THIN_2, False),
]
assert len({c.name for c in CASES}) == len(CASES)

#: rows whose name fixes the side of the whole-tile question (the WHOLE template argument): no entry of the other side can exist
ONE_SIDED = {F16_PIPE2_RAGGED: True, F16_PIPE4_RAGGED: True, F16_PIPE4_WHOLE: False}

#: rows of the tables that no plan of the sweep selects, with the reason each is still shipped and the test that runs it
UNPLANNED = {
    "conv3_f32_wino3_kernel<3, false>": "the addend epilogue of the shared skip half: launched through mi355_conv3d_wino3_ndhwc and "
                                        "mi355_conv3d_wino3_view_ndhwc only (test_gpu_skip_sharing.py, test_gpu_stage0_views.py)",
    "conv3_f32_s2dma_kernel_view<5>": "reads its input through a stage-0 view: launched through mi355_conv3d_s2dma_view_ndhwc only "
                                      "(test_gpu_stage0_views.py)",
    "conv3_f32_s2dma_kernel_view<4>": "the same on narrow volumes (test_gpu_stage0_views.py)",
}

# ------------------------------------------------------------------ the closure sweep (test_conv_rows_cpu.py)
SWEEP_VOLUMES = [(2, 2, 2), (4, 4, 4), (5, 6, 7), (8, 8, 8), (9, 7, 35), (16, 32, 8), (16, 16, 16), (32, 32, 12), (12, 20, 28),
                 (32, 32, 32), (24, 40, 72), (30, 37, 70), (64, 64, 64)]
SWEEP_CIN = (8, 16, 24, 32, 64, 128, 320)
SWEEP_COUT = (32, 64, 96, 128, 320)
SWEEP_N = (1, 2, 4, 8, 16)
SWEEP_ENVS = ([{}] + [{k: "0"} for k in SWITCHES] + [{"MI355_CONV_IMPL": "1"}] +
              [{"MI355_F16_DMA": "0", "MI355_F16_C32": "0", "MI355_F16_S2": "0"}, {"MI355_S2_DMA": "0", "MI355_SPLITK": "0"}])


#: producer norm and head classes, with and without statistics: the rows of the norm and head instantiations are selected by these
#: calls only.  Stride 1 (the stride-2 kernels take neither) at two batch sizes
SWEEP_FUSED = ((False, True, 0), (True, True, 0), (False, False, 3))
SWEEP_N_FUSED = (1, 8)


def sweep():
    """(dtype, (n, d, h, w), cin, cout, stride, stats, in_norm, head_ncls) of every call of the sweep"""
    for dtype, stride, cin, cout, stats, n, vol in itertools.product(("f32", "f16"), (1, 2), SWEEP_CIN, SWEEP_COUT, (False, True), SWEEP_N,
                                                                     SWEEP_VOLUMES):
        yield dtype, (n,) + vol, cin, cout, stride, stats, False, 0
    for dtype, cin, cout, flags, n, vol in itertools.product(("f32", "f16"), SWEEP_CIN, SWEEP_COUT, SWEEP_FUSED, SWEEP_N_FUSED, SWEEP_VOLUMES):
        yield (dtype, (n,) + vol, cin, cout, 1) + flags


SWEEP_CALLS = (2 * 2 * len(SWEEP_CIN) * len(SWEEP_COUT) * 2 * len(SWEEP_N) * len(SWEEP_VOLUMES) +
               2 * len(SWEEP_CIN) * len(SWEEP_COUT) * len(SWEEP_FUSED) * len(SWEEP_N_FUSED) * len(SWEEP_VOLUMES))


def env_key(env):
    return " ".join(f"{k}={v}" for k, v in sorted(env.items())) or "defaults"


def child_env(env):
    """the caller's environment with the dispatch switches set to exactly `env`"""
    return dict({k: v for k, v in os.environ.items() if k not in SWITCHES}, **env)


# ------------------------------------------------------------------ the exact-integer run (test_gpu_conv_rows.py)
# x in [-4, 4], weights in {-1, 0, 1} with at most 27 * 16 non-zeros per output channel, an integer bias in [-8, 8]: every partial
# sum of an output, in whatever order and however split-K slices it, is an integer of magnitude <= 27 * 16 * 4 + 8 = 1736 < 2048,
# exact in fp32 and in fp16; LeakyReLU at slope 0.5 halves the negative ones exactly.  Nothing is rounded anywhere, so the output
# must EQUAL the integer reference: a one-voxel shift, a swapped channel pair, a wrong edge predicate or a dropped split-K slice
# changes some output by at least 0.5.
INT_BOUND = 2048
INT_SLOPE = 0.5


def int_weight_period(cin):
    """with more than 16 input channels only every `period`-th weight of an output channel is non-zero (27 * 16 of them)"""
    return 1 if cin <= 16 else cin // 16


def int_operands(case):
    """(x int64 [N,D,H,W,Cin], weight int64 [Cout,Cin,3,3,3], bias int64 [Cout]) of a case, deterministic per case name"""
    rs = np.random.RandomState(zlib.crc32(case.name.encode()) % (2 ** 31))
    n, d, h, w = case.shape
    x = rs.randint(-4, 5, size=(n, d, h, w, case.cin)).astype(np.int64)
    wt = rs.randint(-1, 2, size=(case.cout, case.cin, 3, 3, 3)).astype(np.int64)
    m = int_weight_period(case.cin)
    if m > 1:
        # thinned: weight p = (cin, tap) of output o survives where (p + o) % m == 0 - and there it is +-1, so that every input
        # channel and tap still reaches cout / m outputs
        p = np.arange(case.cin * 27).reshape(1, case.cin, 3, 3, 3)
        o = np.arange(case.cout).reshape(-1, 1, 1, 1, 1)
        wt = np.where((p + o) % m == 0, np.where(wt == 0, 1, wt), 0)
    b = rs.randint(-8, 9, size=case.cout).astype(np.int64)
    assert int(np.abs(wt).sum(axis=(1, 2, 3, 4)).max()) * 4 + int(np.abs(b).max()) < INT_BOUND
    return x, wt, b


def int_conv(x, wt, b, stride):
    """3x3x3 conv, padding 1, NDHWC, in integers: int64 [N,Do,Ho,Wo,Cout] before the activation.  Sample by sample: the 27 shifted
    windows side by side ([voxels, 27 * Cin]) times the weights as [27 * Cin, Cout].  The product runs in float64, where sums of
    these small integers are exact in any order, and is converted back to int64"""
    n, d, h, w, cin = x.shape
    cout = wt.shape[0]
    do, ho, wo = (d - 1) // stride + 1, (h - 1) // stride + 1, (w - 1) // stride + 1
    xp = np.zeros((n, d + 2, h + 2, w + 2, cin), np.float64)
    xp[:, 1:-1, 1:-1, 1:-1] = x
    wmat = np.ascontiguousarray(wt.transpose(2, 3, 4, 1, 0).reshape(27 * cin, cout), dtype=np.float64)
    cols = np.empty((do, ho, wo, 27, cin), np.float64)
    acc = np.empty((n, do, ho, wo, cout), np.int64)
    for i in range(n):
        for t, (kz, ky, kx) in enumerate(itertools.product(range(3), repeat=3)):
            cols[:, :, :, t] = xp[i, kz:kz + stride * (do - 1) + 1:stride, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
        prod = cols.reshape(-1, 27 * cin) @ wmat
        acc[i] = np.rint(prod).astype(np.int64).reshape(do, ho, wo, cout)
        assert np.array_equal(acc[i].reshape(prod.shape), prod)
    return acc + b


def int_expected_doubled(acc):
    """2 * LeakyReLU(acc, 0.5) as int64: what twice the kernel's output must equal"""
    return np.where(acc >= 0, 2 * acc, acc)
