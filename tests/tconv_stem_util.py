"""GPU cases for the two families of matrix-core kernels outside the 3x3x3 conv row tables (plain data: no GPU import).

conv_rows_util.py covers the 3x3x3 row tables.  The first conv of every network (conv_stem.hip: conv3_stem_f32_kernel,
conv3_stem_f16_kernel<false|true>) and every decoder up-sampling (tconv.hip, the rows of tconv_rows: tconv2_f32_mfma_v2_kernel,
tconv2_f32_mfma_v3_kernel<8>, tconv2_f16_mfma_v2_kernel, tconv2_f16_mfma_v3_kernel<2|4|8>) are launched by rules of their own.
The stem takes every Cin = 4, stride-1 call.  The transposed conv's rule, plan_tconv, is written out here once more as
expected_tconv_kernel; tests/test_tconv_plan_cpu.py compares the two on the CPU through the dry run mi355_tconv3d_plan, and
TCONV_KERNELS with the table.  STEM_CASES and TCONV_CASES hold, per
instantiation, ragged, whole-tile and sample-straddling shapes; tests/test_tconv_stem_cpu.py keeps that set closed and checks
the references, tests/test_gpu_tconv_stem.py runs every case on exact integers, between sentinels.

A NEW INSTANTIATION OR A NEW DISPATCH THRESHOLD IN tconv.hip OR conv_stem.hip NEEDS A CASE HERE (and the rule in
expected_tconv_kernel): a ragged shape, a whole-tile shape and one whose tiles straddle a sample boundary."""
import zlib
from collections import namedtuple

import numpy as np

import conv_rows_util as R

# ------------------------------------------------------------------ stem: tiles of 4 x 4 x 32 outputs (z, y, x), Cin = 4
STEM_TILE = (4, 4, 32)
STEM_KERNEL = {"f32": "conv3_stem_f32_kernel", "f16": "conv3_stem_f16_kernel"}  # (<true> and <false> are reported alike)

# shape = (N, D, H, W); act: 1 = LeakyReLU; ragged_axes: the axes, of "zyx", on which the volume is no whole number of tiles
StemCase = namedtuple("StemCase", "name dtype shape cout act stats ragged_axes")


def stem_ragged_axes(shape):
    return "".join(a for a, v, t in zip("zyx", shape[1:], STEM_TILE) if v % t)


_STEM_SHAPES = [
    # name, shape, cout, act, stats, ragged axes
    ("one_voxel", (1, 1, 1, 1), 32, 1, False, "zyx"),          # every brick piece but one lies outside the volume
    ("ragged", (1, 5, 6, 7), 32, 1, False, "zyx"),             # one x tile, ragged in z, y and x
    ("thin_cout96", (1, 3, 2, 33), 96, 1, False, "zyx"),       # D, H < 4; the second x tile holds one voxel; three cout blocks
    ("tiles_stats", (2, 9, 7, 35), 64, 0, True, "zyx"),        # several tiles, ragged on all three axes, N = 2, statistics
    ("whole", (1, 4, 4, 32), 32, 1, False, ""),                # exactly one whole tile
    ("whole_tiles_stats", (1, 8, 8, 64), 64, 1, True, ""),     # whole tiles, statistics
]
STEM_CASES = [StemCase(f"stem_{dt}_{name}", dt, shape, cout, act, stats, axes)
              for dt in ("f32", "f16") for name, shape, cout, act, stats, axes in _STEM_SHAPES]


def stem_as_conv_case(c):
    """the conv_rows_util.Case a stem case is: Cin = 4, stride 1, default switches (what test_gpu_conv_rows.run_case takes)"""
    return R.Case(c.name, {}, c.dtype, c.shape, 4, c.cout, 1, c.act, 0.01, c.stats, STEM_KERNEL[c.dtype], bool(c.ragged_axes))


# ------------------------------------------------------------------ tconv: tiles of 128 input voxels of the flattened N*D*H*W
TCONV_TILE = 128
V3_MIN_TILES = 1024
F32_V2, F32_V3 = "tconv2_f32_mfma_v2_kernel", "tconv2_f32_mfma_v3_kernel<8>"
F16_V2 = "tconv2_f16_mfma_v2_kernel"
F16_V3 = {32: "tconv2_f16_mfma_v3_kernel<2>", 64: "tconv2_f16_mfma_v3_kernel<4>", 128: "tconv2_f16_mfma_v3_kernel<8>"}
TCONV_KERNELS = (F32_V2, F32_V3, F16_V2) + tuple(F16_V3.values())
V2_KERNELS = (F32_V2, F16_V2)
TCONV_MIN_CIN = {"f32": 8, "f16": 16}   # one MFMA K group
TCONV_CHUNK = 64                        # the v2 kernels stage Cin in chunks of 64 channels, the last one partial

# tail = M % 128; straddles: N > 1 and some 128-voxel tile holds voxels of two samples
TconvCase = namedtuple("TconvCase", "name dtype shape cin cout kernel tail straddles")


def tconv_voxels(shape):
    n, d, h, w = shape
    return n * d * h * w


def tconv_tiles(m):
    return -(-m // TCONV_TILE)


def tconv_straddles(shape):
    n, d, h, w = shape
    return any((i * d * h * w) % TCONV_TILE for i in range(1, n))


def expected_tconv_kernel(dtype, cin, m):
    """the rule of plan_tconv (tconv.hip) under the default MI355_TCONV_V3: the persistent
    kernels take >= 1024 tiles of 128 voxels at Cin = 64 (fp32) or Cin = 32, 64, 128 (fp16); everything else is version 2"""
    many = tconv_tiles(m) >= V3_MIN_TILES
    if dtype == "f32":
        return F32_V3 if many and cin == 64 else F32_V2
    assert dtype == "f16", dtype
    return F16_V3[cin] if many and cin in F16_V3 else F16_V2


def _t(dtype, shape, cin, cout):
    m = tconv_voxels(shape)
    name = f"tconv_{dtype}_{'x'.join(map(str, shape))}_{cin}to{cout}"
    return TconvCase(name, dtype, tuple(shape), cin, cout, expected_tconv_kernel(dtype, cin, m), m % TCONV_TILE, tconv_straddles(shape))


T_M3, T_TILE, T_STRADDLE, T_W1 = (1, 1, 1, 3), (1, 4, 4, 8), (3, 3, 5, 7), (1, 2, 9, 1)
T_V3_RAGGED, T_V3_STRADDLE = (1, 31, 65, 65), (2, 17, 61, 64)

# version 2: (shape, the fp32 Cin, the fp16 Cin (a multiple of 16), Cout).  M = 3 (three of the four fragments empty), one whole
# tile, M = 315 (tail 59, tiles straddle both sample boundaries), W = 1; Cin from the minimum over one partial chunk, one whole
# chunk, a whole chunk and a partial one (72 / 80, 136 / 144: the quads of the chunk before stay in LDS behind it) to 320
_V2 = [
    (T_M3, 8, 16, 32), (T_M3, 72, 80, 96),
    (T_TILE, 8, 16, 96), (T_TILE, 64, 64, 32), (T_TILE, 136, 144, 32),
    (T_STRADDLE, 72, 80, 32), (T_STRADDLE, 136, 144, 96), (T_STRADDLE, 24, 48, 32), (T_STRADDLE, 320, 320, 32),
    (T_W1, 24, 48, 96), (T_W1, 64, 64, 32), (T_W1, 320, 320, 96),
]
# version 3, the smallest shapes that reach it: 1024 tiles with 31 voxels in the last (one partial fragment, three empty), and
# 1037 whole tiles of which tile 518 straddles the samples.  Cout = 64: two cout blocks, 256 workgroups per block
_V3 = [
    ("f32", T_V3_RAGGED, 64, 32), ("f32", T_V3_RAGGED, 64, 64), ("f32", T_V3_STRADDLE, 64, 64),
    ("f16", T_V3_RAGGED, 32, 32), ("f16", T_V3_STRADDLE, 32, 64),
    ("f16", T_V3_RAGGED, 64, 64), ("f16", T_V3_STRADDLE, 64, 32),
    ("f16", T_V3_RAGGED, 128, 32), ("f16", T_V3_STRADDLE, 128, 32),
]
TCONV_CASES = ([_t("f32", s, c32, co) for s, c32, _, co in _V2] + [_t("f16", s, c16, co) for s, _, c16, co in _V2] +
               [_t(*a) for a in _V3])
assert len({c.name for c in STEM_CASES + TCONV_CASES}) == len(STEM_CASES) + len(TCONV_CASES)


def is_v2(c):
    return c.kernel in V2_KERNELS


def full_then_partial_chunk(cin):
    return cin > TCONV_CHUNK and cin % TCONV_CHUNK != 0


# ------------------------------------------------------------------ the exact-integer run
# Stem: conv_rows_util.int_operands / int_conv on stem_as_conv_case(c), unchanged: 27 * 4 * 4 + 8 < 2048.
# tconv: x in [-4, 4], weights [Cin, Cout, 2, 2, 2] in {-1, 0, 1}, no bias, no activation: every partial sum of an output is an
# integer of magnitude <= 4 * Cin <= 1280 < 2048, exact in fp32 and in fp16 in whatever order the chunks and MFMAs add it up.
def int_tconv_operands(case):
    """(x int8 [N,D,H,W,Cin], weight int8 [Cin,Cout,2,2,2]) of a case, deterministic per case name"""
    rs = np.random.RandomState(zlib.crc32(case.name.encode()) % (2 ** 31))
    x = rs.randint(-4, 5, size=case.shape + (case.cin,)).astype(np.int8)
    wt = rs.randint(-1, 2, size=(case.cin, case.cout, 2, 2, 2)).astype(np.int8)
    assert 4 * int(np.abs(wt.astype(np.int64)).sum(axis=0).max()) <= 4 * case.cin < R.INT_BOUND
    return x, wt


def tconv_matrix(wt):
    """[Cin, Cout, 2, 2, 2] -> [Cin, 8 * Cout], columns ordered (a, b, c, cout): the eight 1x1x1 GEMMs side by side"""
    cin, cout = wt.shape[:2]
    return np.ascontiguousarray(wt.transpose(0, 2, 3, 4, 1).reshape(cin, 8 * cout))


def scatter_parities(prod, shape, cout):
    """[voxels, (a, b, c, cout)] -> [N, 2D, 2H, 2W, Cout]: out[n, 2z + a, 2y + b, 2x + c] = prod[(n, z, y, x), (a, b, c)]"""
    n, d, h, w = shape
    return np.ascontiguousarray(prod.reshape(n, d, h, w, 2, 2, 2, cout).transpose(0, 1, 4, 2, 5, 3, 6, 7)).reshape(n, 2 * d, 2 * h, 2 * w, cout)


def int_tconv(x, wt, dtype=np.int64):
    """ConvTranspose3d(kernel 2, stride 2, no bias), NDHWC, in integers: `dtype` [N,2D,2H,2W,Cout].  One matmul of [voxels, Cin]
    by [Cin, 8 * Cout] in float32 - sums of these small integers (< 2048 < 2^24) are exact there in any order - converted to
    `dtype` (int16 holds them: the 1037-tile cases would take 536 MB in int64) and scattered to the eight parities"""
    cin, cout = wt.shape[:2]
    assert 4 * cin < R.INT_BOUND and np.abs(x).max() <= 4 and np.abs(wt).max() <= 1
    prod = x.reshape(-1, cin).astype(np.float32) @ tconv_matrix(wt).astype(np.float32)
    out = prod.astype(dtype)
    assert np.array_equal(np.rint(prod), prod) and np.array_equal(out, prod) and np.abs(prod).max() < R.INT_BOUND
    return scatter_parities(out, x.shape[:4], cout)


# ------------------------------------------------------------------ the per-element fp32 gate
def dot_bound(abs_sum, k):
    """|fl(sum_i x_i w_i) - sum_i x_i w_i| <= gamma_K sum_i |x_i w_i| for a K-term dot product accumulated in fp32 in ANY order
    (Higham, Accuracy and Stability of Numerical Algorithms, 3.1: gamma_K = K u / (1 - K u), u = 2^-24).  (K + 4) u covers
    gamma_K for K <= 320 (K^2 u^2 < u) and leaves three roundings for the bias add, the activation multiply and the conversion
    of the reference.  Derived, not measured"""
    return (k + 4) * 2.0 ** -24 * np.asarray(abs_sum, dtype=np.float64) + 1e-30


def conv_cols(x):
    """[N,D,H,W,C] -> [N*D*H*W, 27 * C]: the 27 shifted windows of a padding-1, stride-1 conv side by side, tap-major like
    conv_matrix's rows"""
    n, d, h, w, c = x.shape
    xp = np.zeros((n, d + 2, h + 2, w + 2, c), x.dtype)
    xp[:, 1:-1, 1:-1, 1:-1] = x
    cols = np.empty((n, d, h, w, 27, c), x.dtype)
    t = 0
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                cols[:, :, :, :, t] = xp[:, kz:kz + d, ky:ky + h, kx:kx + w]
                t += 1
    return cols.reshape(-1, 27 * c)


def conv_matrix(wt):
    """[Cout, Cin, 3, 3, 3] -> [27 * Cin, Cout]"""
    cout, cin = wt.shape[:2]
    return np.ascontiguousarray(wt.transpose(2, 3, 4, 1, 0).reshape(27 * cin, cout))


def dots_f32(a, b, order):
    """[M, K] x [K, N] in numpy float32, every product and every addition rounded to fp32, summed over K in the given order:
    'forward', 'reversed' or 'pairwise' (adjacent pairs, level by level)"""
    terms = a.astype(np.float32)[:, :, None] * b.astype(np.float32)[None, :, :]
    assert terms.dtype == np.float32
    k = terms.shape[1]
    if order == "pairwise":
        while terms.shape[1] > 1:
            odd = terms[:, -1:] if terms.shape[1] % 2 else None
            even = terms.shape[1] - terms.shape[1] % 2
            terms = terms[:, 0:even:2] + terms[:, 1:even:2]
            if odd is not None:
                terms = np.concatenate([terms, odd], axis=1)
        return terms[:, 0]
    acc = np.zeros((terms.shape[0], terms.shape[2]), np.float32)
    for i in (range(k) if order == "forward" else reversed(range(k))):
        acc = acc + terms[:, i]
    assert order in ("forward", "reversed") and acc.dtype == np.float32
    return acc
