"""References, inputs and gates of the single-kernel tests of the kernels AROUND the network: csrc/resample.hip (resize_axis,
clip_to_range_of, threshold_ge, mask_to_float), csrc/elementwise.hip (prob_mean, label_ensemble, zscore_masked,
regions_to_labels) and csrc/extras.hip (crop_mask).  tests/test_gpu_preprocess.py runs the kernels on these inputs,
tests/test_preprocess_refs_cpu.py proves on the CPU that the references agree with scipy / numpy and tell plausible wrong
kernels from the right one.

References are numpy: float64 where values are real numbers, float32 / integers (one numpy operation per rounding) where the
test claims bit equality.  ``mut`` selects a deliberately WRONG variant; None is the operation.

Gates: bit equality; the z-score bound derived from the fp32 roundings of the kernel; and two MEASURED constants, G_RESIZE and
Z_MEASURED, both measured on the CPU from a restatement against the high-precision reference, never from a device result."""
import numpy as np

U = 2.0 ** -24      # fp32 unit roundoff
F32 = np.float32
F64 = np.float64


def rng(seed):
    return np.random.RandomState(seed)


# ------------------------------------------------------------------ resize_axis
RS_PAD = 12   # scipy.ndimage pads a line by 12 edge samples for mode 'nearest' before the spline prefilter
POLE = -0.26794919243112270647   # sqrt(3) - 2

#: (n_in, n_out) pairs with n_in >= 2 at which an output coordinate computed in fp32 changes an order-0 pick
#: (test_preprocess_refs_cpu.py asserts that each is in coord_f32_pairs()).  (2, 41) is the first of that list.
COORD_F32_PAIRS = [(2, 41), (6, 37), (26, 11), (24, 37)]   # the third down-samples

# (name, shape, axis, n_out).  Layouts: "last" - the axis is the last one, inner == 1, 3 x 7 x 13 = 273 lines (> 256);
# "mid" - outer 3, inner 5 x 7 = 35; "first" - outer 1, inner 3 x 5 x 7 = 105.
def _rs_shape(layout, n):
    return {"last": ((3, 7, 13, n), 3), "mid": ((3, n, 5, 7), 1), "first": ((n, 3, 5, 7), 0)}[layout]


_RS_PAIRS = [(1, 4, "last"), (1, 3, "mid"), (2, 5, "mid"), (3, 7, "last"), (5, 12, "first"), (5, 1, "last"), (14, 1, "mid"),
             (14, 7, "last"), (12, 8, "mid"), (6, 9, "first"), (6, 9, "last")] \
    + [(a, b, lay) for (a, b), lay in zip(COORD_F32_PAIRS, ("last", "mid", "first", "mid"))] + [(155, 240, "last")]
RESIZE_CASES = [(f"{a}to{b}_{lay}",) + _rs_shape(lay, a) + (b,) for a, b, lay in _RS_PAIRS]
RESIZE_LARGEST, RESIZE_SMALLEST = "155to240_last", "1to3_mid"   # the scratch test: order 3 on the largest, then on the smallest

#: MEASURED on the CPU (test_preprocess_refs_cpu.py::test_resize_gate_is_the_measured_one repeats it): the worst, over
#: RESIZE_CASES and orders 1 and 3, of |resize_restate - scipy zoom in float64| / max|input line| is 1.296e-7 (3 -> 7, order
#: 3); it is set by the fp32 stores of the causal and anticausal coefficients and of the result.  The gate is twice that,
#: 2.592e-7: the margin of 2 covers fused multiply-adds and the device's pow against numpy's, both float64-level effects far
#: below the fp32 stores.
G_MEASURED = 1.296e-7
G_RESIZE = 2 * G_MEASURED


def resize_input(shape, seed=3):
    """Distinct lines, random, mean 100, sd 50."""
    return (rng(seed).standard_normal(shape) * 50 + 100).astype(F32)


def _dims(shape, axis):
    outer = int(np.prod(shape[:axis], dtype=np.int64))
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    return outer, int(shape[axis]), inner


def resize_zoom(x, axis, n_out, order):
    """THE reference: scipy.ndimage.zoom in float64, mode 'nearest', grid_mode=True, along the one axis."""
    from scipy.ndimage import zoom
    factors = [1.0] * x.ndim
    factors[axis] = n_out / x.shape[axis]
    return zoom(x.astype(F64), factors, order=order, mode="nearest", grid_mode=True)


def resize_mapcoord0(x, axis, n_out):
    """Order 0 as nnU-Net's separate-z path means it: map_coordinates(order=0, mode='nearest') at scale (k + 0.5) - 0.5."""
    from scipy.ndimage import map_coordinates
    n = x.shape[axis]
    coords = (n / n_out) * (np.arange(n_out) + 0.5) - 0.5
    pick = map_coordinates(np.arange(n, dtype=F64), [coords], order=0, mode="nearest").astype(np.int64)
    return np.take(x, pick, axis=axis)


def line_scale(x, axis):
    """max |input line|, broadcastable against the output: the per-line scale of the gate."""
    return np.abs(x.astype(F64)).max(axis=axis, keepdims=True)


def resize_restate(x, axis, n_out, order, mut=None):
    """The kernel restated: float64 arithmetic; order 3 prefilters the line padded by RS_PAD edge samples with fp32 stores of the
    causal and of the anticausal coefficients, the recursions themselves carried in float64; one fp32 store of the result.
    mut: "pad4" (4 edge samples instead of 12), "coord_f32" (output coordinates and the order-0 pick in fp32),
    "outer_inner_swapped" (the tensor read as [inner][n][outer]), "no_edge_clamp" (see below).

    "no_edge_clamp" drops the edge clamps that CAN act: the coordinate clamp of order 1 and the source clamp that builds the
    padded line of order 3; a sample beyond the line is then read from the neighbouring line, as a flat index would.  The tap
    clamp of the order-3 evaluation and the index clamp of order 0 can not act: coordinates lie in [-0.5, n_in - 0.5], so the
    order-0 pick floor(x + 0.5) lies in [0, n_in - 1] and the four taps lie in [pad - 2, n_in + pad + 1], inside the padded
    line for any pad >= 2 - removing them changes nothing, and no test can see them."""
    x = np.ascontiguousarray(x, F32)
    outer, n, inner = _dims(x.shape, axis)
    out_shape = x.shape[:axis] + (n_out,) + x.shape[axis + 1:]
    if mut == "outer_inner_swapped":
        outer, inner = inner, outer
    a = x.reshape(outer, n, inner)
    rows2d = a.reshape(outer * n, inner)
    k = np.arange(n_out)
    if mut == "coord_f32":
        x32 = (k.astype(F32) + F32(0.5)) * (F32(n) / F32(n_out)) - F32(0.5)
        pick0, xk = np.floor(x32 + F32(0.5)).astype(np.int64), x32.astype(F64)
    else:
        xk = (k + 0.5) * (n / n_out) - 0.5
        pick0 = np.floor(xk + 0.5).astype(np.int64)

    def rows(j):
        """a[:, j, :] for an index vector j; without the clamp, the row a flat index reaches."""
        if mut != "no_edge_clamp":
            return a[:, np.clip(j, 0, n - 1), :]
        flat = np.clip(np.arange(outer)[:, None] * n + j[None, :], 0, outer * n - 1)
        return rows2d[flat]

    if order == 0:
        out = a[:, np.clip(pick0, 0, n - 1), :]
    elif order == 1:
        xc = xk if mut == "no_edge_clamp" else np.clip(xk, 0.0, float(n - 1))
        j = np.floor(xc).astype(np.int64)
        j = np.where(j > n - 2, max(n - 2, 0), j)
        f = (xc - j)[None, :, None]
        j1 = np.where(j + 1 < n, j + 1, j)
        out = ((1.0 - f) * rows(j).astype(F64) + f * rows(j1).astype(F64)).astype(F32)
    else:
        pad = 4 if mut == "pad4" else RS_PAD
        m = n + 2 * pad
        p = rows(np.arange(m) - pad).astype(F64)
        z, gain = POLE, 6.0
        z_n_1 = z ** (m - 1)
        c0 = gain * p[:, 0] + z_n_1 * gain * p[:, m - 1]
        z_i = z
        for i in range(1, m - 1):
            c0 = c0 + z_i * (gain * p[:, i] + z_n_1 * gain * p[:, m - 1 - i])
            z_i *= z
        c0 = c0 / (1.0 - z_n_1 * z_n_1)
        d = np.empty((outer, m, inner), F32)
        prev = c0
        d[:, 0] = c0
        for i in range(1, m):
            prev = gain * p[:, i] + z * prev
            d[:, i] = prev
        nxt = (z * d[:, m - 2].astype(F64) + d[:, m - 1].astype(F64)) * z / (z * z - 1.0)
        d[:, m - 1] = nxt
        for i in range(m - 2, -1, -1):
            nxt = z * (nxt - d[:, i].astype(F64))
            d[:, i] = nxt
        xp = np.clip(xk + pad, 0.0, float(m - 1))
        fl = np.floor(xp)
        j0, f = fl.astype(np.int64) - 1, (xp - fl)[None, :, None]
        w = [(1.0 - f) ** 3 / 6.0, (4.0 - 6.0 * f * f + 3.0 * f ** 3) / 6.0,
             (1.0 + 3.0 * f + 3.0 * f * f - 3.0 * f ** 3) / 6.0, f ** 3 / 6.0]
        out = sum(w[t] * d[:, np.clip(j0 + t, 0, m - 1), :].astype(F64) for t in range(4)).astype(F32)
    return np.ascontiguousarray(out).reshape(out_shape)


def coord_f32_pairs(limit=260):
    """All (n_in, n_out), both below `limit`, at which the fp32 coordinate picks another order-0 sample than the fp64 one."""
    k = np.arange(limit - 1)[None, :]
    n_out = np.arange(1, limit)[:, None]
    live = k < n_out
    out = []
    for n_in in range(1, limit):
        p64 = np.floor(((k + 0.5) * (n_in / n_out) - 0.5) + 0.5)
        x32 = (k.astype(F32) + F32(0.5)) * (F32(n_in) / n_out.astype(F32)) - F32(0.5)
        p32 = np.floor(x32 + F32(0.5)).astype(F64)
        bad = (np.clip(p64, 0, n_in - 1) != np.clip(p32, 0, n_in - 1)) & live
        out += [(n_in, int(b)) for b in n_out[bad.any(1), 0]]
    return out


# ------------------------------------------------------------------ clip_to_range_of_ (bit equality)
CLIP_BIG = 1024 * 2048 + 1531   # one group beyond the 1024 blocks x 8 x 256 elements of the capped grids
CLIP_SIGN_FREE = ("zero_extremes",)   # cases whose expected zeros carry no defined sign


def _clip_x(ref, group_dims, shape_tail, seed):
    """x per group uniform over [lo - R, hi + R], R = the group's range: a third of the elements beyond each end (a group whose
    range is the one value v: uniform over v -+ 1.5 |v|, half beyond each end)."""
    g = int(np.prod(ref.shape[:group_dims]))
    r2 = ref.reshape(g, -1).astype(F64)
    lo, hi = r2.min(1), r2.max(1)
    span = np.where(hi > lo, hi - lo, np.where(lo != 0, np.abs(lo), 1.0))
    u = rng(seed).uniform(-1.0, 2.0, (g, int(np.prod(shape_tail)))) - np.where(hi > lo, 0.0, 0.5)[:, None]
    x = (lo[:, None] + u * span[:, None]).astype(F32).reshape(ref.shape[:group_dims] + tuple(shape_tail))
    return x


def clip_cases():
    """name -> (x, ref, group_dims).  Zeros of both signs sit INSIDE the straddling groups' ranges and in x, where they must pass
    unchanged.  Only "zero_extremes" has them AT an extreme (the minimum of group 0, the maximum of group 1): which zero numpy's
    min of {-0.0, +0.0} returns is not defined, so that case is compared by value, and bit for bit only where the result is not
    a zero (CLIP_SIGN_FREE)."""
    r = rng(40)
    cases = {}
    # [C = 3][Z = 5] groups: channel 0 all negative, 1 straddles zero, 2 positive; every slice has its own offset, so a range per
    # channel is not a range per slice; ref 7 x 9 = 63 per slice, x 11 x 13 = 143
    offsets = np.array([-60.0, -25.0, 0.0, 30.0, 75.0])[None, :] * np.array([1.0, 0.02, 1.0])[:, None]
    base = np.array([-700.0, 0.0, 900.0])[:, None] + offsets
    noise = r.standard_normal((3, 5, 7, 9)) * np.array([40.0, 3.0, 50.0])[:, None, None, None]
    ref = (base[:, :, None, None] + noise).astype(F32)
    ref[1, :, 0, 0], ref[1, :, 3, 4] = F32(-0.0), F32(0.0)
    for gd in (2, 1):
        x = _clip_x(ref, gd, (11, 13) if gd == 2 else (5, 11, 13), 41 + gd)
        if gd == 2:
            x[1, :, 2, 2], x[1, :, 5, 7] = F32(-0.0), F32(0.0)
        cases[f"slices_gd{gd}"] = (x, ref, gd)
    one = np.array([[-3.5], [0.25], [-1e-30], [7e20]], F32)              # a single reference element per group
    cases["one_ref_element"] = (_clip_x(one, 1, (50,), 44), one, 1)
    # 40 reference elements: less than a wave
    few = (r.standard_normal((2, 40)) * np.array([[1.0], [1e-3]]) + np.array([[-5.0], [0.0]])).astype(F32)
    cases["forty_ref_elements"] = (_clip_x(few, 1, (300,), 45), few, 1)
    big = r.uniform(-1.0, 0.5, (1, CLIP_BIG)).astype(F32)               # extremes in the ragged tail of the last trip
    big[0, -1], big[0, -700] = F32(-1.25), F32(0.75)
    cases["grid_stride"] = (_clip_x(big, 1, (CLIP_BIG + 300,), 46), big, 1)
    rz = rng(47)
    zero = np.stack([np.concatenate([[-0.0, 0.0], rz.uniform(0.5, 3.0, 48)]),
                     np.concatenate([rz.uniform(-3.0, -0.5, 48), [0.0, -0.0]])]).astype(F32)
    cases["zero_extremes"] = (_clip_x(zero, 1, (200,), 48), zero, 1)
    return cases


def _f2ord(a, signed=True):
    u = a.view(np.uint32)
    if not signed:
        return u
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def clip_ref(x, ref, group_dims, mut=None):
    """np.clip(x[g], ref[g].min(), ref[g].max()) per group, fp32 (a copy and two comparisons: bit equality).
    mut: "per_channel" (group_dims - 1: a range per channel where it is per slice), "n_per_group" (the reference of group g read
    as the n_per_group floats from g * n_per_group on), "no_sign" (the order-preserving integer image of the min / max search
    without its sign handling: floats compared as unsigned integers)."""
    g = int(np.prod(x.shape[:group_dims]))
    x2, r2 = x.reshape(g, -1), ref.reshape(g, -1)
    if mut == "n_per_group":
        n = x2.shape[1]
        r2 = ref.reshape(-1)[np.minimum(np.arange(g)[:, None] * n + np.arange(n)[None, :], ref.size - 1)]
    if mut == "per_channel":
        g1 = int(np.prod(x.shape[:group_dims - 1]))
        r1 = ref.reshape(g1, -1)
        lo, hi = np.repeat(r1.min(1), g // g1), np.repeat(r1.max(1), g // g1)
    elif mut == "no_sign":
        o = _f2ord(np.ascontiguousarray(r2), signed=False)
        lo, hi = o.min(1).view(F32), o.max(1).view(F32)
    else:
        lo, hi = r2.min(1), r2.max(1)
    lo, hi = lo[:, None], hi[:, None]
    return np.where(x2 < lo, lo, np.where(x2 > hi, hi, x2)).astype(F32).reshape(x.shape)


def clip_moved(x, ref, group_dims):
    """Fractions of x below the group's minimum and above its maximum."""
    g = int(np.prod(x.shape[:group_dims]))
    x2, r2 = x.reshape(g, -1), ref.reshape(g, -1)
    return float((x2 < r2.min(1)[:, None]).mean()), float((x2 > r2.max(1)[:, None]).mean())


# ------------------------------------------------------------------ threshold_ge, mask_to_float, prob_mean, label_ensemble (bit equality)
N_BIG = 8192 * 256 + 257   # the capped grid of 8192 blocks strides, and the last trip is ragged
THRESHOLDS = (0.0, 0.5, 0.3)   # 0.3 is no fp32 number: the entry point takes float(thr) rounded to fp32, as np.float32(0.3)


def threshold_input(thr, n):
    """The values at, just below and just above thr, both zeros, +-inf and NaN, repeated, then normal noise about thr."""
    t = F32(thr)
    special = np.array([t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf)), -0.0, 0.0, np.inf, -np.inf, np.nan, -t], F32)
    x = (rng(50).standard_normal(n) * 0.2).astype(F32) + t
    idx = np.arange(0, n, 3)
    x[idx] = special[np.arange(idx.size) % special.size]
    return x


def threshold_ref(x, thr, mut=None):
    """mut "gt": x > thr."""
    return ((x > F32(thr)) if mut == "gt" else (x >= F32(thr))).astype(np.uint8)


def mask_input(n, seed=51):
    return np.array([0, 1, 2, 255], np.uint8)[rng(seed).randint(0, 4, n)]


def mask_to_float_ref(m, mut=None):
    """mut "eq1": only the byte 1 counts; "cast": the byte's value."""
    if mut == "cast":
        return m.astype(F32)
    return ((m == 1) if mut == "eq1" else (m != 0)).astype(F32)


def prob_mean_input(n):
    """Probabilities; pairs whose sum is inexact (1 and 2^-24: a tie, and 1 + 3 x 2^-25); denormals (odd multiples of 2^-149,
    whose half is a tie); sums that overflow to inf in fp32; signed zeros."""
    r = rng(52)
    a, b = r.uniform(0, 1, n).astype(F32), r.uniform(0, 1, n).astype(F32)
    tiny = np.nextafter(F32(0), F32(1))
    sa = np.array([1.0, 1.0, tiny, 3 * tiny, 5 * tiny, 1e-39, 3e38, -3e38, 3.4e38, -0.0, 0.0, 1.1754944e-38, 1 / 3], F32)
    sb = np.array([2.0 ** -24, 3 * 2.0 ** -25, 0.0, 0.0, 2 * tiny, 2e-39, 3e38, -3e38, 1e38, -0.0, -0.0, tiny, 2 / 3], F32)
    idx = np.arange(0, n, 5)
    a[idx], b[idx] = sa[np.arange(idx.size) % sa.size], sb[np.arange(idx.size) % sb.size]
    return a, b


def prob_mean_ref(a, b, mut=None):
    """(a + b) / np.float32(2) in fp32: whatever numpy's fp32 gives, inf included.  mut "half_each": a / 2 + b / 2."""
    with np.errstate(over="ignore"):
        return (a / F32(2) + b / F32(2)) if mut == "half_each" else (a + b) / F32(2)


def label_pair_input(n):
    """The full 256 x 256 table first (when n allows), random bytes after."""
    r = rng(53)
    a, b = r.randint(0, 256, n).astype(np.uint8), r.randint(0, 256, n).astype(np.uint8)
    t = min(n, 65536)
    a[:t], b[:t] = (np.arange(t) >> 8).astype(np.uint8), (np.arange(t) & 255).astype(np.uint8)
    return a, b


def label_ensemble_ref(a, b, mut=None):
    """uint8(np.round((a + b) / 2.0)) as the reference driver writes it (numpy rounds halves to even).  mut "half_up"."""
    s = a.astype(F64) + b.astype(F64)
    return (np.floor(s / 2.0 + 0.5) if mut == "half_up" else np.round(s / 2.0)).astype(np.uint8)


# ------------------------------------------------------------------ zscore_masked_ (derived bound)
#: |got - ref64| <= Z_MARGIN * U * (|mean| / std + 2 |ref64| + 1) per element: the kernel's fp32 rounding of the mean (U |mean| over
#: std), of the difference and of the quotient (U |ref| each) and of the denominator sqrt(var) + 1e-8 (another U |ref|, taken up
#: by the margin), the + 1 for the rounding of a difference that cancels.  MEASURED on the CPU
#: (test_preprocess_refs_cpu.py::test_zscore_bound_is_the_measured_one repeats it): the fp32 restatement zscore_restate32 reaches
#: Z_MEASURED of the bound WITHOUT the margin on the inputs of zscore_cases(); the margin applied is Z_MARGIN = 2.
Z_MEASURED = 0.81
Z_MARGIN = 2.0
Z_STATS = ((1000.0, 300.0), (1e4, 1.0), (-5e3, 20.0))
Z_BIG_SHAPE = (65, 90, 90)    # 526 500 voxels > 2048 x 256: the grid strides and the finish adds 2048 partials
Z_MID_VOXELS = 20011          # 79 blocks: the lane-strided finish makes a second, ragged trip
CONST_03 = F32(0.3)
Z_CONST_VOXELS = 986


def zscore_cases():
    """name -> (vol [C, ...] fp32, mask uint8 with bytes from {0, 1, 2, 255}, non-zero = inside)."""
    r = rng(60)
    cases = {}
    mask = np.array([0, 0, 1, 2, 255], np.uint8)[r.randint(0, 5, Z_BIG_SHAPE)]
    cases["big"] = (np.stack([r.standard_normal(Z_BIG_SHAPE) * sd + mu for mu, sd in Z_STATS[:2]]).astype(F32), mask)
    mask = np.array([0, 0, 1, 2, 255], np.uint8)[r.randint(0, 5, Z_MID_VOXELS)]
    cases["mid"] = (np.stack([r.standard_normal(Z_MID_VOXELS) * sd + mu for mu, sd in Z_STATS]).astype(F32), mask)
    vol = (r.standard_normal((2, Z_MID_VOXELS)) * 300 + 1000).astype(F32)
    one = np.zeros(Z_MID_VOXELS, np.uint8)
    one[17003] = 255
    cases["one_voxel"] = (vol, one)
    cases["empty"] = (vol, np.zeros(Z_MID_VOXELS, np.uint8))
    # a region constant at 0.3f of Z_CONST_VOXELS voxels: at that count the fp32 numpy mean is one ulp off 0.3f, and the one-pass
    # variance sum x^2 / n - mean^2 in float64 is -1.4e-17, below zero
    cmask = np.zeros(Z_MID_VOXELS, np.uint8)
    cmask[r.permutation(Z_MID_VOXELS)[:Z_CONST_VOXELS]] = np.array([1, 2, 255], np.uint8)[r.randint(0, 3, Z_CONST_VOXELS)]
    const = vol.copy()
    const[:, cmask != 0] = CONST_03
    cases["constant"] = (const, cmask)
    return cases


def _partial_sums(x, m, first64):
    """float64 sums of x, x^2 and the count over the mask; first64: only the first 64 of the kernel's per-block partials (block b
    of nblocks = min(2048, ceil(V / 256)) holds the voxels i with (i // 256) % nblocks == b)."""
    if first64:
        nblocks = min(2048, -(-x.size // 256))
        m = m & ((np.arange(x.size) // 256) % nblocks < 64)
    xm = x[m].astype(F64)
    return xm.sum(), (xm * xm).sum(), float(m.sum())


def zscore_stats(vol, mask, mut=None):
    """Per channel (mean, std) in float64.  mut: "ddof1", "no_clamp" (the variance as sum x^2 / n - mean^2 without its clamp at
    0), "first64", "eq1" (the mask tested as == 1)."""
    m = (mask.reshape(-1) == 1) if mut == "eq1" else (mask.reshape(-1) != 0)
    out = []
    for c in range(vol.shape[0]):
        s1, s2, cnt = _partial_sums(vol[c].reshape(-1), m, mut == "first64")
        if cnt == 0:
            out.append((F64(0), F64(0)))
            continue
        mean = s1 / cnt
        if mut in ("no_clamp", "first64"):     # the kernel's own expression: E[x^2] - mean^2
            var = s2 / cnt - mean * mean
            if mut == "first64":
                var = max(var, 0.0)
        else:                                  # the definition, two-pass
            d = vol[c].reshape(-1)[m].astype(F64) - mean
            var = (d * d).sum() / F64(cnt - 1 if mut == "ddof1" else cnt)
        with np.errstate(invalid="ignore"):
            out.append((F64(mean), np.sqrt(F64(var))))
    return m, out


def zscore_ref(vol, mask, mut=None):
    """float64 (ref, bound): (x - mean) / (std + 1e-8) over the mask, 0 outside; bound WITHOUT the margin, 0 outside the mask."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return _zscore_ref(vol, mask, mut)


def _zscore_ref(vol, mask, mut):
    m, stats = zscore_stats(vol, mask, mut)
    ref, bound = np.zeros(vol.shape, F64), np.zeros(vol.shape, F64)
    for c, (mean, std) in enumerate(stats):
        r = (vol[c].reshape(-1).astype(F64) - mean) / (std + 1e-8)
        r[~m] = 0.0
        ref[c] = r.reshape(vol.shape[1:])
        bound[c] = np.where(m, U * (abs(mean) / std + 2 * np.abs(r) + 1), 0.0).reshape(vol.shape[1:])
    return ref, bound


def zscore_restate32(vol, mask):
    """The kernel's fp32 steps on float64 statistics: mean rounded to fp32, fp32(sqrt(var)) + 1e-8f, an fp32 difference and an
    fp32 quotient."""
    m, stats = zscore_stats(vol, mask)
    out = np.zeros(vol.shape, F32)
    for c, (mean, std) in enumerate(stats):
        r = (vol[c].reshape(-1) - F32(mean)) / (F32(std) + F32(1e-8))
        r[~m] = 0
        out[c] = r.reshape(vol.shape[1:])
    return out


def zscore_numpy32(vol, mask):
    """The whole expression in fp32 numpy (mean and std in fp32): NOT the reference - on a region constant at 0.3f it
    returns 0.75 (the rounding of the fp32 mean over 1e-8) where the definition gives 0."""
    out = np.array(vol, F32, copy=True)
    m = mask != 0
    for c in range(out.shape[0]):
        mn, sd = out[c][m].mean(), out[c][m].std()
        out[c][m] = (out[c][m] - mn) / (sd + F32(1e-8))
        out[c][~m] = 0
    return out


# ------------------------------------------------------------------ crop_mask (bit equality with tiler_ref.crop_to_nonzero)
SERPENTINE_TURNS = 13


def serpentine(closed):
    """[1, 5, 32, 18], a 3 x 29 x 15 block at (1, 2, 1): tissue everywhere but a one-voxel corridor of background in the middle
    slice that runs along the odd rows and turns at alternating ends, SERPENTINE_TURNS times; open to the border at the start of
    its first row unless `closed`.  The open corridor is outside and stays unfilled - one row per round of sweeps -, the closed
    one is a hole and fills."""
    rows = SERPENTINE_TURNS + 1
    v = np.ones((1, 3, 2 * rows + 1, 15), F32) * F32(2.5)
    for i in range(rows):
        y = 2 * i + 1
        v[0, 1, y, 1:14] = 0
        if i + 1 < rows:
            v[0, 1, y + 1, 13 if i % 2 == 0 else 1] = 0
    if not closed:
        v[0, 1, 1, 0] = 0
    return np.pad(v, ((0, 0), (1, 1), (2, 1), (1, 2)))   # a background margin: the box is not the volume


def crop_cases():
    """name -> vol [C, Z, Y, X] fp32, every volume below 40 000 voxels."""
    r = rng(70)
    cases = {"serpentine_open": serpentine(False), "serpentine_closed": serpentine(True)}
    # C = 4: a hollow box (12 x 14 x 16 at (3, 4, 5), cavity inside) whose six walls are non-zero in DIFFERENT channels, and a
    # blob per channel elsewhere: the cavity is a hole only for the OR over the channels
    v = np.zeros((4, 20, 24, 28), F32)
    bz, by, bx = slice(3, 15), slice(4, 18), slice(5, 21)
    walls = [(slice(3, 4), by, bx), (slice(14, 15), by, bx), (bz, slice(4, 5), bx), (bz, slice(17, 18), bx),
             (bz, by, slice(5, 6)), (bz, by, slice(20, 21))]
    for i, w in enumerate(walls):
        v[(i % 4,) + w] = r.uniform(1, 2, v[(i % 4,) + w].shape)
    for c, (z, y, x) in enumerate([(17, 2, 3), (1, 20, 24), (16, 21, 2), (18, 10, 25)]):
        v[c, z:z + 2, y:y + 2, x:x + 2] = -1.5
    cases["channels"] = v
    for shape in ((1, 9, 11), (7, 1, 1), (5, 6, 1)):
        v = r.standard_normal((2,) + shape).astype(F32) * (r.uniform(0, 1, (2,) + shape) < 0.3)
        v[1].reshape(-1)[-2 if v[1].size > 2 else -1] = 4.0
        cases["x".join(map(str, shape))] = v.astype(F32)
    v = np.zeros((2, 4, 5, 6), F32)
    v[1, 3, 4, 5] = -2.5
    cases["corner_voxel"] = v
    # -0.0 is background: a shell of tissue around a cavity, -0.0 scattered through the outside, the cavity and a second channel
    v = np.zeros((2, 9, 10, 11), F32)
    v[0, 2:7, 2:8, 3:9] = 3.0
    v[0, 3:6, 3:7, 4:8] = -0.0
    v[0, 0], v[0, :, 9], v[1] = -0.0, -0.0, -0.0
    cases["negative_zero"] = v
    return cases


def crop_expected(vol):
    """(mask [Z, Y, X] uint8 - the oracle's inside-mask in its box, zero outside -, bbox) from oracle/tiler_ref.crop_to_nonzero."""
    from oracle import tiler_ref
    _, inside, bbox = tiler_ref.crop_to_nonzero(vol)
    mask = np.zeros(vol.shape[1:], np.uint8)
    mask[tuple(slice(lo, hi) for lo, hi in bbox)] = inside
    return mask, [list(b) for b in bbox]


def crop_restate(vol, mut=None):
    """The device algorithm: state 1 = tissue (any channel != 0), background reached from the border 2; per round a forward and a
    backward walk of every line along z, then y, then x; until a round changes nothing.  Returns (mask, bbox, rounds that changed
    something).  mut: "channel0" (only channel 0 looked at), "one_round"."""
    tissue = (vol[0] != 0) if mut == "channel0" else (vol != 0).any(0)
    state = tissue.astype(np.uint8)
    rounds = 0
    while True:
        changed = False
        for axis in range(3):
            s = np.moveaxis(state, axis, 0)
            for order in (range(s.shape[0]), range(s.shape[0] - 1, -1, -1)):
                reach = np.ones(s.shape[1:], bool)
                for i in order:
                    reach = np.where(s[i] == 1, False, np.where(s[i] == 2, True, reach))
                    new = reach & (s[i] == 0)
                    changed |= bool(new.any())
                    s[i][new] = 2
        rounds += changed
        if not changed or mut == "one_round":
            break
    mask = (state != 2).astype(np.uint8)
    idx = np.where(mask)
    return mask, [[int(i.min()), int(i.max()) + 1] for i in idx], rounds


# ------------------------------------------------------------------ regions_to_labels (bit equality)
HALF_UP = np.nextafter(F32(0.5), F32(1))
R2L_ORDER8 = (3, 0, 5, 5, 1, 0, 7, 2)     # repeats and zeros
# (name, C, order, box shape, lo, full shape) of the small GPU cases: 8 channels with the box flush with the far corner and equal
# to the full shape, 3 channels with the box inside, argmax with ties and with one channel.  Probabilities: r2l_probs(C, shape,
# R2L_SEED + C)
R2L_SEED = 80
R2L_CASES = [("regions_c8_far_corner", 8, R2L_ORDER8, (5, 6, 7), (3, 3, 4), (8, 9, 11)),
             ("regions_c8_full", 8, R2L_ORDER8, (5, 6, 7), (0, 0, 0), None),
             ("regions_c3_inside", 3, (1, 2, 3), (5, 6, 7), (1, 2, 3), (8, 9, 11)),
             ("argmax_c4_ties", 4, None, (5, 6, 7), (3, 3, 4), (8, 9, 11)),
             ("argmax_c1", 1, None, (5, 6, 7), (0, 0, 0), None)]
R2L_BIG = dict(shape=(129, 128, 128), lo=(1, 2, 3), full=(131, 131, 133))   # 2 113 536 voxels > 8192 x 256


def r2l_probs(c, shape, seed):
    """Values from a small set - 0.5 and the next float above it among them -, so channels tie exactly."""
    vals = np.array([0.1, 0.5, HALF_UP, 0.9, 0.49999997, 0.7], F32)
    return vals[rng(seed).randint(0, vals.size, (c,) + tuple(shape))]


def r2l_ref(probs, order, lo=(0, 0, 0), full=None, mut=None):
    """seg = 0; for k in channel order: seg[probs[k] > 0.5] = order[k]; order None: argmax over the channels, the first maximum
    wins; pasted at lo into zeros of the full shape.
    mut: "ge" (>= 0.5), "argmax_last" (the last maximum wins), "lo_yx" (the y and x offsets exchanged)."""
    c = probs.shape[0]
    if order is None:
        seg = (c - 1 - np.argmax(probs[::-1], 0)) if mut == "argmax_last" else np.argmax(probs, 0)
    else:
        seg = np.zeros(probs.shape[1:], np.int64)
        for k in range(c):
            seg[(probs[k] >= F32(0.5)) if mut == "ge" else (probs[k] > F32(0.5))] = order[k]
    full = probs.shape[1:] if full is None else full
    if mut == "lo_yx":
        lo = (lo[0], lo[2], lo[1])
    out = np.zeros(full, np.uint8)
    out[tuple(slice(o, o + s) for o, s in zip(lo, probs.shape[1:]))] = seg.astype(np.uint8)
    return out
