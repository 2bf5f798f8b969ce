"""References, inputs and gates of the single-kernel tests of csrc/elementwise.hip, stage0_gather.hip and aggregate.hip (tests/test_gpu_plumbing.py runs the kernels,
tests/test_plumbing_refs_cpu.py checks on the CPU that these references tell plausible wrong kernels from the right one).

Every reference restates its operation from the contract in csrc/kernels.h / include/mi355_nnunet.h with whole-array numpy
indexing: in float64 where the test carries a derived bound, in float32 (one numpy operation per rounding) where it claims
bit equality.  ``mut`` selects a deliberately WRONG variant (the CPU test); None is the operation.

Inputs are random with fixed seeds, every weight map is a random non-symmetric array (the real Gaussian is symmetric under
every flip and would hide a weight read at the flipped voxel), every extent triple is pairwise different.

Gates are of three kinds and every gate function says which: bit equality; a bound derived from the fp32 / fp16 formats
(U = 2^-24 is the unit roundoff of fp32, 2^-11 that of fp16); the one measured constant T_NONLIN."""
import numpy as np

U = 2.0 ** -24      # fp32 unit roundoff
UH = 2.0 ** -11     # fp16 unit roundoff
F32 = np.float32
SLOPE = F32(0.01)


def rng(seed):
    return np.random.RandomState(seed)


# ------------------------------------------------------------------ layouts and mirrors
def to_blocked(x):
    """[N, V, C] -> the channel-blocked [N, C / 8, V, 8] the library keeps fp16 tensors in."""
    n, v, c = x.shape
    return np.ascontiguousarray(x.reshape(n, v, c // 8, 8).transpose(0, 2, 1, 3))


def from_blocked(x):
    n, cb, v, _ = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3).reshape(n, v, cb * 8))


def production_mirrors(axes):
    """Masks (bit0 = z, bit1 = y, bit2 = x) in the order nnU-Net v1 evaluates its flips: m = 0..7, bit0 of m = the LAST axis."""
    out = []
    for m in range(8):
        fx, fy, fz = m & 1, m & 2, m & 4
        if (fx and 2 not in axes) or (fy and 1 not in axes) or (fz and 0 not in axes):
            continue
        out.append((1 if fz else 0) | (2 if fy else 0) | (4 if fx else 0))
    return out


def mask_axes(mask, mut=None):
    """Axes (0 = z, 1 = y, 2 = x) a mirror mask flips.  mut "bit_order": read with bit0 = x."""
    if mut == "bit_order":
        return tuple(a for a in range(3) if mask >> (2 - a) & 1)
    return tuple(a for a in range(3) if mask >> a & 1)


def flip_tile(t, mask, mut=None):
    """Flip the last three axes of t as `mask` says.  mut "swap_p1p2": the flipped y index taken with the x extent and the other
    way round (P2 - 1 - py, P1 - 1 - px), as an index that leaves the tile wraps in a flat [P0][P1][P2] array."""
    axes = mask_axes(mask, mut)
    if mut == "swap_p1p2" and (1 in axes or 2 in axes):
        p0, p1, p2 = t.shape[-3:]
        z, y, x = np.meshgrid(np.arange(p0), np.arange(p1), np.arange(p2), indexing="ij")
        if 0 in axes:
            z = p0 - 1 - z
        if 1 in axes:
            y = p2 - 1 - y
        if 2 in axes:
            x = p1 - 1 - x
        flat = ((z * p1 + y) * p2 + x) % (p0 * p1 * p2)
        return t.reshape(t.shape[:-3] + (-1,))[..., flat]
    return np.flip(t, tuple(a - 3 for a in axes)) if axes else t


# ------------------------------------------------------------------ extract_tiles (bit equality)
EXTRACT_VOL, EXTRACT_PATCH = (4, 13, 22, 37), (16, 24, 40)
# the volume padded up to the patch: 3, 2 and 3 voxels missing, split below // above = d // 2, d - d // 2: z and x get 1 | 2
EXTRACT_PAD = (1, 1, 1)
EXTRACT_PAD_HI = (2, 1, 2)
EXTRACT_GRID_PATCH = (36, 160, 192)   # 1 105 920 voxels: above the 4096 x 256 threads of the capped grid


def extract_case(c, grid=False):
    """(vol [c, Z, Y, X] fp32, pad, tiles, patch).  Small: all 8 masks, origins that push the tile over the low face, the high
    face or both on every axis (the patch is larger than the padded volume's data on each).  grid: two samples, one mask."""
    r = rng(100 + c + (50 if grid else 0))
    if grid:
        vol = r.standard_normal((c, 30, 150, 170)).astype(F32)
        return vol, (3, 4, 9), [(-2, 1, 5, 5), (1, -3, -4, 5)], EXTRACT_GRID_PATCH
    vol = r.standard_normal((c,) + EXTRACT_VOL[1:]).astype(F32)
    origins = [(0, 0, 0), (-2, 1, 0), (1, -1, 2), (0, 2, -3), (-1, -2, 1), (2, 0, -1), (-3, 3, 3), (1, 1, -2)]
    tiles = [o + (m,) for o, m in zip(origins, production_mirrors((0, 1, 2)))]
    return vol, EXTRACT_PAD, tiles, EXTRACT_PATCH


def extract_ref(vol, pad, tiles, patch, cpad, mut=None):
    """x [n, PV, cpad] fp32: sample b = the patch-sized box at tiles[b][:3] of the zero volume that holds vol at offset pad,
    flipped along the axes of tiles[b][3]; channels >= C zero.  mut: "swap_p1p2", "bit_order", "pad_hi" (the volume placed by its
    high-side padding)."""
    c = vol.shape[0]
    if mut == "pad_hi":
        pad = EXTRACT_PAD_HI
    out = np.zeros((len(tiles),) + tuple(patch) + (cpad,), F32)
    for b, (z0, y0, x0, mask) in enumerate(tiles):
        box = np.zeros((c,) + tuple(patch), F32)
        idx, ok = [], []
        for a, (o, p, n) in enumerate(zip((z0, y0, x0), patch, vol.shape[1:])):
            g = o + np.arange(p) - pad[a]
            ok.append((g >= 0) & (g < n))
            idx.append(np.clip(g, 0, n - 1))
        sub = vol[:, idx[0]][:, :, idx[1]][:, :, :, idx[2]]
        valid = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
        box[:] = np.where(valid[None], sub, F32(0))
        out[b, ..., :c] = np.moveaxis(flip_tile(box, mask, mut), 0, -1)
    return out.reshape(len(tiles), -1, cpad)


# ------------------------------------------------------------------ norm_finalize (derived bound)
NORM_COUNT = 2097152
# Constant signals c with s1 = c count, s2 = fl32(c^2) count: the variance s2 / count - c^2 is the rounding error of the fp32
# square.  For 0.1f that error is +4.1e-10 (the variance stays just above zero), for 0.3f it is -3.6e-9: below zero, and the
# clamp decides the result - without it 1 / sqrt(var + 1e-5) moves by 1.8e-4 of itself.
CONST_C = (F32(0.1), F32(0.3))
CONST_CH = (1, 3)


def finalize_case(n, c, seed, affine):
    """(stats [n, c, 2] fp64, gamma, beta).  Channels 1 and 3 of sample 0 carry the sums of the constant signals 0.1f and 0.3f - s2
    built from the fp32-ROUNDED square, as a conv epilogue that squares in fp32 would - and channel 2 a variance of about eps."""
    r = rng(seed)
    mean = r.standard_normal((n, c))
    var = r.uniform(0.5, 2.0, (n, c))
    mean[0, 2], var[0, 2] = 0.3, 1.1e-5
    stats = np.stack([mean * NORM_COUNT, (var + mean * mean) * NORM_COUNT], -1)
    for ch, cc in zip(CONST_CH, CONST_C):
        stats[0, ch, 0] = float(cc) * NORM_COUNT
        stats[0, ch, 1] = float(F32(cc * cc)) * NORM_COUNT
    gamma = r.uniform(0.5, 1.5, c).astype(F32) if affine else None
    beta = r.standard_normal(c).astype(F32) if affine else None
    return np.ascontiguousarray(stats), gamma, beta


def finalize_ref(stats, count, kind, groups, eps, gamma, beta, mut=None):
    """float64 (scale, shift, slack): biased variance clamped at 0, eps (an fp32 number) inside the root; group statistics are
    those of the group's channels together.  slack = |beta| + |mean rstd gamma|, the terms of shift's subtraction.
    mut: "no_clamp", "group_base" (the group of channel c starts at channel c // cpg)."""
    n, c, _ = stats.shape
    s1, s2, cnt = stats[..., 0], stats[..., 1], float(count)
    if kind == "group":
        cpg = c // groups
        if mut == "group_base":
            base = np.arange(c) // cpg
            sel = np.minimum(base[:, None] + np.arange(cpg)[None, :], c - 1)
            s1, s2 = stats[:, sel, 0].sum(-1), stats[:, sel, 1].sum(-1)
        else:
            s1 = np.repeat(stats[..., 0].reshape(n, groups, cpg).sum(-1), cpg, axis=1)
            s2 = np.repeat(stats[..., 1].reshape(n, groups, cpg).sum(-1), cpg, axis=1)
        cnt *= cpg
    mean = s1 / cnt
    var = s2 / cnt - mean * mean
    if mut != "no_clamp":
        var = np.maximum(var, 0.0)
    rstd = 1.0 / np.sqrt(var + float(F32(eps)))
    g = np.ones(c) if gamma is None else gamma.astype(np.float64)
    b = np.zeros(c) if beta is None else beta.astype(np.float64)
    return g * rstd, b - mean * rstd * g, np.abs(b) + np.abs(mean * rstd * g)


def finalize_gates(scale, shift, slack):
    """Derived: both sides evaluate in fp64 and round to fp32 once - U |ref|; the subtraction behind shift may cancel, so the
    fp64 roundings of its two terms (a few 2^-53 each) count against their size: + 2^-50 (|beta| + |mean rstd gamma|)."""
    return U * np.abs(scale), U * np.abs(shift) + 2.0 ** -50 * slack


# ------------------------------------------------------------------ norm_apply (derived bound)
def apply_case(n, v, c, seed, half=False):
    r = rng(seed)
    x = r.standard_normal((n, v, c)).astype(F32)
    if half:
        x = x.astype(np.float16).astype(F32)
    return x, r.uniform(0.5, 1.5, (n, c)).astype(F32), r.standard_normal((n, c)).astype(F32)


def apply_ref(x, scale, shift, act, half=False, mut=None):
    """(y, bound) float64 over x [n, V, C]: y = act(x scale[n][c] + shift[n][c]).  Derived bound: the product and the sum round
    once each when not fused, the sum alone when fused - U (|x s| + |y|) covers both; LeakyReLU multiplies by the fp32 slope (one
    more rounding of the result, U |out|; where the rounded sum has the other sign than the exact one both are within the first
    term of 0).  fp16 storage rounds the result once more: 2^-11 |out|, or half the 2^-24 spacing of fp16 subnormals.
    mut "sample0": every sample normalised with the coefficients of sample 0."""
    bound = np.empty(x.shape)
    y = np.empty(x.shape)
    for i in range(x.shape[0]):   # (per sample: the large cases stay within a few hundred MB)
        j = 0 if mut == "sample0" else i
        xs = x[i].astype(np.float64) * scale[j].astype(np.float64)[None]
        lin = xs + shift[j].astype(np.float64)[None]
        out = np.where(lin > 0, lin, lin * float(SLOPE)) if act else lin
        b = U * (np.abs(xs) + np.abs(lin)) * (1 + 2 * U)
        if act:
            b += U * np.abs(out)
        if half:
            b += UH * np.abs(out) + 2.0 ** -25
        y[i], bound[i] = out, b
    return y, bound


# ------------------------------------------------------------------ head (derived bound)
def head_case(n, v, c, ncls, seed, half=False):
    """(feat [n, v, c] fp32 - fp16-representable when half -, weight [ncls, c], bias [ncls], scale [n, c], shift [n, c])."""
    r = rng(seed)
    f = r.standard_normal((n, v, c)).astype(F32)
    if half:
        f = f.astype(np.float16).astype(F32)
    return (f, r.standard_normal((ncls, c)).astype(F32), r.standard_normal(ncls).astype(F32),
            r.uniform(0.5, 1.5, (n, c)).astype(F32), r.standard_normal((n, c)).astype(F32))


def head_ref(f, w, b, scale=None, shift=None, slope=1.0, mut=None):
    """(logits [n, ncls, v], bound) float64.  Features are max(y, slope y) of y = f scale + shift when scale is given.  Derived
    bound: a sum of C products and the bias, every step rounded once in fp32, errs by at most (C + 1) U S, S = sum |f w| + |b|,
    in any association, fused or not; (C + 2) U S as the issue states it.  A normalised feature carries the rounding of its
    fused multiply-add and of the slope product, 2 U |f'|: 2 U S more.
    mut "sample0": scale / shift of sample 0 for every sample."""
    f = f.astype(np.float64)
    extra = 0.0
    if scale is not None:
        sc, sh = scale.astype(np.float64), shift.astype(np.float64)
        if mut == "sample0":
            sc, sh = sc[:1].repeat(f.shape[0], 0), sh[:1].repeat(f.shape[0], 0)
        y = f * sc[:, None, :] + sh[:, None, :]
        f = np.maximum(y, y * float(F32(slope)))
        extra = 2.0
    w64 = w.astype(np.float64)
    b64 = np.zeros(w.shape[0]) if b is None else b.astype(np.float64)
    logits = np.einsum("nvc,kc->nkv", f, w64) + b64[None, :, None]
    s = np.einsum("nvc,kc->nkv", np.abs(f), np.abs(w64)) + np.abs(b64)[None, :, None]
    return logits, (f.shape[2] + 2 + extra) * U * s


# ------------------------------------------------------------------ aggregation
AGG_PATCH, AGG_PADDED, AGG_ORIGIN = (6, 10, 14), (11, 17, 23), (3, 5, 7)
AGG_ORIGIN2 = (1, 2, 4)   # a second tile that overlaps the first
AGG_FIRST = 2             # samples in front of the tile's own: first_sample > 0
AGG_GRID_PATCH, AGG_GRID_PADDED, AGG_GRID_ORIGIN = (130, 129, 251), (131, 130, 253), (1, 1, 2)   # 4 209 270 voxels > 16384 x 256
MIRROR_LISTS = {"none": production_mirrors(()), "z": production_mirrors((0,)), "zx": production_mirrors((0, 2)),
                "zyx": production_mirrors((0, 1, 2)), "zyx_reversed": production_mirrors((0, 1, 2))[::-1]}

#: MEASURED, the one gate of this file that is: measure_t() - the largest difference between the float32 restatement of the
#: mirror-averaged sigmoid / softmax below and the float64 one, both fed the logits of nonlin_case (uniform over [-30, 30]; ncls
#: 1, 3, 8; 8 mirrors) - gave 1.132e-7 for sigmoid and 7.43e-8 for softmax with numpy's float32 exp on the CPU.  The device expf
#: may differ from it by an ulp of the exponential, so the gate takes 4 x the larger figure: T_NONLIN = 4.56e-7.
#: test_plumbing_refs_cpu.py repeats the measurement.
T_MEASURED = 1.14e-7
T_NONLIN = 4 * T_MEASURED
LIPSCHITZ = {"identity": 1.0, "sigmoid": 0.25, "softmax": 0.5}


def sentinel(shape, seed):
    """A pattern no aggregation writes by accident: distinct negative values."""
    return (-1000.0 - rng(seed).permutation(int(np.prod(shape))).reshape(shape) % 4093).astype(F32)


def weight_map(patch, seed):
    return rng(seed).uniform(0.05, 1.0, patch).astype(F32)


def logits_case(n_mirrors, ncls, patch, seed, span=3.0):
    """logits [AGG_FIRST + n_mirrors, ncls, PV]: the samples in front belong to another tile."""
    return rng(seed).uniform(-span, span, (AGG_FIRST + n_mirrors, ncls, int(np.prod(patch)))).astype(F32)


def nonlin_case(ncls, seed):
    """Logits over [-30, 30]: sigmoid saturates on both sides and softmax needs its max shift."""
    return logits_case(8, ncls, AGG_PATCH, seed, span=30.0)


NONLIN_CASES = [(nonlin, ncls) for nonlin in ("sigmoid", "softmax") for ncls in (1, 3, 8)]


def measure_t():
    """Largest |float32 restatement - float64 restatement| of the mirror-averaged probabilities over NONLIN_CASES."""
    worst = {}
    for nonlin, ncls in NONLIN_CASES:
        lg = nonlin_case(ncls, 300 + ncls)[AGG_FIRST:]
        d = np.abs(tile_result(lg, MIRROR_LISTS["zyx"], AGG_PATCH, nonlin, np.float32).astype(np.float64)
                   - tile_result(lg, MIRROR_LISTS["zyx"], AGG_PATCH, nonlin, np.float64)).max()
        worst[nonlin] = max(worst.get(nonlin, 0.0), float(d))
    return worst


def nonlin32(lg, nonlin):
    """float32 restatement, one numpy operation per rounding, in the order of the contract: sigmoid 1 / (1 + exp(-x)); softmax
    exp(x - max) / sum in class order.  lg [ncls, ...]."""
    if nonlin == "sigmoid":
        return F32(1) / (F32(1) + np.exp(-lg))
    if nonlin == "softmax":
        e = np.exp(lg - lg.max(0, keepdims=True))
        den = np.zeros(lg.shape[1:], F32)
        for k in range(lg.shape[0]):
            den = den + e[k]
        return e / den[None]
    return lg


def nonlin64(lg, nonlin):
    lg = lg.astype(np.float64)
    if nonlin == "sigmoid":
        return 1.0 / (1.0 + np.exp(-lg))
    if nonlin == "softmax":
        e = np.exp(lg - lg.max(0, keepdims=True))
        return e / e.sum(0, keepdims=True)
    return lg


def tile_result(lg, mirrors, patch, nonlin, dtype, mut=None, fused=False):
    """res [ncls, P0, P1, P2] = sum over the list, in list order, of (1 / n) flip_back(nonlin(lg[i])).  dtype float32: every step
    rounded to fp32 (fused: product and sum through float64 with ONE rounding, as a fused multiply-add gives).
    mut: "swap_p1p2", "bit_order", "no_mult", "flip_dest" (the samples added unflipped and the tile then flipped as the last
    mask says)."""
    n = len(mirrors)
    f = F32 if dtype == np.float32 else np.float64
    mult = f(1) if mut == "no_mult" else f(1) / f(n)
    res = np.zeros((lg.shape[1],) + tuple(patch), dtype)
    for i, m in enumerate(mirrors):
        p = (nonlin32 if dtype == np.float32 else nonlin64)(lg[i].astype(dtype), nonlin).reshape(res.shape)
        if mut != "flip_dest":
            p = flip_tile(p, m, mut)
        if fused:
            res = (res.astype(np.float64) + np.float64(mult) * p.astype(np.float64)).astype(dtype)
        else:
            res = res + mult * p
    if mut == "flip_dest":
        res = flip_tile(res, mirrors[-1])
    return res


def scatter(res, gauss, agg, cnt, origin, mut=None):
    """agg[:, tile] += res * g, cnt[tile] += g (g = 1 without a map), in place, in the dtype of agg.  mut "gauss_flipped": the map
    read at the voxel flipped on every axis."""
    box = tuple(slice(o, o + p) for o, p in zip(origin, res.shape[1:]))
    g = np.ones(res.shape[1:], agg.dtype) if gauss is None else gauss.astype(agg.dtype)
    gr = g[::-1, ::-1, ::-1] if mut == "gauss_flipped" else g
    agg[(slice(None),) + box] += res * gr[None]
    if cnt is not None:
        cnt[box] += g
    return box


def overlap_bound(res, gauss, agg_after):
    """Derived: agg + res g onto a non-zero aggregate rounds the product (when the device does not fuse the two) and the sum:
    2^-24 (|res g| + |agg|), agg the exact new value, res and g fp32 numbers."""
    return U * (np.abs(res.astype(np.float64) * gauss.astype(np.float64)[None]) + np.abs(agg_after)) * (1 + 2 * U)


def cnt_case():
    """(cnt [140, 131, 133] random, gauss [130, 129, 127], origin): 2 129 790 tile voxels > 8192 x 256."""
    return rng(77).uniform(0.0, 4.0, (140, 131, 133)).astype(F32), weight_map((130, 129, 127), 78), (7, 2, 5)


# ------------------------------------------------------------------ finish (bit equality)
FINISH_PATCH = (16, 24, 40)


def finish_case(vol_shape, seed, k=3):
    padded = tuple(max(a, b) for a, b in zip(vol_shape, FINISH_PATCH))
    r = rng(seed)
    return r.standard_normal((k,) + padded).astype(F32), r.uniform(0.5, 8.0, padded).astype(F32)


def finish_ref(agg, cnt, vol_shape, n_folds, mut=None):
    """fp32: probs = agg / cnt cropped at pad_below = (padded - size) // 2, then / n_folds: one correctly rounded divide each.
    mut "pad_hi": cropped at the high-side padding."""
    lo = [(p - s) // 2 for p, s in zip(cnt.shape, vol_shape)]
    if mut == "pad_hi":
        lo = [(p - s) - (p - s) // 2 for p, s in zip(cnt.shape, vol_shape)]
    box = tuple(slice(l, l + s) for l, s in zip(lo, vol_shape))
    probs = agg[(slice(None),) + box] / cnt[box][None]
    return probs / F32(n_folds) if n_folds > 1 else probs


# ------------------------------------------------------------------ shared stage 0 (bit equality: copies)
S0_P, S0_T, S0_R, S0_VE, S0_C = (12, 24, 40), (4, 8, 8), 2, (20, 32, 48), 8
S0_WIDE = dict(P=(6, 10, 136), t=(4, 8, 8), r=2, Ve=(8, 16, 144), C=32)   # 136 * 32 / 4 = 1088 quads per row: a second, ragged trip


def s0_tensors(P, t, Ve, C, seed, n_wv=2, n_slab=3):
    r = rng(seed)
    wv = r.standard_normal((n_wv,) + tuple(Ve) + (C,)).astype(F32)
    slabs = []
    for a in range(3):
        s = [t[k] if k == a else P[k] for k in range(3)]
        slabs.append(r.standard_normal((n_slab,) + tuple(s) + (C,)).astype(F32))
    return wv, slabs


def s0_samples():
    """Built by hand: no face; each single face; the corner z lo + y hi + x lo (priority); all six; wv index 1; slab indices
    other than 0 throughout."""
    none = [-1] * 6
    out = [dict(wv=0, origin=(3, 5, 7), slab=list(none))]
    for f in range(6):
        s = list(none)
        s[f] = (f + 1) % 3
        out.append(dict(wv=f & 1, origin=(f, 8 - f, 2 + f), slab=s))
    out.append(dict(wv=1, origin=(8, 0, 8), slab=[2, -1, -1, 1, 2, -1]))
    out.append(dict(wv=1, origin=(4, 4, 4), slab=[1, 2, 0, 1, 2, 0]))
    out.append(dict(wv=0, origin=(0, 8, 0), slab=[0, 1, 2, 0, 1, 2]))
    return out


def s0_gather_ref(wv, slabs, samples, P, t, r, mut=None):
    """out [n, P0, P1, P2, C]: a voxel within r of a face that has a slab comes from that slab - the first such face in the order
    z lo, z hi, y lo, y hi, x lo, x hi - and every other voxel from the whole-volume result at origin + voxel.  A low-face slab
    covers the first t layers of the tile along its axis, a high-face slab the last t.
    mut: "hi_offset" (a high-face slab read as if it covered the last r layers), "y_first" (the y faces ahead of the z faces)."""
    out = np.empty((len(samples),) + tuple(P) + (wv.shape[-1],), F32)
    order = [2, 3, 0, 1, 4, 5] if mut == "y_first" else list(range(6))
    for i, sm in enumerate(samples):
        o = sm["origin"]
        out[i] = wv[sm["wv"], o[0]:o[0] + P[0], o[1]:o[1] + P[1], o[2]:o[2] + P[2]]
        for f in reversed(order):   # (the first face of the order is written last: it wins)
            if sm["slab"][f] < 0:
                continue
            a, hi = f >> 1, f & 1
            sl = slabs[a][sm["slab"][f]]
            dst, src = [slice(None)] * 3, [slice(None)] * 3
            if hi:
                dst[a] = slice(P[a] - r, P[a])
                src[a] = slice(0, r) if mut == "hi_offset" else slice(t[a] - r, t[a])
            else:
                dst[a], src[a] = slice(0, r), slice(0, r)
            out[i][tuple(dst)] = sl[tuple(src)]
    return out


MASK_VE, MASK_ZP, MASK_C, MASK_N = (12, 16, 24), (9, 16, 17), 8, 2   # (Ve == Zp on y: that box is empty)


def s0_mask_ref(x, keep):
    y = x.copy()
    y[:, keep[0]:] = 0
    y[:, :, keep[1]:] = 0
    y[:, :, :, keep[2]:] = 0
    return y
