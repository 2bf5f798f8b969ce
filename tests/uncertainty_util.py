"""float64 restatements of the ensemble-uncertainty definitions (uncertainty.py, csrc/uncertainty.hip, the M2 aggregation kernels of
csrc/aggregate.hip), for tests/test_gpu_uncertainty_*.py and tests/test_uncertainty_cpu.py.

For one ensemble member, one class k and one voxel v the samples are s = (fold, tile that covers v, mirror) with probability p_s and
weight w_s = g_t(v) / (cnt(v) n_folds n_mirrors), cnt(v) = sum_t g_t(v):  mean = sum w_s p_s,  m2 = sum w_s p_s^2,
var = max(m2 - mean^2, 0).  Two members of equal weight: the means of their means and of their m2.  Entropy in bits, in [0, 1],
0 log 0 = 0: per channel -m log2 m - (1 - m) log2 (1 - m) for sigmoid heads, per voxel -sum_k m_k log2 m_k / log2 K for softmax."""
import numpy as np

import plumbing_util as pu

#: MEASURED (tolerance convention of plumbing_util.T_MEASURED): the largest difference between the float32 restatement maps32 and
#: the float64 one maps64 on the inputs of maps_case (seeds 10 and 11; one and two members, sigmoid and softmax), on the CPU, was
#: 1.725e-04 for std (where m2 is within an ulp or two of mean^2 the float32 difference m2 - mean^2 is all rounding and the root
#: magnifies it: sqrt(2^-25) = 1.7e-4) and 5.38e-07 for the entropy; the device sqrt / log2 may differ from numpy's by an ulp, so
#: the gates take 4 x each.  test_uncertainty_cpu.py repeats the measurement.
T_STD_MEASURED = 1.73e-4
T_ENT_MEASURED = 5.4e-7
T_STD = 4 * T_STD_MEASURED
T_ENT = 4 * T_ENT_MEASURED

THRESHOLDS = (0.25, 0.5, 0.75)


# ------------------------------------------------------------------ one tile
def tile_moments(logits, mirrors, patch, nonlin):
    """(mean term, square term) [ncls, P0, P1, P2] float64 of one tile from its logits [n_mirrors, ncls, PV]: the sums over the
    mirror list of (1 / n) flip_back(p) and (1 / n) flip_back(p)^2."""
    n = len(mirrors)
    res = np.zeros((logits.shape[1],) + tuple(patch))
    res2 = np.zeros_like(res)
    for i, m in enumerate(mirrors):
        p = pu.flip_tile(pu.nonlin64(logits[i], nonlin).reshape(res.shape), m)
        res += p / n
        res2 += p * p / n
    return res, res2


# ------------------------------------------------------------------ the whole predictor
def predict_moments(net_fns, data, patch, step, mirror_axes, nonlin, use_gaussian=True):
    """(mean, m2) [K, Z, Y, X] float64 of one ensemble member: loops folds, tiles and mirrors as oracle.tiler_ref's
    predict_3d_tiled does, accumulating p and p^2 in float64.  net_fns: one callable per fold, NCDHW float32 torch -> logits."""
    import torch
    from oracle import tiler_ref
    data = np.asarray(data, dtype=np.float32)
    padded, lo = tiler_ref.pad_to_patch(data, patch)
    shape = padded.shape[1:]
    steps = tiler_ref.compute_steps_for_sliding_window(patch, shape, step)
    n_tiles = len(steps[0]) * len(steps[1]) * len(steps[2])
    g = tiler_ref.get_gaussian(patch, 1.0 / 8).astype(np.float64) if use_gaussian and n_tiles > 1 else np.ones(patch)
    sched = tiler_ref.mirror_schedule(mirror_axes) if mirror_axes else [()]
    agg = agg2 = None
    cnt = np.zeros(shape)
    with torch.no_grad():
        for f, net_fn in enumerate(net_fns):
            for z in steps[0]:
                for y in steps[1]:
                    for x in steps[2]:
                        sl = (slice(None), slice(z, z + patch[0]), slice(y, y + patch[1]), slice(x, x + patch[2]))
                        tile = torch.from_numpy(np.ascontiguousarray(padded[sl][None]))
                        s1 = s2 = 0.0
                        for dims in sched:
                            p = tiler_ref.apply_nonlin(net_fn(torch.flip(tile, dims) if dims else tile), nonlin)
                            p = (torch.flip(p, dims) if dims else p)[0].double().numpy()
                            s1 = s1 + p / len(sched)
                            s2 = s2 + p * p / len(sched)
                        if agg is None:
                            agg, agg2 = np.zeros((s1.shape[0],) + tuple(shape)), np.zeros((s1.shape[0],) + tuple(shape))
                        agg[sl] += s1 * g[None]
                        agg2[sl] += s2 * g[None]
                        if f == 0:
                            cnt[sl[1:]] += g
    crop = tuple(slice(l, l + s) for l, s in zip(lo, data.shape[1:]))
    n = float(len(net_fns))
    return agg[(slice(None),) + crop] / cnt[crop][None] / n, agg2[(slice(None),) + crop] / cnt[crop][None] / n


# ------------------------------------------------------------------ maps
def _plogp(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > 0, -x * np.log2(np.where(x > 0, x, 1)), 0).astype(x.dtype)


def _maps(mean_a, m2_a, mean_b, m2_b, nonlin, f):
    mu, m2 = mean_a.astype(f), m2_a.astype(f)
    if mean_b is not None:
        mu, m2 = (mu + mean_b.astype(f)) / f(2), (m2 + m2_b.astype(f)) / f(2)
    var = np.maximum(m2 - mu * mu, f(0))
    std = np.sqrt(var)
    if nonlin == "softmax":
        k = mu.shape[0]
        cat = np.zeros(mu.shape[1:], f)
        for c in range(k):
            cat = cat + _plogp(mu[c])
        cat = cat * f(1.0 / np.log2(k)) if k > 1 else cat * f(0)
        ent = np.broadcast_to(np.clip(cat, f(0), f(1))[None], mu.shape).copy()
    else:
        ent = np.clip(_plogp(mu) + _plogp(f(1) - mu), f(0), f(1))
    return dict(mean=mu, var=var, std=std, entropy=ent, std_max=std.max(0), entropy_max=ent.max(0))


def maps64(mean_a, m2_a, mean_b=None, m2_b=None, nonlin="sigmoid"):
    """float64: the definitions."""
    return _maps(mean_a, m2_a, mean_b, m2_b, nonlin, np.float64)


def maps32(mean_a, m2_a, mean_b=None, m2_b=None, nonlin="sigmoid"):
    """float32, one numpy operation per rounding in the kernel's order (the product mean^2 rounded before the subtraction)."""
    return _maps(mean_a, m2_a, mean_b, m2_b, nonlin, np.float32)


MAPS_SHAPE = (3, 37, 41, 29)
MAPS_LO, MAPS_FULL = (2, 3, 5), (41, 47, 40)


def maps_case(seed, nonlin="sigmoid", second=False):
    """(mean, m2) float32 [3, 37, 41, 29]: random probabilities with a random spread, softmax rows summing to one; the first voxels
    of every channel hold the special values - mean exactly 0, 1, 0.5, 0.25, 0.75 with m2 = mean^2 (no spread), and means whose
    m2 is one float32 ulp BELOW the float32 square (var must come out 0, not NaN)."""
    r = pu.rng(seed)
    if nonlin == "softmax":
        mean = r.dirichlet(np.ones(MAPS_SHAPE[0]) * 0.7, MAPS_SHAPE[1:]).transpose(3, 0, 1, 2)
    else:
        mean = r.beta(0.4, 0.4, MAPS_SHAPE)
    mean = mean.astype(np.float32)
    spread = (r.uniform(0, 1, MAPS_SHAPE) ** 3).astype(np.float32)
    m2 = (mean * mean + spread * mean * (np.float32(1) - mean)).astype(np.float32)   # mean^2 <= m2 <= mean
    fm, f2 = mean.reshape(MAPS_SHAPE[0], -1), m2.reshape(MAPS_SHAPE[0], -1)
    special = np.array([0.0, 1.0, 0.5, 0.25, 0.75], np.float32)
    if not second:
        fm[:, :5], f2[:, :5] = special, special * special
        sq = (fm[:, 5:45] * fm[:, 5:45]).astype(np.float32)
        f2[:, 5:45] = np.nextafter(sq, np.float32(-1))
    return mean, m2


# ------------------------------------------------------------------ stats
def stats64(mean, var, entropy, thresholds=THRESHOLDS):
    """(counts int64 [C, T + 1], sums float64 [C, 7]) of float32 maps [C, ...]: exact counts (strict >), float64 sums (math.fsum-free:
    numpy's pairwise float64 sum), max var."""
    c = mean.shape[0]
    m, v, e = (a.reshape(c, -1) for a in (mean, var, entropy))
    fg = m > np.float32(0.5)
    counts = np.stack([(m > np.float32(t)).sum(1) for t in thresholds] + [fg.sum(1)], 1).astype(np.int64)
    d = lambda a: a.astype(np.float64)
    sums = np.stack([d(m).sum(1), d(v).sum(1), d(e).sum(1), (d(m) * fg).sum(1), (d(v) * fg).sum(1), (d(e) * fg).sum(1), d(v).max(1)], 1)
    mass = np.stack([np.abs(d(m)).sum(1), np.abs(d(v)).sum(1), np.abs(d(e)).sum(1)] * 2, 1)
    return counts, sums, mass
