"""-m gpu: the second-moment (M2) instantiations of the aggregation kernels of csrc/aggregate.hip, finish_moments_kernel, and
the maps / stats kernels of csrc/uncertainty.hip, one by one.

Shapes are the ones the plumbing tests pin (plumbing_util.AGG_*, MIRROR_LISTS, FINISH_PATCH; test_gpu_aggregate_tiles.py's patch
8 x 8 x 16 in 12 x 8 x 24).  Gates, each test says which: BIT EQUALITY (agg / cnt with and without agg2; the one-launch kernel
against the launches per tile; the mean of the finish); DERIVED bounds against the float64 restatements of uncertainty_util.py;
the two MEASURED constants uncertainty_util.T_STD / T_ENT."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import plumbing_util as pu
import uncertainty_util as uu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unc(amd):
    """the uncertainty module: the package does not import it by itself"""
    return importlib.import_module(amd.__name__ + ".uncertainty")


# (the helpers of test_gpu_plumbing.py)
def dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = got.view(np.uint8) == want.view(np.uint8)
    assert same.all(), f"{what}: {int((~same.reshape(got.size, -1).all(1)).sum())} of {got.size} elements differ"


def assert_within(got, ref, bound, what=""):
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max err {float(err.max()):.3e}, {ratio:.3f} of its bound")
    assert np.isfinite(got).all() and (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements beyond the bound, worst {ratio:.3f} x"


def _feat(gpu, f, dtype):
    return dev(pu.to_blocked(f), gpu).half() if dtype == "f16" else dev(f, gpu)


def _fresh(ncls, seed):
    """agg / cnt pre-filled with a sentinel pattern, zero inside the first tile's box."""
    agg, cnt = pu.sentinel((ncls,) + pu.AGG_PADDED, seed), pu.sentinel(pu.AGG_PADDED, seed + 1)
    box = tuple(slice(o, o + p) for o, p in zip(pu.AGG_ORIGIN, pu.AGG_PATCH))
    agg[(slice(None),) + box] = 0
    cnt[box] = 0
    return agg, cnt

# test_gpu_aggregate_tiles.py
PATCH, PADDED = (8, 8, 16), (12, 8, 24)
TILES = [(0, 0, 0), (4, 0, 0), (0, 0, 8), (4, 0, 8)]
THREE = [(0, 0, 0), (4, 0, 0), (4, 0, 8)]     # leaves z < 4, x >= 16 uncovered
MIRRORS = {1: [0], 8: [0, 4, 2, 6, 1, 5, 3, 7]}
PV = int(np.prod(PATCH))


def _tiles_case(gpu, n_tiles, nm, ncls, seed, gauss=True):
    r = np.random.default_rng(seed)
    lg = r.uniform(-6, 6, (n_tiles * nm, ncls, PV)).astype(np.float32)
    g = r.uniform(0.05, 1.0, PATCH).astype(np.float32) if gauss else None
    sent = lambda shape, s: np.random.default_rng(s).uniform(0.5, 2.0, shape).astype(np.float32)
    return dev(lg, gpu), dev(g, gpu), sent((ncls,) + PADDED, seed + 1), sent((ncls,) + PADDED, seed + 3), sent(PADDED, seed + 2)


def _run_tiles(amd, gpu, lg, g, agg, agg2, cnt, origins, mirrors, nonlin, how, with_cnt=True):
    """(agg, agg2, cnt) after: "tiles_m2" one launch with the second moment, "seq_m2" one m2 launch per tile, "tiles" the plain launch"""
    a, a2, c = dev(agg, gpu), dev(agg2, gpu), dev(cnt, gpu)
    cc = c if with_cnt else None
    if how == "tiles_m2":
        amd.ops.logits_aggregate_tiles_m2_(lg, mirrors, PATCH, nonlin, a, a2, cc, origins, g)
    elif how == "tiles":
        amd.ops.logits_aggregate_tiles_(lg, mirrors, PATCH, nonlin, a, cc, origins, g)
    else:
        for i, o in enumerate(origins):
            amd.ops.logits_aggregate_m2_(lg, mirrors, PATCH, nonlin, a, a2, cc, o, g, i * len(mirrors))
    return a.cpu().numpy(), a2.cpu().numpy(), c.cpu().numpy()


def _check_tiles(amd, gpu, case, origins, mirrors, nonlin, with_cnt=True):
    lg, g, agg, agg2, cnt = case
    one = _run_tiles(amd, gpu, lg, g, agg, agg2, cnt, origins, mirrors, nonlin, "tiles_m2", with_cnt)
    seq = _run_tiles(amd, gpu, lg, g, agg, agg2, cnt, origins, mirrors, nonlin, "seq_m2", with_cnt)
    plain = _run_tiles(amd, gpu, lg, g, agg, agg2, cnt, origins, mirrors, nonlin, "tiles", with_cnt)
    assert_bits(one[1], seq[1], "agg2: one launch against the launches per tile")
    for got, what in ((one, "tiles_m2"), (seq, "per-tile m2")):
        assert_bits(got[0], plain[0], f"agg of {what} against the plain call")
        assert_bits(got[2], plain[2], f"cnt of {what} against the plain call")
    assert_bits(plain[1], agg2, "the plain call does not touch agg2")
    assert not np.array_equal(one[1], agg2)
    return one


# ------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("nonlin,ncls", [("sigmoid", 3), ("softmax", 3), ("sigmoid", 1), ("softmax", 1)])
@pytest.mark.parametrize("nm", [1, 8])
def test_tiles_m2_equals_the_sequence(amd, gpu, nm, nonlin, ncls):
    """BIT EQUALITY: agg2 of the one-launch kernel = the per-tile m2 launches in order; agg and cnt of both = the plain call."""
    _check_tiles(amd, gpu, _tiles_case(gpu, len(TILES), nm, ncls, 1100 + nm + ncls), TILES, MIRRORS[nm], nonlin)


def test_tiles_m2_cnt_null_permuted_and_chunked(amd, gpu):
    """BIT EQUALITY: cnt = None (the normaliser untouched); a permuted tile list; 65 tiles (a second launch behind the first 64)."""
    case = _tiles_case(gpu, len(TILES), 8, 3, 1200)
    one = _check_tiles(amd, gpu, case, TILES, MIRRORS[8], "sigmoid", with_cnt=False)
    assert_bits(one[2], case[4], "cnt = None")
    perm = [2, 0, 3, 1]
    lgp = case[0].reshape(len(TILES), 8, 3, PV)[perm].reshape(case[0].shape).contiguous()
    _check_tiles(amd, gpu, (lgp,) + case[1:], [TILES[p] for p in perm], MIRRORS[8], "softmax")
    _check_tiles(amd, gpu, _tiles_case(gpu, 65, 1, 3, 1300), [TILES[i % 4] for i in range(65)], MIRRORS[1], "sigmoid")


@pytest.mark.parametrize("nm", [1, 8])
def test_uncovered_voxels_keep_the_agg2_sentinel(amd, gpu, nm):
    """BIT EQUALITY: three tiles whose bounding box holds voxels none covers - those keep agg2's sentinel; covered ones grow."""
    case = _tiles_case(gpu, len(THREE), nm, 3, 1400 + nm)
    one = _check_tiles(amd, gpu, case, THREE, MIRRORS[nm], "softmax")
    free = np.ones(PADDED, bool)
    for o in THREE:
        free[tuple(slice(k, k + p) for k, p in zip(o, PATCH))] = False
    assert free.any() and free[:4, :, 16:].all()
    assert_bits(one[1][:, free], case[3][:, free], "agg2 outside the tiles")
    # (a term p^2 g may vanish against a sentinel of about 1; the terms are never negative, and most of them register)
    assert (one[1][:, ~free] >= case[3][:, ~free]).all() and (one[1][:, ~free] != case[3][:, ~free]).mean() > 0.5


# ------------------------------------------------------------------ against float64
@pytest.mark.parametrize("nonlin,ncls", [("sigmoid", 1), ("sigmoid", 3), ("softmax", 3), ("softmax", 8)])
@pytest.mark.parametrize("name", ["zyx", "zx", "none"])
def test_logits_aggregate_m2_against_float64(amd, gpu, nonlin, ncls, name):
    """DERIVED from the measured T_NONLIN: |d(p^2)| = 2 p |dp| <= 2 T_NONLIN with p <= 1, plus one rounding U of the square, times
    the weight: agg2 within (2 T_NONLIN + U) g of float64.  Logits over [-30, 30], first_sample = 2, a non-symmetric weight map,
    onto zeros inside the box; the sentinel outside untouched.  agg, cnt BIT EQUAL to the plain call."""
    mirrors = pu.MIRROR_LISTS[name]
    lg = pu.logits_case(len(mirrors), ncls, pu.AGG_PATCH, 1500 + ncls, span=30.0)
    g = pu.weight_map(pu.AGG_PATCH, 1501)
    agg, cnt = _fresh(ncls, 1502)
    agg2, _ = _fresh(ncls, 1504)
    a, a2, c, ap, cp = dev(agg, gpu), dev(agg2, gpu), dev(cnt, gpu), dev(agg, gpu), dev(cnt, gpu)
    amd.ops.logits_aggregate_m2_(dev(lg, gpu), mirrors, pu.AGG_PATCH, nonlin, a, a2, c, pu.AGG_ORIGIN, dev(g, gpu), pu.AGG_FIRST)
    amd.ops.logits_aggregate_(dev(lg, gpu), mirrors, pu.AGG_PATCH, nonlin, ap, cp, pu.AGG_ORIGIN, dev(g, gpu), pu.AGG_FIRST)
    assert_bits(a.cpu().numpy(), ap.cpu().numpy(), "agg")
    assert_bits(c.cpu().numpy(), cp.cpu().numpy(), "cnt")
    _, res2 = uu.tile_moments(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, nonlin)
    ref = agg2.astype(np.float64)
    box = pu.scatter(res2, g, ref, None, pu.AGG_ORIGIN)
    bound = np.zeros_like(ref)
    bound[(slice(None),) + box] = (2 * pu.T_NONLIN + pu.U) * g[None]
    assert_within(a2.cpu().numpy(), ref, bound, f"agg2 logits {nonlin} ncls {ncls} {name}")


@pytest.mark.parametrize("nonlin,ncls,c", [("sigmoid", 3, 32), ("sigmoid", 8, 24), ("softmax", 3, 24), ("softmax", 8, 32)])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_head_aggregate_m2(amd, gpu, dtype, nonlin, ncls, c):
    """DERIVED + MEASURED: with B = L x (the head_logits bound, mirror-averaged) + T_NONLIN the bound of test_head_aggregate on a
    probability, agg2 is within (2 B + U) g of float64.  C 32 (compile-time) and 24, 8 mirrors (the unrolled instantiation) and the 4
    of axes (0, 2), the head normalising its features itself (NORM, slope 0.01) and not, first_sample = 2.  agg, cnt BIT EQUAL to the
    plain call; the sentinel outside the box untouched (bound 0)."""
    for name in ("zyx", "zx"):
        for norm in (True, False):
            mirrors = pu.MIRROR_LISTS[name]
            n = pu.AGG_FIRST + len(mirrors)
            f, w, b, scale, shift = pu.head_case(n, int(np.prod(pu.AGG_PATCH)), c, ncls, 1600 + c + ncls, dtype == "f16")
            w = w * np.float32(2)
            sc, sh, slope = (scale, shift, float(pu.SLOPE)) if norm else (None, None, 1.0)
            lg, lb = pu.head_ref(f, w, b, sc, sh, slope)
            g = pu.weight_map(pu.AGG_PATCH, 1601)
            agg, cnt = _fresh(ncls, 1602)
            agg2, _ = _fresh(ncls, 1604)
            a, a2, cd, ap, cp = dev(agg, gpu), dev(agg2, gpu), dev(cnt, gpu), dev(agg, gpu), dev(cnt, gpu)
            feat = _feat(gpu, f, dtype)
            amd.ops.head_aggregate_m2_(feat, w, b, mirrors, pu.AGG_PATCH, nonlin, a, a2, cd, pu.AGG_ORIGIN, dev(g, gpu), pu.AGG_FIRST,
                                       dev(sc, gpu), dev(sh, gpu), slope)
            amd.ops.head_aggregate_(feat, w, b, mirrors, pu.AGG_PATCH, nonlin, ap, cp, pu.AGG_ORIGIN, dev(g, gpu), pu.AGG_FIRST, dev(sc, gpu),
                                    dev(sh, gpu), slope)
            what = f"head m2 {dtype} {nonlin} ncls {ncls} C {c} {name} norm {norm}"
            assert_bits(a.cpu().numpy(), ap.cpu().numpy(), "agg " + what)
            assert_bits(cd.cpu().numpy(), cp.cpu().numpy(), "cnt " + what)
            _, res2 = uu.tile_moments(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, nonlin)
            ref = agg2.astype(np.float64)
            box = pu.scatter(res2, g, ref, None, pu.AGG_ORIGIN)
            mean_lb = pu.tile_result(lb[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, "identity", np.float64)
            if nonlin == "softmax":
                mean_lb = np.broadcast_to(pu.tile_result(lb[pu.AGG_FIRST:].max(1, keepdims=True), mirrors, pu.AGG_PATCH, "identity", np.float64),
                                          mean_lb.shape)
            bound = np.zeros_like(ref)
            bound[(slice(None),) + box] = (2 * (pu.LIPSCHITZ[nonlin] * mean_lb + pu.T_NONLIN) + pu.U) * g[None]
            assert_within(a2.cpu().numpy(), ref, bound, "agg2 " + what)


# ------------------------------------------------------------------ refusals
def test_identity_and_a_tile_outside_the_grid_are_refused(amd, gpu):
    lg, g, agg, agg2, cnt = _tiles_case(gpu, 2, 1, 3, 1700, gauss=False)
    a, a2, c = dev(agg, gpu), dev(agg2, gpu), dev(cnt, gpu)
    with pytest.raises(amd._lib.Mi355Error, match="identity"):
        amd.ops.logits_aggregate_m2_(lg, [0], PATCH, "identity", a, a2, c, (0, 0, 0))
    with pytest.raises(amd._lib.Mi355Error, match="identity"):
        amd.ops.logits_aggregate_tiles_m2_(lg, [0], PATCH, "identity", a, a2, c, [(0, 0, 0), (4, 0, 8)])
    f = torch.zeros((1, PV, 8), device=gpu)
    with pytest.raises(amd._lib.Mi355Error, match="identity"):
        amd.ops.head_aggregate_m2_(f, np.zeros((3, 8), np.float32), None, [0], PATCH, "identity", a, a2, c, (0, 0, 0))
    with pytest.raises(ValueError, match="leaves the padded grid"):
        amd.ops.logits_aggregate_tiles_m2_(lg, [0], PATCH, "sigmoid", a, a2, c, [(0, 0, 0), (5, 0, 8)])
    with pytest.raises(ValueError, match="leaves the padded grid"):
        amd.ops.logits_aggregate_m2_(lg, [0], PATCH, "sigmoid", a, a2, c, (5, 0, 8))
    # the library's own check, behind the wrapper's
    lib, i3 = amd._lib.load(), lambda v: (ctypes.c_int32 * 3)(*v)
    rc = lib.mi355_logits_aggregate_m2(lg.data_ptr(), 3, 0, (ctypes.c_int32 * 1)(0), 1, i3(PATCH), amd._lib.NONLIN_SIGMOID, None, a.data_ptr(),
                                       a2.data_ptr(), c.data_ptr(), i3(PADDED), i3((5, 0, 8)), None)
    assert rc < 0 and b"leaves the padded grid" in lib.mi355_last_error()
    for t, ref in ((a, agg), (a2, agg2), (c, cnt)):
        assert_bits(t.cpu().numpy(), ref, "a refused call writes nothing")
    with pytest.raises(ValueError, match="identity"):
        amd.predictor.predict_folds_moments([object()], np.zeros((4, 8, 8, 8), np.float32), nonlin="identity")


# ------------------------------------------------------------------ finish
@pytest.mark.parametrize("n_folds", [1, 3])
def test_finish_moments(amd, gpu, n_folds):
    """mean BIT EQUAL to finish_sharded (mi355_sw_finish_folds); m2 DERIVED: two correctly rounded divisions of fp32 numbers,
    2 U |ref| (1 + U) about the float64 quotient.  Volume 13 x 30 x 37 under the patch 16 x 24 x 40: padded on z and x by 3
    (1 below, 2 above), not on y."""
    vol = (13, 30, 37)
    agg, cnt = pu.finish_case(vol, 1800)
    agg2 = np.abs(pu.finish_case(vol, 1801)[0])
    mean, m2 = amd.predictor.finish_sharded_moments(dev(agg, gpu), dev(agg2, gpu), dev(cnt, gpu), vol, pu.FINISH_PATCH, n_folds)
    want = amd.predictor.finish_sharded(dev(agg, gpu), dev(cnt, gpu), vol, pu.FINISH_PATCH, n_folds)
    assert_bits(mean.cpu().numpy(), want.cpu().numpy(), "mean against finish_sharded")
    assert_bits(mean.cpu().numpy(), pu.finish_ref(agg, cnt, vol, n_folds), "mean against the float32 restatement")
    lo = [(p - s) // 2 for p, s in zip(cnt.shape, vol)]
    box = tuple(slice(l, l + s) for l, s in zip(lo, vol))
    ref = agg2.astype(np.float64)[(slice(None),) + box] / cnt.astype(np.float64)[box][None] / n_folds
    assert_within(m2.cpu().numpy(), ref, 2 * pu.U * np.abs(ref) * (1 + pu.U) + 2.0 ** -149, f"m2 folds {n_folds}")


# ------------------------------------------------------------------ maps and stats
@pytest.fixture(scope="module")
def maps_inputs():
    return {nl: (uu.maps_case(10, nl), uu.maps_case(11, nl, True)) for nl in ("sigmoid", "softmax")}


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("nonlin", ["sigmoid", "softmax"])
def test_uncertainty_maps(unc, gpu, maps_inputs, nonlin, two):
    """MEASURED: std within T_STD, entropy within T_ENT of float64 (uncertainty_util: 4 x the float32-against-float64 figure on
    these inputs).  [3, 37, 41, 29] = 132 053 voxels per channel (no multiple of 256), pasted at (2, 3, 5) into 41 x 47 x 40 zeros.
    Exact: var = 0 where m2 = mean^2 or one ulp below it, entropy 0 at mean 0 and 1 and 1 at 0.5 (sigmoid); no NaN anywhere; the
    reduced maps are the channel maxima of the per-channel ones bit for bit (softmax: the categorical entropy), zero outside the box."""
    (ma, m2a), (mb, m2b) = maps_inputs[nonlin]
    b = (dev(mb, gpu), dev(m2b, gpu)) if two else (None, None)
    out = unc.maps(dev(ma, gpu), dev(m2a, gpu), *b, nonlin=nonlin, bbox_lo=uu.MAPS_LO, full_shape=uu.MAPS_FULL)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ref = uu.maps64(ma, m2a, mb if two else None, m2b if two else None, nonlin)
    assert all(np.isfinite(v).all() for v in got.values())
    assert_within(got["std"], ref["std"], np.full(ref["std"].shape, uu.T_STD), f"std {nonlin} two {two}")
    assert_within(got["entropy"], ref["entropy"], np.full(ref["std"].shape, uu.T_ENT), f"entropy {nonlin} two {two}")
    assert got["entropy"].min() >= 0 and got["entropy"].max() <= 1 and got["std"].min() >= 0
    if not two:
        flat_s, flat_e = got["std"].reshape(3, -1), got["entropy"].reshape(3, -1)
        assert (flat_s[:, :45] == 0).all(), "m2 = mean^2, or one ulp below: var is exactly 0"
        if nonlin == "sigmoid":
            assert (flat_e[:, :2] == 0).all() and (flat_e[:, 2] == 1).all()
    box = tuple(slice(l, l + s) for l, s in zip(uu.MAPS_LO, uu.MAPS_SHAPE[1:]))
    for name, per in (("std_max", "std"), ("entropy_max", "entropy")):
        full = np.zeros(uu.MAPS_FULL, np.float32)
        full[box] = got[per].max(0)
        assert_bits(got[name], full, name)
    # either per-channel output may be left out
    lean = unc.maps(dev(ma, gpu), dev(m2a, gpu), *b, nonlin=nonlin, bbox_lo=uu.MAPS_LO, full_shape=uu.MAPS_FULL, per_channel=False)
    assert lean["std"] is None and lean["entropy"] is None
    assert_bits(lean["std_max"].cpu().numpy(), got["std_max"], "std_max alone")
    assert_bits(lean["entropy_max"].cpu().numpy(), got["entropy_max"], "entropy_max alone")


def test_uncertainty_maps_refusals(amd, unc, gpu, maps_inputs):
    (ma, m2a), _ = maps_inputs["sigmoid"]
    with pytest.raises(ValueError, match="identity"):
        unc.maps(dev(ma, gpu), dev(m2a, gpu), nonlin="identity")
    lib, i3 = amd._lib.load(), lambda v: (ctypes.c_int32 * 3)(*v)
    a, a2 = dev(ma, gpu), dev(m2a, gpu)
    out = torch.zeros(uu.MAPS_FULL, device=gpu)
    rc = lib.mi355_uncertainty_maps(a.data_ptr(), a2.data_ptr(), None, None, 3, 37, 41, 29, amd._lib.NONLIN_IDENTITY, None, None, i3(uu.MAPS_LO),
                                    i3(uu.MAPS_FULL), out.data_ptr(), None, None)
    assert rc < 0 and b"no probabilities" in lib.mi355_last_error()
    with pytest.raises(amd._lib.Mi355Error, match="does not fit"):
        unc.maps(a, a2, bbox_lo=(5, 3, 5), full_shape=uu.MAPS_FULL)
    with pytest.raises(ValueError, match="classes"):
        unc.maps(a, a2, a[:2], a2[:2])


@pytest.mark.parametrize("nonlin", ["sigmoid", "softmax"])
def test_uncertainty_stats(unc, gpu, maps_inputs, nonlin):
    """Counts EXACT (strict >: the special voxels sit exactly at 0.25, 0.5 and 0.75 and count for none of their own thresholds).
    Sums DERIVED: against float64 sums of the downloaded device maps at N 2^-53 sum |x| (N additions, each one rounding of a partial
    sum no larger than sum |x|); max var exact.  Two runs BIT EQUAL."""
    (ma, m2a), _ = maps_inputs[nonlin]
    out = unc.maps(dev(ma, gpu), dev(m2a, gpu), nonlin=nonlin)
    mean, var, ent = dev(ma, gpu), out["std"] * out["std"], out["entropy"]
    counts, sums = unc.region_stats(mean, var, ent, uu.THRESHOLDS)
    counts2, sums2 = unc.region_stats(mean, var, ent, uu.THRESHOLDS)
    assert_bits(sums, sums2, "two runs")
    assert np.array_equal(counts, counts2)
    rc, rs, mass = uu.stats64(ma, var.cpu().numpy(), ent.cpu().numpy(), uu.THRESHOLDS)
    assert counts.dtype == np.int64 and np.array_equal(counts, rc), (counts, rc)
    n = ma[0].size
    assert_within(sums[:, :6], rs[:, :6], n * 2.0 ** -53 * mass, f"sums {nonlin}")
    assert np.array_equal(sums[:, 6], rs[:, 6])
    # strictness, spelled out: a volume of exactly 0.5 has no voxel above 0.5 and all above 0.25
    half = torch.full((1, 1000), 0.5, device=gpu)
    c, s = unc.region_stats(half, torch.zeros_like(half), torch.ones_like(half), uu.THRESHOLDS)
    assert c.tolist() == [[1000, 0, 0, 0]] and s[0].tolist() == [500.0, 0.0, 1000.0, 0.0, 0.0, 0.0, 0.0]
