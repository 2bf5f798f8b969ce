"""not gpu: the references of tests/plumbing_util.py must DISCRIMINATE.  For every kernel test_gpu_plumbing.py pins, a plausible
wrong kernel - restated as a variant of the numpy reference - must miss that kernel's gate on the very inputs the GPU test
uses; and the float32 restatements the bit-equality claims rest on must not depend on whether the device fuses a multiply-add.
(In the spirit of test_reference_mutations_exceed_the_gates for the convolutions.)"""
import numpy as np
import pytest

import plumbing_util as pu


def differs(a, b):
    """A bit-equality gate is missed."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape != b.shape or bool((a.view(np.uint8) != b.view(np.uint8)).any())


def beyond(wrong, ref, bound):
    """Fraction of elements of a wrong result that miss a bound gate."""
    return float((np.abs(wrong - ref) > bound).mean())


# ------------------------------------------------------------------ extract_tiles
@pytest.mark.parametrize("c,cpad", [(4, 4), (4, 8), (3, 8)])
@pytest.mark.parametrize("mut", ["swap_p1p2", "bit_order", "pad_hi"])
def test_extract_mutations_are_seen(c, cpad, mut):
    """P1 / P2 swapped in the flip; masks read with bit0 = x; the volume placed by its high-side padding (z and x: 1 | 2)."""
    vol, pad, tiles, patch = pu.extract_case(c)
    assert differs(pu.extract_ref(vol, pad, tiles, patch, cpad, mut), pu.extract_ref(vol, pad, tiles, patch, cpad))


def test_extract_every_tile_hangs_over_and_blocked_is_not_plain():
    vol, pad, tiles, patch = pu.extract_case(4)
    ref = pu.extract_ref(vol, pad, tiles, patch, 8).reshape((len(tiles),) + patch + (8,))
    faces = np.zeros(6, bool)
    for (z0, y0, x0, _) in tiles:
        for a, (o, p, n) in enumerate(zip((z0, y0, x0), patch, vol.shape[1:])):
            faces[2 * a] |= o - pad[a] < 0
            faces[2 * a + 1] |= o - pad[a] + p > n
    assert faces.all()
    assert (ref[..., 4:] == 0).all() and (ref[..., :4] != 0).any(-1).mean() > 0.2
    # the blocked layout read as plain: a different tensor (and back is the identity)
    assert differs(pu.to_blocked(np.repeat(ref.reshape(len(tiles), -1, 8), 2, axis=2)).reshape(len(tiles), -1, 16),
                   np.repeat(ref.reshape(len(tiles), -1, 8), 2, axis=2))
    x = pu.rng(1).standard_normal((2, 11, 24)).astype(np.float32)
    assert not differs(pu.from_blocked(pu.to_blocked(x)), x) and differs(pu.to_blocked(x).reshape(2, 11, 24), x)
    # a flip of the destination instead of the source is the same copy (a flip is an involution): nothing to tell apart here,
    # the aggregation below is where the two differ
    vol_g, pad_g, tiles_g, patch_g = pu.extract_case(4, grid=True)
    assert int(np.prod(patch_g)) > 4096 * 256 and len(tiles_g) == 2


# ------------------------------------------------------------------ norm_finalize
def test_finalize_mutations_are_seen():
    """The variance clamp removed (the 0.3f constant channel: variance -3.6e-9); the group base c // cpg without x cpg."""
    stats, gamma, beta = pu.finalize_case(3, 40, 541, True)
    scale, shift, slack = pu.finalize_ref(stats, pu.NORM_COUNT, "instance", 1, 1e-5, gamma, beta)
    b_scale, b_shift = pu.finalize_gates(scale, shift, slack)
    w_scale, w_shift, _ = pu.finalize_ref(stats, pu.NORM_COUNT, "instance", 1, 1e-5, gamma, beta, "no_clamp")
    ch = pu.CONST_CH[1]
    assert abs(w_scale[0, ch] - scale[0, ch]) > 100 * b_scale[0, ch] and abs(w_shift[0, ch] - shift[0, ch]) > 100 * b_shift[0, ch]
    # 0.1f squares ABOVE its exact square: that channel sits just above the clamp and the clamp changes nothing there
    assert w_scale[0, pu.CONST_CH[0]] == scale[0, pu.CONST_CH[0]]
    # var ~ eps: eps inside the root matters (without it the scale moves by tens of per cent)
    no_eps = 1.0 / np.sqrt(1.1e-5)
    assert abs(no_eps * gamma[2] - scale[0, 2]) > 1e6 * b_scale[0, 2]
    stats, gamma, beta = pu.finalize_case(2, 48, 500 + 48 + 8, True)
    scale, shift, slack = pu.finalize_ref(stats, pu.NORM_COUNT, "group", 8, 1e-5, gamma, beta)
    b_scale, b_shift = pu.finalize_gates(scale, shift, slack)
    w_scale, w_shift, _ = pu.finalize_ref(stats, pu.NORM_COUNT, "group", 8, 1e-5, gamma, beta, "group_base")
    assert beyond(w_scale, scale, b_scale) > 0.8 and beyond(w_shift, shift, b_shift) > 0.8
    # group statistics are not instance statistics
    i_scale, _, _ = pu.finalize_ref(stats, pu.NORM_COUNT, "instance", 1, 1e-5, gamma, beta)
    assert beyond(i_scale, scale, b_scale) > 0.9


# ------------------------------------------------------------------ norm_apply / head_logits
@pytest.mark.parametrize("half", [False, True])
def test_apply_mutations_are_seen(half):
    """Scale / shift of sample 0 for every sample; the blocked fp16 layout read as plain; a dropped or doubly applied element."""
    x, scale, shift = pu.apply_case(2, 997, 32, 632, half)
    for act in (0, 1):
        ref, bound = pu.apply_ref(x, scale, shift, act, half)
        wrong, _ = pu.apply_ref(x, scale, shift, act, half, "sample0")
        assert beyond(wrong[1], ref[1], bound[1]) > 0.99
        if half:
            plain, _ = pu.apply_ref(pu.to_blocked(x).reshape(x.shape), scale, shift, act, half)
            assert beyond(pu.from_blocked(plain.reshape(2, 4, 997, 8)), ref, bound) > 0.5
        twice, _ = pu.apply_ref(ref.astype(np.float32), scale, shift, act, half)
        assert beyond(twice, ref, bound) > 0.99 and beyond(x.astype(np.float64), ref, bound) > 0.99
    assert bound.max() < 1e-2 and (bound > 0).all()


@pytest.mark.parametrize("c", [8, 24, 32, 64])
def test_head_mutations_are_seen(c):
    """Scale / shift of sample 0 for every sample; the blocked layout read as plain; a weight row off by one class."""
    f, w, b, scale, shift = pu.head_case(2, 4099, c, 3, 700 + c + 3)
    ref, bound = pu.head_ref(f, w, b, scale, shift, float(pu.SLOPE))
    wrong, _ = pu.head_ref(f, w, b, scale, shift, float(pu.SLOPE), "sample0")
    assert beyond(wrong[1], ref[1], bound[1]) > 0.99
    if c > 8:
        plain, _ = pu.head_ref(pu.to_blocked(f).reshape(f.shape), w, b, scale, shift, float(pu.SLOPE))
        assert beyond(plain, ref, bound) > 0.99
    rolled, _ = pu.head_ref(f, np.roll(w, 1, 0), b, scale, shift, float(pu.SLOPE))
    assert beyond(rolled, ref, bound) > 0.99
    no_act, _ = pu.head_ref(f, w, b, scale, shift, 1.0)
    assert beyond(no_act, ref, bound) > 0.5
    assert float((bound / np.maximum(np.abs(ref), 1e-30)).mean()) < 1e-3


# ------------------------------------------------------------------ aggregation
AGG_MUTS = ["swap_p1p2", "bit_order", "no_mult", "flip_dest"]


def _tile(mirrors, mut=None, nonlin="identity", ncls=3, lg=None):
    lg = pu.logits_case(len(mirrors), ncls, pu.AGG_PATCH, 800 + len(mirrors)) if lg is None else lg
    return pu.tile_result(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, nonlin, np.float32, mut)


@pytest.mark.parametrize("mut", AGG_MUTS)
def test_aggregate_index_mutations_are_seen(mut):
    """P1 / P2 swapped in the flip-back; the flip on the destination; the other bit order; the 1 / n factor omitted - each on
    the 8-mirror list (bit equality is the gate: any differing element misses it), and where the list can show it on the
    shorter ones."""
    for name, mirrors in pu.MIRROR_LISTS.items():
        shows = any(m & 6 for m in mirrors) if mut == "swap_p1p2" else len(mirrors) > 1
        assert differs(_tile(mirrors, mut), _tile(mirrors)) == shows, (name, mut)


def test_aggregate_weight_map_first_sample_and_order_are_seen():
    mirrors = pu.MIRROR_LISTS["zyx"]
    lg = pu.logits_case(8, 3, pu.AGG_PATCH, 808)
    g = pu.weight_map(pu.AGG_PATCH, 801)
    res = pu.tile_result(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, "identity", np.float32)

    def run(res, mut=None, origin=pu.AGG_ORIGIN):
        agg, cnt = np.zeros((3,) + pu.AGG_PADDED, np.float32), np.zeros(pu.AGG_PADDED, np.float32)
        pu.scatter(res, g, agg, cnt, origin, mut)
        return agg, cnt
    agg, cnt = run(res)
    assert differs(run(res, "gauss_flipped")[0], agg)                      # the weight map read at the flipped voxel
    assert not differs(run(res, "gauss_flipped")[1], cnt)                  # (cnt reads it unflipped either way: agg alone shows it)
    assert differs(run(pu.tile_result(lg[:8], mirrors, pu.AGG_PATCH, "identity", np.float32))[0], agg)   # first_sample ignored
    swapped = tuple(pu.AGG_ORIGIN[k] for k in (0, 2, 1))
    assert all(o + p <= q for o, p, q in zip(swapped, pu.AGG_PATCH, pu.AGG_PADDED)) and differs(run(res, origin=swapped)[0], agg)
    # Yp / Xp swapped in the scatter stride: the same flat buffer read as [Zp][Xp][Yp]
    z, y, x = pu.AGG_PADDED
    assert differs(agg.reshape(3, z, x, y).transpose(0, 1, 3, 2), agg)
    # the reversed list is another summation order of the same eight terms: close, and not the same bits
    rev = pu.tile_result(lg[pu.AGG_FIRST:], pu.MIRROR_LISTS["zyx_reversed"], pu.AGG_PATCH, "identity", np.float32)
    assert differs(rev, res) and np.abs(rev - res).max() > 1e-2   # (the samples belong to their masks: reversed masks, other tile)
    assert len(set(pu.AGG_PATCH)) == len(set(pu.AGG_PADDED)) == len(set(pu.AGG_ORIGIN)) == 3
    assert differs(g, g[::-1]) and differs(g, g[:, ::-1]) and differs(g, g[:, :, ::-1])


@pytest.mark.parametrize("name", sorted(pu.MIRROR_LISTS))
def test_float32_restatement_does_not_depend_on_fusing(name):
    """For a power-of-two mirror count 1 / n is exact and so is every product with it: res + (1 / n) p rounds once whether the
    device fuses the multiply-add or not, and onto zeros (or with g = 1) so does agg + res g.  The restatement must give the
    same bits with every step rounded separately and with each step fused through float64."""
    mirrors = pu.MIRROR_LISTS[name]
    assert len(mirrors) in (1, 2, 4, 8)
    lg = pu.logits_case(len(mirrors), 3, pu.AGG_PATCH, 800 + len(mirrors))[pu.AGG_FIRST:]
    stepwise = pu.tile_result(lg, mirrors, pu.AGG_PATCH, "identity", np.float32)
    fused = pu.tile_result(lg, mirrors, pu.AGG_PATCH, "identity", np.float32, fused=True)
    assert not differs(stepwise, fused)
    g = pu.weight_map(pu.AGG_PATCH, 801)
    onto_zero = (np.zeros(stepwise.shape) + stepwise.astype(np.float64) * g.astype(np.float64)[None]).astype(np.float32)
    assert not differs(onto_zero, stepwise * g[None])
    prior = pu.rng(5).standard_normal(stepwise.shape).astype(np.float32)
    assert not differs((prior.astype(np.float64) + stepwise.astype(np.float64) * 1.0).astype(np.float32), prior + stepwise * np.float32(1))
    # with a map onto a non-zero aggregate the two DO differ: that case carries the derived gate 2^-24 (|res g| + |agg|) about the
    # exact sum (the product's rounding when it is not fused, and the sum's), which both must meet
    exact = prior.astype(np.float64) + stepwise.astype(np.float64) * g[None]
    a, b = exact.astype(np.float32), prior + stepwise * g[None]
    assert differs(a, b)
    bound = pu.overlap_bound(stepwise, g, exact)
    assert (np.abs(a - exact) <= bound).all() and (np.abs(b - exact) <= bound).all()


@pytest.mark.parametrize("nonlin,ncls", pu.NONLIN_CASES)
def test_nonlinearity_gate(nonlin, ncls):
    """The measured constant holds here, and the gate built on it still tells sigmoid from softmax, a missing max shift's
    overflow, an omitted 1 / n and a wrong flip."""
    mirrors = pu.MIRROR_LISTS["zyx"]
    lg = pu.nonlin_case(ncls, 300 + ncls)
    assert lg.min() < -29 and lg.max() > 29
    ref = pu.tile_result(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, nonlin, np.float64)
    f32 = pu.tile_result(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, nonlin, np.float32)
    t = float(np.abs(f32 - ref).max())
    print(f"float32 against float64 {nonlin} ncls {ncls}: {t:.3e}")
    assert t <= pu.T_MEASURED
    for mut in AGG_MUTS:
        wrong = pu.tile_result(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, nonlin, np.float64, mut)
        if nonlin == "softmax" and ncls == 1:
            assert mut == "no_mult" or not differs(wrong, ref)   # (one class: every probability is 1)
        else:
            assert beyond(wrong, ref, pu.T_NONLIN) > 0.5, mut
    if ncls > 1:
        other = pu.tile_result(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, "sigmoid" if nonlin == "softmax" else "softmax", np.float64)
        assert beyond(other, ref, pu.T_NONLIN) > 0.5
    with np.errstate(over="ignore", invalid="ignore"):
        unshifted = np.exp(lg.astype(np.float32) * np.float32(4))   # (a softmax without its max shift overflows at these logits x 4)
    assert nonlin != "softmax" or np.isinf(unshifted).any()


def test_measured_t_is_what_the_docstring_says():
    worst = pu.measure_t()
    print(f"measure_t: {worst}")
    assert max(worst.values()) <= pu.T_MEASURED and pu.T_NONLIN == 4 * pu.T_MEASURED
    assert max(worst.values()) >= pu.T_MEASURED / 4   # (the constant is the measurement, not a generous round number)


def test_head_aggregate_gate_sees_index_mutations():
    """The derived head bound, averaged over the mirrors, is orders of magnitude below what a wrong index does."""
    mirrors = pu.MIRROR_LISTS["zyx"]
    f, w, b, scale, shift = pu.head_case(pu.AGG_FIRST + 8, int(np.prod(pu.AGG_PATCH)), 32, 3, 840 + 32 + 3)
    w = w * np.float32(2)
    lg, lb = pu.head_ref(f, w, b, scale, shift, float(pu.SLOPE))
    assert np.abs(lg).max() > 30
    ref = pu.tile_result(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, "identity", np.float64)
    bound = pu.tile_result(lb[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, "identity", np.float64)
    for mut in AGG_MUTS:
        assert beyond(pu.tile_result(lg[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, "identity", np.float64, mut), ref, bound) > 0.9, mut
    assert beyond(pu.tile_result(lg[:8], mirrors, pu.AGG_PATCH, "identity", np.float64), ref, bound) > 0.9   # first_sample ignored
    wrong, _ = pu.head_ref(f, w, b, scale, shift, float(pu.SLOPE), "sample0")   # every mirror with sample 0's scale / shift
    assert beyond(pu.tile_result(wrong[pu.AGG_FIRST:], mirrors, pu.AGG_PATCH, "identity", np.float64), ref, bound) > 0.9


# ------------------------------------------------------------------ finish / cnt
@pytest.mark.parametrize("n_folds", [1, 3])
def test_finish_mutations_are_seen(n_folds):
    """Pad-high used for pad-low (13 x 22 x 37 in 16 x 24 x 40: 1 | 2 on z and x); the fold divide omitted; a product with the
    rounded reciprocal instead of the divide."""
    vol_shape = (13, 22, 37)
    agg, cnt = pu.finish_case(vol_shape, 900)
    ref = pu.finish_ref(agg, cnt, vol_shape, n_folds)
    assert ref.shape == (3,) + vol_shape and ref.dtype == np.float32
    assert differs(pu.finish_ref(agg, cnt, vol_shape, n_folds, "pad_hi"), ref)
    if n_folds > 1:
        assert differs(pu.finish_ref(agg, cnt, vol_shape, 1), ref)
        assert differs(pu.finish_ref(agg, cnt, vol_shape, 1) * (np.float32(1) / np.float32(n_folds)), ref)
    big, _ = pu.finish_case((130, 129, 127), 900)
    assert big[0].size > 8192 * 256
    c, g, origin = pu.cnt_case()
    assert g.size > 8192 * 256 and all(o + p <= q for o, p, q in zip(origin, g.shape, c.shape)) and len(set(g.shape)) == 3


# ------------------------------------------------------------------ shared stage 0
@pytest.mark.parametrize("mut", ["hi_offset", "y_first"])
def test_stage0_gather_mutations_are_seen(mut):
    """The hi-shell offset z - (P - r) instead of z - (P - t) (t = 4, 8, 8 > r = 2); the y face winning over the z face."""
    wv, slabs = pu.s0_tensors(pu.S0_P, pu.S0_T, pu.S0_VE, pu.S0_C, 910)
    samples = pu.s0_samples()
    ref = pu.s0_gather_ref(wv, slabs, samples, pu.S0_P, pu.S0_T, pu.S0_R)
    wrong = pu.s0_gather_ref(wv, slabs, samples, pu.S0_P, pu.S0_T, pu.S0_R, mut)
    per_sample = [differs(wrong[i], ref[i]) for i in range(len(samples))]
    if mut == "hi_offset":
        assert per_sample == [any(sm["slab"][f] >= 0 for f in (1, 3, 5)) for sm in samples]
    else:
        assert per_sample == [any(sm["slab"][f] >= 0 for f in (0, 1)) and any(sm["slab"][f] >= 0 for f in (2, 3)) for sm in samples]
    assert any(per_sample)


def test_stage0_samples_cover_what_the_issue_lists():
    samples = pu.s0_samples()
    flags = [tuple(int(s >= 0) for s in sm["slab"]) for sm in samples]
    assert (0,) * 6 in flags and (1,) * 6 in flags and (1, 0, 0, 1, 1, 0) in flags
    for f in range(6):
        assert tuple(int(k == f) for k in range(6)) in flags
    assert {sm["wv"] for sm in samples} == {0, 1} and any(s > 0 for sm in samples for s in sm["slab"])
    for sm in samples:
        assert all(0 <= o and o + p <= v for o, p, v in zip(sm["origin"], pu.S0_P, pu.S0_VE))
    # the whole-volume source is read at the sample's origin, with the volume's strides
    wv, slabs = pu.s0_tensors(pu.S0_P, pu.S0_T, pu.S0_VE, pu.S0_C, 910)
    ref = pu.s0_gather_ref(wv, slabs, samples[:1], pu.S0_P, pu.S0_T, pu.S0_R)
    o = samples[0]["origin"]
    assert not differs(ref[0, 5, 7, 11], wv[0, o[0] + 5, o[1] + 7, o[2] + 11])
    w = pu.S0_WIDE
    assert w["P"][2] * w["C"] // 4 > 1024 and all(t >= 2 * w["r"] for t in w["t"])


def test_stage0_mask_reference():
    x = pu.rng(920).standard_normal((pu.MASK_N,) + pu.MASK_VE + (pu.MASK_C,)).astype(np.float32)
    y = pu.s0_mask_ref(x, pu.MASK_ZP)
    z, yy, xx = pu.MASK_ZP
    assert not differs(y[:, :z, :yy, :xx], x[:, :z, :yy, :xx]) and pu.MASK_VE[1] == pu.MASK_ZP[1]
    assert (y[:, z:] == 0).all() and (y[:, :, :, xx:] == 0).all() and int((y == 0).sum()) == x.size - pu.MASK_N * z * yy * xx * pu.MASK_C
    # the kept extents taken in another order zero another region
    assert differs(pu.s0_mask_ref(x, (pu.MASK_ZP[0], pu.MASK_ZP[2], pu.MASK_ZP[1])), y)
