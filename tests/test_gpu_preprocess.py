"""-m gpu: the kernels around the network - masked z-score, separable resampler and its range clip, crop mask, region-to-label
paste, threshold / mask / mean / ensemble - one entry point each through amd.ops, against the numpy references of
tests/preprocess_util.py (whose power test_preprocess_refs_cpu.py proves on these very inputs).

Every gate is named in the test's docstring: BIT EQUALITY with numpy / scipy; the DERIVED z-score bound (fp32 roundings of the
mean, the difference and the quotient, margin 2); or the MEASURED resampler gate preprocess_util.G_RESIZE (twice what a
float64 restatement with fp32 coefficient stores shows against scipy on the CPU).  Refusal tests pass only arguments the entry
point rejects before it launches anything."""
import numpy as np
import pytest
import torch

import preprocess_util as pp

pytestmark = pytest.mark.gpu


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = (got.view(np.uint8) == want.view(np.uint8)).reshape(got.size, -1).all(1)
    assert same.all(), f"{what}: {int((~same).sum())} of {got.size} elements differ, first at flat index {int(np.argmin(same))}"


# ------------------------------------------------------------------ resize_axis
@pytest.fixture(scope="module")
def resize_refs():
    """name -> (x, axis, n_out, {order: scipy zoom in float64}), computed once."""
    out = {}
    for name, shape, axis, n_out in pp.RESIZE_CASES:
        x = pp.resize_input(shape)
        out[name] = (x, axis, n_out, {order: pp.resize_zoom(x, axis, n_out, order) for order in (0, 1, 3)})
    return out


def check_resize(got, x, axis, n_out, order, ref, what):
    if order == 0:
        assert_bits(got, ref.astype(np.float32), f"{what} against zoom")
        assert_bits(got, pp.resize_mapcoord0(x, axis, n_out), f"{what} against map_coordinates")
        return
    ratio = np.abs(got.astype(np.float64) - ref) / pp.line_scale(x, axis)
    print(f"{what}: worst |got - ref64| / max|line| = {float(ratio.max()):.3e} (gate {pp.G_RESIZE:.3e})")
    assert got.shape == ref.shape and np.isfinite(got).all() and (ratio <= pp.G_RESIZE).all(), f"{what}: worst {float(ratio.max()):.3e}"


@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("name", [c[0] for c in pp.RESIZE_CASES])
def test_resize_axis(amd, gpu, resize_refs, name, order):
    """Order 0 BIT EQUAL to scipy zoom(order=0, mode='nearest', grid_mode=True) and to map_coordinates at scale (k + 0.5) - 0.5;
    orders 1 and 3 MEASURED: per line |got - zoom in float64| <= G_RESIZE max|input line|.  n_in 1, 2, 3, 5 up-sampled,
    n_out = 1, the exact-tie ratios 14 -> 7, 12 -> 8, 6 -> 9, four pairs at which an fp32 coordinate picks another sample,
    155 -> 240; the axis last (inner == 1, 273 lines), in the middle (outer 3, inner 35) and first (outer 1)."""
    x, axis, n_out, refs = resize_refs[name]
    got = amd.ops.resize_axis(dev(x, gpu), axis, n_out, order).cpu().numpy()
    check_resize(got, x, axis, n_out, order, refs[order], f"resize_axis {name} order {order}")


def test_resize_axis_scratch_reuse(amd, gpu, resize_refs):
    """The order-3 coefficient scratch is shared between calls: the smallest tensor, the largest, the smallest again - all within
    the gate, and the small result after the large call BIT EQUAL to the one before it."""
    xs, axs, ns, rs = resize_refs[pp.RESIZE_SMALLEST]
    xl, axl, nl, rl = resize_refs[pp.RESIZE_LARGEST]
    before = amd.ops.resize_axis(dev(xs, gpu), axs, ns, 3).cpu().numpy()
    large = amd.ops.resize_axis(dev(xl, gpu), axl, nl, 3).cpu().numpy()
    after = amd.ops.resize_axis(dev(xs, gpu), axs, ns, 3).cpu().numpy()
    check_resize(large, xl, axl, nl, 3, rl[3], "resize_axis largest")
    check_resize(after, xs, axs, ns, 3, rs[3], "resize_axis smallest after the largest")
    assert_bits(after, before, "resize_axis smallest, after against before the large call")


def test_resize_axis_refusals(amd, gpu):
    x = torch.zeros((2, 3, 4, 5), device=gpu)
    with pytest.raises(amd._lib.Mi355Error, match="interpolation order 2"):
        amd.ops.resize_axis(x, 2, 7, 2)
    with pytest.raises(amd._lib.Mi355Error, match="resize_axis: bad argument"):
        amd.ops.resize_axis(x, 2, 0, 1)


# ------------------------------------------------------------------ clip_to_range_of_
@pytest.fixture(scope="module")
def clip_cases():
    return pp.clip_cases()


@pytest.mark.parametrize("name", ["slices_gd2", "slices_gd1", "one_ref_element", "forty_ref_elements", "grid_stride", "zero_extremes"])
def test_clip_to_range_of(amd, gpu, clip_cases, name):
    """BIT EQUALITY with np.clip(x[g], ref[g].min(), ref[g].max()) per group: groups per slice (group_dims 2, 63 reference and 143
    clipped elements each) and per channel (1); all-negative groups, groups that straddle zero and hold both zeros, one reference
    element, 40 of them, and one group of 2 098 683 elements whose extremes sit in the ragged tail.  A third of x lies beyond
    each end.  zero_extremes: -0.0 and +0.0 are the minimum of one group and the maximum of the other; which of the two zeros
    numpy's min returns is not defined, so that case is compared by value, and bit for bit where the result is not a zero."""
    x, ref, gd = clip_cases[name]
    ref_d = dev(ref, gpu)
    got = amd.ops.clip_to_range_of_(dev(x, gpu), ref_d, gd).cpu().numpy()
    want = pp.clip_ref(x, ref, gd)
    if name in pp.CLIP_SIGN_FREE:
        assert np.array_equal(got, want) and (want == 0).mean() > 0.25
        got, want = got[want != 0], want[want != 0]
    assert_bits(got, want, f"clip_to_range_of_ {name}")
    assert_bits(ref_d.cpu().numpy(), ref, "the reference tensor is left alone")


# ------------------------------------------------------------------ threshold_ge, mask_to_float, prob_mean, label_ensemble
SIZES = [1, 4099, pp.N_BIG]   # N_BIG = 8192 x 256 + 257: the capped grid strides, the last trip is ragged


@pytest.mark.parametrize("n", SIZES)
def test_threshold_ge(amd, gpu, n):
    """BIT EQUALITY with x >= np.float32(thr): x at thr, one float below and above, both zeros, infinities, NaN; thr 0, 0.5, 0.3."""
    for thr in pp.THRESHOLDS:
        x = pp.threshold_input(thr, n)
        assert_bits(amd.ops.threshold_ge(dev(x, gpu), thr).cpu().numpy(), pp.threshold_ref(x, thr), f"threshold_ge {thr} n {n}")


@pytest.mark.parametrize("n", SIZES)
def test_mask_to_float(amd, gpu, n):
    """BIT EQUALITY with (mask != 0) as fp32: bytes 0, 1, 2, 255."""
    m = pp.mask_input(n)
    assert_bits(amd.ops.mask_to_float(dev(m, gpu)).cpu().numpy(), pp.mask_to_float_ref(m), f"mask_to_float n {n}")


@pytest.mark.parametrize("n", SIZES)
def test_prob_mean(amd, gpu, n):
    """BIT EQUALITY with (a + b) / np.float32(2) in fp32: inexact sums, denormals (their halves are ties), sums that overflow to
    inf - whatever numpy's fp32 gives."""
    a, b = pp.prob_mean_input(n)
    assert_bits(amd.ops.prob_mean(dev(a, gpu), dev(b, gpu)).cpu().numpy(), pp.prob_mean_ref(a, b), f"prob_mean n {n}")


@pytest.mark.parametrize("n", SIZES)
def test_label_ensemble(amd, gpu, n):
    """BIT EQUALITY with uint8(np.round((a + b) / 2.0)): the full 256 x 256 table (n >= 65536), random bytes after it."""
    a, b = pp.label_pair_input(n)
    assert_bits(amd.ops.label_ensemble(dev(a, gpu), dev(b, gpu)).cpu().numpy(), pp.label_ensemble_ref(a, b), f"label_ensemble n {n}")


def test_elementwise_refusals(amd, gpu):
    """No elements (and with that null pointers): refused before any launch."""
    f, u = torch.empty(0, device=gpu), torch.empty(0, dtype=torch.uint8, device=gpu)
    with pytest.raises(amd._lib.Mi355Error, match="threshold_ge: bad argument"):
        amd.ops.threshold_ge(f, 0.5)
    with pytest.raises(amd._lib.Mi355Error, match="mask_to_float: bad argument"):
        amd.ops.mask_to_float(u)
    with pytest.raises(amd._lib.Mi355Error, match="prob_mean: bad argument"):
        amd.ops.prob_mean(f, f)
    with pytest.raises(amd._lib.Mi355Error, match="label_ensemble: bad argument"):
        amd.ops.label_ensemble(u, u)


# ------------------------------------------------------------------ zscore_masked_
@pytest.fixture(scope="module")
def zscore_cases():
    return pp.zscore_cases()


@pytest.mark.parametrize("name", ["big", "mid"])
def test_zscore_masked(amd, gpu, zscore_cases, name):
    """DERIVED: per element |got - ref64| <= 2 x 2^-24 (|mean| / std + 2 |ref64| + 1), ref64 = (x - mean) / (std + 1e-8) in float64
    over the mask; exactly 0 outside the mask (the bound is 0 there); two calls BIT EQUAL.  (mean, sd) = (1000, 300), (1e4, 1),
    (-5e3, 20); mask bytes 0, 1, 2, 255.  big: C = 2, 65 x 90 x 90 = 526 500 voxels > 2048 x 256 - the grid strides and the
    finish adds 2048 partials; mid: C = 3, 20 011 voxels, 79 blocks - the lane-strided finish makes a second, ragged trip."""
    vol, mask = zscore_cases[name]
    ref, bound = pp.zscore_ref(vol, mask)
    mask_d = dev(mask, gpu)
    got = amd.ops.zscore_masked_(dev(vol, gpu), mask_d).cpu().numpy()
    again = amd.ops.zscore_masked_(dev(vol, gpu), mask_d).cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref)
    inside = bound > 0
    gate = pp.Z_MARGIN * bound
    print(f"zscore_masked_ {name}: max err {float(err.max()):.3e}, {float((err[inside] / gate[inside]).max()):.3f} of its bound")
    assert np.isfinite(got).all() and (err <= gate).all(), f"{int((err > gate).sum())} elements beyond the bound"
    assert (got[:, mask == 0] == 0).all()
    assert_bits(again, got, "zscore_masked_ twice")


@pytest.mark.parametrize("name", ["one_voxel", "empty", "constant"])
def test_zscore_masked_degenerate(amd, gpu, zscore_cases, name):
    """BIT EQUALITY with zeros: a one-voxel mask (x - mean is 0 over 1e-8), an empty mask (nothing non-finite) and a region
    constant at 0.3f (986 voxels).  On that last one the fp32 numpy expression - mean and std in fp32 - returns 0.75, the rounding
    of the fp32 mean over 1e-8: it is not the reference; the float64 definition gives 0, and so must the kernel, whether or not
    its one-pass variance comes out below zero."""
    vol, mask = zscore_cases[name]
    got = amd.ops.zscore_masked_(dev(vol, gpu), dev(mask, gpu)).cpu().numpy()
    assert_bits(got, np.zeros(vol.shape, np.float32), f"zscore_masked_ {name}")


def test_zscore_masked_refusals(amd, gpu):
    with pytest.raises(amd._lib.Mi355Error, match="zscore: bad argument"):
        amd.ops.zscore_masked_(torch.empty((2, 0), device=gpu), torch.empty(0, dtype=torch.uint8, device=gpu))
    with pytest.raises(amd._lib.Mi355Error, match="zscore: 65 channels"):
        amd.ops.zscore_masked_(torch.zeros((65, 4), device=gpu), torch.ones(4, dtype=torch.uint8, device=gpu))


# ------------------------------------------------------------------ crop_mask
@pytest.fixture(scope="module")
def crop_cases():
    return pp.crop_cases()


@pytest.mark.parametrize("name", ["serpentine_open", "serpentine_closed", "channels", "1x9x11", "7x1x1", "5x6x1", "corner_voxel",
                                  "negative_zero"])
def test_crop_mask(amd, gpu, crop_cases, name):
    """BIT EQUALITY with oracle/tiler_ref.crop_to_nonzero (scipy's binary_fill_holes): the mask inside the box, the box, nothing
    outside.  A background corridor with 13 turns, open to the border (14 rounds of sweeps, stays unfilled) and closed (fills);
    C = 4 with every wall of a hollow box in another channel; extents of 1; a single voxel in the far corner; -0.0 background."""
    vol = crop_cases[name]
    want_mask, want_box = pp.crop_expected(vol)
    mask, box = amd.ops.crop_mask(dev(vol, gpu))
    assert box == want_box
    assert_bits(mask.cpu().numpy(), want_mask, f"crop_mask {name}")


def test_crop_mask_refuses_an_all_zero_volume(amd, gpu):
    """Zeros of both signs: after the (legitimate) sweeps the entry point finds no voxel and says so."""
    vol = torch.zeros((2, 4, 5, 6), device=gpu)
    vol[1, 2] = -0.0
    with pytest.raises(amd._lib.Mi355Error, match="all zeros"):
        amd.ops.crop_mask(vol)


# ------------------------------------------------------------------ regions_to_labels
@pytest.mark.parametrize("name,c,order,shape,lo,full", pp.R2L_CASES)
def test_regions_to_labels(amd, gpu, name, c, order, shape, lo, full):
    """BIT EQUALITY with the numpy restatement: 8 channels and an order with repeats and zeros, values at 0.5 (not above) and one
    float above it; order=None - argmax, the first maximum wins - with exact ties and with one channel; the box flush with the
    far corner, equal to the full shape, and inside."""
    probs = pp.r2l_probs(c, shape, pp.R2L_SEED + c)
    got = amd.ops.regions_to_labels(dev(probs, gpu), order, lo, full).cpu().numpy()
    assert_bits(got, pp.r2l_ref(probs, order, lo, full), f"regions_to_labels {name}")


def test_regions_to_labels_grid_stride(amd, gpu):
    """BIT EQUALITY.  C = 3, 129 x 128 x 128 = 2 113 536 voxels > 8192 x 256, pasted at (1, 2, 3) into 131 x 131 x 133; the
    surround is zero."""
    b = pp.R2L_BIG
    probs = pp.r2l_probs(3, b["shape"], 90)
    got = amd.ops.regions_to_labels(dev(probs, gpu), (1, 2, 3), b["lo"], b["full"]).cpu().numpy()
    want = pp.r2l_ref(probs, (1, 2, 3), b["lo"], b["full"])
    assert_bits(got, want, "regions_to_labels grid stride")
    outside = np.ones(b["full"], bool)
    outside[tuple(slice(o, o + s) for o, s in zip(b["lo"], b["shape"]))] = False
    assert (got[outside] == 0).all() and (got[~outside] != 0).mean() > 0.5


def test_regions_to_labels_refusals(amd, gpu):
    """Nine channels; a box that hangs over the full volume by one voxel, on each axis in turn (checked before the launch)."""
    with pytest.raises(amd._lib.Mi355Error, match="9 channels"):
        amd.ops.regions_to_labels(torch.zeros((9, 2, 3, 4), device=gpu), None)
    probs = torch.zeros((3, 5, 6, 7), device=gpu)
    for axis in range(3):
        lo = [3, 3, 4]
        lo[axis] += 1
        with pytest.raises(amd._lib.Mi355Error, match="does not fit"):
            amd.ops.regions_to_labels(probs, (1, 2, 3), lo, (8, 9, 11))
