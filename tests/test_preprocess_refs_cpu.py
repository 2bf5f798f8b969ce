"""not gpu: the references of tests/preprocess_util.py agree with scipy / numpy, and they DISCRIMINATE - for every kernel
test_gpu_preprocess.py pins, a plausible wrong kernel, restated as a variant of the numpy reference, misses that kernel's gate
on the very inputs the GPU test uses.  The coverage conditions the GPU tests rely on (how much the clip moves, which size
pairs expose fp32 coordinates, how many rounds the serpentine takes) are asserted here, and the two measured constants
(G_RESIZE, Z_MEASURED) are measured again.  (The pattern of test_plumbing_refs_cpu.py.)"""
import numpy as np
import pytest

import preprocess_util as pp


def differs(a, b):
    """A bit-equality gate is missed."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape != b.shape or a.dtype != b.dtype or bool((a.view(np.uint8) != b.view(np.uint8)).any())


# ------------------------------------------------------------------ resize_axis
@pytest.fixture(scope="module")
def resize_refs():
    """name -> (x, axis, n_out, {order: scipy zoom in float64})."""
    out = {}
    for name, shape, axis, n_out in pp.RESIZE_CASES:
        x = pp.resize_input(shape)
        out[name] = (x, axis, n_out, {order: pp.resize_zoom(x, axis, n_out, order) for order in (0, 1, 3)})
    return out


def _resize_ratio(got, ref, x, axis):
    return float((np.abs(got.astype(np.float64) - ref) / pp.line_scale(x, axis)).max())


def test_resize_cases_cover_what_they_claim():
    pairs = {(shape[axis], n_out) for _, shape, axis, n_out in pp.RESIZE_CASES}
    assert {1, 2, 3, 5} <= {a for a, b in pairs if b > a} and any(b == 1 and a > 1 for a, b in pairs)
    assert {(14, 7), (12, 8), (6, 9), (155, 240)} <= pairs
    inner1 = outer_inner = False
    for _, shape, axis, n_out in pp.RESIZE_CASES:
        outer, n, inner = pp._dims(shape, axis)
        assert (outer * n_out * inner) % 256 != 0
        inner1 |= inner == 1 and outer > 256
        outer_inner |= inner > 1 and outer > 1
    assert inner1 and outer_inner
    # the pairs that expose fp32 coordinates: in the list (of which (2, 41) is the first with n_in >= 2), n_in >= 2
    listed = pp.coord_f32_pairs()
    assert len(pp.COORD_F32_PAIRS) >= 3 and set(pp.COORD_F32_PAIRS) <= set(listed) & pairs
    assert all(a >= 2 for a, _ in pp.COORD_F32_PAIRS) and min(p for p in listed if p[0] >= 2) == (2, 41)


def test_resize_order0_references_agree_bit_for_bit(resize_refs):
    """zoom(order=0, grid_mode=True), map_coordinates on nnU-Net's coordinate expression and the restatement pick the same
    samples, exact ties (14 -> 7, 12 -> 8, 6 -> 9) included."""
    for name, (x, axis, n_out, refs) in resize_refs.items():
        want = pp.resize_mapcoord0(x, axis, n_out)
        assert not differs(refs[0].astype(np.float32), want), name
        assert not differs(pp.resize_restate(x, axis, n_out, 0), want), name


def test_resize_gate_is_the_measured_one(resize_refs):
    """G_MEASURED is the worst ratio of the unmutated restatement against scipy over the GPU test's inputs (orders 1 and 3), as
    recorded (to the four digits it is written with); the gate is twice that."""
    worst = max(_resize_ratio(pp.resize_restate(x, axis, n_out, order), refs[order], x, axis)
                for x, axis, n_out, refs in resize_refs.values() for order in (1, 3))
    print(f"resize: worst |restatement - scipy| / max|line| = {worst:.3e}, recorded {pp.G_MEASURED:.3e}, gate {pp.G_RESIZE:.3e}")
    assert abs(worst - pp.G_MEASURED) <= 0.0005e-7 and pp.G_RESIZE == 2 * pp.G_MEASURED


@pytest.mark.parametrize("mut,orders", [("pad4", (3,)), ("coord_f32", (0,)), ("no_edge_clamp", (1, 3)), ("outer_inner_swapped", (0, 1, 3))])
def test_resize_mutations_are_seen(resize_refs, mut, orders):
    """Each wrong resampler misses the gate (bit equality for order 0, G_RESIZE per line otherwise) on inputs of the GPU test -
    for every order named; fp32 coordinates change an order-0 pick at every pair of COORD_F32_PAIRS."""
    for order in orders:
        seen = []
        for name, (x, axis, n_out, refs) in resize_refs.items():
            wrong = pp.resize_restate(x, axis, n_out, order, mut)
            if (differs(wrong, refs[0].astype(np.float32)) if order == 0 else _resize_ratio(wrong, refs[order], x, axis) > pp.G_RESIZE):
                seen.append((x.shape[axis], n_out))
        assert seen, (mut, order)
        if mut == "coord_f32":
            assert set(pp.COORD_F32_PAIRS) <= set(seen)
        if mut == "pad4":   # (errs by 3e-6 to 2e-5 of the line: a gate of 2e-5 max|ref| lets most of this through)
            assert len(seen) >= 10


# ------------------------------------------------------------------ clip_to_range_of_
@pytest.fixture(scope="module")
def clip_cases():
    return pp.clip_cases()


def test_clip_reference_is_numpy_clip_and_the_clip_acts(clip_cases):
    """clip_ref is np.clip(x[g], ref[g].min(), ref[g].max()) bit for bit; in every case at least a quarter of the elements is
    moved at each end; groups per slice with 63 reference and 143 clipped elements, all-negative and zero-straddling groups with
    both zeros inside, one and 40 reference elements, one group past 1024 x 2048 elements with its extremes in the ragged tail,
    zeros of both signs at an extreme."""
    for name, (x, ref, gd) in clip_cases.items():
        g = int(np.prod(x.shape[:gd]))
        x2, r2 = x.reshape(g, -1), ref.reshape(g, -1)
        want = np.stack([np.clip(x2[i], r2[i].min(), r2[i].max()) for i in range(g)]).reshape(x.shape)
        if name in pp.CLIP_SIGN_FREE:   # (which zero numpy's min returns is not defined: values, and bits where not zero)
            got = pp.clip_ref(x, ref, gd)
            assert np.array_equal(got, want) and not differs(got[want != 0], want[want != 0]), name
        else:
            assert not differs(pp.clip_ref(x, ref, gd), want), name
        lo, hi = pp.clip_moved(x, ref, gd)
        print(f"clip {name}: {lo:.3f} moved up to the minimum, {hi:.3f} down to the maximum")
        assert lo >= 0.25 and hi >= 0.25, name
    x, ref, _ = clip_cases["slices_gd2"]
    assert (ref[0] < 0).all() and (ref[1].min((1, 2)) < 0).all() and (ref[1].max((1, 2)) > 0).all() and (ref[2] > 0).all()
    assert x.shape[2:] != ref.shape[2:]
    zeros = {0x80000000, 0}
    for z in range(ref.shape[1]):   # both zeros inside every straddling group, and in x, where they stay as they are
        assert zeros <= set(ref[1, z].view(np.uint32).ravel().tolist()) and zeros <= set(x[1, z].view(np.uint32).ravel().tolist())
    rz = clip_cases["zero_extremes"][1]
    assert rz[0].min() == 0 and rz[1].max() == 0 and all(zeros <= set(rz[g].view(np.uint32).tolist()) for g in range(2))
    assert clip_cases["one_ref_element"][1].shape[1] == 1 and clip_cases["forty_ref_elements"][1].shape[1] == 40
    xb, rb, _ = clip_cases["grid_stride"]
    assert xb.shape[0] == rb.shape[0] == 1 and min(xb.size, rb.size) > 1024 * 2048
    assert rb.argmin() >= rb.size - 256 and rb.argmax() >= rb.size - 1024 and rb.argmax() % 256 != rb.argmin() % 256


@pytest.mark.parametrize("mut,case", [("no_sign", "slices_gd2"), ("no_sign", "slices_gd1"), ("no_sign", "forty_ref_elements"),
                                      ("no_sign", "grid_stride"), ("no_sign", "zero_extremes"), ("per_channel", "slices_gd2"),
                                      ("n_per_group", "slices_gd2"), ("n_per_group", "forty_ref_elements"),
                                      ("n_per_group", "one_ref_element")])
def test_clip_mutations_are_seen(clip_cases, mut, case):
    x, ref, gd = clip_cases[case]
    assert not np.array_equal(pp.clip_ref(x, ref, gd, mut), pp.clip_ref(x, ref, gd))   # (values: more than a zero's sign)


# ------------------------------------------------------------------ threshold_ge, mask_to_float, prob_mean, label_ensemble
@pytest.mark.parametrize("n", [1, 4099, pp.N_BIG])
def test_elementwise_mutations_are_seen(n):
    """>, a mask byte compared with 1 or cast, a / 2 + b / 2, halves rounded up: each differs from the reference on the GPU
    test's inputs (n = 1 holds one special value and cannot tell all of them apart: only the larger sizes are asked to)."""
    big = n > 1
    for thr in pp.THRESHOLDS:
        x = pp.threshold_input(thr, n)
        assert x[0] == np.float32(thr)
        assert differs(pp.threshold_ref(x, thr, "gt"), pp.threshold_ref(x, thr))
    m = pp.mask_input(n)
    a, b = pp.prob_mean_input(n)
    la, lb = pp.label_pair_input(n)
    if big:
        assert set(np.unique(m)) == {0, 1, 2, 255}
        assert differs(pp.mask_to_float_ref(m, "eq1"), pp.mask_to_float_ref(m))
        assert differs(pp.mask_to_float_ref(m, "cast"), pp.mask_to_float_ref(m))
        ref = pp.prob_mean_ref(a, b)
        assert differs(pp.prob_mean_ref(a, b, "half_each"), ref)
        assert np.isinf(ref).any() and (np.abs(ref[ref != 0]) < 1.1754944e-38).any()     # overflow to inf, denormal results
        assert (ref.astype(np.float64) != (a.astype(np.float64) + b.astype(np.float64)) / 2).any()   # inexact sums
        assert differs(pp.label_ensemble_ref(la, lb, "half_up"), pp.label_ensemble_ref(la, lb))
    if n >= 65536:    # the full table, and something after the last full trip of the capped grid
        assert len(set(zip(la[:65536].tolist(), lb[:65536].tolist()))) == 65536
        tail = slice(n - 257, n)
        assert pp.threshold_ref(pp.threshold_input(0.5, n), 0.5)[tail].any() and pp.mask_to_float_ref(m)[tail].any()
        assert n > 8192 * 256 and n % 256 != 0


def test_label_ensemble_reference_is_the_drivers_expression():
    a, b = pp.label_pair_input(65536)
    assert not differs(pp.label_ensemble_ref(a, b), np.round((a.astype(np.int64) + b) / 2.0).astype(np.uint8))


# ------------------------------------------------------------------ zscore_masked_
@pytest.fixture(scope="module")
def zscore_cases():
    return pp.zscore_cases()


def test_zscore_cases_and_reference(zscore_cases):
    """The reference is the float64 definition (numpy's own mean / std in float64 agree with it); C = 2 past 2048 x 256
    voxels, C = 3 with 64 to 128 blocks, mask bytes 0, 1, 2, 255; one-voxel, empty and constant cases expect exact zeros; the
    fp32 numpy expression gives 0.75 on the constant region and is therefore not the reference."""
    vol, mask = zscore_cases["mid"]
    ref, _ = pp.zscore_ref(vol, mask)
    m = mask != 0
    for c in range(vol.shape[0]):
        v = vol[c].astype(np.float64)
        want = np.where(m, (v - v[m].mean()) / (v[m].std() + 1e-8), 0.0)
        assert np.abs(ref[c] - want).max() <= 1e-12 * (abs(v[m].mean()) / v[m].std() + 4)
    assert 64 < -(-vol[0].size // 256) < 128 and vol.shape[0] == 3
    big, bmask = zscore_cases["big"]
    assert big.shape[0] == 2 and big[0].size > 2048 * 256
    for vol_, mask_ in (zscore_cases["big"], zscore_cases["mid"], zscore_cases["constant"]):
        assert set(np.unique(mask_)) == {0, 1, 2, 255}
    for name in ("one_voxel", "empty", "constant"):
        vol, mask = zscore_cases[name]
        ref, _ = pp.zscore_ref(vol, mask)
        assert (ref == 0).all() and not differs(pp.zscore_restate32(vol, mask), np.zeros(vol.shape, np.float32)), name
    assert int((zscore_cases["one_voxel"][1] != 0).sum()) == 1 and not zscore_cases["empty"][1].any()
    vol, mask = zscore_cases["constant"]
    assert int((mask != 0).sum()) == pp.Z_CONST_VOXELS and (vol[:, mask != 0] == pp.CONST_03).all()
    assert abs(np.abs(pp.zscore_numpy32(vol, mask)).max() - 0.75) < 0.01


def test_zscore_bound_is_the_measured_one(zscore_cases):
    """The kernel's fp32 steps (restated on float64 statistics) reach Z_MEASURED of the derived bound on the test's inputs; the
    gate applies the margin Z_MARGIN = 2 on top."""
    worst = 0.0
    for name in ("big", "mid"):
        vol, mask = zscore_cases[name]
        ref, bound = pp.zscore_ref(vol, mask)
        m = bound > 0
        worst = max(worst, float((np.abs(pp.zscore_restate32(vol, mask) - ref)[m] / bound[m]).max()))
    print(f"zscore: fp32 restatement reaches {worst:.3f} of the bound without its margin, recorded {pp.Z_MEASURED}")
    assert 0.97 * pp.Z_MEASURED <= worst <= pp.Z_MEASURED and pp.Z_MARGIN == 2.0


@pytest.mark.parametrize("mut,case", [("ddof1", "mid"), ("first64", "mid"), ("first64", "big"), ("eq1", "mid"), ("eq1", "big"),
                                      ("no_clamp", "constant")])
def test_zscore_mutations_are_seen(zscore_cases, mut, case):
    """n - 1 in the variance (2.5e-5 of the result at 16 000 masked voxels), only the first 64 block partials added, the mask
    tested as == 1: beyond the gate.  Without the clamp the one-pass variance of the constant region is negative in the
    restatement (-1.4e-17) and the result is NaN where exact zeros are expected."""
    vol, mask = zscore_cases[case]
    ref, bound = pp.zscore_ref(vol, mask)
    wrong, _ = pp.zscore_ref(vol, mask, mut)
    if case == "constant":
        assert np.isnan(pp.zscore_stats(vol, mask, mut)[1][0][1])   # the root of a negative variance
        assert not np.isfinite(wrong[:, mask != 0]).any()
    else:
        with np.errstate(invalid="ignore"):
            assert (~(np.abs(wrong - ref) <= pp.Z_MARGIN * bound)).mean() > 0.05


# ------------------------------------------------------------------ crop_mask
@pytest.fixture(scope="module")
def crop_cases():
    return pp.crop_cases()


def test_crop_restatement_matches_the_oracle_and_cases_are_what_they_claim(crop_cases):
    rounds = {}
    for name, vol in crop_cases.items():
        assert vol.dtype == np.float32 and vol[0].size < 40000
        mask, bbox = pp.crop_expected(vol)
        got_mask, got_bbox, rounds[name] = pp.crop_restate(vol)
        assert not differs(got_mask, mask) and got_bbox == bbox, name
    print(f"crop: rounds of sweeps that changed something: {rounds}")
    assert rounds["serpentine_open"] > 2 and rounds["serpentine_open"] >= pp.SERPENTINE_TURNS
    open_mask = pp.crop_expected(crop_cases["serpentine_open"])[0]
    closed_mask = pp.crop_expected(crop_cases["serpentine_closed"])[0]
    corridor = (crop_cases["serpentine_closed"][0] == 0) & (closed_mask == 1)       # enclosed background: the closed copy fills it
    assert int(corridor.sum()) >= 13 * pp.SERPENTINE_TURNS and not open_mask[corridor].any()
    vol = crop_cases["channels"]
    want = pp.crop_expected(vol)[0]      # no channel alone gives the mask: the cavity is closed only by the OR
    assert vol.shape[0] == 4 and all(differs(pp.crop_restate(vol[c:c + 1])[0], want) for c in range(4))
    assert {"1x9x11", "7x1x1", "5x6x1"} <= set(crop_cases)
    corner = crop_cases["corner_voxel"]
    assert int((corner != 0).sum()) == 1 and pp.crop_expected(corner)[1] == [[3, 4], [4, 5], [5, 6]]
    nz = crop_cases["negative_zero"]
    assert np.signbit(nz[nz == 0]).sum() > 100 and pp.crop_expected(nz)[1] == [[2, 7], [2, 8], [3, 9]]


@pytest.mark.parametrize("mut,case", [("channel0", "channels"), ("channel0", "1x9x11"), ("one_round", "serpentine_open")])
def test_crop_mutations_are_seen(crop_cases, mut, case):
    mask, bbox = pp.crop_expected(crop_cases[case])
    got_mask, got_bbox, _ = pp.crop_restate(crop_cases[case], mut)
    assert differs(got_mask, mask)


# ------------------------------------------------------------------ regions_to_labels
def _r2l_inputs():
    """name -> (probs, order, lo, full) of every GPU case, the grid-stride one left out (same reference, 2 M voxels)."""
    return {name: (pp.r2l_probs(c, shape, pp.R2L_SEED + c), order, lo, full) for name, c, order, shape, lo, full in pp.R2L_CASES}


def test_regions_to_labels_reference_and_cases():
    """The restatement is the oracle's regions_to_labels + paste and numpy's argmax; the GPU cases hold 8 channels with values at
    0.5 and one float above it, exact ties between channels in the argmax case, a box flush with the far corner and one equal to
    the full shape; the large case is past the capped grid."""
    from oracle import tiler_ref
    cases = _r2l_inputs()
    p, order, lo, full = cases["regions_c3_inside"]
    box = [[o, o + n] for o, n in zip(lo, p.shape[1:])]
    assert not differs(pp.r2l_ref(p, order), tiler_ref.regions_to_labels(p).astype(np.uint8))
    pasted = tiler_ref.paste_into_original(tiler_ref.regions_to_labels(p), box, full)
    assert not differs(pp.r2l_ref(p, order, lo, full), pasted.astype(np.uint8))
    p8, order8, lo8, full8 = cases["regions_c8_far_corner"]
    assert p8.shape[0] == 8 and (p8 == np.float32(0.5)).any() and (p8 == pp.HALF_UP).any()
    assert len(set(order8)) < 8 and 0 in order8 and tuple(o + n for o, n in zip(lo8, p8.shape[1:])) == full8
    assert cases["regions_c8_full"][3] is None and cases["argmax_c1"][0].shape[0] == 1 and cases["argmax_c1"][1] is None
    p4, order4, _, _ = cases["argmax_c4_ties"]
    assert order4 is None and ((p4 == p4.max(0)[None]).sum(0) > 1).mean() > 0.2     # exact ties between channels
    assert not differs(pp.r2l_ref(p4, None), p4.argmax(0).astype(np.uint8))
    assert int(np.prod(pp.R2L_BIG["shape"])) > 8192 * 256


@pytest.mark.parametrize("mut", ["ge", "argmax_last", "lo_yx"])
def test_regions_to_labels_mutations_are_seen(mut):
    """>= 0.5, the last maximum, the y and x offsets exchanged: each is seen on at least one case of the GPU test (lo_yx is tried
    where the exchanged box still fits the volume)."""
    seen = []
    for name, (p, order, lo, full) in _r2l_inputs().items():
        if mut == "lo_yx" and (full is None or lo[2] + p.shape[2] > full[1] or lo[1] + p.shape[3] > full[2]):
            continue
        if differs(pp.r2l_ref(p, order, lo, full, mut), pp.r2l_ref(p, order, lo, full)):
            seen.append(name)
    print(f"regions_to_labels {mut}: seen on {seen}")
    assert seen
    if mut == "ge":
        assert {"regions_c8_far_corner", "regions_c8_full", "regions_c3_inside"} <= set(seen)
    if mut == "argmax_last":
        assert "argmax_c4_ties" in seen
