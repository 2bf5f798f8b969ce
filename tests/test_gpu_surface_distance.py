"""Surface distances on the MI355X (csrc/surface_distance.hip, brats_amd.evaluate.surface_*): the surfaces of up to
four regions of two label maps bit-equal to scipy's mask & ~binary_erosion(mask), the fp64 distance map and everything derived from
it within 1e-12 relative of scipy.ndimage.distance_transform_edt(~surface, sampling=spacing), the ordered gather, counts and
surface sizes exact, and the command.  Every test prints the largest relative difference it saw and whether the device result
was bit-equal to scipy's, so one run with -s is the record.  On the MI355X the device result was in fact bit-equal to scipy's in
every case of this file - all distance maps (the three spacings, the boxes, the tile limit), all end-to-end distance arrays and the
240 x 240 x 155 pair: the largest relative difference printed was 0.  The 1e-12 gate stays as the bound that is reasoned for.
The child processes this file starts run under a time limit of their own; nothing is retried."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

import components_util as cu
import surface_distance_util as su
from test_gpu_components import VOLUMES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LINE = 512      # MI355_SURFACE_EDT_MAX_LINE
CHUNK = 2048        # MI355_GATHER_CHUNK
U8P, I32P, F64P, I64P = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
FLOATS = ("hd", "hd95", "assd", "surface_dice")
INTEGERS = ("within_tolerance_pred", "within_tolerance_gt", "surface_voxels_pred", "surface_voxels_gt")


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _stream(gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


def _box(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.int32), np.asarray(hi, dtype=np.int32)
    return lo, hi, lo.ctypes.data_as(I32P), hi.ctypes.data_as(I32P)


def _err(lib):
    return lib.mi355_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- surfaces
def region_surfaces(amd, gpu, pred, gt, table_pred, table_gt, fill=0xA5):
    lib = amd._lib.load()
    flags = torch.full(pred.shape, fill, dtype=torch.uint8, device=gpu)
    dp, dg = _dev(pred, gpu), _dev(gt, gpu)   # (held until the call has finished)
    rc = lib.mi355_region_surfaces(dp.data_ptr(), dg.data_ptr(), *pred.shape, table_pred.ctypes.data_as(U8P),
                                   table_gt.ctypes.data_as(U8P), flags.data_ptr(), flags.numel(), _stream(gpu))
    torch.cuda.synchronize()
    assert rc == 0, _err(lib)
    return flags.cpu().numpy()


def smooth_labels(seed, shape, stray=0.05):
    """labels 0..3 in smooth blobs (interiors and surfaces), plus a sprinkle of values 4, 5, 7, 200 and 255 that belong to no region"""
    rs = np.random.RandomState(seed)
    field = ndimage.gaussian_filter(rs.standard_normal(shape), 1.2, mode="nearest")
    seg = np.digitize(field, np.quantile(field, (0.4, 0.6, 0.8))).astype(np.uint8) if field.size > 1 else np.full(shape, 3, np.uint8)
    other = rs.random_sample(shape) < stray
    seg[other] = rs.choice(np.array([4, 5, 7, 200, 255], dtype=np.uint8), int(other.sum()))
    return seg


SURFACE_SHAPES = [(1, 1, 1), (1, 1, 301), (301, 1, 1), (5, 9, 70), (13, 3, 65), (7, 17, 130)]
REGION_SETS = [(1, 2, 3), (1, 3), (3,), (2,)]


@pytest.mark.parametrize("shape", SURFACE_SHAPES)
def test_surfaces_equal_scipy(amd, gpu, shape):
    pred, gt = smooth_labels(31, shape), smooth_labels(32, shape)
    got = region_surfaces(amd, gpu, pred, gt, su.table(REGION_SETS), su.table(REGION_SETS))
    want = su.surface_flags(pred, gt, REGION_SETS)
    assert got.dtype == np.uint8 and got.shape == pred.shape
    assert np.array_equal(got, want), (shape, int((got != want).sum()))
    if pred.size > 1:
        assert (pred >= 4).any() and not got[(pred >= 4) & (gt >= 4)].any(), "a label of no region is on a surface"


def test_surfaces_of_full_empty_and_one_sided_maps(amd, gpu):
    shape = (9, 20, 100)
    ones, zeros = np.ones(shape, np.uint8), np.zeros(shape, np.uint8)
    t = su.table([(1,)])
    got = region_surfaces(amd, gpu, ones, zeros, t, t)
    shell = np.ones(shape, bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(got, shell.astype(np.uint8)), "an all-foreground map: exactly the boundary shell, in the prediction's bit only"
    assert np.array_equal(region_surfaces(amd, gpu, zeros, ones, t, t), shell.astype(np.uint8) << 4)
    assert not region_surfaces(amd, gpu, zeros, zeros, t, t).any()
    # a region listed in one table only: bit 1 = label 2 in the prediction's table, nothing in the ground truth's
    pred, gt = smooth_labels(33, (7, 17, 130)), smooth_labels(34, (7, 17, 130))
    got = region_surfaces(amd, gpu, pred, gt, su.table([(1, 3), (2,)]), su.table([(1, 3)]))
    assert np.array_equal(got, su.surface_flags(pred, gt, [(1, 3), (2,)], [(1, 3)])) and not (got & 0x20).any() and (got & 0x02).any()
    # labels >= 4 only: nothing leaks into any of the four regions
    stray = np.random.RandomState(35).choice(np.array([4, 6, 9, 128, 255], dtype=np.uint8), (5, 9, 70))
    assert not region_surfaces(amd, gpu, stray, stray, su.table(REGION_SETS), su.table(REGION_SETS)).any()


def test_surfaces_refuse_bad_calls(amd, gpu):
    lib = amd._lib.load()
    a = torch.zeros((3, 4, 5), dtype=torch.uint8, device=gpu)
    flags = torch.full((3, 4, 5), 7, dtype=torch.uint8, device=gpu)
    good, bad = su.table([(1,)]), su.table([(1,)])
    bad[9] = 16
    for table, nbytes, match in ((bad, 60, "beyond the four"), (good, 59, "needs 60")):
        rc = lib.mi355_region_surfaces(a.data_ptr(), a.data_ptr(), 3, 4, 5, table.ctypes.data_as(U8P), good.ctypes.data_as(U8P), flags.data_ptr(), nbytes, _stream(gpu))
        torch.cuda.synchronize()
        assert rc == -1 and match in _err(lib)
    assert bool((flags == 7).all()), "a refused call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------- distance map
def edt_to_flagged(amd, gpu, flags, lo, hi, select, spacing):
    """-> (rc, box-shaped numpy array of squared distances, or None when refused)"""
    lib = amd._lib.load()
    lo, hi, plo, phi = _box(lo, hi)
    n = int(np.prod((hi - lo).astype(np.int64)))
    dist2 = torch.full((max(n, 1),), -7.0, dtype=torch.float64, device=gpu)
    count = torch.full((2,), -1, dtype=torch.int32, device=gpu)
    sp = np.asarray(spacing, dtype=np.float64)
    dflags = _dev(flags, gpu)
    rc = lib.mi355_edt_to_flagged_f64(dflags.data_ptr(), *flags.shape, plo, phi, select, sp.ctypes.data_as(F64P), dist2.data_ptr(), n,
                                      count.data_ptr(), _stream(gpu))
    torch.cuda.synchronize()
    if rc != 0:
        assert bool((dist2 == -7.0).all()), "a refused call wrote to its output"
        return rc, None
    return rc, dist2.cpu().numpy()[:n].reshape(tuple(int(v) for v in hi - lo))


def check_distance_map(amd, gpu, sites, spacing, lo=None, hi=None, what=""):
    """sites: bool volume.  The flag byte carries the sites in bit 5 and clutter in the other bits, which select = 0x20 must ignore."""
    lo = (0, 0, 0) if lo is None else lo
    hi = sites.shape if hi is None else hi
    clutter = np.random.RandomState(5).randint(0, 256, sites.shape).astype(np.uint8) & 0xDF
    flags = (clutter | (sites.astype(np.uint8) << 5)).astype(np.uint8)
    rc, got2 = edt_to_flagged(amd, gpu, flags, lo, hi, 0x20, spacing)
    assert rc == 0, _err(amd._lib.load())
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    want = su.distance_to(sites[box], spacing)
    got = np.sqrt(got2)
    worst, ok = su.close(got, want)
    print(f"distance map {what} spacing {spacing}: worst relative difference {worst:.3g}, bit-equal to scipy: {np.array_equal(got, want)}")
    assert ok, (what, spacing, worst)
    assert np.array_equal(got2 == 0, sites[box]), "zero exactly at the sites"


@pytest.mark.parametrize("spacing", su.SPACINGS)
@pytest.mark.parametrize("name", ["ragged_small", "serpentine", "checkerboard", "line_last_axis", "line_first_axis"])
def test_distance_map_equals_scipy(amd, gpu, name, spacing):
    check_distance_map(amd, gpu, VOLUMES[name]() != 0, spacing, what=name)


@pytest.mark.parametrize("spacing", su.SPACINGS)
def test_distance_map_of_single_sites_and_sparse_noise(amd, gpu, spacing):
    for corner in ((0, 0, 0), (5, 6, 69), (0, 6, 0)):
        sites = np.zeros((6, 7, 70), bool)
        sites[corner] = True
        check_distance_map(amd, gpu, sites, spacing, what=f"one site at {corner}")
    check_distance_map(amd, gpu, cu.noise(61, (40, 70, 33), 0.002) != 0, spacing, what="sparse noise (columns and lines without a site)")


@pytest.mark.parametrize("shape", [(2, MAX_LINE, 3), (2, 3, MAX_LINE), (600, 2, 3)])
def test_distance_map_at_the_tile_limit(amd, gpu, shape):
    check_distance_map(amd, gpu, cu.noise(62, shape, 0.01) != 0, (0.9375, 1.5, 3.3), what=f"limit {shape}")


@pytest.mark.parametrize("shape", [(1, MAX_LINE + 1, 1), (1, 2, MAX_LINE + 1)])
def test_distance_map_refuses_one_past_the_tile_limit(amd, gpu, shape):
    flags = np.full(shape, 0x20, np.uint8)
    rc, _ = edt_to_flagged(amd, gpu, flags, (0, 0, 0), shape, 0x20, (1, 1, 1))
    assert rc == -1 and f"{MAX_LINE} entries" in _err(amd._lib.load())
    # the same volume with a box that fits is taken
    hi = tuple(min(v, MAX_LINE) for v in shape)
    rc, got = edt_to_flagged(amd, gpu, flags, (0, 0, 0), hi, 0x20, (1, 1, 1))
    assert rc == 0 and not got.any()


@pytest.mark.parametrize("spacing", su.SPACINGS)
def test_distance_map_on_a_box_ignores_sites_outside(amd, gpu, spacing):
    shape, lo, hi = (12, 20, 40), (2, 3, 5), (9, 17, 33)
    sites = cu.noise(63, shape, 0.02) != 0
    sites[0, 0, 0] = sites[11, 19, 39] = sites[1, 10, 20] = sites[5, 2, 20] = sites[5, 10, 33] = True   # just outside the box, on every side kind
    assert sites[tuple(slice(a, b) for a, b in zip(lo, hi))].any()
    check_distance_map(amd, gpu, sites, spacing, what="whole volume")
    check_distance_map(amd, gpu, sites, spacing, lo, hi, what="inner box")


def test_distance_map_refusals(amd, gpu):
    lib = amd._lib.load()
    flags = np.zeros((6, 7, 8), np.uint8)
    flags[0, 0, 0] = 0x20      # a site, but outside the box below
    flags[3, 3, 3] = 0x01      # inside the box, but not a selected bit
    rc, _ = edt_to_flagged(amd, gpu, flags, (1, 1, 1), (6, 7, 8), 0x20, (1, 1, 1))
    assert rc == -1 and "no site" in _err(lib)
    for lo, hi, select, spacing, match in (((0, 0, 0), (6, 7, 9), 0x20, (1, 1, 1), "box"), ((2, 0, 0), (2, 7, 8), 0x20, (1, 1, 1), "box"),
                                           ((0, 0, 0), (6, 7, 8), 0, (1, 1, 1), "select"), ((0, 0, 0), (6, 7, 8), 0x20, (1, 0, 1), "spacing"),
                                           ((0, 0, 0), (6, 7, 8), 0x20, (1, 1, float("nan")), "spacing"),
                                           ((0, 0, 0), (6, 7, 8), 0x20, (float("inf"), 1, 1), "spacing")):
        rc, _ = edt_to_flagged(amd, gpu, flags, lo, hi, select, spacing)
        assert rc == -1 and match in _err(lib), (lo, hi, select, spacing, _err(lib))
    # a map that is too small
    lo, hi, plo, phi = _box((0, 0, 0), (6, 7, 8))
    d = torch.zeros(6 * 7 * 8, dtype=torch.float64, device=gpu)
    cnt = torch.zeros(2, dtype=torch.int32, device=gpu)
    sp = np.ones(3)
    dflags = _dev(flags, gpu)
    rc = lib.mi355_edt_to_flagged_f64(dflags.data_ptr(), 6, 7, 8, plo, phi, 0x20, sp.ctypes.data_as(F64P), d.data_ptr(), 6 * 7 * 8 - 1, cnt.data_ptr(),
                                      _stream(gpu))
    assert rc == -1 and "needs 336" in _err(lib)


# ---------------------------------------------------------------------------------------------------------------- gather
def gather(amd, gpu, values, flags, lo, hi, select, capacity=None, fill=0):
    """-> (rc, count, out array as left on the device)"""
    lib = amd._lib.load()
    lo, hi, plo, phi = _box(lo, hi)
    n = int(np.prod((hi - lo).astype(np.int64)))
    words = (n + CHUNK - 1) // CHUNK + 1
    blocks = torch.full((words,), fill, dtype=torch.int32, device=gpu)
    box = tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))
    exact = int(((flags[box] & select) != 0).sum())
    capacity = exact if capacity is None else capacity
    out = torch.full((max(capacity, 1),), -7.0, dtype=torch.float64, device=gpu)
    count = np.full(1, -1, dtype=np.int64)
    dvalues, dflags = _dev(values, gpu), _dev(flags, gpu)
    rc = lib.mi355_gather_flagged_f64(dvalues.data_ptr(), dflags.data_ptr(), *flags.shape, plo, phi, select, out.data_ptr(), capacity,
                                      blocks.data_ptr(), words, count.ctypes.data_as(I64P), _stream(gpu))
    torch.cuda.synchronize()
    return rc, int(count[0]), out.cpu().numpy()


GATHER_CASES = {
    "ragged_small": ((5, 9, 70), None, None, 0x03),
    "ragged_medium": ((7, 17, 130), None, None, 0x10),
    "several_workgroups_ragged_tail": ((13, 37, 200), None, None, 0x41),   # 96200 voxels: 46 full chunks and a tail of 1992
    "inner_box": ((13, 37, 200), (1, 2, 3), (12, 30, 190), 0x08),
    "one_voxel": ((1, 1, 1), None, None, 0xFF),
}


@pytest.mark.parametrize("name", list(GATHER_CASES))
def test_gather_equals_numpy_in_raster_order(amd, gpu, name):
    shape, lo, hi, select = GATHER_CASES[name]
    lo, hi = (0, 0, 0) if lo is None else lo, shape if hi is None else hi
    rs = np.random.RandomState(71)
    flags = (rs.randint(0, 256, shape) * (rs.random_sample(shape) < 0.4)).astype(np.uint8)
    flags[..., : shape[2] // 3] &= ~np.uint8(select)   # whole stretches (and whole chunks) with nothing selected
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    values = np.ascontiguousarray(rs.standard_normal(flags[box].shape))
    want = values[(flags[box] & select) != 0]
    for fill in (0, -1):   # the block counts hold zeros, then 0xFFFFFFFF words, on entry
        rc, count, out = gather(amd, gpu, values, flags, lo, hi, select, fill=fill)
        assert rc == 0, _err(amd._lib.load())
        assert count == len(want) and np.array_equal(out[:count], want), (name, count, len(want))


def test_gather_nothing_everything_and_a_short_capacity(amd, gpu):
    lib = amd._lib.load()
    shape = (7, 17, 130)
    rs = np.random.RandomState(72)
    values = rs.standard_normal(shape)
    flags = np.full(shape, 0x04, np.uint8)
    rc, count, out = gather(amd, gpu, values, flags, (0, 0, 0), shape, 0x08)
    assert rc == 0 and count == 0 and (out == -7.0).all(), "nothing selected"
    rc, count, out = gather(amd, gpu, values, flags, (0, 0, 0), shape, 0x0C)
    assert rc == 0 and count == values.size and np.array_equal(out, values.reshape(-1)), "everything selected"
    rc, count, out = gather(amd, gpu, values, flags, (0, 0, 0), shape, 0x04, capacity=values.size - 1)
    assert rc == -1 and "nothing was written" in _err(lib) and count == values.size, "a capacity one short is an error, not a truncation"
    assert (out == -7.0).all()
    # count-only call: no output, no values
    lo, hi, plo, phi = _box((0, 0, 0), shape)
    words = (values.size + CHUNK - 1) // CHUNK + 1
    blocks = torch.empty(words, dtype=torch.int32, device=gpu)
    n = np.zeros(1, dtype=np.int64)
    dflags = _dev(flags, gpu)
    rc = lib.mi355_gather_flagged_f64(None, dflags.data_ptr(), *shape, plo, phi, 0x04, None, 0, blocks.data_ptr(), words, n.ctypes.data_as(I64P), _stream(gpu))
    assert rc == 0 and int(n[0]) == values.size
    rc = lib.mi355_gather_flagged_f64(None, dflags.data_ptr(), *shape, plo, phi, 0x04, None, 0, blocks.data_ptr(), words - 1, n.ctypes.data_as(I64P), _stream(gpu))
    assert rc == -1 and "block counts" in _err(lib)


# ---------------------------------------------------------------------------------------------------------------- metrics end to end
@functools.lru_cache(maxsize=None)
def pair(shape):
    return su.label_pair(81, shape)


@functools.lru_cache(maxsize=None)
def oracle_distances(shape, spacing):
    pred, gt = pair(shape)
    return {name: su.region_distances(pred, gt, labels, spacing) for name, labels in su.REGIONS.items()}


def same_metrics(got, want, what):
    worst = 0.0
    for k in FLOATS:
        w, ok = su.close(got[k], want[k])
        assert ok, (what, k, got[k], want[k], w)
        worst = max(worst, w)
    for k in INTEGERS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    return worst


@pytest.mark.parametrize("spacing", su.SPACINGS)
@pytest.mark.parametrize("shape", [(24, 40, 72), (19, 23, 17)])
def test_metrics_end_to_end(amd, gpu, shape, spacing):
    pred, gt = pair(shape)
    want_d = oracle_distances(shape, spacing)
    tol = su.clear_tolerance([d for ab in want_d.values() for d in ab])
    allv = np.hstack([d for ab in want_d.values() for d in ab])
    assert np.min(np.abs(allv - tol)) > 1e-9, "an oracle distance lies at the tolerance: the counts would hinge on a rounding"
    dp, dg = _dev(pred, gpu), _dev(gt, gpu)
    got_d = amd.evaluate.surface_distances(dp, dg, spacing)
    worst, equal = 0.0, True
    for name in su.REGIONS:
        for got, want in zip(got_d[name], want_d[name]):
            assert got.dtype == np.float64 and len(want) > 0
            w, ok = su.close(got, want)
            assert ok, (name, spacing, w)
            worst, equal = max(worst, w), equal and np.array_equal(got, want)
    got_m = amd.evaluate.surface_metrics(dp, dg, spacing, tolerance_mm=tol)
    for name in su.REGIONS:
        worst = max(worst, same_metrics(got_m[name], su.metrics(*want_d[name], tol), (name, spacing)))
    print(f"end to end {shape} spacing {spacing}: worst relative difference {worst:.3g}, distances bit-equal to scipy: {equal}")
    plain = amd.evaluate.evaluate(dp, dg)
    merged = amd.evaluate.evaluate_with_surfaces(dp, dg, spacing, tolerance_mm=tol)
    assert set(merged) == set(plain)
    for key, val in plain.items():
        if isinstance(val, dict):
            for k, v in val.items():
                assert merged[key][k] == v, (key, k)
        else:
            assert merged[key] == val, key
    for name in su.REGIONS:
        for k in FLOATS + INTEGERS:
            assert merged[name][k] == got_m[name][k], (name, k)


def test_custom_regions_and_their_limit(amd, gpu):
    pred, gt = pair((19, 23, 17))
    regions = {"edema": (2,), "core": (1, 3), "all": (1, 2, 3), "necrosis": (1,)}
    got = amd.evaluate.surface_metrics(_dev(pred, gpu), _dev(gt, gpu), (5.0, 0.7, 0.7), regions=regions)
    want = su.case_metrics(pred, gt, (5.0, 0.7, 0.7), regions=regions)
    assert list(got) == list(regions)
    for name in regions:
        same_metrics(got[name], want[name], name)
    with pytest.raises(ValueError, match="regions"):
        amd.evaluate.surface_metrics(_dev(pred, gpu), _dev(gt, gpu), (1, 1, 1), regions=dict(regions, fifth=(3,)))
    with pytest.raises(ValueError, match="label values"):
        amd.evaluate.surface_metrics(_dev(pred, gpu), _dev(gt, gpu), (1, 1, 1), regions={"stray": (9,)})


# ---------------------------------------------------------------------------------------------------------------- analytic, empties
def ball(shape, centre, radius):
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    return (sum((g[k] - centre[k]) ** 2 for k in range(3)) <= radius * radius).astype(np.uint8)


def test_shifted_ball_has_the_hausdorff_distance_of_its_shift(amd, gpu):
    """independent of scipy: a ball and its translate by t are t apart in the Hausdorff sense; two voxels of 1.5 mm along axis 0"""
    a, b = ball((32, 32, 32), (14, 16, 16), 6), ball((32, 32, 32), (16, 16, 16), 6)
    regions = {"ball": (1,)}
    m = amd.evaluate.surface_metrics(_dev(a, gpu), _dev(b, gpu), (1.5, 1.0, 1.0), regions=regions)["ball"]
    assert m["hd"] == 3.0
    assert 0 < m["assd"] < m["hd95"] <= 3.0 and 0 < m["surface_dice"] < 1
    assert m["surface_voxels_pred"] == m["surface_voxels_gt"] > 0
    same = amd.evaluate.surface_metrics(_dev(a, gpu), _dev(a, gpu), (1.5, 1.0, 1.0), regions=regions)["ball"]
    assert (same["hd"], same["hd95"], same["assd"], same["surface_dice"]) == (0.0, 0.0, 0.0, 1.0)
    assert same["within_tolerance_pred"] == same["surface_voxels_pred"] == m["surface_voxels_pred"]
    d_ab, d_ba = amd.evaluate.surface_distances(_dev(a, gpu), _dev(a, gpu), (1.5, 1.0, 1.0), regions=regions)["ball"]
    assert not d_ab.any() and not d_ba.any() and len(d_ab) == len(d_ba)


@pytest.mark.parametrize("penalty", [None, 373.13])
@pytest.mark.parametrize("absent", ["prediction", "ground truth", "both"])
def test_a_region_absent_from_one_map_or_both(amd, gpu, absent, penalty):
    pred, gt = (m.copy() for m in pair((19, 23, 17)))
    if absent in ("prediction", "both"):
        pred[pred == 3] = 1
    if absent in ("ground truth", "both"):
        gt[gt == 3] = 1
    spacing = (0.9375, 1.5, 3.3)
    got = amd.evaluate.surface_metrics(_dev(pred, gpu), _dev(gt, gpu), spacing, penalty_mm=penalty)
    want = su.case_metrics(pred, gt, spacing, penalty_mm=penalty)
    for name in su.REGIONS:
        same_metrics(got[name], want[name], (name, absent))
    et = got["ET"]
    if absent == "both":
        assert (et["hd"], et["hd95"], et["assd"], et["surface_dice"]) == (0.0, 0.0, 0.0, 1.0)
    else:
        assert et["hd"] == penalty and et["hd95"] == penalty and et["assd"] == penalty and et["surface_dice"] == 0.0
        assert (et["surface_voxels_pred"] == 0) == (absent == "prediction") and (et["surface_voxels_gt"] == 0) == (absent == "ground truth")
    assert got["WT"]["hd"] is not None and got["WT"]["surface_voxels_pred"] > 0
    d = amd.evaluate.surface_distances(_dev(pred, gpu), _dev(gt, gpu), spacing)["ET"]
    want_d = su.region_distances(pred, gt, (3,), spacing)
    assert np.array_equal(d[0], want_d[0]) and np.array_equal(d[1], want_d[1])


# ---------------------------------------------------------------------------------------------------------------- dirty buffers
def test_results_do_not_depend_on_what_the_work_buffers_held(amd, gpu):
    pred, gt = pair((19, 23, 17))
    dp, dg = _dev(pred, gpu), _dev(gt, gpu)
    handed_out = []

    def filled(byte):
        def allocate(numel, dtype):
            t = torch.empty(numel, dtype=dtype, device=gpu)
            t.view(torch.uint8).fill_(byte)   # 0xFF: NaN doubles, -1 counts, every flag bit set
            handed_out.append((numel, dtype))
            return t
        return allocate

    runs = [amd.evaluate.surface_distances(dp, dg, (0.9375, 1.5, 3.3), allocate=filled(b)) for b in (0xFF, 0x00)]
    runs.append(amd.evaluate.surface_distances(dp, dg, (0.9375, 1.5, 3.3)))
    assert {d for _, d in handed_out} == {torch.uint8, torch.int32, torch.float64}, "flag volume, count words and fp64 buffers all come from the caller"
    for other in runs[1:]:
        for name in su.REGIONS:
            for a, b in zip(runs[0][name], other[name]):
                assert len(a) > 0 and np.array_equal(a, b), name


# ---------------------------------------------------------------------------------------------------------------- command
def run_command(args, timeout=240):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "brats_amd.evaluate", *args], capture_output=True, text=True, env=env, cwd=ROOT, timeout=timeout)


def test_command_reports_and_writes_what_the_api_returns(amd, gpu, tmp_path):
    from test_surface_distance_cpu import check_report_contract
    zooms = (1.0, 1.5, 3.0)
    pred, gt = su.label_pair(91, (12, 14, 10))
    for name, seg in (("pred", pred), ("gt", gt)):
        amd.nifti.save_like(tmp_path / f"{name}.nii.gz", seg, amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.uint8))
    out = tmp_path / "metrics.json"
    res = run_command(["--pred", str(tmp_path / "pred.nii.gz"), "--gt", str(tmp_path / "gt.nii.gz"), "--output", str(out), "--tolerance-mm", "1.25",
                       "--penalty-mm", "50"])
    assert res.returncode == 0, res.stdout + res.stderr
    api = amd.evaluate.evaluate_with_surfaces(_dev(pred, gpu), _dev(gt, gpu), zooms, tolerance_mm=1.25, penalty_mm=50.0)
    assert json.loads(out.read_text()) == json.loads(json.dumps(api))
    assert api["WT"]["hd95"] is not None and api["WT"]["hd95"] > 0
    check_report_contract(res.stdout.splitlines(), {"mean_dice": api["mean_dice"], "WT": api["WT"]["dice"], "TC": api["TC"]["dice"], "ET": api["ET"]["dice"]})
    assert "HD95" in res.stdout and "ASSD" in res.stdout


def test_command_fails_on_a_shape_mismatch_and_a_missing_file(amd, gpu, tmp_path):
    for name, shape in (("a", (12, 14, 10)), ("b", (12, 14, 11))):
        amd.nifti.save_like(tmp_path / f"{name}.nii.gz", np.zeros(shape, np.uint8), amd.nifti.make_header(shape, zooms=(1, 1, 1), dtype=np.uint8))
    res = run_command(["--pred", str(tmp_path / "a.nii.gz"), "--gt", str(tmp_path / "b.nii.gz")])
    assert res.returncode == 1 and "shape mismatch" in res.stderr and "Mean Dice Score" not in res.stdout
    res = run_command(["--pred", str(tmp_path / "a.nii.gz"), "--gt", str(tmp_path / "missing.nii.gz")])
    assert res.returncode == 1 and "missing.nii.gz" in res.stderr


# ---------------------------------------------------------------------------------------------------------------- full size
def test_full_size_case_against_scipy(amd, gpu):
    """240 x 240 x 155, whole tumour only: two lesions, the second map with other radii and centres"""
    shape = (240, 240, 155)
    pred = amd.synthetic.label_map(5, shape, [((120, 110, 80), 34), ((70, 150, 60), 13)], fragments=12)
    gt = amd.synthetic.label_map(6, shape, [((122, 108, 81), 31), ((70, 151, 62), 15)], fragments=0)
    spacing, regions = (0.9375, 1.5, 3.3), {"WT": (1, 2, 3)}   # the stray fragments stretch the joint box over most of the volume
    want = su.region_distances(pred, gt, regions["WT"], spacing)
    got = amd.evaluate.surface_distances(_dev(pred, gpu), _dev(gt, gpu), spacing, regions=regions)["WT"]
    for g, w in zip(got, want):
        worst, ok = su.close(g, w)
        print(f"full size: {len(w)} surface voxels, worst relative difference {worst:.3g}, bit-equal to scipy: {np.array_equal(g, w)}")
        assert len(w) > 10000 and ok, worst
    m = amd.evaluate.surface_metrics_from_distances(*got)
    same_metrics(m, su.metrics(*want), "full size")
