"""CPU oracle of the surface-distance path (csrc/surface_distance.hip, brats_amd.evaluate.surface_*), shared by
test_surface_distance_cpu.py and test_gpu_surface_distance.py: MedPy's definitions - which nnU-Net v1's evaluator calls - restated
with scipy.ndimage.binary_erosion and distance_transform_edt(~surface, sampling=spacing), and seeded label-map generators."""
import numpy as np
from scipy import ndimage

REGIONS = {"WT": (1, 2, 3), "TC": (1, 3), "ET": (3,)}
SPACINGS = ((1.0, 1.0, 1.0), (0.9375, 1.5, 3.3), (5.0, 0.7, 0.7))
# Our sum and scipy's add the same three fp64 terms in the same order; two evaluation orders of the products can differ by a few
# roundings of 2^-53 ~ 1.1e-16 relative.  1e-12 is four orders of magnitude above that and far below any real difference (the
# next candidate site changes a distance by at least ~1e-3 relative at these sizes).
RTOL = 1e-12


def surface(mask):
    """mask & ~binary_erosion(mask): 6-neighbour cross, one iteration, border_value = 0, on the whole volume"""
    mask = np.asarray(mask).astype(bool)
    return mask & ~ndimage.binary_erosion(mask, structure=ndimage.generate_binary_structure(3, 1), iterations=1, border_value=0)


def region_mask(seg, labels):
    return np.isin(seg, list(labels))


def surface_flags(pred, gt, regions_pred, regions_gt=None):
    """the flag byte mi355_region_surfaces writes: bit r the surface of region r in pred, bit 4 + r in gt"""
    regions_gt = regions_pred if regions_gt is None else regions_gt
    flags = np.zeros(pred.shape, dtype=np.uint8)
    for r, labels in enumerate(regions_pred):
        flags |= (surface(region_mask(pred, labels)).astype(np.uint8) << r).astype(np.uint8)
    for r, labels in enumerate(regions_gt):
        flags |= (surface(region_mask(gt, labels)).astype(np.uint8) << (4 + r)).astype(np.uint8)
    return flags


def table(regions):
    t = np.zeros(256, dtype=np.uint8)
    for r, labels in enumerate(regions):
        for v in labels:
            t[v] |= 1 << r
    return t


def distance_to(sites, spacing):
    """distance from every voxel to the nearest True voxel of `sites` (at least one), in the units of `spacing`"""
    return ndimage.distance_transform_edt(~np.asarray(sites, dtype=bool), sampling=spacing)


def directed(sa, sb, spacing):
    """D(A -> B) for two surfaces, in raster order of A's voxels"""
    return distance_to(sb, spacing)[sa]


def region_distances(pred, gt, labels, spacing, crop=False):
    """(D(pred -> gt), D(gt -> pred)) of one region; an absent side as brats_amd.evaluate.surface_distances reports it.  crop: take
    the distance transforms on the joint bounding box of the two surfaces only (surfaces first, crop second)."""
    sa, sb = surface(region_mask(pred, labels)), surface(region_mask(gt, labels))
    if not sa.any() or not sb.any():
        return (np.full(int(sa.sum()), np.inf) if sa.any() else np.zeros(0), np.full(int(sb.sum()), np.inf) if sb.any() else np.zeros(0))
    if crop:
        idx = np.nonzero(sa | sb)
        box = tuple(slice(int(i.min()), int(i.max()) + 1) for i in idx)
        sa, sb = sa[box], sb[box]
    return directed(sa, sb, spacing), directed(sb, sa, spacing)


def metrics(d_ab, d_ba, tolerance_mm=1.0, penalty_mm=None):
    """the issue's definitions, written out independently of brats_amd.evaluate"""
    n_a, n_b = len(d_ab), len(d_ba)
    if n_a == 0 and n_b == 0:
        return {"hd": 0.0, "hd95": 0.0, "assd": 0.0, "surface_dice": 1.0, "within_tolerance_pred": 0, "within_tolerance_gt": 0,
                "surface_voxels_pred": 0, "surface_voxels_gt": 0}
    if n_a == 0 or n_b == 0:
        return {"hd": penalty_mm, "hd95": penalty_mm, "assd": penalty_mm, "surface_dice": 0.0, "within_tolerance_pred": 0, "within_tolerance_gt": 0,
                "surface_voxels_pred": n_a, "surface_voxels_gt": n_b}
    w_a, w_b = int(np.count_nonzero(d_ab <= tolerance_mm)), int(np.count_nonzero(d_ba <= tolerance_mm))
    return {"hd": max(np.max(d_ab), np.max(d_ba)), "hd95": np.percentile(np.hstack((d_ab, d_ba)), 95),
            "assd": (np.mean(d_ab) + np.mean(d_ba)) / 2, "surface_dice": (w_a + w_b) / (n_a + n_b),
            "within_tolerance_pred": w_a, "within_tolerance_gt": w_b, "surface_voxels_pred": n_a, "surface_voxels_gt": n_b}


def case_metrics(pred, gt, spacing, tolerance_mm=1.0, penalty_mm=None, regions=REGIONS):
    return {name: metrics(*region_distances(pred, gt, labels, spacing), tolerance_mm, penalty_mm) for name, labels in regions.items()}


def nested_labels(seed, shape, levels=(0.50, 0.62, 0.72), sigma=2.5):
    """A smooth Gaussian-filtered random field thresholded into nested labels: 2 where the field's rank exceeds levels[0], 1 inside that
    above levels[1], 3 inside that above levels[2] (so WT = {1,2,3} contains TC = {1,3} contains ET = {3})."""
    field = ndimage.gaussian_filter(np.random.RandomState(seed).standard_normal(shape), sigma, mode="constant")
    q = np.quantile(field, levels)
    seg = np.zeros(shape, dtype=np.uint8)
    seg[field > q[0]] = 2
    seg[field > q[1]] = 1
    seg[field > q[2]] = 3
    return seg


def label_pair(seed, shape):
    """prediction and ground truth: the same field with a little independent smooth noise, so the surfaces lie near each other"""
    rs = np.random.RandomState(seed)
    base = ndimage.gaussian_filter(rs.standard_normal(shape), 2.5, mode="constant")
    maps = []
    for k in range(2):
        f = base + 0.35 * ndimage.gaussian_filter(np.random.RandomState(seed + 1 + k).standard_normal(shape), 2.0, mode="constant")
        q = np.quantile(f, (0.50, 0.62, 0.72))
        seg = np.zeros(shape, dtype=np.uint8)
        seg[f > q[0]] = 2
        seg[f > q[1]] = 1
        seg[f > q[2]] = 3
        maps.append(seg)
    return maps[0], maps[1]


def clear_tolerance(distance_arrays, candidates=(1.0, 1.25, 0.8, 1.6, 2.1), margin=1e-9):
    """the first candidate tolerance that no finite oracle distance comes within `margin` of: a within-tolerance count then cannot hinge
    on a rounding"""
    allv = np.hstack([np.asarray(d, dtype=np.float64).reshape(-1) for d in distance_arrays] + [np.zeros(0)])
    allv = allv[np.isfinite(allv)]
    for t in candidates:
        if allv.size == 0 or np.min(np.abs(allv - t)) > margin:
            return t
    raise AssertionError("no candidate tolerance keeps clear of every oracle distance")


def close(got, want, rtol=RTOL):
    """largest relative difference and whether it is within rtol (0 against 0 is equal; None only equals None)"""
    if got is None or want is None:
        return (0.0, got is None and want is None)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return (np.inf, False)
    if got.size == 0:
        return (0.0, True)
    same_inf = np.isinf(want) & (got == want)
    denom = np.where(want == 0, 1.0, np.abs(want))
    with np.errstate(invalid="ignore"):
        rel = np.where(same_inf, 0.0, np.abs(got - want) / denom)
    rel = np.where(np.isnan(rel), np.inf, rel)
    worst = float(rel.max())
    return worst, worst <= rtol
