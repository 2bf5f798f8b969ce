"""GPU mirror of the reference evaluator and label converter.

``evaluate_segmentation.py`` builds float masks and sums them four times per label; here one
pass over the two uint8 label maps on the device yields the K x K confusion counts, and every
metric of ``calculate_metrics`` (:12-49) / ``calculate_metrics_binary`` (:181-195) and the compound
WT / TC / ET regions (:129-162) is derived from those integers with the reference's formulas
(same 1e-8 epsilons).  ``convert_labels`` is convert_labels_to_brats.py:34-55 as a 256-entry map.

Beside the reference's overlap numbers: surface distances per region (``surface_*``, csrc/surface_distance.hip) and the lesion-wise
Dice and HD95 the BraTS challenges rank by since 2023 (``lesionwise_*``, csrc/lesionwise.hip); neither has a counterpart in the
reference tree.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

LABEL_MAPS = {
    "nnunet": {},
    "brats2025": {1: 2, 2: 1, 3: 3},   # convert_labels_to_brats.py:34-43
    "brats2021": {1: 2, 2: 1, 3: 4},   # :46-55
}


def convert_labels(seg, fmt="brats2025"):
    """seg: CUDA uint8 tensor of nnU-Net labels -> same shape in the requested convention
    (labels the reference's converter does not mention become 0, as ``np.zeros_like`` leaves them)."""
    import torch
    if fmt not in LABEL_MAPS:
        raise ValueError(f"unknown label format {fmt}")
    if fmt == "nnunet":
        return seg.clone()
    table = np.zeros(256, dtype=np.uint8)
    for k, v in LABEL_MAPS[fmt].items():
        table[k] = v
    seg = seg.contiguous()
    out = torch.empty_like(seg)
    stream = torch.cuda.current_stream(seg.device).cuda_stream
    _lib.check(_lib.load().mi355_label_remap(seg.data_ptr(), out.data_ptr(), seg.numel(),
                                             table.ctypes.data_as(C.POINTER(C.c_uint8)), stream), "mi355_label_remap")
    return out


def apply_brats_threshold(seg, threshold=200, replace_with=2):
    """KAIST post-processing (archived/kaist_original_inference.py:33, ``apply_threshold_to_folder(..., 200, 2)``):
    a case with fewer than `threshold` voxels of label 3 (enhancing tumour) gets them relabelled to `replace_with`.
    seg: CUDA uint8 label map.  Returns (new label map, number of label-3 voxels found)."""
    n3 = int(confusion(seg, seg, num_labels=5)[3, 3])  # one device pass; bin 4 = "other" keeps labels >= 4 out of bin 3
    if n3 >= threshold:
        return seg.clone(), n3
    import torch
    table = np.arange(256, dtype=np.uint8)
    table[3] = replace_with
    seg = seg.contiguous()
    out = torch.empty_like(seg)
    stream = torch.cuda.current_stream(seg.device).cuda_stream
    _lib.check(_lib.load().mi355_label_remap(seg.data_ptr(), out.data_ptr(), seg.numel(),
                                             table.ctypes.data_as(C.POINTER(C.c_uint8)), stream), "mi355_label_remap")
    return out, n3


def confusion(pred, gt, num_labels=6):
    """K x K integer matrix, rows = predicted label, columns = ground truth.  The last bin (K-1) is "other": it
    collects every label >= K-1 (the reference compares ``== label`` per label, evaluate_segmentation.py:20-21, so a
    stray label must never be counted as a real one); the matrix always sums to the voxel count."""
    import torch
    if pred.shape != gt.shape or pred.dtype != torch.uint8 or gt.dtype != torch.uint8:
        raise ValueError("confusion: two uint8 tensors of equal shape expected (evaluate_segmentation.py:78-81)")
    pred, gt = pred.contiguous(), gt.contiguous()
    counts = np.zeros(num_labels * num_labels, dtype=np.uint64)
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    _lib.check(_lib.load().mi355_label_confusion(pred.data_ptr(), gt.data_ptr(), pred.numel(), num_labels,
                                                 counts.ctypes.data_as(C.POINTER(C.c_uint64)), stream),
               "mi355_label_confusion")
    return counts.reshape(num_labels, num_labels).astype(np.int64)


def _metrics(tp, fp, fn, tn=None):
    out = {"dice": (2 * tp) / (2 * tp + fp + fn + 1e-8), "iou": tp / (tp + fp + fn + 1e-8),
           "sensitivity": tp / (tp + fn + 1e-8), "tp": float(tp), "fp": float(fp), "fn": float(fn)}
    if tn is not None:
        out["specificity"] = tn / (tn + fp + 1e-8)
        out["tn"] = float(tn)
    return out


def metrics_from_confusion(cm, labels=(1, 2, 3)):
    """Per-label metrics (calculate_metrics) + WT {1,2,3}, TC {1,3}, ET {3} in the BraTS convention
    (evaluate_segmentation.py:129-162) + the mean Dice the pipeline reports."""
    cm = np.asarray(cm, dtype=np.float64)
    total = cm.sum()
    res = {}
    for lab in labels:
        tp = cm[lab, lab]
        fp = cm[lab, :].sum() - tp
        fn = cm[:, lab].sum() - tp
        res[lab] = _metrics(tp, fp, fn, total - tp - fp - fn)

    def region(members):
        m = list(members)
        tp = cm[np.ix_(m, m)].sum()
        fp = cm[m, :].sum() - tp
        fn = cm[:, m].sum() - tp
        return _metrics(tp, fp, fn)

    res["WT"], res["TC"], res["ET"] = region((1, 2, 3)), region((1, 3)), region((3,))
    res["mean_dice"] = float(np.mean([res["WT"]["dice"], res["TC"]["dice"], res["ET"]["dice"]]))
    return res


def evaluate(pred, gt):
    """pred, gt: CUDA uint8 label maps in the BraTS convention -> metrics dict."""
    return metrics_from_confusion(confusion(pred, gt, 6))  # labels 0..4 + "other"


# ---- feature_extraction/utils.py:167-216 on the device --------------------------------------------------------
REGION_LABELS = {"ncr": (1,), "ed": (2,), "et": (3, 4), "tc": (1, 3, 4), "wt": (1, 2, 3, 4)}  # utils.py:171-178


def label_stats(seg, num_labels=5):
    """seg: CUDA uint8 label map [d0, d1, d2] -> int64 array [num_labels, 10]: count, coordinate sums (3), minima (3),
    maxima (3) per label value (one pass on the device)."""
    import torch
    if seg.dtype != torch.uint8 or not seg.is_cuda or seg.dim() != 3:
        raise ValueError("label_stats: CUDA uint8 [d0, d1, d2] tensor expected")
    seg = seg.contiguous()
    out = np.zeros(num_labels * 10, dtype=np.int64)
    stream = torch.cuda.current_stream(seg.device).cuda_stream
    _lib.check(_lib.load().mi355_label_stats(seg.data_ptr(), seg.shape[0], seg.shape[1], seg.shape[2], num_labels,
                                             out.ctypes.data_as(C.POINTER(C.c_int64)), stream), "mi355_label_stats")
    return out.reshape(num_labels, 10)


def tumor_region_features(seg, voxel_volume_cm3):
    """Volumes, centroids and bounding boxes of the reference's tumour regions (utils.py:167-216: get_tumor_masks,
    calculate_volume, get_centroid, get_bounding_box) from one device pass; axes named x, y, z in array order as there."""
    st = label_stats(seg, 5)
    out = {}
    for name, labels in REGION_LABELS.items():
        rows = st[list(labels)]
        n = int(rows[:, 0].sum())
        feat = {"volume_cm3": float(n * voxel_volume_cm3), "centroid": None, "bounding_box": None}
        if n > 0:
            present = rows[rows[:, 0] > 0]
            sums = rows[:, 1:4].sum(axis=0)
            lo, hi = present[:, 4:7].min(axis=0), present[:, 7:10].max(axis=0)
            feat["centroid"] = {k: float(sums[i] / n) for i, k in enumerate("xyz")}
            feat["bounding_box"] = {**{f"min_{k}": int(lo[i]) for i, k in enumerate("xyz")},
                                    **{f"max_{k}": int(hi[i]) for i, k in enumerate("xyz")},
                                    **{f"size_{k}": int(hi[i] - lo[i] + 1) for i, k in enumerate("xyz")}}
        out[name] = feat
    return out


# ---- surface distances: HD95, ASSD and the surface Dice (MedPy's definitions, which nnU-Net v1's evaluator reports beside Dice) ----
SURFACE_REGIONS = {"WT": (1, 2, 3), "TC": (1, 3), "ET": (3,)}   # metrics_from_confusion's regions, BraTS convention
MAX_SURFACE_REGIONS = 4     # region bits per map in a flag byte (mi355_region_surfaces)
GATHER_CHUNK = 2048         # MI355_GATHER_CHUNK
_STATS_LABELS = 8           # label_stats reports label values below this: where the boxes come from


def _check_regions(regions):
    regions = dict(SURFACE_REGIONS if regions is None else regions)
    if not 1 <= len(regions) <= MAX_SURFACE_REGIONS:
        raise ValueError(f"surface distances: {len(regions)} regions (1..{MAX_SURFACE_REGIONS} per call)")
    out = {}
    for name, labels in regions.items():
        labels = tuple(int(v) for v in labels)
        if not labels or any(not 1 <= v < _STATS_LABELS for v in labels):
            raise ValueError(f"surface distances: region {name!r} = {labels} (label values 1..{_STATS_LABELS - 1}, at least one)")
        out[name] = labels
    return out


def _check_spacing(spacing):
    try:
        sp = [float(v) for v in spacing]
    except (TypeError, ValueError):
        sp = []
    if len(sp) != 3 or not all(np.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"surface distances: spacing {spacing!r} (three finite positive voxel sizes, one per array axis)")
    return np.array(sp, dtype=np.float64)


def _region_table(regions):
    table = np.zeros(256, dtype=np.uint8)
    for r, labels in enumerate(regions.values()):
        for v in labels:
            table[v] |= 1 << r
    return table


def surface_distances(pred, gt, spacing, regions=None, allocate=None):
    """pred, gt: CUDA uint8 label maps [d0, d1, d2]; spacing: the voxel size along each array axis ->
    {name: (D(pred -> gt), D(gt -> pred))}, float64 numpy arrays in raster order of the surface voxels: the distance from every
    surface voxel of the region in one map to the nearest surface voxel of the region in the other (surface = mask &
    ~binary_erosion(mask), taken on the whole volume).  A region that is absent from both maps gives two empty arrays; one that is
    absent from one map only gives an empty array for that map and +inf for every surface voxel of the other.

    One pass marks all surfaces of both maps, then each direction is one distance transform on the joint bounding box of the
    region (from label_stats) and one ordered gather; the device returns squared distances, the root is taken here.  torch only
    allocates: `allocate(numel, dtype)` (default torch.empty on pred's device) supplies every work buffer."""
    import torch
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dtype != torch.uint8 or gt.dtype != torch.uint8:
        raise ValueError("surface distances: two uint8 label maps expected")
    if pred.shape != gt.shape or pred.dim() != 3:
        raise ValueError(f"surface distances: shapes {tuple(pred.shape)} and {tuple(gt.shape)} (two [d0, d1, d2] maps of equal shape)")
    sp = _check_spacing(spacing)
    regions = _check_regions(regions)
    if not (pred.is_cuda and gt.is_cuda):
        raise ValueError("surface distances: CUDA tensors expected")
    pred, gt = pred.contiguous(), gt.contiguous()
    table = _region_table(regions)
    stats = (label_stats(pred, _STATS_LABELS), label_stats(gt, _STATS_LABELS))
    plans = {}
    for r, (name, labels) in enumerate(regions.items()):
        rows = [st[list(labels)] for st in stats]
        counts = [int(rw[:, 0].sum()) for rw in rows]
        present = np.concatenate([rw[rw[:, 0] > 0] for rw in rows])
        lo = hi = None
        if len(present):
            lo = present[:, 4:7].min(axis=0).astype(np.int32)
            hi = (present[:, 7:10].max(axis=0) + 1).astype(np.int32)
        plans[name] = (r, counts, lo, hi)
    return _flagged_distances(pred, gt, sp, table, table, plans, allocate)


def _flagged_distances(pred, gt, sp, pred_table, gt_table, plans, allocate=None):
    """The device half of ``surface_distances`` with everything that call derives from label values handed in: the two 256-entry tables
    (value of `pred` / of `gt` -> bits 0..3 of the regions it belongs to in that map, one table per map) and per region
    ``plans[name] = (bit r, (voxels of the region in pred, in gt), lo, hi)`` with [lo, hi) the index box the distances are taken on (None
    where the region is absent from both maps).  pred, gt: contiguous CUDA uint8 maps of one shape, sp: float64 [3]."""
    import torch
    if allocate is None:
        def allocate(numel, dtype):
            return torch.empty(numel, dtype=dtype, device=pred.device)
    lib = _lib.load()
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    d0, d1, d2 = (int(v) for v in pred.shape)
    u8p, i32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    flags = allocate(pred.numel(), torch.uint8)
    _lib.check(lib.mi355_region_surfaces(pred.data_ptr(), gt.data_ptr(), d0, d1, d2, pred_table.ctypes.data_as(u8p), gt_table.ctypes.data_as(u8p),
                                         flags.data_ptr(), flags.numel(), stream), "mi355_region_surfaces")
    both = [p for p in plans.values() if p[1][0] and p[1][1]]
    box_voxels = max([int(np.prod((p[3] - p[2]).astype(np.int64))) for p in plans.values() if p[2] is not None], default=0)
    block_words = (box_voxels + GATHER_CHUNK - 1) // GATHER_CHUNK + 1
    blocks = allocate(block_words, torch.int32)
    count_word = allocate(2, torch.int32)
    dist2 = allocate(max([int(np.prod((p[3] - p[2]).astype(np.int64))) for p in both], default=1), torch.float64)
    picked = allocate(max([max(p[1]) for p in both], default=1), torch.float64)   # a surface has no more voxels than its mask
    n_host = np.zeros(1, dtype=np.int64)

    def box_args(lo, hi):
        return lo.ctypes.data_as(i32p), hi.ctypes.data_as(i32p)

    def directed(lo, hi, from_bit, to_bit, capacity):
        _lib.check(lib.mi355_edt_to_flagged_f64(flags.data_ptr(), d0, d1, d2, *box_args(lo, hi), to_bit, sp.ctypes.data_as(f64p), dist2.data_ptr(),
                                                dist2.numel(), count_word.data_ptr(), stream), "mi355_edt_to_flagged_f64")
        _lib.check(lib.mi355_gather_flagged_f64(dist2.data_ptr(), flags.data_ptr(), d0, d1, d2, *box_args(lo, hi), from_bit, picked.data_ptr(), capacity,
                                                blocks.data_ptr(), block_words, n_host.ctypes.data_as(C.POINTER(C.c_int64)), stream),
                   "mi355_gather_flagged_f64")
        return np.sqrt(picked[:int(n_host[0])].cpu().numpy())

    def surface_size(lo, hi, bit):
        _lib.check(lib.mi355_gather_flagged_f64(None, flags.data_ptr(), d0, d1, d2, *box_args(lo, hi), bit, None, 0, blocks.data_ptr(), block_words,
                                                n_host.ctypes.data_as(C.POINTER(C.c_int64)), stream), "mi355_gather_flagged_f64")
        return int(n_host[0])

    out = {}
    for name, (r, (n_pred, n_gt), lo, hi) in plans.items():
        p_bit, g_bit = 1 << r, 16 << r
        if n_pred and n_gt:
            out[name] = (directed(lo, hi, p_bit, g_bit, n_pred), directed(lo, hi, g_bit, p_bit, n_gt))
        elif n_pred:
            out[name] = (np.full(surface_size(lo, hi, p_bit), np.inf), np.zeros(0))
        elif n_gt:
            out[name] = (np.zeros(0), np.full(surface_size(lo, hi, g_bit), np.inf))
        else:
            out[name] = (np.zeros(0), np.zeros(0))
    return out


def surface_metrics_from_distances(d_ab, d_ba, tolerance_mm=1.0, penalty_mm=None):
    """The two directed distance arrays of a region (``surface_distances``) -> hd (the larger of the two maxima), hd95 (numpy's
    95th percentile of the two arrays pooled), assd (the mean of the two means), surface_dice at `tolerance_mm` with its two
    within-tolerance counts, and the two surface sizes.  Both surfaces empty: distances 0.0, surface_dice 1.0.  Exactly one
    empty: distances None - or `penalty_mm` when given (BraTS 2021 used the volume diagonal) - and surface_dice 0.0.  Pure numpy."""
    d_ab, d_ba = np.asarray(d_ab, dtype=np.float64).reshape(-1), np.asarray(d_ba, dtype=np.float64).reshape(-1)
    out = {"hd": 0.0, "hd95": 0.0, "assd": 0.0, "surface_dice": 1.0, "tolerance_mm": float(tolerance_mm),
           "within_tolerance_pred": 0, "within_tolerance_gt": 0, "surface_voxels_pred": int(d_ab.size), "surface_voxels_gt": int(d_ba.size)}
    if d_ab.size == 0 and d_ba.size == 0:
        return out
    if d_ab.size == 0 or d_ba.size == 0:
        missing = None if penalty_mm is None else float(penalty_mm)
        out.update(hd=missing, hd95=missing, assd=missing, surface_dice=0.0)
        return out
    n_ab, n_ba = int((d_ab <= tolerance_mm).sum()), int((d_ba <= tolerance_mm).sum())
    out.update(hd=float(max(d_ab.max(), d_ba.max())), hd95=float(np.percentile(np.hstack((d_ab, d_ba)), 95)),
               assd=float((d_ab.mean() + d_ba.mean()) / 2), surface_dice=(n_ab + n_ba) / (d_ab.size + d_ba.size),
               within_tolerance_pred=n_ab, within_tolerance_gt=n_ba)
    return out


def surface_metrics(pred, gt, spacing, regions=None, tolerance_mm=1.0, penalty_mm=None):
    """{region name: surface_metrics_from_distances(...)} of two CUDA uint8 label maps."""
    return {name: surface_metrics_from_distances(d_ab, d_ba, tolerance_mm, penalty_mm)
            for name, (d_ab, d_ba) in surface_distances(pred, gt, spacing, regions).items()}


def evaluate_with_surfaces(pred, gt, spacing, tolerance_mm=1.0, penalty_mm=None):
    """``evaluate()``'s dict with the surface metrics of WT, TC and ET merged into those three entries."""
    res = evaluate(pred, gt)
    for name, m in surface_metrics(pred, gt, spacing, None, tolerance_mm, penalty_mm).items():
        res[name] = {**res[name], **m}
    return res


# ---- lesion-wise Dice and HD95: the ground truth dilated, its components grouped into lesions, predicted components matched to them ----
LESION_DILATION = 3             # steps of the 18-neighbourhood that group ground-truth components into lesions
LESION_MIN_VOLUME_MM3 = 50.0    # a lesion counts only above this volume
LESION_PENALTY_MM = 374.0       # HD95 of a missed lesion and of a false-positive component
LESION_BATCH = MAX_SURFACE_REGIONS   # lesions whose surfaces one pass of mi355_region_surfaces marks


def _check_lesion_params(dilation, min_volume_mm3, penalty_mm):
    try:
        ok = int(dilation) == dilation and 1 <= int(dilation) <= 16
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"lesion-wise metrics: dilation {dilation!r} (1..16 steps)")
    for what, v in (("min_volume_mm3", min_volume_mm3), ("penalty_mm", penalty_mm)):
        try:
            ok = bool(np.isfinite(float(v)) and float(v) >= 0)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"lesion-wise metrics: {what} {v!r} (finite and not negative)")
    return int(dilation), float(min_volume_mm3), float(penalty_mm)


def _lesion_matches(gt_in_dilated, pred_in_dilated):
    """-> (merge, members, matched): merge[c] = the lesion that ground-truth component c belongs to (merge[0] = 0), members[L] = the
    ground-truth components of lesion L, matched[L] = the sorted predicted components with a voxel inside dilated component L."""
    gg = np.asarray(gt_in_dilated, dtype=np.int64)
    pd = np.asarray(pred_in_dilated, dtype=np.int64)
    if gg.ndim != 2 or pd.ndim != 2 or gg.shape[1] != pd.shape[1] or gg.shape[0] < 1 or pd.shape[0] < 1 or (gg < 0).any() or (pd < 0).any():
        raise ValueError(f"lesion-wise metrics: pair tables of shapes {gg.shape} and {pd.shape} (one column per dilated component and column 0)")
    n_lesions = gg.shape[1] - 1
    merge = np.zeros(gg.shape[0], dtype=np.int32)
    for c in range(1, gg.shape[0]):
        cols = np.flatnonzero(gg[c])
        if len(cols) != 1 or cols[0] == 0:
            raise ValueError(f"lesion-wise metrics: ground-truth component {c} lies in dilated components {cols.tolist()} (exactly one, not 0: "
                             "the second map is not a dilation of the first)")
        merge[c] = cols[0]
    members = {L: [int(c) for c in np.flatnonzero(merge == L)] for L in range(1, n_lesions + 1)}
    if any(not m for m in members.values()):
        raise ValueError("lesion-wise metrics: a dilated component without a ground-truth component")
    matched = {L: [int(c) for c in np.flatnonzero(pd[1:, L] > 0) + 1] for L in range(1, n_lesions + 1)}
    return merge, members, matched


def lesionwise_from_tables(gt_in_dilated, pred_in_dilated, pred_in_lesions, spacing, distances, dilation=LESION_DILATION,
                           min_volume_mm3=LESION_MIN_VOLUME_MM3, penalty_mm=LESION_PENALTY_MM):
    """Lesion-wise Dice and HD95 of one region from three joint histograms of label maps (``components.pair_counts``; row 0 / column 0 =
    label 0), all 26-connected and numbered as scipy numbers them:
      gt_in_dilated   [n_gt + 1, n + 1]    components of the ground truth  x  components of the dilated ground truth
      pred_in_dilated [n_pred + 1, n + 1]  components of the prediction    x  components of the dilated ground truth
      pred_in_lesions [n_pred + 1, n + 1]  components of the prediction    x  the lesion map (ground-truth voxels numbered by lesion)
    Lesion L = the ground truth inside dilated component L; the predicted components with a voxel inside dilated component L are matched
    to it (a component may be matched to several lesions and counts in each); their union is P_L.  `distances`: per lesion with a
    match the two directed surface-distance arrays between P_L and L - a mapping {L: (d_pred_to_gt, d_gt_to_pred)}, or a callable
    (L, matched component ids) -> that pair.  Returns the region's dict: one row per lesion in order of L (gt_voxels, gt_components,
    pred_components, pred_voxels, intersection, dice, hd95 = ``surface_metrics_from_distances(...)["hd95"]``, counted = gt_voxels *
    prod(spacing) > min_volume_mm3), the components matched to no lesion as false positives, and over N = counted rows + false
    positives lesionwise_dice = sum of counted dice / N, lesionwise_hd95 = (sum of counted hd95 + penalty_mm * false positives) / N
    (N == 0: 1.0 and 0.0).  An unmatched lesion has dice 0.0 and hd95 penalty_mm.  Pure host arithmetic."""
    sp = _check_spacing(spacing)
    dilation, min_volume_mm3, penalty_mm = _check_lesion_params(dilation, min_volume_mm3, penalty_mm)
    merge, members, matched = _lesion_matches(gt_in_dilated, pred_in_dilated)
    gg, pd, pl = (np.asarray(t, dtype=np.int64) for t in (gt_in_dilated, pred_in_dilated, pred_in_lesions))
    if pl.shape != pd.shape or (pl < 0).any() or not np.array_equal(pl.sum(axis=1), pd.sum(axis=1)):
        raise ValueError("lesion-wise metrics: the two tables of the prediction disagree in shape or in the sizes of its components")
    if not np.array_equal(pl.sum(axis=0)[1:], gg[1:].sum(axis=0)[1:]):
        raise ValueError("lesion-wise metrics: the lesion map and the ground-truth table disagree in the sizes of the lesions")
    sizes = pd.sum(axis=1)     # voxels per predicted component
    voxel_mm3 = float(np.prod(sp))
    rows, used = [], set()
    for L in sorted(members):
        comps = matched[L]
        used.update(comps)
        gt_voxels = int(gg[1:, L].sum())
        pred_voxels = int(sizes[comps].sum()) if comps else 0
        inter = int(pl[comps, L].sum()) if comps else 0
        if comps:
            d_ab, d_ba = distances(L, comps) if callable(distances) else distances[L]
            dice = 2 * inter / (pred_voxels + gt_voxels)
            hd95 = surface_metrics_from_distances(d_ab, d_ba)["hd95"]
        else:
            dice, hd95 = 0.0, penalty_mm
        rows.append({"lesion": int(L), "gt_voxels": gt_voxels, "gt_components": len(members[L]), "pred_components": comps, "pred_voxels": pred_voxels,
                     "intersection": inter, "dice": float(dice), "hd95": float(hd95), "counted": bool(gt_voxels * voxel_mm3 > min_volume_mm3)})
    false_pos = [{"id": c, "voxels": int(sizes[c])} for c in range(1, pd.shape[0]) if c not in used]
    counted = [r for r in rows if r["counted"]]
    n = len(counted) + len(false_pos)
    dice = sum(r["dice"] for r in counted) / n if n else 1.0
    hd95 = (sum(r["hd95"] for r in counted) + penalty_mm * len(false_pos)) / n if n else 0.0
    return {"lesionwise_dice": float(dice), "lesionwise_hd95": float(hd95), "num_lesions": len(rows), "num_counted": len(counted),
            "num_tp": sum(1 for r in counted if r["pred_components"]), "num_fn": sum(1 for r in counted if not r["pred_components"]),
            "num_fp": len(false_pos), "fp_components": false_pos, "lesions": rows,
            "dilation": dilation, "min_volume_mm3": min_volume_mm3, "penalty_mm": penalty_mm}


def _check_maps(pred, gt, what):
    import torch
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dtype != torch.uint8 or gt.dtype != torch.uint8:
        raise ValueError(f"{what}: two uint8 label maps expected")
    if pred.shape != gt.shape or pred.dim() != 3:
        raise ValueError(f"{what}: shapes {tuple(pred.shape)} and {tuple(gt.shape)} (two [d0, d1, d2] maps of equal shape)")


def _region_lesionwise(pred, gt, labels, sp, dilation, min_volume_mm3, penalty_mm, name):
    """One region on the device: three labellings, one dilation, three joint histograms, one lookup for the lesion map; then per batch
    of up to four matched lesions two byte maps (ground truth: the lesion's slot 1..4, prediction: the bits of the slots its component
    is matched to) whose surfaces one pass marks, and per lesion the two directed distance arrays on the joint box of L and P_L."""
    from . import components as cc
    from .volume_ops import binary_dilation_nb
    p_mask, g_mask = cc._indicator(pred, labels), cc._indicator(gt, labels)
    pcc, n_pred = cc.label_components(p_mask, 3)
    gcc, n_gt = cc.label_components(g_mask, 3)
    gdcc, n_les = cc.label_components(binary_dilation_nb(g_mask, 18, dilation), 3)
    for what, n in (("the prediction", n_pred), ("the ground truth", n_gt), ("the dilated ground truth", n_les)):
        if n > cc.MAX_COMPONENTS:
            raise ValueError(f"lesion-wise metrics: region {name!r} of {what} has {n} components ({cc.MAX_COMPONENTS} at most)")
    gg = cc.pair_counts(gcc, n_gt, gdcc, n_les, (f"region {name!r} of the ground truth", "its dilation"))
    pd = cc.pair_counts(pcc, n_pred, gdcc, n_les, (f"region {name!r} of the prediction", "the dilated ground truth"))
    merge, members, matched = _lesion_matches(gg, pd)
    lesion_map = cc.lookup(gcc, n_gt, merge)
    pl = cc.pair_counts(pcc, n_pred, lesion_map, n_les, (f"region {name!r} of the prediction", "the lesions"))
    todo = [L for L in sorted(members) if matched[L]]
    distances = {}
    if todo:
        p_stats, g_stats = cc.component_stats(pcc, n_pred), cc.component_stats(gcc, n_gt)
        p_bits = np.zeros(256, dtype=np.uint8)
        p_bits[:16] = np.arange(16)                      # the prediction's byte is the mask of its slots already
        g_bits = np.zeros(256, dtype=np.uint8)
        g_bits[1:LESION_BATCH + 1] = 1 << np.arange(LESION_BATCH)   # the ground truth's byte is one slot 1..4
        for b in range(0, len(todo), LESION_BATCH):
            batch = todo[b:b + LESION_BATCH]
            g_table, p_table, plans = np.zeros(n_gt + 1, dtype=np.uint8), np.zeros(n_pred + 1, dtype=np.uint8), {}
            for slot, L in enumerate(batch):
                g_table[members[L]] = slot + 1
                p_table[matched[L]] |= 1 << slot
                rows = np.concatenate([g_stats[np.array(members[L]) - 1], p_stats[np.array(matched[L]) - 1]])
                lo = rows[:, cc.MIN0:cc.MIN0 + 3].min(axis=0).astype(np.int32)
                hi = (rows[:, cc.MAX0:cc.MAX0 + 3].max(axis=0) + 1).astype(np.int32)
                counts = [int(p_stats[np.array(matched[L]) - 1, cc.COUNT].sum()), int(g_stats[np.array(members[L]) - 1, cc.COUNT].sum())]
                plans[L] = (slot, counts, lo, hi)
            distances.update(_flagged_distances(cc.lookup(pcc, n_pred, p_table), cc.lookup(gcc, n_gt, g_table), sp, p_bits, g_bits, plans))
    return lesionwise_from_tables(gg, pd, pl, sp, distances, dilation, min_volume_mm3, penalty_mm)


def lesionwise_metrics(pred, gt, spacing, regions=None, dilation=LESION_DILATION, min_volume_mm3=LESION_MIN_VOLUME_MM3, penalty_mm=LESION_PENALTY_MM):
    """pred, gt: CUDA uint8 label maps [d0, d1, d2]; spacing: the voxel size along each array axis -> {region name:
    ``lesionwise_from_tables(...)``} for WT, TC and ET (or `regions`, as ``surface_distances`` takes them): the lesion-wise Dice and
    HD95 the BraTS challenges rank by since 2023, with the project's pooled-percentile HD95 per lesion."""
    _check_maps(pred, gt, "lesion-wise metrics")
    sp = _check_spacing(spacing)
    regions = _check_regions(regions)
    dilation, min_volume_mm3, penalty_mm = _check_lesion_params(dilation, min_volume_mm3, penalty_mm)
    if not (pred.is_cuda and gt.is_cuda):
        raise ValueError("lesion-wise metrics: CUDA tensors expected")
    pred, gt = pred.contiguous(), gt.contiguous()
    return {name: _region_lesionwise(pred, gt, labels, sp, dilation, min_volume_mm3, penalty_mm, name) for name, labels in regions.items()}


def evaluate_lesionwise(pred, gt, spacing, tolerance_mm=1.0, surface_penalty_mm=None, dilation=LESION_DILATION,
                        min_volume_mm3=LESION_MIN_VOLUME_MM3, penalty_mm=LESION_PENALTY_MM):
    """``evaluate_with_surfaces()``'s dict with a "lesionwise" entry (``lesionwise_metrics``) in WT, TC and ET.  `surface_penalty_mm` is
    that function's penalty for a region absent from one map, `penalty_mm` the lesion-wise one."""
    res = evaluate_with_surfaces(pred, gt, spacing, tolerance_mm, surface_penalty_mm)
    for name, m in lesionwise_metrics(pred, gt, spacing, None, dilation, min_volume_mm3, penalty_mm).items():
        res[name] = {**res[name], "lesionwise": m}
    return res


# ---- the command: evaluate_segmentation.py's two arguments, a report run_full_pipeline.py:253-269 can parse ----
REGION_TITLES = {"WT": "Whole Tumor", "TC": "Tumor Core", "ET": "Enhancing Tumor"}


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m brats_amd.evaluate", description="Overlap and surface-distance metrics of a predicted label map "
                                 "against a ground truth (BraTS convention), computed on the GPU")
    ap.add_argument("--pred", required=True, help="predicted segmentation (.nii / .nii.gz)")
    ap.add_argument("--gt", required=True, help="ground-truth segmentation (.nii / .nii.gz)")
    ap.add_argument("--output", default=None, help="write every metric to this JSON file")
    ap.add_argument("--tolerance-mm", type=float, default=1.0, help="tolerance of the surface Dice")
    ap.add_argument("--penalty-mm", type=float, default=None, help="distance reported when a region is absent from one map only (default: null)")
    ap.add_argument("--no-surface", action="store_true", help="overlap metrics only")
    ap.add_argument("--lesionwise", action="store_true", help="add the lesion-wise scores of WT, TC and ET")
    ap.add_argument("--dilation", type=int, default=LESION_DILATION, help="18-neighbour dilation steps that group ground-truth components into lesions")
    ap.add_argument("--min-lesion-mm3", type=float, default=LESION_MIN_VOLUME_MM3, help="a lesion counts only above this volume")
    ap.add_argument("--lesion-penalty-mm", type=float, default=LESION_PENALTY_MM, help="HD95 of a missed lesion and of a false-positive component")
    return ap


def _mm(v):
    return "    n/a" if v is None else f"{v:7.2f}"


def report_lines(res, pred_path="", gt_path=""):
    """The printed report of a metrics dict (``evaluate`` or ``evaluate_with_surfaces``).  run_full_pipeline.py:253-269 finds
    the four Dice scores by substring, so exactly one line carries each of its four phrases, with the score as NN.NN%."""
    lines = ["=" * 64, "Segmentation evaluation on the GPU", f"  prediction   : {pred_path}", f"  ground truth : {gt_path}", "=" * 64,
             "Per label value          overlap      IoU   sensitivity"]
    for lab in (1, 2, 3):
        m = res[lab]
        lines.append(f"  value {lab}              {100 * m['dice']:6.2f}%  {100 * m['iou']:6.2f}%  {100 * m['sensitivity']:6.2f}%")
    lines += ["-" * 64, "BraTS regions            overlap      IoU   sensitivity"]
    for key, title in REGION_TITLES.items():
        m = res[key]
        lines.append(f"  {title + ' (' + key + ')':22s} {100 * m['dice']:6.2f}%  {100 * m['iou']:6.2f}%  {100 * m['sensitivity']:6.2f}%")
    lines += ["-" * 64, f"Mean Dice Score (WT, TC, ET): {100 * res['mean_dice']:.2f}%"]
    if "hd95" in res["WT"]:
        lines += ["-" * 64, f"Surface distances in mm  HD95     ASSD       HD   NSD at {res['WT']['tolerance_mm']:g} mm   surface voxels (pred / gt)"]
        for key in REGION_TITLES:
            m = res[key]
            lines.append(f"  {key}                  {_mm(m['hd95'])}  {_mm(m['assd'])}  {_mm(m['hd'])}   {m['surface_dice']:8.4f}       "
                         f"{m['surface_voxels_pred']} / {m['surface_voxels_gt']}")
    if "lesionwise" in res["WT"]:   # the regions by their short names only: the four phrases above stay on one line each
        first = res["WT"]["lesionwise"]
        lines += ["-" * 64, f"Lesion-wise ({first['dilation']} dilation steps, > {first['min_volume_mm3']:g} mm3, penalty {first['penalty_mm']:g} mm)",
                  "                      Dice   HD95 mm   lesions / counted / TP / FN / FP"]
        for key in REGION_TITLES:
            m = res[key]["lesionwise"]
            lines.append(f"  {key}                {m['lesionwise_dice']:8.4f}  {m['lesionwise_hd95']:8.2f}   "
                         f"{m['num_lesions']} / {m['num_counted']} / {m['num_tp']} / {m['num_fn']} / {m['num_fp']}")
    lines.append("=" * 64)
    return lines


def main(argv=None):
    import json
    import sys
    from . import nifti
    args = build_parser().parse_args(argv)
    images = []
    for path in (args.pred, args.gt):
        try:
            images.append(nifti.load(path))
        except (OSError, ValueError, EOFError) as e:
            print(f"[ERROR] cannot read {path}: {e}", file=sys.stderr)
            return 1
    maps = [np.ascontiguousarray(np.round(im.data).astype(np.uint8)) for im in images]   # (x, y, z), as case_io.load_case
    if maps[0].shape != maps[1].shape:
        print(f"[ERROR] shape mismatch: prediction {maps[0].shape}, ground truth {maps[1].shape}", file=sys.stderr)
        return 1
    import torch
    pred, gt = (torch.from_numpy(m).cuda() for m in maps)
    if args.no_surface:
        res = evaluate(pred, gt)
    else:
        res = evaluate_with_surfaces(pred, gt, images[1].zooms[:3], args.tolerance_mm, args.penalty_mm)
    if args.lesionwise:
        try:
            lesions = lesionwise_metrics(pred, gt, images[1].zooms[:3], None, args.dilation, args.min_lesion_mm3, args.lesion_penalty_mm)
        except ValueError as e:
            print(f"[ERROR] {e}", file=sys.stderr)
            return 1
        for name, m in lesions.items():
            res[name] = {**res[name], "lesionwise": m}
    print("\n".join(report_lines(res, args.pred, args.gt)))
    if args.output:
        with open(args.output, "w") as f:
            json.dump(res, f, indent=2)
        print(f"metrics written to {args.output}")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
