"""GPU mirror of the reference evaluator and label converter.

``evaluate_segmentation.py`` builds float masks and sums them four times per label; here one
pass over the two uint8 label maps on the device yields the K x K confusion counts, and every
metric of ``calculate_metrics`` (:12-49) / ``calculate_metrics_binary`` (:181-195) and the compound
WT / TC / ET regions (:129-162) is derived from those integers with the reference's formulas
(same 1e-8 epsilons).  ``convert_labels`` is convert_labels_to_brats.py:34-55 as a 256-entry map.
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
    if allocate is None:
        def allocate(numel, dtype):
            return torch.empty(numel, dtype=dtype, device=pred.device)
    pred, gt = pred.contiguous(), gt.contiguous()
    lib = _lib.load()
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    d0, d1, d2 = (int(v) for v in pred.shape)
    u8p, i32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    table = _region_table(regions)
    flags = allocate(pred.numel(), torch.uint8)
    _lib.check(lib.mi355_region_surfaces(pred.data_ptr(), gt.data_ptr(), d0, d1, d2, table.ctypes.data_as(u8p), table.ctypes.data_as(u8p),
                                         flags.data_ptr(), flags.numel(), stream), "mi355_region_surfaces")
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
    print("\n".join(report_lines(res, args.pred, args.gt)))
    if args.output:
        with open(args.output, "w") as f:
            json.dump(res, f, indent=2)
        print(f"metrics written to {args.output}")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
