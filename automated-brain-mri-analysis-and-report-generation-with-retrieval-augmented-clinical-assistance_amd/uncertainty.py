"""Ensemble uncertainty: what the spread of the samples behind every voxel says about a segmentation.

The predictor averages, per voxel, the probabilities of every (fold, covering tile, mirror) sample of an ensemble member
(run_brats2021_inference_singlethread.py:97-128) and keeps the mean.  ``predictor.predict_folds_moments`` keeps the second moment
``m2`` beside it; from ``(mean, m2)`` of one member, or of two with equal weight, this module derives

* per-voxel maps (``maps``): ``std = sqrt(max(m2 - mean^2, 0))`` and the entropy of the mean in bits, in [0, 1] - binary per
  channel for sigmoid (region) heads, categorical over the channels divided by ``log2 K`` for softmax heads - and their maxima
  over the channels, pasted into the full volume;
* per-region numbers (``region_stats`` on the device, ``summarize`` on the host): a volume interval from the counts at the
  thresholds 0.25 / 0.5 / 0.75, the expected volume, the mean confidence and spread inside the region, and the share of it that
  is a coin toss;
* ``member_agreement``: Dice per region between the label maps of the two members.

The reference's counterpart (feature_extraction/step5_quality.py:457-500, ``calculate_measurement_confidence``) returns the
literals 'High' / 'Moderate' whatever the prediction; ``quality._measurement_confidence`` restates it and stays as it is.
``var`` is always derived AFTER the moments were resampled for export, never before: interpolation with non-negative weights
keeps ``m2 >= mean^2`` up to rounding, and the clamp takes the rounding.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

THRESHOLDS = (0.25, 0.5, 0.75)
REGION_NAMES = ("whole_tumor", "tumor_core", "enhancing_tumor")
#: columns of ``region_stats``' sums
SUM_COLUMNS = ("sum_mean", "sum_var", "sum_entropy", "sum_mean_fg", "sum_var_fg", "sum_entropy_fg", "max_var")


def _nonlin(nonlin):
    if nonlin not in ("sigmoid", "softmax"):
        raise ValueError(f"uncertainty: nonlin {nonlin!r} has no probabilities (sigmoid or softmax)")
    return {"sigmoid": _lib.NONLIN_SIGMOID, "softmax": _lib.NONLIN_SOFTMAX}[nonlin]


def _moment(t, name, shape=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise ValueError(f"uncertainty: {name} must be a CUDA fp32 [C, Z, Y, X] tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"uncertainty: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.contiguous()


def maps(mean_a, m2_a, mean_b=None, m2_b=None, nonlin="sigmoid", bbox_lo=(0, 0, 0), full_shape=None, per_channel=True):
    """``mi355_uncertainty_maps``.  Returns a dict: ``std`` and ``entropy`` ``[C, Z, Y, X]`` (``per_channel``), ``std_max`` and
    ``entropy_max`` ``[full_shape]`` - the maxima over the channels (softmax: the categorical entropy), pasted at ``bbox_lo`` into
    zeros.  With ``mean_b`` / ``m2_b`` the moments are those of the two members together: ``(a + b) / 2`` each."""
    import torch
    from .volume_ops import stream_of
    nl = _nonlin(nonlin)
    mean_a = _moment(mean_a, "mean_a")
    m2_a = _moment(m2_a, "m2_a", mean_a.shape)
    if (mean_b is None) != (m2_b is None):
        raise ValueError("uncertainty: a second member is its mean and its second moment")
    if mean_b is not None:
        if mean_b.dim() == 4 and mean_b.shape[0] != mean_a.shape[0]:
            raise ValueError(f"uncertainty: the members have {mean_a.shape[0]} and {mean_b.shape[0]} classes")
        mean_b = _moment(mean_b, "mean_b", mean_a.shape)
        m2_b = _moment(m2_b, "m2_b", mean_a.shape)
    c, z, y, x = mean_a.shape
    full = tuple(int(v) for v in full_shape) if full_shape is not None else (z, y, x)
    dev = mean_a.device
    std = torch.empty_like(mean_a) if per_channel else None
    ent = torch.empty_like(mean_a) if per_channel else None
    std_max = torch.empty(full, dtype=torch.float32, device=dev)
    ent_max = torch.empty(full, dtype=torch.float32, device=dev)
    lo = (C.c_int32 * 3)(*[int(v) for v in bbox_lo])
    fu = (C.c_int32 * 3)(*full)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().mi355_uncertainty_maps(mean_a.data_ptr(), m2_a.data_ptr(), ptr(mean_b), ptr(m2_b), c, z, y, x, nl, ptr(std), ptr(ent),
                                                  lo, fu, std_max.data_ptr(), ent_max.data_ptr(), stream_of(mean_a)), "mi355_uncertainty_maps")
    return {"std": std, "entropy": ent, "std_max": std_max, "entropy_max": ent_max}


def region_stats(mean, var, entropy, thresholds=THRESHOLDS):
    """``mi355_uncertainty_stats`` over ``[C, ...]`` CUDA fp32 tensors of one shape.  Returns ``(counts, sums)``: ``counts`` int64
    ``[C, len(thresholds) + 1]`` - ``#{mean > t}`` per threshold (strict), then the size of ``F = {mean > 0.5}`` - and ``sums``
    float64 ``[C, 7]`` (``SUM_COLUMNS``).  The sums are reproducible bit for bit from run to run."""
    import torch
    from .volume_ops import stream_of
    ts = [float(t) for t in thresholds]
    if len(ts) > 8:
        raise ValueError("uncertainty: at most 8 thresholds")
    for t, name in ((mean, "mean"), (var, "var"), (entropy, "entropy")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() < 2 or t.shape != mean.shape:
            raise ValueError(f"uncertainty: {name} must be a CUDA fp32 [C, ...] tensor of mean's shape")
    mean, var, entropy = mean.contiguous(), var.contiguous(), entropy.contiguous()
    c = int(mean.shape[0])
    n = mean.numel() // c
    counts = np.zeros((c, len(ts) + 1), dtype=np.int64)
    sums = np.zeros((c, len(SUM_COLUMNS)), dtype=np.float64)
    th = np.asarray(ts, dtype=np.float32)
    _lib.check(_lib.load().mi355_uncertainty_stats(mean.data_ptr(), var.data_ptr(), entropy.data_ptr(), c, n, _lib.fptr(th) if ts else None, len(ts),
                                                   counts.ctypes.data_as(C.POINTER(C.c_int64)), sums.ctypes.data_as(C.POINTER(C.c_double)),
                                                   stream_of(mean)), "mi355_uncertainty_stats")
    return counts, sums


def summarize(counts, sums, voxel_volume_mm3, region_names=REGION_NAMES, thresholds=THRESHOLDS):
    """The per-region JSON block from ``region_stats``' output (pure host arithmetic).  ``thresholds`` must hold 0.25, 0.5 and
    0.75: the volume is the count at 0.5, its interval ``[V(0.75), V(0.25)]``."""
    counts = np.asarray(counts, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    ts = [float(t) for t in thresholds]
    if counts.ndim != 2 or counts.shape[1] != len(ts) + 1 or sums.shape != (counts.shape[0], len(SUM_COLUMNS)):
        raise ValueError("summarize: counts [C, thresholds + 1] and sums [C, 7] expected")
    if len(region_names) != counts.shape[0]:
        raise ValueError(f"summarize: {len(region_names)} region names for {counts.shape[0]} channels")
    try:
        i25, i50, i75 = ts.index(0.25), ts.index(0.5), ts.index(0.75)
    except ValueError:
        raise ValueError("summarize: the thresholds must hold 0.25, 0.5 and 0.75") from None
    cm3 = float(voxel_volume_mm3) / 1000.0
    out = {}
    for k, name in enumerate(region_names):
        n25, n50, n75, nf = (int(counts[k, i]) for i in (i25, i50, i75, len(ts)))
        fg = lambda col: (float(sums[k, col]) / nf) if nf > 0 else None
        mean_var = fg(4)
        out[name] = {
            "voxels": n50,
            "volume_cm3": n50 * cm3,
            "volume_interval_cm3": [n75 * cm3, n25 * cm3],
            "expected_volume_cm3": float(sums[k, 0]) * cm3,
            "mean_confidence": fg(3),
            # (the root of the mean variance over the region: a spread in probability units)
            "mean_std": None if mean_var is None else float(np.sqrt(max(mean_var, 0.0))),
            "mean_entropy_bits": fg(5),
            "boundary_fraction": (n25 - n75) / max(n50, 1),
            "max_std": float(np.sqrt(max(float(sums[k, 6]), 0.0))),
        }
    return out


def member_agreement(labels_a, labels_b, order=(1, 2, 3), region_names=REGION_NAMES):
    """Dice per region between the two members' label maps (CUDA uint8, equal shape), from ``mi355_label_confusion``.  Region i
    is what ``regions_to_labels`` painted with ``order[i:]`` (the regions are nested: a later one overwrites an earlier one).
    Two empty regions agree: Dice 1."""
    from .evaluate import confusion
    order = [int(v) for v in order]
    if len(order) != len(region_names):
        raise ValueError("member_agreement: one region name per entry of order")
    k = max(order) + 2
    m = confusion(labels_a, labels_b, k)
    out = {}
    for i, name in enumerate(region_names):
        sel = np.zeros(k, dtype=bool)
        sel[order[i:]] = True
        both = int(m[np.ix_(sel, sel)].sum())
        na, nb = int(m[sel, :].sum()), int(m[:, sel].sum())
        out[name] = 1.0 if na + nb == 0 else 2.0 * both / (na + nb)
    return out
