"""The reference's normal-structures assessment (step 6) on the device.

``feature_extraction/step6_normal_structures.py`` finds the ventricles twice with the same arguments (:91, :214): three percentiles
over the brain, a conjunction of five masks, an opening, an 18-neighbour labelling and one whole-volume comparison per component
(:48-82).  It dilates whole volumes 5 + 10 + 10 steps (:152, :215, :345), takes two percentiles of a float64 Euclidean distance
map (:207, :224) and erodes the brain mask for a surface it never reads (:272).  Here the label map and the volumes stay on the
device: the regions are the bits of one flag byte per voxel (eleven regions, so four bits are used twice), the ventricles are
found once, the labelling is ``label_components_neighbours(mask, 18)``, one city-block distance transform of the tumour serves
its 5-step and its 10-step dilation and one of the ventricles theirs, the percentiles of the distance map are exact order
statistics of the squared distances, and every count and sum comes from two ``masked_moments`` calls.  Everything step 6
reports is host arithmetic on those integers and fp64 sums, in the reference's order of operations
(``normal_structures_from_stats``: a pure function, testable without a device).  ``voxel_info`` and the report prose of step 6
(``text_summary``) are out of scope, as in the sibling steps.

Where the reference fails, this module raises ``ValueError`` and says where:

* an empty brain mask: the reference takes percentiles of empty arrays (:48-50);
* ``cortical_mask`` is assigned only inside ``if periventricular.sum() > 0`` (:219-226) but read whenever
  ``deep_wm_mask.sum() > 100`` (:246-248).  A case without a periventricular voxel - typically: no ventricle was kept - and with
  more than 100 deep voxels makes the reference raise ``UnboundLocalError``; with at most 100 deep voxels its "could not be
  assessed" / "Could not assess" path is followed.

As a command (the reference's arguments, :506-519):

    python -m brats_amd.normal_structures --input CASE_DIR --segmentation SEG.nii.gz [--output JSON]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

from . import _lib
from .mass_effect import axis_counts
from .morphology import (_check_volume, _stream, binary_dilation, binary_erosion, case_id_and_paths, distance_transform_edt_sq, flag_from_flags,
                         flag_from_labels, masked_moments)
from .percentile import masked_percentiles, percentile_from_order_stats

#: region bits of the flag map ``normal_structures_stats`` builds (one uint8 per voxel).  VENTRICLE holds the CSF predicate until
#: the kept components replace it; the upper four bits are reduced once (T1, FLAIR) and then reused (T1, T1ce)
BRAIN, TUMOUR, VENTRICLE, NORMAL, OBSTRUCTED, PERIVENTRICULAR, CORTICAL, DEEP = range(8)
INFERIOR, FLOW_VOID, PERITUMORAL = 4, 5, 6
SECTIONS = ('ventricular_system', 'parenchyma', 'major_vessels')
STEP = 'Step 6 - Normal structures assessment'
MIN_VENTRICLE_VOXELS = 1000                    # :70-71: "1 cm3", in voxels whatever the spacing
CENTRAL_FRACTION = 0.3                         # :81
OBSTRUCTION_STEPS, PERI_STEPS = 5, 10          # :152, :215 / :345
CITYBLOCK_FAR = 1 << 30                        # MI355_CITYBLOCK_FAR
_I32_MAX = 2 ** 31 - 1


# ---- thin wrappers over the entry points ------------------------------------------------------------------------------
def cityblock_distance(mask, to_foreground=True):
    """mask: CUDA uint8 [d0, d1, d2], foreground = nonzero -> int32 map of the exact city-block (taxicab) distance.
    ``to_foreground``: to the nearest foreground voxel (0 on the mask, ``CITYBLOCK_FAR`` = 2^30 everywhere when the mask is empty);
    ``dist <= n`` is ``scipy.ndimage.binary_dilation(mask, iterations=n)``.  Otherwise: to the nearest background voxel, every
    position outside the volume being background; ``dist > n`` is ``scipy.ndimage.binary_erosion(mask, iterations=n)``."""
    import torch
    mask = _check_volume(mask, torch.uint8, "cityblock_distance")
    out = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().mi355_cityblock_distance(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2], int(bool(to_foreground)), out.data_ptr(),
                                                    _stream(mask)), "mi355_cityblock_distance")
    return out


def _check_values(values, flags, what):
    import torch
    if not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or not flags.is_cuda:
        raise ValueError(f"{what}: CUDA uint8 flags expected")
    if not isinstance(values, torch.Tensor) or values.dtype != torch.int32 or not values.is_cuda or values.shape != flags.shape:
        raise ValueError(f"{what}: CUDA int32 values of the shape of the flags expected")
    if not values.is_contiguous() or not flags.is_contiguous():
        raise ValueError(f"{what}: contiguous tensors expected")


def flag_from_i32(flags, bit, values, lo=0, hi=_I32_MAX, require=0, forbid=0):
    """Bit ``bit`` of ``flags`` (in place) = all bits of the mask ``require`` set, none of ``forbid``, and ``lo <= values <= hi``
    (int32 map of the shape of the flags; bounds beyond int32 are clamped, an empty range clears the bit)."""
    _check_values(values, flags, "flag_from_i32")
    lo, hi = max(int(lo), -_I32_MAX - 1), min(int(hi), _I32_MAX)
    if lo > hi:
        lo, hi = 1, 0
    _lib.check(_lib.load().mi355_flag_from_i32(flags.data_ptr(), int(bit), int(require), int(forbid), values.data_ptr(), lo, hi, flags.numel(), _stream(flags)),
               "mi355_flag_from_i32")
    return flags


def flag_from_box(flags, bit, box, require=0, forbid=0):
    """Bit ``bit`` of ``flags`` [d0, d1, d2] (in place) = all bits of ``require`` set, none of ``forbid``, and the voxel inside the
    half-open index box ``(lo0, hi0, lo1, hi1, lo2, hi2)``, clipped to the volume."""
    import torch
    if not flags.is_contiguous():
        raise ValueError("flag_from_box: contiguous flags expected")
    _check_volume(flags, torch.uint8, "flag_from_box")
    b = np.ascontiguousarray(np.clip(np.asarray(box, dtype=np.int64).reshape(6), -_I32_MAX, _I32_MAX).astype(np.int32))
    _lib.check(_lib.load().mi355_flag_from_box(flags.data_ptr(), int(bit), int(require), int(forbid), flags.shape[0], flags.shape[1], flags.shape[2],
                                               b.ctypes.data_as(_lib.c_int32_p), _stream(flags)), "mi355_flag_from_box")
    return flags


def masked_order_stats_i32(values, qs, flags=None, require=0, forbid=0):
    """values: CUDA int32 tensor with nothing below 0; flags: CUDA uint8 tensor of its shape or None.  Returns ``(count, below,
    above)``: the number of selected voxels and per percentile the two int32 order statistics that bracket it (ranks ``floor(v)``
    and ``min(floor(v) + 1, count - 1)``, ``v = (count - 1) * q / 100``); zeros when nothing is selected."""
    import torch
    if not isinstance(values, torch.Tensor) or values.dtype != torch.int32 or not values.is_cuda:
        raise ValueError("masked_order_stats_i32: CUDA int32 tensor expected")
    if flags is not None and (not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or not flags.is_cuda or flags.shape != values.shape):
        raise ValueError("masked_order_stats_i32: CUDA uint8 flags of the shape of the values expected")
    values = values.contiguous()
    flags = None if flags is None else flags.contiguous()
    q = np.ascontiguousarray(np.atleast_1d(np.asarray(qs, dtype=np.float64)))
    count = C.c_int64(0)
    below, above = np.zeros(q.size, dtype=np.int32), np.zeros(q.size, dtype=np.int32)
    _lib.check(_lib.load().mi355_masked_order_stats_i32(values.data_ptr(), values.numel(), None if flags is None else flags.data_ptr(), int(require), int(forbid),
                                                        q.ctypes.data_as(C.POINTER(C.c_double)), q.size, C.byref(count), below.ctypes.data_as(_lib.c_int32_p),
                                                        above.ctypes.data_as(_lib.c_int32_p), _stream(values)), "mi355_masked_order_stats_i32")
    return int(count.value), below, above


def column_count_max(flags, i1_from, require=0, forbid=0):
    """``np.max(np.sum(selected[:, i1_from:, :], axis=0))`` of the voxels of ``flags`` [d0, d1, d2] with every bit of ``require`` and
    no bit of ``forbid``; 0 when that slab selects nothing."""
    import torch
    flags = _check_volume(flags, torch.uint8, "column_count_max")
    out = C.c_int64(0)
    _lib.check(_lib.load().mi355_column_count_max(flags.data_ptr(), int(require), int(forbid), flags.shape[0], flags.shape[1], flags.shape[2], int(i1_from),
                                                  C.byref(out), _stream(flags)), "mi355_column_count_max")
    return int(out.value)


# ---- pure host helpers ------------------------------------------------------------------------------------------------
def sqrt_bounds(threshold):
    """For a float64 ``threshold >= 0``: ``(k_le, k_ge)``, the largest integer with ``np.sqrt(k) <= threshold`` and the smallest
    with ``np.sqrt(k) >= threshold``.  For integers d2, ``np.sqrt(d2) > threshold`` is ``d2 > k_le`` and ``np.sqrt(d2) < threshold``
    is ``d2 < k_ge``: the comparisons of a Euclidean distance map with a float become integer bounds on the squared distances."""
    t = np.float64(threshold)
    if not t >= 0 or np.isinf(t):
        raise ValueError(f"sqrt_bounds: threshold {threshold!r} (a finite float, 0 or more)")
    k = int(np.floor(t * t))  # off by the rounding of the product at most: corrected by testing np.sqrt itself
    while k > 0 and np.sqrt(np.float64(k)) > t:
        k -= 1
    while np.sqrt(np.float64(k + 1)) <= t:
        k += 1
    return k, (k if np.sqrt(np.float64(k)) == t else k + 1)


def coordinate_percentile(counts, q):
    """``np.percentile(np.where(mask)[axis], q)`` from ``counts``, the number of mask voxels at each index of that axis: the two
    order statistics are read off the cumulative histogram.  None for an empty mask."""
    cum = np.cumsum(np.asarray(counts, dtype=np.int64))
    n = int(cum[-1]) if cum.size else 0
    if n == 0:
        return None
    r = int(np.floor((n - 1) * np.true_divide(np.float64(q), 100)))
    below, above = (int(np.searchsorted(cum, k, side='right')) for k in (r, min(r + 1, n - 1)))
    return np.float64(percentile_from_order_stats(n, q, below, above))


def _mean(n, total):
    """``values.mean()`` of n integer-valued float64: an exact sum divided once; NaN for no value, as numpy"""
    return np.float64(total) / np.int64(n) if n else np.float64('nan')


# ---- step6_normal_structures.py:87-386 on the integers and sums -------------------------------------------------------
def _ventricular_system(s, dims, voxel_dims):  # analyze_ventricular_system, :87-185
    voxel_vol = np.prod(voxel_dims) / 1000
    n_vent = int(s['n_ventricle'])
    total_volume = np.int64(n_vent) * voxel_vol
    brain_volume = np.int64(s['n_normal']) * voxel_vol
    vbr = (total_volume / brain_volume * 100) if brain_volume > 0 else 0
    left_vol = np.int64(s['n_ventricle_left']) * voxel_vol
    right_vol = np.int64(s['n_ventricle_right']) * voxel_vol
    asymmetry = abs(left_vol - right_vol) / (left_vol + right_vol) if left_vol + right_vol > 0 else 0
    larger_side = 'left' if left_vol > right_vol else 'right' if right_vol > left_vol else 'symmetric'
    if n_vent > 0:
        evans_index = (np.int64(s['frontal_width']) * voxel_dims[0]) / (dims[0] * voxel_dims[0])
    else:
        evans_index = 0
    if evans_index > 0.3 and vbr > 5:
        hydrocephalus, hydrocephalus_type = True, "Communicating hydrocephalus suggested"
    elif vbr > 7:
        hydrocephalus, hydrocephalus_type = True, "Ventriculomegaly noted"
    else:
        hydrocephalus, hydrocephalus_type = False, "No hydrocephalus"
    obstruction_risk = np.int64(s['n_obstructed']) / np.int64(n_vent) if n_vent > 0 else 0
    if vbr < 2:
        size_assessment, size_note = "Normal", "Ventricles within normal size limits"
    elif vbr < 4:
        size_assessment, size_note = "Mildly prominent", "Mild prominence of ventricular system"
    elif vbr < 6:
        size_assessment, size_note = "Moderately dilated", "Moderate ventricular enlargement"
    else:
        size_assessment, size_note = "Markedly dilated", "Marked ventriculomegaly"
    return {'total_volume_cm3': float(total_volume), 'left_volume_cm3': float(left_vol), 'right_volume_cm3': float(right_vol),
            'ventricle_brain_ratio_percent': float(vbr), 'asymmetry_index': float(asymmetry), 'larger_side': larger_side,
            'evans_index_estimate': float(evans_index), 'size_assessment': size_assessment, 'size_note': size_note, 'hydrocephalus_present': hydrocephalus,
            'hydrocephalus_type': hydrocephalus_type, 'obstruction_risk': float(obstruction_risk),
            'obstruction_note': 'Tumor adjacent to ventricular system' if obstruction_risk > 0.1 else 'No direct ventricular involvement',
            'symmetry_assessment': 'Symmetric' if asymmetry < 0.15 else f'Asymmetric ({larger_side} larger)'}


def _parenchyma(s, voxel_dims):  # analyze_parenchyma, :188-289
    if s['n_normal'] == 0:
        return {'assessment': 'Unable to assess', 'note': 'Insufficient normal brain tissue for analysis'}
    voxel_vol = np.prod(voxel_dims) / 1000
    n_pv, n_deep = int(s['periventricular'][0]), int(s['deep'][0])
    if n_pv == 0 and n_deep > 100:
        raise ValueError(f"normal_structures: no periventricular voxel (no ventricle was kept, or the tumour covers their surroundings) and {n_deep} deep "
                         "white-matter voxels: the reference reads its cortical mask (step6_normal_structures.py:248) without having assigned it (:224) and "
                         "raises UnboundLocalError")
    n_cortical = int(s['cortical'][0]) if n_pv > 0 else 0
    if n_pv > 0:
        pv_flair_mean = _mean(n_pv, s['periventricular'][1])
        cortical_flair_mean = _mean(n_cortical, s['cortical'][1])
        pv_hyperintensity_ratio = pv_flair_mean / cortical_flair_mean if cortical_flair_mean > 0 else 1.0
        if pv_hyperintensity_ratio > 1.3:
            wm_disease = True
            wm_description = "FLAIR hyperintensities in periventricular white matter, may represent chronic small vessel disease"
        elif pv_hyperintensity_ratio > 1.15:
            wm_disease, wm_description = True, "Mild periventricular FLAIR signal changes"
        else:
            wm_disease, wm_description = False, "No significant periventricular white matter changes"
    else:
        pv_hyperintensity_ratio, wm_disease, wm_description = 1.0, False, "Periventricular region could not be assessed"
    if n_deep > 100:
        deep_wm_t1 = _mean(n_deep, s['deep'][1])
        cortical_t1 = _mean(n_cortical, s['cortical'][2]) if n_cortical > 100 else deep_wm_t1
        gw_ratio = deep_wm_t1 / cortical_t1 if cortical_t1 > 0 else 1.0
        if gw_ratio > 1.1:
            gw_differentiation, gw_note = "Preserved", "Normal gray-white matter differentiation"
        elif gw_ratio > 1.0:
            gw_differentiation, gw_note = "Mildly reduced", "Slightly reduced gray-white differentiation"
        else:
            gw_differentiation, gw_note = "Reduced", "Loss of gray-white differentiation (may indicate edema or diffuse pathology)"
    else:
        gw_differentiation, gw_ratio, gw_note = "Could not assess", 1.0, "Insufficient tissue for gray-white analysis"
    brain_volume = np.int64(s['n_brain']) * voxel_vol
    normal_brain_volume = np.int64(s['n_normal']) * voxel_vol
    return {'normal_brain_volume_cm3': float(normal_brain_volume), 'total_brain_volume_cm3': float(brain_volume),
            'periventricular_assessment': {'hyperintensity_ratio': float(pv_hyperintensity_ratio), 'white_matter_disease_present': wm_disease,
                                           'description': wm_description},
            'gray_white_differentiation': {'assessment': gw_differentiation, 'ratio': float(gw_ratio), 'note': gw_note},
            'overall_assessment': 'Normal' if not wm_disease and gw_differentiation == 'Preserved' else 'Abnormal findings present',
            'atrophy_assessment': 'Not formally assessed (requires age-matched normative data)'}


def _major_vessels(s, voxel_dims):  # analyze_major_vessels, :292-386 (T1ce is always there)
    n_inferior = int(s['n_inferior'])
    if n_inferior > 0:
        n_void = np.int64(s['n_flow_void'])
        flow_void_volume = n_void * np.prod(voxel_dims) / 1000
        flow_void_fraction = n_void / np.int64(n_inferior)
        if 0.001 < flow_void_fraction < 0.05:
            flow_void_assessment, flow_void_note = "Present", "Flow voids identified in expected vessel locations"
        elif flow_void_fraction < 0.001:
            flow_void_assessment = "Not well visualized"
            flow_void_note = "Major vessel flow voids not clearly identified (may be normal variant or sequence-dependent)"
        else:
            flow_void_assessment = "Prominent"
            flow_void_note = "Prominent dark signal in basal regions (may include vessels and air-bone interfaces)"
    else:
        flow_void_assessment, flow_void_note, flow_void_volume = "Could not assess", "Insufficient inferior brain for vessel assessment", 0
    n_peri = int(s['peritumoral'][0])
    if n_peri > 0:
        peritumoral_t1, peritumoral_t1ce = _mean(n_peri, s['peritumoral'][1]), _mean(n_peri, s['peritumoral'][2])
        peritumoral_enhancement_ratio = peritumoral_t1ce / peritumoral_t1 if peritumoral_t1 > 0 else 1.0
        if peritumoral_enhancement_ratio > 1.5:
            vascular_involvement, vascular_note = "Possible", "Enhancement in peritumoral region may indicate vascular involvement"
        else:
            vascular_involvement, vascular_note = "Not evident", "No obvious vascular encasement or involvement"
    else:
        vascular_involvement, vascular_note, peritumoral_enhancement_ratio = "Could not assess", "Insufficient peritumoral tissue", 1.0
    return {'flow_voids': {'assessment': flow_void_assessment, 'note': flow_void_note, 'volume_cm3': float(flow_void_volume)},
            'vascular_involvement': {'assessment': vascular_involvement, 'note': vascular_note,
                                     'peritumoral_enhancement_ratio': float(peritumoral_enhancement_ratio)},
            'limitations': ["Detailed vascular assessment requires MRA/MRV sequences", "Flow void analysis is limited on standard structural MRI",
                            "Cannot assess vessel patency or flow direction"],
            'overall_assessment': 'Limited assessment on structural sequences'}


def normal_structures_from_stats(stats, voxel_dims):
    """The three dicts of step 6 from what the device delivers.  Pure host arithmetic in float64.

    stats  a dict with
      shape              (d0, d1, d2)
      n_brain            voxels of the brain mask ``t1 > P5(t1[t1 > 0])``; 0 raises (nothing else is read then)
      n_normal           voxels of ``brain & ~tumour``
      n_ventricle        voxels of the ventricle mask of :33-84, ``n_ventricle_left`` / ``n_ventricle_right`` those with an axis-0 index
                         below / from ``d0 // 2`` on, ``frontal_width`` = ``np.max(np.sum(ventricle[:, int(frontal_y):, :], axis=0))``
                         with ``frontal_y`` the 75th percentile of their axis-1 indices (read when there is a ventricle voxel), and
                         ``n_obstructed``, those within 5 dilations of the tumour
      periventricular    (n, sum of FLAIR) over ``normal & ~ventricle`` within 10 dilations of the ventricles
      cortical           (n, sum of FLAIR, sum of T1) over the normal voxels whose distance to the brain's background lies below its
                         40th percentile over the brain (read when there is a periventricular voxel), and ``deep``, (n, sum of T1)
                         over those above the 60th
      n_inferior         brain voxels in ``[:, :, :d2 // 3]``, ``n_flow_void`` those outside the tumour with T1 below its 5th
                         percentile over them
      peritumoral        (n, sum of T1, sum of T1ce) over ``brain & ~tumour`` within 10 dilations of the tumour
    voxel_dims  voxel sizes along axis 0, 1, 2
    """
    voxel_dims = [float(v) for v in voxel_dims]
    dims = tuple(int(v) for v in stats['shape'])
    if int(stats['n_brain']) == 0:
        raise ValueError("normal_structures: the brain mask t1 > P5(t1[t1 > 0]) is empty (the reference takes percentiles of empty arrays there, "
                         "step6_normal_structures.py:48-50)")
    return {'ventricular_system': _ventricular_system(stats, dims, voxel_dims), 'parenchyma': _parenchyma(stats, voxel_dims),
            'major_vessels': _major_vessels(stats, voxel_dims)}


def keep_ventricles(component_stats, d0):
    """The keep-rule of :70-82 on the rows of ``component_stats``: more than 1000 voxels (whatever the spacing) and the mean
    axis-0 index within ``0.3 d0`` of ``d0 / 2``.  Returns n + 1 booleans, [0] for the background."""
    from .components import COUNT, SUM0
    keep = [False]
    for row in component_stats:
        n = int(row[COUNT])
        keep.append(bool(n > MIN_VENTRICLE_VOXELS and abs(np.float64(int(row[SUM0])) / n - d0 / 2) < d0 * CENTRAL_FRACTION))
    return keep


def normal_structures_stats(seg, chans, ctx=None):
    """What ``normal_structures_from_stats`` reads, from a CUDA uint8 label map with the labels 0..4 and the four CUDA float32
    volumes T1, T1ce, T2, FLAIR.  ``ctx``: the ``features.CaseContext`` of these tensors, which has the brain's percentiles and the
    tumour's distance transform."""
    import torch
    from . import components
    t1, t1ce, t2, flair = chans
    d0, d1, d2 = seg.shape
    stats = {'shape': (d0, d1, d2), 'n_brain': 0}
    flags = torch.zeros_like(seg)
    if ctx is None:
        count, p5 = masked_percentiles(t1, 5, lo=0)                                      # utils.get_brain_mask, utils.py:63-68
        if count == 0:
            return stats
        flag_from_flags(flags, BRAIN, x=t1, lo=float(p5[0]))
    elif not ctx.brain_into(flags, BRAIN):
        return stats
    flag_from_labels(seg, range(1, 256), TUMOUR, flags)                                  # utils.py:177
    flag_from_flags(flags, NORMAL, require=1 << BRAIN, forbid=1 << TUMOUR)               # :101, :193
    # identify_ventricles, :33-84, once
    brain = 1 << BRAIN
    n_brain, p15 = masked_percentiles(t1, 15, flags, require=brain) if ctx is None else ctx.brain_percentiles(0, 15)  # :48-50
    if n_brain == 0:
        return stats
    if ctx is None:
        p85, p25 = masked_percentiles(t2, 85, flags, require=brain)[1], masked_percentiles(flair, 25, flags, require=brain)[1]
    else:
        p85, p25 = ctx.brain_percentiles(2, 85)[1], ctx.brain_percentiles(3, 25)[1]
    flag_from_flags(flags, VENTRICLE, require=1 << NORMAL, x=t1, hi=float(p15[0]))       # :53-59
    flag_from_flags(flags, VENTRICLE, require=1 << VENTRICLE, x=t2, lo=float(p85[0]))
    flag_from_flags(flags, VENTRICLE, require=1 << VENTRICLE, x=flair, hi=float(p25[0]))
    csf = components._indicator(flags, [v for v in range(256) if v & (1 << VENTRICLE)])
    csf = binary_dilation(binary_erosion(csf, 1), 1)                                     # :62-63
    labels, n = components.label_components_neighbours(csf, 18)                          # :66-67
    if n > components.MAX_COMPONENTS:
        raise ValueError(f"normal_structures: the CSF mask falls into {n} components, the statistics table holds {components.MAX_COMPONENTS}")
    keep = keep_ventricles(components.component_stats(labels, n), d0)                    # :73-82
    flag_from_labels(components.component_filter(labels, csf, keep), (1,), VENTRICLE, flags)
    counts0, counts1, _ = axis_counts(flags, 1 << VENTRICLE)
    n_vent = int(counts0.sum())
    stats.update(n_ventricle=n_vent, n_ventricle_left=int(counts0[:d0 // 2].sum()), n_ventricle_right=int(counts0[d0 // 2:].sum()))  # :107-112
    if n_vent:
        frontal_y = coordinate_percentile(counts1, 75)                                   # :127-131
        stats['frontal_width'] = column_count_max(flags, int(frontal_y), 1 << VENTRICLE)
    # one transform of the tumour for :152 and :345, one of the ventricles for :215
    tumour_dist = cityblock_distance(seg, True) if ctx is None else ctx.tumour_distance
    flag_from_i32(flags, OBSTRUCTED, tumour_dist, 0, OBSTRUCTION_STEPS, require=1 << VENTRICLE)                       # :152-153
    flag_from_i32(flags, PERIVENTRICULAR, cityblock_distance(components._indicator(flags, [v for v in range(256) if v & (1 << VENTRICLE)]), True), 0,
                  PERI_STEPS, require=1 << NORMAL, forbid=1 << VENTRICLE)                                             # :215-216
    dist2 = distance_transform_edt_sq(components._indicator(flags, [v for v in range(256) if v & brain]))             # :206
    _, below, above = masked_order_stats_i32(dist2, (60, 40), flags, require=brain)                                   # :207, :224
    deep_threshold, cortical_threshold = percentile_from_order_stats(n_brain, (60, 40), np.sqrt(below.astype(np.float64)), np.sqrt(above.astype(np.float64)))
    flag_from_i32(flags, DEEP, dist2, sqrt_bounds(deep_threshold)[0] + 1, _I32_MAX, require=1 << NORMAL)              # :210
    flag_from_i32(flags, CORTICAL, dist2, 0, sqrt_bounds(cortical_threshold)[1] - 1, require=1 << NORMAL)             # :224
    m = masked_moments(torch.stack((t1, flair)), flags)
    stats.update(n_brain=int(m[BRAIN][0][0]), n_normal=int(m[NORMAL][0][0]), n_obstructed=int(m[OBSTRUCTED][0][0]),
                 periventricular=(int(m[PERIVENTRICULAR][0][0]), m[PERIVENTRICULAR][1][1]),
                 cortical=(int(m[CORTICAL][0][0]), m[CORTICAL][1][1], m[CORTICAL][0][1]), deep=(int(m[DEEP][0][0]), m[DEEP][0][1]))
    # the upper bits again: the inferior third, its flow voids, the tumour's surroundings
    flag_from_box(flags, INFERIOR, (0, d0, 0, d1, 0, d2 // 3), require=brain)                                         # :306-308
    n_inferior, p5_inferior = masked_percentiles(t1, 5, flags, require=1 << INFERIOR)                                 # :312-313
    flag_from_flags(flags, FLOW_VOID, require=1 << INFERIOR, forbid=1 << TUMOUR, x=t1,
                    hi=float(p5_inferior[0]) if n_inferior else 0.0)                                                  # :315-319 (no inferior brain: cleared)
    flag_from_i32(flags, PERITUMORAL, tumour_dist, 0, PERI_STEPS, require=1 << NORMAL)                                # :345-346
    m = masked_moments(torch.stack((t1, t1ce)), flags)
    stats.update(n_inferior=int(m[INFERIOR][0][0]), n_flow_void=int(m[FLOW_VOID][0][0]),
                 peritumoral=(int(m[PERITUMORAL][0][0]), m[PERITUMORAL][0][1], m[PERITUMORAL][1][1]))
    return stats


def normal_structures(seg, t1, t1ce, t2, flair, voxel_dims, ctx=None):
    """seg: CUDA uint8 label map [d0, d1, d2] (1 = ncr, 2 = ed, 3 / 4 = et, nothing above 4); t1, t1ce, t2, flair: CUDA float32
    volumes of that shape -> the dicts ``ventricular_system``, ``parenchyma`` and ``major_vessels`` of the reference's step 6.
    ``ctx``: the ``features.CaseContext`` of these tensors (it has checked them), or None."""
    import torch
    if ctx is not None:
        seg, chans = ctx.volumes(seg, (t1, t1ce, t2, flair), "normal_structures")
        return normal_structures_from_stats(normal_structures_stats(seg, chans, ctx), voxel_dims)
    seg = _check_volume(seg, torch.uint8, "normal_structures")
    chans = [_check_volume(v, torch.float32, "normal_structures") for v in (t1, t1ce, t2, flair)]
    if any(v.shape != seg.shape for v in chans):
        raise ValueError("normal_structures: the volumes and the label map differ in shape")
    if int(seg.max()) > 4:
        raise ValueError("normal_structures: the label map holds values above 4 (0 = background, 1 = ncr, 2 = ed, 3 / 4 = et)")
    return normal_structures_from_stats(normal_structures_stats(seg, chans), voxel_dims)


# ---- the command ------------------------------------------------------------------------------------------------------
def analyze(input_folder, segmentation_path, output_path=None):
    import torch
    from . import nifti
    case_id, paths = case_id_and_paths(input_folder)
    images = {k: nifti.load(p) for k, p in paths.items()}
    seg = np.ascontiguousarray(np.round(nifti.load(segmentation_path).data).astype(np.uint8))  # :443-444
    zooms = [float(v) for v in images['t1'].zooms]
    dev = [torch.from_numpy(np.ascontiguousarray(images[k].data.astype(np.float32))).cuda() for k in ('t1', 't1ce', 't2', 'flair')]
    res = {'case_id': case_id, 'step': STEP}
    res.update(normal_structures(torch.from_numpy(seg).cuda(), *dev, zooms))
    if output_path:
        Path(output_path).parent.mkdir(parents=True, exist_ok=True)
        with open(output_path, 'w') as f:
            json.dump(res, f, indent=2)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description='Step 6: normal structures assessment (MI355X)')
    ap.add_argument('--input', required=True, help='Input folder containing MRI sequences')
    ap.add_argument('--segmentation', required=True, help='Path to segmentation mask (NIfTI)')
    ap.add_argument('--output', default=None, help='Output path for JSON results')
    args = ap.parse_args(argv)
    res = analyze(args.input, args.segmentation, args.output)
    vent, par, ves = (res[k] for k in SECTIONS)
    print(f"{res['case_id']}: ventricles {vent['size_assessment']} (VBR {vent['ventricle_brain_ratio_percent']:.1f}%), {vent['hydrocephalus_type']}; "
          f"parenchyma {par.get('overall_assessment', par.get('assessment'))}; flow voids {ves['flow_voids']['assessment']}; "
          f"vascular involvement {ves['vascular_involvement']['assessment']}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
