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

import sys

import numpy as np

from .case_io import StepSpec, run_step, step_main
from .percentile import masked_percentiles, percentile_from_order_stats
from .volume_ops import (axis_counts, binary_dilation, binary_erosion, check_volume, cityblock_distance, column_count_max, distance_transform_edt_sq,
                         flag_from_box, flag_from_flags, flag_from_i32, flag_from_labels, masked_moments, masked_order_stats_i32)

#: region bits of the flag map ``normal_structures_stats`` builds (one uint8 per voxel).  VENTRICLE holds the CSF predicate until
#: the kept components replace it; the upper four bits are reduced once (T1, FLAIR) and then reused (T1, T1ce)
BRAIN, TUMOUR, VENTRICLE, NORMAL, OBSTRUCTED, PERIVENTRICULAR, CORTICAL, DEEP = range(8)
INFERIOR, FLOW_VOID, PERITUMORAL = 4, 5, 6
SECTIONS = ('ventricular_system', 'parenchyma', 'major_vessels')
STEP = 'Step 6 - Normal structures assessment'
MIN_VENTRICLE_VOXELS = 1000                    # :70-71: "1 cm3", in voxels whatever the spacing
CENTRAL_FRACTION = 0.3                         # :81
OBSTRUCTION_STEPS, PERI_STEPS = 5, 10          # :152, :215 / :345


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
    flag_from_i32(flags, DEEP, dist2, sqrt_bounds(deep_threshold)[0] + 1, require=1 << NORMAL)                        # :210
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
    seg = check_volume(seg, torch.uint8, "normal_structures")
    chans = [check_volume(v, torch.float32, "normal_structures") for v in (t1, t1ce, t2, flair)]
    if any(v.shape != seg.shape for v in chans):
        raise ValueError("normal_structures: the volumes and the label map differ in shape")
    if int(seg.max()) > 4:
        raise ValueError("normal_structures: the label map holds values above 4 (0 = background, 1 = ncr, 2 = ed, 3 / 4 = et)")
    return normal_structures_from_stats(normal_structures_stats(seg, chans), voxel_dims)


# ---- the command ------------------------------------------------------------------------------------------------------
def _summary(res):
    vent, par, ves = (res[k] for k in SECTIONS)
    return (f"ventricles {vent['size_assessment']} (VBR {vent['ventricle_brain_ratio_percent']:.1f}%), {vent['hydrocephalus_type']}; "
            f"parenchyma {par.get('overall_assessment', par.get('assessment'))}; flow voids {ves['flow_voids']['assessment']}; "
            f"vascular involvement {ves['vascular_involvement']['assessment']}")


STEP_SPEC = StepSpec(key='step6_normal_structures', title=STEP, description='Step 6: normal structures assessment (MI355X)', voxel_info=False,
                     call=lambda seg, chans, zooms, ctx=None: normal_structures(seg, chans['t1'], chans['t1ce'], chans['t2'], chans['flair'], zooms, ctx=ctx),
                     summary=_summary)


def analyze(input_folder, segmentation_path, output_path=None):
    return run_step(STEP_SPEC, input_folder, segmentation_path, output_path)


def main(argv=None):
    return step_main(STEP_SPEC, argv)


if __name__ == '__main__':
    sys.exit(main())
