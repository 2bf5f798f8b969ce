"""The reference's mass-effect metrics (step 2) on the device.

``feature_extraction/step2_mass_effect.py`` takes ``np.where`` of the brain mask for its extent and the centres of mass of its two
halves (:54-99), a 15th percentile of the brain's T1 values for a CSF mask and its two halves (:179-193), 1000 + 1000 voxels drawn
by ``np.random.choice`` for a tumour-to-CSF distance (:214-232), ten dilations of the tumour for two standard deviations
(:373-393) and five sliced lobe masks (:472-518).  Here the label map and T1 stay on the device: the regions are the bits of one
flag byte per voxel, counts per index of an axis, counts inside boxes, the voxels of given ranks, the distance between two point
lists and a masked minimum are the kernels of csrc/mass_effect.hip, the percentiles come from ``masked_percentiles``, the
dilation from ``binary_dilation``, the sums from ``masked_moments`` and ``label_stats``.  Everything step 2 reports is host
arithmetic on those integers and fp64 sums, in the reference's order of operations and with its number types
(``mass_effect_from_stats``: a pure function, testable without a device).  The report prose of step 2 (``text_summary``) is out
of scope.

The sampled distance draws from numpy's generator exactly as the reference does, so under ``np.random.seed(s)`` it is the
reference's number bit for bit; ``distance='exact'`` draws nothing and returns the minimum over all pairs (a distance transform
of the CSF mask's complement, minimised over the tumour).

As a command (the reference's arguments, :755-768, and two of its own):

    python -m brats_amd.mass_effect --input CASE_DIR --segmentation SEG.nii.gz [--output JSON] [--distance sampled|exact] [--seed N]
"""
from __future__ import annotations

import sys

import numpy as np

from .case_io import StepSpec, run_step, step_main
from .percentile import masked_percentiles
from .volume_ops import (axis_counts, binary_dilation, box_counts, check_volume, distance_transform_edt_sq, flag_from_flags, flag_from_labels, masked_min,
                         masked_moments, mean_std, min_pair_dist2, select_ranked)

#: region bits of the flag map ``mass_effect_stats`` builds (one uint8 per voxel)
BRAIN, TUMOUR, CSF, DILATED, PERITUMORAL, DISTANT = range(6)
SECTIONS = ('anatomical_location', 'midline_shift', 'ventricular_compression', 'sulcal_effacement', 'herniation_risk')
STEP = 'Step 2 - Mass effect metrics'
SHIFT_NOISE_THRESHOLD_MM = 1.0                 # :29
DILATIONS, SAMPLES = 10, 1000                  # :373, :214 / :223
AXIS_MAX, MAX_BOXES, MAX_POINTS = 4096, 16, 65536   # MI355_AXIS_COUNTS_MAX, MI355_MAX_BOXES, MI355_MAX_POINTS
DISTANCES = ('sampled', 'exact')


# ---- step2_mass_effect.py:32-602 on the integers and sums -------------------------------------------------------------
def lobe_boxes(dims):
    """The sliced atlas masks of :472-517 as half-open boxes: frontal, parietal, temporal (two), occipital, deep structures."""
    d0, d1, d2 = (int(v) for v in dims)
    y = (int(d1 * 0.2), int(d1 * 0.7))
    return [(0, d0, 0, int(d1 * 0.45), int(d2 * 0.3), d2),
            (0, d0, int(d1 * 0.3), int(d1 * 0.7), int(d2 * 0.5), d2),
            (0, int(d0 * 0.35), y[0], y[1], 0, int(d2 * 0.55)),
            (int(d0 * 0.65), d0, y[0], y[1], 0, int(d2 * 0.55)),
            (0, d0, int(d1 * 0.65), d1, 0, d2),
            (int(d0 * 0.3), int(d0 * 0.7), int(d1 * 0.3), int(d1 * 0.6), int(d2 * 0.25), int(d2 * 0.6))]


def _tumour_row(label_stats):
    """count, coordinate sums, minima and maxima of ``seg > 0`` from the rows of the labels 1..4"""
    rows = label_stats[1:5]
    rows = rows[rows[:, 0] > 0]
    return np.concatenate([rows[:, :4].sum(axis=0), rows[:, 4:7].min(axis=0), rows[:, 7:10].max(axis=0)])


def _anatomical_location(n_tumour, label_stats, tumour_counts0, boxes, dims, voxel_dims):  # determine_anatomical_location, :417-602
    if n_tumour == 0:
        return {'hemisphere': 'None', 'laterality': 'N/A', 'lobes': [], 'primary_lobe': 'None', 'depth': 'No tumor detected', 'approximate_gyri': [],
                'details': 'No tumor present'}
    row = _tumour_row(label_stats)
    tumor_centroid = {k: float(np.float64(int(row[1 + i])) / int(row[0])) for i, k in enumerate('xyz')}  # utils.get_centroid: exact sums, one division
    lo, hi = [int(v) for v in row[4:7]], [int(v) for v in row[7:10]]
    tumor_bbox = {'min_x': lo[0], 'max_x': hi[0], 'min_y': lo[1], 'max_y': hi[1], 'min_z': lo[2], 'max_z': hi[2],
                  'size_x': hi[0] - lo[0] + 1, 'size_y': hi[1] - lo[1] + 1, 'size_z': hi[2] - lo[2] + 1}
    total_voxels = np.int64(n_tumour)
    midline_x = dims[0] / 2
    left_voxels = np.int64(tumour_counts0[:int(midline_x)].sum())
    right_voxels = np.int64(tumour_counts0[int(midline_x):].sum())
    if left_voxels > 0.9 * total_voxels:
        hemisphere, laterality = 'left', 'Unilateral (left hemisphere)'
    elif right_voxels > 0.9 * total_voxels:
        hemisphere, laterality = 'right', 'Unilateral (right hemisphere)'
    elif left_voxels > 0.6 * total_voxels:
        hemisphere, laterality = 'left-predominant', 'Bilateral, left-predominant'
    elif right_voxels > 0.6 * total_voxels:
        hemisphere, laterality = 'right-predominant', 'Bilateral, right-predominant'
    else:
        hemisphere, laterality = 'bilateral', 'Bilateral (crosses midline)'
    lobes, lobe_percentages, lobe_details = [], {}, {}
    b = [np.int64(v) for v in boxes]
    for name, overlap in (('frontal', b[0]), ('parietal', b[1]), ('temporal', b[2] + b[3]), ('occipital', b[4])):  # :472-510
        if overlap > 0.05 * total_voxels:
            lobes.append(name)
            pct = (overlap / total_voxels) * 100
            lobe_percentages[name] = float(pct)
            lobe_details[name] = f'{pct:.0f}% of tumor in {name} lobe'
    if b[5] > 0.1 * total_voxels:  # :513-524
        lobes.append('deep structures')
        pct = (b[5] / total_voxels) * 100
        lobe_percentages['deep_structures'] = float(pct)
        lobe_details['deep_structures'] = f'{pct:.0f}% involving deep structures (basal ganglia/thalamus)'
    if lobe_percentages:
        primary_lobe = max(lobe_percentages, key=lobe_percentages.get)
        primary_percentage = lobe_percentages[primary_lobe]
    else:
        primary_lobe, primary_percentage, lobes = 'indeterminate', 0, ['location indeterminate']
    center = np.array([dims[0] / 2, dims[1] / 2, dims[2] / 2])  # :537-542
    tumor_center = np.array([tumor_centroid['x'], tumor_centroid['y'], tumor_centroid['z']])
    distance_from_center = np.linalg.norm((tumor_center - center) * voxel_dims)
    brain_radius = min(dims) * min(voxel_dims) / 2
    relative_depth = 1 - (distance_from_center / brain_radius)
    if relative_depth > 0.7:
        depth, depth_detail = 'Deep (periventricular/central)', 'Tumor located in deep brain structures near ventricles'
    elif relative_depth > 0.4:
        depth, depth_detail = 'Subcortical', 'Tumor located in subcortical white matter'
    else:
        depth, depth_detail = 'Cortical/Superficial', 'Tumor involves cortical surface or is superficially located'
    gyri, z = [], tumor_centroid['z']  # :558-585
    if 'frontal' in lobes:
        gyri.append('superior frontal gyrus region' if z > dims[2] * 0.7 else 'middle frontal gyrus region' if z > dims[2] * 0.5
                    else 'inferior frontal gyrus region')
    if 'parietal' in lobes:
        gyri.append('superior parietal lobule region' if z > dims[2] * 0.65 else 'inferior parietal lobule region')
    if 'temporal' in lobes:
        gyri.append('superior temporal gyrus region' if z > dims[2] * 0.45 else 'middle temporal gyrus region' if z > dims[2] * 0.3
                    else 'inferior temporal gyrus region')
    if 'occipital' in lobes:
        gyri.append('occipital cortex region')
    if not gyri:
        gyri = ['gyral localization not determined']
    return {'hemisphere': hemisphere, 'laterality': laterality, 'lobes': lobes, 'lobe_percentages': lobe_percentages, 'lobe_details': lobe_details,
            'primary_lobe': primary_lobe, 'primary_lobe_percentage': float(primary_percentage) if primary_percentage else 0, 'depth': depth,
            'depth_detail': depth_detail, 'relative_depth_score': float(relative_depth), 'approximate_gyri': gyri, 'tumor_centroid': tumor_centroid,
            'tumor_bounding_box': tumor_bbox,
            'note': 'Anatomical localization estimated from standard brain atlas coordinates - clinical correlation recommended'}


def _half(counts, lo, hi):
    """(voxels, centre of mass along the axis) of the indices lo .. hi - 1 of a profile: ``ndimage.center_of_mass`` of a mask is
    an exact sum of integer coordinates divided once"""
    n = int(counts[lo:hi].sum())
    s = int((counts[lo:hi] * np.arange(lo, hi, dtype=np.int64)).sum())
    return n, (np.float64(s) / n if n else None)


def _midline_shift(n_tumour, tumour_sum0, n_brain, brain_counts0, voxel_dims):  # calculate_midline_shift, :32-156
    if n_tumour == 0:
        return {'shift_mm': 0, 'shift_direction': 'Not applicable', 'severity': 'No tumor detected',
                'clinical_significance': 'No tumor present to cause mass effect', 'is_significant': False}
    if n_brain == 0:
        return {'shift_mm': None, 'shift_direction': 'Unknown', 'severity': 'Could not calculate',
                'clinical_significance': 'Brain mask could not be determined', 'is_significant': False}
    occupied = np.flatnonzero(brain_counts0)
    brain_x_min, brain_x_max = np.int64(occupied[0]), np.int64(occupied[-1])
    anatomical_midline_x = (brain_x_min + brain_x_max) / 2
    brain_width = brain_x_max - brain_x_min
    tumor_centroid_x = np.float64(int(tumour_sum0)) / int(n_tumour)  # np.mean of integer coordinates
    tumor_side = 'left' if tumor_centroid_x < anatomical_midline_x else 'right'
    distance_to_midline = abs(tumor_centroid_x - anatomical_midline_x) * voxel_dims[0]
    midline_idx = int(anatomical_midline_x)
    n_left, left_com = _half(brain_counts0, 0, midline_idx)
    n_right, right_com = _half(brain_counts0, midline_idx, len(brain_counts0))
    if n_left > 0 and n_right > 0:
        expected_left_x = anatomical_midline_x - (brain_width / 4)
        expected_right_x = anatomical_midline_x + (brain_width / 4)
        left_shift = (left_com - expected_left_x) * voxel_dims[0]
        right_shift = (right_com - expected_right_x) * voxel_dims[0]
        estimated_shift = (left_shift + right_shift) / 2
    else:
        estimated_shift = 0
    shift_mm = abs(estimated_shift)
    is_significant = bool(shift_mm >= SHIFT_NOISE_THRESHOLD_MM)
    if estimated_shift > 0:  # :116-119, repeated for every severity
        direction = 'Left to right' if tumor_side == 'left' else 'Right to left'
    else:
        direction = 'Right to left' if tumor_side == 'left' else 'Left to right'
    if not is_significant:
        shift_direction, severity, clinical = 'Not applicable (below measurement threshold)', 'None', 'No significant midline shift detected'
    elif shift_mm < 3:
        shift_direction, severity, clinical = direction, 'Minimal', 'No significant midline shift detected'
    elif shift_mm < 5:
        shift_direction, severity, clinical = direction, 'Mild', 'Mild midline shift, close monitoring recommended'
    elif shift_mm < 10:
        shift_direction, severity, clinical = direction, 'Moderate', 'Moderate midline shift, close monitoring recommended'
    else:
        shift_direction, severity, clinical = direction, 'Severe', 'Severe midline shift, may require urgent intervention'
    return {'shift_mm': float(shift_mm), 'shift_direction': shift_direction, 'tumor_hemisphere': tumor_side, 'severity': severity,
            'clinical_significance': clinical, 'is_significant': is_significant, 'brain_midline_x': float(anatomical_midline_x),
            'tumor_centroid_x': float(tumor_centroid_x), 'distance_to_midline_mm': float(distance_to_midline),
            'measurement_threshold_mm': SHIFT_NOISE_THRESHOLD_MM, 'note': 'Estimated from tissue asymmetry - clinical correlation recommended'}


def _ventricular_compression(n_brain, csf_counts0, dims, dist2, voxel_dims):  # analyze_ventricular_compression, :159-253
    if n_brain == 0:
        return {'compression_detected': False, 'severity': 'Could not analyze', 'asymmetry_ratio': 0,
                'details': 'Could not analyze - no brain tissue detected'}
    midline_x = dims[0] // 2
    left_csf_volume = np.int64(csf_counts0[:midline_x].sum()) * np.prod(voxel_dims) / 1000
    right_csf_volume = np.int64(csf_counts0[midline_x:].sum()) * np.prod(voxel_dims) / 1000
    total_csf = left_csf_volume + right_csf_volume
    asymmetry_ratio = abs(left_csf_volume - right_csf_volume) / total_csf if total_csf > 0 else 0
    if left_csf_volume < right_csf_volume * 0.7:
        compressed_side, compression_detected = 'left', True
    elif right_csf_volume < left_csf_volume * 0.7:
        compressed_side, compression_detected = 'right', True
    else:
        compressed_side, compression_detected = 'none', False
    distance = None if dist2 is None else float(np.sqrt(np.float64(int(dist2))) * voxel_dims[0])  # :227-232: the root is monotone, min first
    severity = 'Severe' if asymmetry_ratio > 0.5 else 'Moderate' if asymmetry_ratio > 0.3 else 'Mild' if asymmetry_ratio > 0.15 else 'None/Minimal'
    return {'compression_detected': compression_detected, 'compressed_side': compressed_side, 'asymmetry_ratio': float(asymmetry_ratio),
            'left_ventricle_volume_cm3': float(left_csf_volume), 'right_ventricle_volume_cm3': float(right_csf_volume), 'severity': severity,
            'tumor_to_ventricle_distance_mm': distance, 'note': 'Based on CSF intensity analysis - MRI sequence-dependent'}


def _sulcal_effacement(n_tumour, peritumoral, distant):  # analyze_sulcal_effacement, :358-414
    if n_tumour == 0:
        return {'effacement_detected': False, 'severity': 'No tumor detected', 'details': 'No tumor detected'}
    if peritumoral[0] == 0:
        return {'effacement_detected': False, 'severity': 'Could not analyze', 'details': 'Could not analyze peritumoral region'}
    if distant[0] == 0:
        return {'effacement_detected': True, 'severity': 'Severe', 'details': 'Tumor occupies majority of brain volume'}
    peritumoral_std, distant_std = mean_std(peritumoral)[1], mean_std(distant)[1]
    variance_ratio = peritumoral_std / distant_std if distant_std > 0 else 1.0
    if variance_ratio < 0.6:
        effacement, severity = True, 'Moderate to Severe'
    elif variance_ratio < 0.8:
        effacement, severity = True, 'Mild to Moderate'
    else:
        effacement, severity = False, 'None/Minimal'
    return {'effacement_detected': effacement, 'severity': severity, 'variance_ratio': float(variance_ratio),
            'peritumoral_intensity_std': float(peritumoral_std), 'normal_brain_intensity_std': float(distant_std),
            'note': 'Based on intensity variance analysis'}


def _herniation_risk(midline, ventricular, sulcal, tumor_volume_cm3):  # assess_herniation_risk, :256-355
    risk_factors, herniation_signs = [], []
    shift_mm = midline.get('shift_mm', 0) or 0
    shift_is_significant = midline.get('is_significant', False)
    ventricular_asymmetry = ventricular.get('asymmetry_ratio', 0) or 0
    ventricular_severity = ventricular.get('severity', 'None/Minimal')
    sulcal_severity = sulcal.get('severity', 'None/Minimal')
    mass_effect_score = 0
    if shift_mm >= 10:
        mass_effect_score += 4
        risk_factors.append(f'Midline shift: {shift_mm:.1f}mm (severe)')
        herniation_signs.append('Severe midline shift (>10mm) - high subfalcine herniation risk')
    elif shift_mm >= 5:
        mass_effect_score += 3
        risk_factors.append(f'Midline shift: {shift_mm:.1f}mm (moderate)')
        herniation_signs.append('Moderate midline shift (5-10mm) - subfalcine herniation possible')
    elif shift_mm >= 3:
        mass_effect_score += 2
        risk_factors.append(f'Midline shift: {shift_mm:.1f}mm (mild)')
        herniation_signs.append('Mild midline shift (3-5mm) - early mass effect')
    elif shift_mm >= 1:
        mass_effect_score += 1
        risk_factors.append(f'Midline shift: {shift_mm:.1f}mm (minimal)')
    if ventricular_asymmetry > 0.5:
        mass_effect_score += 2
        risk_factors.append(f'Ventricular asymmetry: {ventricular_asymmetry:.2f} (severe)')
        herniation_signs.append('Severe ventricular asymmetry - significant mass effect')
    elif ventricular_asymmetry > 0.3:
        mass_effect_score += 1
        risk_factors.append(f'Ventricular asymmetry: {ventricular_asymmetry:.2f} (moderate)')
    elif ventricular_asymmetry > 0.15:
        mass_effect_score += 0.5
        risk_factors.append(f'Ventricular asymmetry: {ventricular_asymmetry:.2f} (mild)')
    if sulcal_severity in ['Moderate to Severe', 'Severe']:
        mass_effect_score += 1
        risk_factors.append(f'Sulcal effacement: {sulcal_severity}')
    elif sulcal_severity in ['Mild to Moderate']:
        mass_effect_score += 0.5
        risk_factors.append(f'Sulcal effacement: {sulcal_severity}')
    risk_level = 'High' if mass_effect_score >= 5 else 'Moderate' if mass_effect_score >= 3 else 'Mild' if mass_effect_score >= 1.5 else 'Low'
    if not herniation_signs:
        if tumor_volume_cm3 > 50:
            herniation_signs.append(f'Large tumor ({tumor_volume_cm3:.1f}cm³) without significant mass effect currently')
            herniation_signs.append('Recommend close monitoring for interval mass effect development')
        else:
            herniation_signs.append('No significant herniation risk - no measurable mass effect')
    return {'risk_level': risk_level, 'herniation_signs': herniation_signs, 'risk_factors': risk_factors, 'mass_effect_score': float(mass_effect_score),
            'mass_effect_metrics': {'midline_shift_mm': float(shift_mm), 'midline_shift_significant': shift_is_significant,
                                    'ventricular_asymmetry': float(ventricular_asymmetry), 'ventricular_severity': ventricular_severity,
                                    'sulcal_effacement_severity': sulcal_severity},
            'tumor_volume_cm3': float(tumor_volume_cm3),
            'clinical_note': 'Risk derived from measurable displacement metrics, not tumor proximity alone'}


def mass_effect_from_stats(stats, voxel_dims):
    """The five dicts of step 2 from what the device delivers.  Pure host arithmetic in float64, except where the reference
    itself works in float32: ``voxel_dims`` are the float32 zooms of the NIfTI header there, so their product (the voxel volume)
    and ``min(dims) * min(voxel_dims) / 2`` are float32.

    stats  a dict with
      shape           (d0, d1, d2)
      label_stats     int64 [K >= 5, 10], ``mi355_label_stats`` of the label map
      n_brain         voxels of the brain mask ``t1 > P5(t1[t1 > 0])``, and ``brain_counts0``, its ``axis_counts`` along axis 0
                      (read when there is a tumour and a brain)
      csf_counts0     axis-0 counts of the CSF mask ``0 < t1 < P15(t1[brain])``, tumour excluded (read when there is a brain)
      peritumoral     (n, sum, sum of squares) of T1 over ``dilated & ~tumour & brain``, ``dilated`` being the tumour after 10
                      dilations, and ``distant``, the same over ``brain & ~dilated`` (read when there is a tumour)
      tumour_counts0  axis-0 counts of ``seg > 0``, and ``box_counts``, its voxels inside the six boxes of ``lobe_boxes`` (read
                      when there is a tumour)
      dist2           the squared tumour-to-CSF distance in voxel units, or None when either set is empty
    voxel_dims  voxel sizes along axis 0, 1, 2
    """
    voxel_dims = [np.float32(v) for v in voxel_dims]
    label_stats = np.asarray(stats['label_stats'], dtype=np.int64).reshape(-1, 10)
    dims = tuple(int(v) for v in stats['shape'])
    n_tumour, n_brain = int(label_stats[1:5, 0].sum()), int(stats['n_brain'])
    tumour_sum0 = int(label_stats[1:5, 1].sum())
    location = _anatomical_location(n_tumour, label_stats, None if n_tumour == 0 else np.asarray(stats['tumour_counts0'], dtype=np.int64),
                                    stats.get('box_counts'), dims, voxel_dims)
    midline = _midline_shift(n_tumour, tumour_sum0, n_brain, None if not (n_tumour and n_brain) else np.asarray(stats['brain_counts0'], dtype=np.int64),
                             voxel_dims)
    ventricular = _ventricular_compression(n_brain, None if n_brain == 0 else np.asarray(stats['csf_counts0'], dtype=np.int64), dims, stats.get('dist2'),
                                           voxel_dims)
    sulcal = _sulcal_effacement(n_tumour, stats.get('peritumoral'), stats.get('distant'))
    tumor_volume_cm3 = np.int64(n_tumour) * np.prod(voxel_dims) / 1000  # :712-713
    return {'anatomical_location': location, 'midline_shift': midline, 'ventricular_compression': ventricular, 'sulcal_effacement': sulcal,
            'herniation_risk': _herniation_risk(midline, ventricular, sulcal, tumor_volume_cm3)}


def sample_ranks(n_tumour, n_csf, rng=None):
    """The draws of :214-225, in the reference's order and sizes: always ``choice(n_tumour, min(1000, n_tumour), replace=False)``,
    then ``choice(n_csf, 1000, replace=False)`` only when there are more than 1000 CSF voxels (all of them otherwise).  ``rng``:
    a ``numpy.random.RandomState`` or ``Generator``; None = the ``numpy.random`` module, as in the reference."""
    gen = np.random if rng is None else rng
    tumour = gen.choice(n_tumour, min(SAMPLES, n_tumour), replace=False)
    csf = gen.choice(n_csf, SAMPLES, replace=False) if n_csf > SAMPLES else np.arange(n_csf)
    return tumour, csf


def mass_effect_stats(seg, t1, rng=None, distance='sampled', ctx=None):
    """What ``mass_effect_from_stats`` reads, from a CUDA uint8 label map with the labels 0..4 and the CUDA float32 T1 volume.
    ``ctx``: the ``features.CaseContext`` of these tensors, which has the label statistics, the percentiles and the dilation."""
    import torch
    from . import components, evaluate
    if distance not in DISTANCES:
        raise ValueError(f"mass_effect: distance {distance!r} (one of {', '.join(DISTANCES)})")
    stats = {'shape': tuple(seg.shape), 'label_stats': evaluate.label_stats(seg, 8) if ctx is None else ctx.label_stats, 'n_brain': 0, 'dist2': None}
    n_tumour = int(stats['label_stats'][1:5, 0].sum())
    flags = torch.zeros_like(seg)
    if ctx is None:
        count, p5 = masked_percentiles(t1, 5, lo=0)                                      # utils.get_brain_mask, utils.py:63-68
        if count:
            flag_from_flags(flags, BRAIN, x=t1, lo=float(p5[0]))
    else:
        count = ctx.brain_into(flags, BRAIN)
    if count:                                                                            # (no positive voxel: `data > 0`, an empty mask)
        stats['brain_counts0'] = axis_counts(flags, 1 << BRAIN)[0]                       # :54-99
        stats['n_brain'] = int(stats['brain_counts0'].sum())
        if stats['n_brain'] == 0:
            raise ValueError("mass_effect: the 5th percentile of T1's positive voxels is their maximum (a plateau), so no voxel exceeds it and the brain "
                             "mask is empty although the volume is not; such a volume is not supported")
    n_csf = 0
    if n_tumour:
        flag_from_labels(seg, range(1, 256), TUMOUR, flags)
    if stats['n_brain']:
        p15 = (masked_percentiles(t1, 15, flags, require=1 << BRAIN) if ctx is None else ctx.brain_percentiles(0, 15))[1]  # :179
        flag_from_flags(flags, CSF, forbid=1 << TUMOUR, x=t1, lo=0.0, hi=float(p15[0]))  # :180-181
        stats['csf_counts0'] = axis_counts(flags, 1 << CSF)[0]                           # :186-193
        n_csf = int(stats['csf_counts0'].sum())
    if n_tumour:
        if ctx is None:
            flag_from_labels(binary_dilation(seg, DILATIONS), (1,), DILATED, flags)      # :373
        else:
            ctx.dilated_into(flags, DILATED, DILATIONS)
        flag_from_flags(flags, PERITUMORAL, require=(1 << DILATED) | (1 << BRAIN), forbid=1 << TUMOUR)  # :374
        flag_from_flags(flags, DISTANT, require=1 << BRAIN, forbid=1 << DILATED)         # :383
        m = masked_moments(t1.reshape((1,) + tuple(t1.shape)), flags)[:, 0, :]           # :392-393
        stats['peritumoral'], stats['distant'] = m[PERITUMORAL], m[DISTANT]
        stats['tumour_counts0'] = axis_counts(flags, 1 << TUMOUR)[0]                     # :447-448
        stats['box_counts'] = box_counts(flags, lobe_boxes(seg.shape), 1 << TUMOUR)      # :472-518
    if n_tumour and n_csf:                                                               # :213
        if distance == 'sampled':
            ranks_tumour, ranks_csf = sample_ranks(n_tumour, n_csf, rng)
            points_tumour = select_ranked(flags, ranks_tumour, 1 << TUMOUR)[0]
            points_csf = select_ranked(flags, ranks_csf, 1 << CSF)[0]
            stats['dist2'] = min_pair_dist2(points_tumour, points_csf, seg.shape)        # :227-232
        else:
            not_csf = components._indicator(flags, [v for v in range(256) if not v & (1 << CSF)])
            stats['dist2'] = masked_min(distance_transform_edt_sq(not_csf), flags, 1 << TUMOUR)[0]
    return stats


def mass_effect(seg, t1, voxel_dims, rng=None, distance='sampled', ctx=None):
    """seg: CUDA uint8 label map [d0, d1, d2] (1 = ncr, 2 = ed, 3 / 4 = et, nothing above 4); t1: CUDA float32 volume of that
    shape -> the dicts ``anatomical_location``, ``midline_shift``, ``ventricular_compression``, ``sulcal_effacement`` and
    ``herniation_risk`` of the reference's step 2.

    ``distance='sampled'`` measures the tumour-to-CSF distance between the voxels the reference would draw: from ``rng`` (a
    ``numpy.random.RandomState`` or ``Generator``), or from the ``numpy.random`` module's global state when ``rng`` is None - after
    ``np.random.seed(s)`` the result is the reference's under that seed.  ``distance='exact'`` takes the minimum over all pairs
    and leaves every generator alone.  ``ctx``: the ``features.CaseContext`` of these tensors (it has checked them), or None."""
    import torch
    if ctx is not None:
        if distance not in DISTANCES:
            raise ValueError(f"mass_effect: distance {distance!r} (one of {', '.join(DISTANCES)})")
        seg, (t1,) = ctx.volumes(seg, (t1,), "mass_effect")
        return mass_effect_from_stats(mass_effect_stats(seg, t1, rng, distance, ctx), voxel_dims)
    seg = check_volume(seg, torch.uint8, "mass_effect")
    t1 = check_volume(t1, torch.float32, "mass_effect")
    if t1.shape != seg.shape:
        raise ValueError("mass_effect: the volume and the label map differ in shape")
    if distance not in DISTANCES:
        raise ValueError(f"mass_effect: distance {distance!r} (one of {', '.join(DISTANCES)})")
    if int(seg.max()) > 4:
        raise ValueError("mass_effect: the label map holds values above 4 (0 = background, 1 = ncr, 2 = ed, 3 / 4 = et)")
    return mass_effect_from_stats(mass_effect_stats(seg, t1, rng, distance), voxel_dims)


# ---- the command ------------------------------------------------------------------------------------------------------
def _summary(res):
    loc, vc = res['anatomical_location'], res['ventricular_compression']
    return (f"{loc['laterality']}, {loc['primary_lobe']}; midline shift {res['midline_shift']['severity']}; ventricles {vc['severity']}; "
            f"sulci {res['sulcal_effacement']['severity']}; herniation risk {res['herniation_risk']['risk_level']}")


STEP_SPEC = StepSpec(key='step2_mass_effect', title=STEP, description='Step 2: mass effect metrics (MI355X)', modalities=('t1',), zooms='t1_float32',
                     call=lambda seg, chans, zooms, ctx=None, rng=None, distance='sampled': mass_effect(seg, chans['t1'], zooms, rng, distance, ctx=ctx),
                     summary=_summary, step_args=('rng', 'distance'))


def _distance_args(ap):
    ap.add_argument('--distance', default='sampled', choices=DISTANCES, help='tumour-to-CSF distance: between sampled voxels as the reference, or exact')
    ap.add_argument('--seed', type=int, default=None, help='seed of the generator the sampled distance draws from (default: unseeded)')
    return lambda args: {'rng': None if args.seed is None else np.random.RandomState(args.seed), 'distance': args.distance}


def analyze(input_folder, segmentation_path, output_path=None, rng=None, distance='sampled'):
    return run_step(STEP_SPEC, input_folder, segmentation_path, output_path, rng=rng, distance=distance)


def main(argv=None):
    return step_main(STEP_SPEC, argv, _distance_args)


if __name__ == '__main__':
    sys.exit(main())
