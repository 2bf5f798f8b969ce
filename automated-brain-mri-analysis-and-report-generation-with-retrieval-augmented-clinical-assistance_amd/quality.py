"""The reference's quality control and confidence metrics (step 5) on the device.

``feature_extraction/step5_quality.py`` labels the whole tumour with 26 neighbours (:88-89), fills its holes (:103), takes five
percentiles and about a dozen boolean-mask reductions per sequence (:175-241, :320-343), measures every brain voxel's distance
from the brain's centroid (:280-300), looks for signal in four face slabs of T1 (:385-390) and runs three whole-volume Sobel
passes over a float64 copy of T1 for one coefficient of variation on the tumour's edge (:406-419).  Here the label map and the
volumes stay on the device: the regions are the bits of one flag byte per voxel, counts and sums come from
``masked_moments``, percentiles from ``masked_percentiles``, the labelling from ``label_components``, the erosion from
``binary_erosion``, and hole filling, the Sobel statistics, the radial shells and the face slabs are the kernels of
csrc/quality.hip.  Everything step 5 reports is host arithmetic on those integers and fp64 sums, in the reference's order of
operations (``quality_from_stats``: a pure function, testable without a device).  The report prose of step 5
(``text_summary``) is out of scope.

As a command (the reference's arguments, :704-717):

    python -m brats_amd.quality --input CASE_DIR --segmentation SEG.nii.gz [--output JSON]
"""
from __future__ import annotations

import sys

import numpy as np

from .case_io import StepSpec, run_step, step_main
from .percentile import masked_percentiles
from .volume_ops import (binary_erosion, binary_fill_holes, check_volume, face_slab_counts, flag_from_flags, flag_from_labels, masked_moments, mean_std,
                         radial_shell_moments, second_moments, sobel_magnitude_stats)

#: region bits of the flag map ``quality_control`` builds (one uint8 per voxel); BACKGROUND .. LOW are rewritten per sequence
BRAIN, BACKGROUND, ZERO, GHOST, HIGH, LOW, EDGE, ERODED = range(8)
SEQUENCES = ('T1', 'T1ce', 'T2', 'FLAIR')
SECTIONS = ('segmentation_quality', 'image_quality', 'artifact_detection', 'measurement_confidence', 'limitations_and_caveats')
STEP = 'Step 5 - Quality control and confidence metrics'
BOUNDARY_MARGIN, EDGE_MARGIN = 3, 5            # :113, :382
INNER_FRACTION, OUTER_FRACTION = 0.3, 0.7      # :293-294
_TINY = float(np.nextafter(0.0, 1.0))          # -_TINY < x < _TINY: x == 0


# ---- step5_quality.py:32-545 on the integers and sums -----------------------------------------------------------------
def _segmentation_quality(label_stats, num_components, filled, shape, voxel_dims):  # assess_segmentation_quality, :32-159
    issues, warnings = [], []
    quality_score = 100
    voxel_vol = np.prod(voxel_dims) / 1000
    n_wt = int(label_stats[1:5, 0].sum())
    wt_vol = np.int64(n_wt) * voxel_vol
    if wt_vol == 0:
        issues.append("No tumor segmentation detected")
        quality_score -= 50
        return {'quality_score': quality_score, 'grade': 'Poor', 'issues': issues, 'warnings': warnings,
                'recommendation': 'Manual review required - no segmentation found'}
    if wt_vol < 0.5:
        warnings.append(f"Very small tumor volume ({wt_vol:.2f} cm³) - may be artifact")
        quality_score -= 10
    if wt_vol > 300:
        warnings.append(f"Very large tumor volume ({wt_vol:.0f} cm³) - verify boundaries")
        quality_score -= 10
    # :83-85 "Tumor core volume exceeds whole tumor" cannot fire: tc is a subset of wt by get_tumor_masks (utils.py:176-177)
    if num_components > 5:
        warnings.append(f"Multiple disconnected components ({num_components}) - possible over-segmentation")
        quality_score -= 5
    # :96-100 "enhancing tumor voxels outside tumor core" cannot fire: et is a subset of tc (utils.py:175-176)
    hole_fraction = np.int64(filled) / np.int64(n_wt)
    if hole_fraction > 0.1:
        warnings.append(f"Segmentation has internal holes ({hole_fraction*100:.0f}% of volume)")
        quality_score -= 5
    at_boundary = False  # :112-127: a tumour voxel among the first or the last 3 indices of an axis
    for row in label_stats[1:5]:
        if row[0] > 0:
            at_boundary = at_boundary or any(int(row[4 + k]) < BOUNDARY_MARGIN or int(row[7 + k]) >= shape[k] - BOUNDARY_MARGIN for k in range(3))
    if at_boundary:
        warnings.append("Tumor extends to image boundary - may be truncated")
        quality_score -= 10
    if quality_score >= 90:
        grade, recommendation = 'Excellent', 'High confidence in segmentation quality'
    elif quality_score >= 75:
        grade, recommendation = 'Good', 'Acceptable quality, routine review recommended'
    elif quality_score >= 60:
        grade, recommendation = 'Fair', 'Some concerns identified, careful review advised'
    elif quality_score >= 40:
        grade, recommendation = 'Poor', 'Multiple issues detected, manual verification required'
    else:
        grade, recommendation = 'Unacceptable', 'Significant problems, re-segmentation may be needed'
    return {'quality_score': max(0, quality_score), 'grade': grade, 'issues': issues, 'warnings': warnings, 'num_components': int(num_components),
            'hole_fraction': float(hole_fraction), 'at_image_boundary': bool(at_boundary), 'recommendation': recommendation}


def _image_quality(n_brain, sequences):  # assess_image_quality, :162-258
    quality_metrics, overall_issues = {}, []
    for seq_name in SEQUENCES:
        seq_issues = []
        if n_brain == 0:
            seq_issues.append("No brain tissue detected")
            quality_metrics[seq_name] = {'snr_estimate': 0, 'issues': seq_issues, 'quality': 'Poor'}
            continue
        s = sequences[seq_name]
        signal_mean, brain_std = mean_std(s['brain'])
        if s['background'][0] > 100:
            background_std = mean_std(s['background'])[1]
            snr = signal_mean / background_std if background_std > 0 else 0
        else:
            snr = signal_mean / brain_std if brain_std > 0 else 0
        zero_fraction = np.int64(s['zeros']) / np.int64(n_brain)
        if zero_fraction > 0.01:
            seq_issues.append(f"Missing data: {zero_fraction*100:.1f}% zeros within brain")
        outlier_fraction = (np.int64(s['outliers_high']) + np.int64(s['outliers_low'])) / n_brain
        if outlier_fraction > 0.01:
            seq_issues.append(f"Intensity outliers detected ({outlier_fraction*100:.1f}%)")
        if snr > 20 and len(seq_issues) == 0:
            quality = 'Excellent'
        elif snr > 10 and len(seq_issues) <= 1:
            quality = 'Good'
        elif snr > 5:
            quality = 'Fair'
        else:
            quality = 'Poor'
        quality_metrics[seq_name] = {'snr_estimate': float(snr), 'zero_fraction': float(zero_fraction), 'outlier_fraction': float(outlier_fraction),
                                     'mean_intensity': float(signal_mean), 'std_intensity': float(brain_std), 'issues': seq_issues, 'quality': quality}
        overall_issues.extend([f"{seq_name}: {issue}" for issue in seq_issues])
    qualities = [m['quality'] for m in quality_metrics.values()]
    if all(q == 'Excellent' for q in qualities):
        overall_quality = 'Excellent'
    elif all(q in ['Excellent', 'Good'] for q in qualities):
        overall_quality = 'Good'
    elif any(q == 'Poor' for q in qualities):
        overall_quality = 'Poor'
    else:
        overall_quality = 'Fair'
    return {'sequences': quality_metrics, 'overall_quality': overall_quality, 'issues': overall_issues}


def _artifacts(n_brain, n_wt, sequences, shell, face_counts, n_edge, edge_gradient):  # detect_artifacts, :261-454
    artifacts_detected, artifact_details = [], {}
    if n_brain > 0:  # :280-315
        _, n_inner, sum_inner, n_outer, sum_outer = shell
        if n_inner > 100 and n_outer > 100:
            inner_mean, outer_mean = np.float64(sum_inner) / n_inner, np.float64(sum_outer) / n_outer
            inhomogeneity_ratio = outer_mean / inner_mean if inner_mean > 0 else 1.0
            if inhomogeneity_ratio < 0.7 or inhomogeneity_ratio > 1.4:
                artifacts_detected.append("Intensity inhomogeneity")
                artifact_details['intensity_inhomogeneity'] = {
                    'detected': True, 'severity': 'Moderate' if 0.6 < inhomogeneity_ratio < 1.6 else 'Severe', 'ratio': float(inhomogeneity_ratio),
                    'description': 'Significant signal intensity variation across the brain (bias field artifact)',
                    'impact': 'May affect intensity-based measurements'}
            else:
                artifact_details['intensity_inhomogeneity'] = {'detected': False, 'ratio': float(inhomogeneity_ratio)}
    for seq_name in SEQUENCES:  # :320-346
        ghost = sequences[seq_name]['ghost']
        if ghost[0] > 1000:
            bg_mean, bg_std = mean_std(ghost)
            cv_background = bg_std / bg_mean if bg_mean > 0 else 0
            if cv_background > 0.5:
                if 'motion_ghosting' not in artifact_details:
                    artifacts_detected.append("Possible motion artifact")
                    artifact_details['motion_ghosting'] = {
                        'detected': True, 'affected_sequences': [seq_name], 'background_cv': float(cv_background),
                        'description': 'Elevated background signal variation suggests possible motion/ghosting',
                        'impact': 'May affect tumor boundary delineation'}
                else:
                    artifact_details['motion_ghosting']['affected_sequences'].append(seq_name)
    if 'motion_ghosting' not in artifact_details:
        artifact_details['motion_ghosting'] = {'detected': False}
    # :351-376 the susceptibility block cannot fire: a brain voxel exceeds a positive threshold, so (t1 == 0) & brain is empty
    artifact_details['susceptibility'] = {'detected': False}
    edge_signal = {'x_min': face_counts[0] > 0, 'x_max': face_counts[1] > 0, 'y_min': face_counts[2] > 0, 'y_max': face_counts[3] > 0}  # :385-390
    if sum(edge_signal.values()) >= 3:
        artifacts_detected.append("Possible wrap-around")
        artifact_details['wrap_around'] = {'detected': True, 'description': 'Brain tissue extends to image boundaries - possible aliasing or tight FOV',
                                           'edges_affected': [k for k, v in edge_signal.items() if v], 'impact': 'Anatomy at edges may be compromised'}
    else:
        artifact_details['wrap_around'] = {'detected': False}
    if n_wt > 0:  # :406-434
        if n_edge > 100:
            _, mean, std = edge_gradient
            edge_cv = std / mean if mean > 0 else 0
            if edge_cv > 1.5:
                artifacts_detected.append("Possible Gibbs ringing")
                artifact_details['gibbs_ringing'] = {
                    'detected': True, 'edge_gradient_cv': float(edge_cv),
                    'description': 'High gradient variation at tumor margins, may indicate Gibbs/truncation artifact',
                    'impact': 'May affect precise tumor boundary measurement'}
            else:
                artifact_details['gibbs_ringing'] = {'detected': False}
        else:
            artifact_details['gibbs_ringing'] = {'detected': False, 'note': 'Insufficient edge for analysis'}
    else:
        artifact_details['gibbs_ringing'] = {'detected': False}
    if len(artifacts_detected) == 0:
        overall_assessment, artifact_severity = "No significant artifacts detected", "None"
    elif len(artifacts_detected) <= 2:
        overall_assessment, artifact_severity = f"Minor artifacts detected: {', '.join(artifacts_detected)}", "Mild"
    else:
        overall_assessment, artifact_severity = f"Multiple artifacts present: {', '.join(artifacts_detected)}", "Moderate to Severe"
    return {'artifacts_detected': artifacts_detected, 'artifact_count': len(artifacts_detected), 'severity': artifact_severity,
            'overall_assessment': overall_assessment, 'details': artifact_details,
            'impact_on_analysis': 'Review recommended' if len(artifacts_detected) > 1 else 'Minimal impact expected'}


def _measurement_confidence():  # calculate_measurement_confidence, :457-500
    return {'volume_measurements': {'confidence': 'High', 'note': 'Volume calculations are mathematically precise given the segmentation'},
            'enhancement_analysis': {'confidence': 'High', 'note': 'Based on objective intensity comparisons'},
            'midline_shift': {'confidence': 'Moderate', 'note': 'Estimated from tissue asymmetry; clinical correlation recommended'},
            'margin_analysis': {'confidence': 'Moderate', 'note': 'Based on intensity gradients; subjective component remains'},
            'anatomical_localization': {'confidence': 'Moderate', 'note': 'Based on standard atlas coordinates; individual variation exists'},
            'multiplicity': {'confidence': 'High', 'note': '3D connected component analysis is objective'}}


def _limitations(seg_quality, image_quality, n_et):  # identify_limitations, :503-545
    limitations = ["Automated analysis should be verified by qualified radiologist",
                   "Segmentation based on BraTS 2021 model trained on glioma cases",
                   "DWI/ADC sequences not available - diffusion characteristics not assessed",
                   "Perfusion imaging not available - cannot assess tumor vascularity"]
    caveats = []
    if n_et == 0:
        caveats.append("Non-enhancing pattern: Can be seen with lower-grade glioma, treatment effect, or other pathology; clinical and "
                       "histopathological correlation required")
    if seg_quality.get('at_image_boundary', False):
        caveats.append("Tumor at image boundary: Volume may be underestimated")
    t2_snr = image_quality.get('sequences', {}).get('T2', {}).get('snr_estimate', 10)
    if t2_snr < 6:
        caveats.append(f"Low T2 SNR ({t2_snr:.1f}): Necrosis fraction and cystic/solid classification less reliable")
    if image_quality.get('overall_quality') in ['Fair', 'Poor']:
        caveats.append("Suboptimal image quality may affect measurement accuracy")
    caveats.append("Model optimized for adult gliomas; performance may vary for other tumor types")
    caveats.append("Peritumoral edema vs infiltrating tumor cannot be distinguished on conventional MRI")
    return {'limitations': limitations, 'caveats': caveats}


def quality_from_stats(stats, voxel_dims):
    """The five dicts of step 5 from what the device delivers.  Pure host arithmetic in float64.

    stats  a dict with
      shape           (d0, d1, d2)
      label_stats     int64 [K >= 5, 10], ``mi355_label_stats`` of the label map
      num_components  26-connected components of ``seg > 0``, and ``filled``, the voxels ``binary_fill_holes`` adds to it (both
                      unused without a tumour: the reference returns before it computes them)
      n_brain         voxels of the brain mask ``t1 > P5(t1[t1 > 0])``
      sequences       per name of SEQUENCES a dict of: ``brain``, ``background`` (outside the brain, ``0 < x < P10(x[x > 0])``) and
                      ``ghost`` (outside the brain, ``x > 0``), each (n, sum, sum of squares) of that sequence; ``zeros``, the brain
                      voxels with ``x == 0``; ``outliers_high`` / ``outliers_low``, the brain voxels above ``P99 + 3 (P75 - P25)``
                      / below ``P1 - 3 (P75 - P25)`` of the brain values.  Only ``ghost`` is read when the brain is empty
      shell           ``radial_shell_moments`` of T1 over the brain about its centroid, fractions 0.3 and 0.7 (unused when the
                      brain is empty)
      face_counts     ``face_slab_counts`` of T1 with margin 5
      n_edge          voxels of ``wt & ~binary_erosion(wt, iterations=2)``, and ``edge_gradient``, ``sobel_magnitude_stats`` of T1
                      over them (read when there are more than 100)
    voxel_dims  voxel sizes along axis 0, 1, 2
    """
    voxel_dims = [float(v) for v in voxel_dims]
    label_stats = np.asarray(stats['label_stats'], dtype=np.int64).reshape(-1, 10)
    shape = tuple(int(v) for v in stats['shape'])
    n_wt, n_et, n_brain = int(label_stats[1:5, 0].sum()), int(label_stats[3:5, 0].sum()), int(stats['n_brain'])
    if n_wt > 0 and stats['n_edge'] > 100 and stats.get('edge_gradient') is None:
        raise ValueError("quality_from_stats: an edge of more than 100 voxels needs its gradient statistics")
    seg_quality = _segmentation_quality(label_stats, stats.get('num_components'), stats.get('filled'), shape, voxel_dims)
    image_quality = _image_quality(n_brain, stats['sequences'])
    return {'segmentation_quality': seg_quality,
            'image_quality': image_quality,
            'artifact_detection': _artifacts(n_brain, n_wt, stats['sequences'], stats.get('shell'), stats['face_counts'], stats.get('n_edge', 0),
                                             stats.get('edge_gradient')),
            'measurement_confidence': _measurement_confidence(),
            'limitations_and_caveats': _limitations(seg_quality, image_quality, n_et)}


def quality_stats(seg, chans, ctx=None):
    """What ``quality_from_stats`` reads, from a CUDA uint8 label map with the labels 0..4 and the four CUDA float32 volumes in
    the order of SEQUENCES.  ``ctx``: the ``features.CaseContext`` of these tensors, which has the label statistics, the tumour's
    labelling, its erosion and the percentiles."""
    import torch
    from . import components, evaluate
    t1 = chans[0]
    stats = {'shape': tuple(seg.shape), 'label_stats': evaluate.label_stats(seg, 8) if ctx is None else ctx.label_stats}
    n_wt = int(stats['label_stats'][1:5, 0].sum())
    if n_wt:
        stats['num_components'] = (components.label_components(seg, 3) if ctx is None else ctx.tumour_components)[1]  # :88-89
        stats['filled'] = binary_fill_holes(seg)[1]                                      # :103-105
    flags = torch.zeros_like(seg)
    if ctx is None:
        count, p = masked_percentiles(t1, 5, lo=0)                                       # utils.get_brain_mask, utils.py:63-68
        if count:                                                                        # (no positive voxel: `data > 0`, an empty mask)
            flag_from_flags(flags, BRAIN, x=t1, lo=float(p[0]))
    else:
        ctx.brain_into(flags, BRAIN)
    brain_moments = second_moments(flags)                                                # only the BRAIN bit is set so far
    n_brain = stats['n_brain'] = int(brain_moments[0])
    if n_wt:                                                                             # :407-409
        flag_from_labels(seg, range(1, 256), EDGE, flags)
        if ctx is None:
            flag_from_labels(binary_erosion(seg, 2), (1,), ERODED, flags)
        else:
            ctx.eroded_into(flags, ERODED, 2)
        flag_from_flags(flags, EDGE, require=1 << EDGE, forbid=1 << ERODED)
    stats['sequences'] = {}
    for c, (name, x) in enumerate(zip(SEQUENCES, chans)):
        if n_brain:
            count, p10 = masked_percentiles(x, 10, lo=0) if ctx is None else ctx.positive_percentiles(c, 10)  # :194
            if count == 0:
                raise ValueError(f"quality_control: {name} has no positive voxel (the reference takes a percentile of an empty array there)")
            flag_from_flags(flags, BACKGROUND, forbid=1 << BRAIN, x=x, lo=0.0, hi=float(p10[0]))
            flag_from_flags(flags, ZERO, require=1 << BRAIN, x=x, lo=-_TINY, hi=_TINY)   # :203
            q01, q25, q75, q99 = (np.float64(v) for v in (masked_percentiles(x, (1, 25, 75, 99), flags, require=1 << BRAIN) if ctx is None
                                                          else ctx.brain_percentiles(c, (1, 25, 75, 99)))[1])  # :210-212
            iqr = q75 - q25
            flag_from_flags(flags, HIGH, require=1 << BRAIN, x=x, lo=float(q99 + 3 * iqr))  # :214-215
            flag_from_flags(flags, LOW, require=1 << BRAIN, x=x, hi=float(q01 - 3 * iqr))
        flag_from_flags(flags, GHOST, forbid=1 << BRAIN, x=x, lo=0.0)                    # :322
        m = masked_moments(x.reshape((1,) + tuple(x.shape)), flags)[:, 0, :]
        stats['sequences'][name] = {'brain': m[BRAIN], 'background': m[BACKGROUND], 'ghost': m[GHOST], 'zeros': int(m[ZERO][0]),
                                    'outliers_high': int(m[HIGH][0]), 'outliers_low': int(m[LOW][0])}
        if name == 'T1':
            stats['n_edge'] = int(m[EDGE][0])
    if n_brain:
        centre = [np.float64(int(brain_moments[1 + k])) / n_brain for k in range(3)]     # np.mean of integer coordinates, :283
        stats['shell'] = radial_shell_moments(t1, flags, 1 << BRAIN, centre, INNER_FRACTION, OUTER_FRACTION)
    stats['face_counts'] = face_slab_counts(t1, EDGE_MARGIN)
    if n_wt and stats['n_edge'] > 100:
        stats['edge_gradient'] = sobel_magnitude_stats(t1, flags, 1 << EDGE)             # :413-419
    return stats


def quality_control(seg, t1, t1ce, t2, flair, voxel_dims, ctx=None):
    """seg: CUDA uint8 label map [d0, d1, d2] (1 = ncr, 2 = ed, 3 / 4 = et, nothing above 4); t1, t1ce, t2, flair: CUDA float32
    volumes of that shape -> the dicts ``segmentation_quality``, ``image_quality``, ``artifact_detection``,
    ``measurement_confidence`` and ``limitations_and_caveats`` of the reference's step 5.  ``ctx``: the ``features.CaseContext`` of these
    tensors (it has checked them), or None."""
    import torch
    if ctx is not None:
        seg, chans = ctx.volumes(seg, (t1, t1ce, t2, flair), "quality_control")
        return quality_from_stats(quality_stats(seg, chans, ctx), voxel_dims)
    seg = check_volume(seg, torch.uint8, "quality_control")
    chans = [check_volume(v, torch.float32, "quality_control") for v in (t1, t1ce, t2, flair)]
    if any(v.shape != seg.shape for v in chans):
        raise ValueError("quality_control: the volumes and the label map differ in shape")
    if int(seg.max()) > 4:
        raise ValueError("quality_control: the label map holds values above 4 (0 = background, 1 = ncr, 2 = ed, 3 / 4 = et)")
    return quality_from_stats(quality_stats(seg, chans), voxel_dims)


# ---- the command ------------------------------------------------------------------------------------------------------
def _summary(res):
    seg, art = res['segmentation_quality'], res['artifact_detection']
    return (f"segmentation {seg['grade']} ({seg['quality_score']}/100); image quality {res['image_quality']['overall_quality']}; "
            f"artifacts {art['severity']} ({art['artifact_count']}); {len(res['limitations_and_caveats']['caveats'])} caveats")


STEP_SPEC = StepSpec(key='step5_quality', title=STEP, description='Step 5: quality control and confidence assessment (MI355X)', voxel_info=False,
                     call=lambda seg, chans, zooms, ctx=None: quality_control(seg, chans['t1'], chans['t1ce'], chans['t2'], chans['flair'], zooms, ctx=ctx),
                     summary=_summary)


def analyze(input_folder, segmentation_path, output_path=None):
    return run_step(STEP_SPEC, input_folder, segmentation_path, output_path)


def main(argv=None):
    return step_main(STEP_SPEC, argv)


if __name__ == '__main__':
    sys.exit(main())
