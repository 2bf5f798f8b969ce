"""The reference's sequence-specific findings (step 1) on the device.

``feature_extraction/step1_sequence_findings.py`` indexes the four modalities with the boolean masks of the three tumour labels
and of the "normal brain" (``utils.get_normal_brain_stats``, utils.py:54-60: brighter than the 5th percentile of the nonzero
voxels of that modality, outside the tumour), takes mean and standard deviation of each, dilates the necrotic core twice and
counts the enhancing voxels it reaches (:223-228).  Here the label map and the volumes stay on the device: the four percentiles
come from ``masked_percentiles`` (csrc/percentile.hip), the masks are the bits of one flag byte per voxel, the dilation and the
one reduction over the four stacked volumes are the kernels of csrc/morphology.hip, and everything step 1 reports is host
arithmetic on the counts and sums (``sequence_findings_from_stats``: a pure function, testable without a device).  The
header prose of step 1 (``technique``) and its report text (``text_summary``) are out of scope.

As a command (the reference's arguments, :552-565):

    python -m brats_amd.sequence_findings --input CASE_DIR --segmentation SEG.nii.gz [--output JSON]
"""
from __future__ import annotations

import sys

import numpy as np

from .case_io import FLAIR, T1, T1CE, T2, StepSpec, run_step, step_main
from .percentile import masked_percentiles
from .volume_ops import NBITS, binary_dilation, check_volume, flag_from_flags, flag_from_labels, masked_moments, mean_std

#: region bits of the flag map ``sequence_findings`` builds: the three labels, the normal brain of each modality (in channel
#: order) and the enhancing voxels within two dilations of the necrotic core
NCR, ED, ET, NORMAL_T1, NORMAL_T1CE, NORMAL_T2, NORMAL_FLAIR, RING = range(8)
NORMAL = (NORMAL_T1, NORMAL_T1CE, NORMAL_T2, NORMAL_FLAIR)
TUMOUR = 1 << NCR | 1 << ED | 1 << ET
SECTIONS = ("region_signal_analysis", "contrast_enhancement", "t2_flair_mismatch", "volumes")


def get_signal_label(ratio):  # :41-60
    if ratio < 0.6:
        return "markedly hypointense"
    elif ratio < 0.85:
        return "hypointense"
    elif ratio < 1.15:
        return "isointense"
    elif ratio < 1.5:
        return "hyperintense"
    else:
        return "markedly hyperintense"


def _region_signals(region_name, rows, normal_mean):  # analyze_region_signals, :71-132; rows[channel] = (n, sum, sum of squares)
    if rows[T1][0] == 0:
        return None
    mean, std = {}, {}
    for c in (T1, T1CE, T2, FLAIR):
        mean[c], std[c] = (float(v) for v in mean_std(rows[c]))
    ratio = {c: mean[c] / normal_mean[c] if normal_mean[c] and normal_mean[c] > 0 else 1.0 for c in (T1, T1CE, T2, FLAIR)}
    label = {c: get_signal_label(ratio[c]) for c in ratio}
    enhancement_ratio = mean[T1CE] / mean[T1] if mean[T1] and mean[T1] > 0 else 1.0

    def entry(c):
        return {'mean_intensity': mean[c], 'std': std[c], 'ratio_to_normal': round(float(ratio[c]), 3), 'signal_label': label[c]}
    t1ce = entry(T1CE)
    t1ce['enhancement_ratio'] = round(float(enhancement_ratio), 3)
    return {'region': region_name, 'voxel_count': int(rows[T1][0]), 'T1': entry(T1), 'T2': entry(T2), 'FLAIR': entry(FLAIR), 'T1ce': t1ce,
            'signal_summary': ", ".join([f"T1 {label[T1]}", f"T2 {label[T2]}", f"FLAIR {label[FLAIR]}", f"T1ce {label[T1CE]}"])}  # :63-68


def _all_region_signals(m):  # analyze_all_region_signals, :135-176
    normal_mean = {c: float(mean_std(m[NORMAL[c]][c])[0]) if m[NORMAL[c]][c][0] > 0 else None for c in (T1, T1CE, T2, FLAIR)}
    results = {'normal_brain_reference': {'methodology': 'Combined gray matter + white matter (non-tumor, non-CSF brain tissue)',
                                          'T1_mean': normal_mean[T1], 'T2_mean': normal_mean[T2], 'FLAIR_mean': normal_mean[FLAIR],
                                          'T1ce_mean': normal_mean[T1CE], 'voxel_count': int(m[NORMAL_T1][T1][0])},
               'regions': {}}
    for key, bit, display_name in (('ncr', NCR, 'Necrotic Core (NCR)'), ('ed', ED, 'Peritumoral Edema (ED)'), ('et', ET, 'Enhancing Tumor (ET)')):
        region_analysis = _region_signals(display_name, m[bit], normal_mean)
        if region_analysis:
            results['regions'][key] = region_analysis
    return results


def _contrast_enhancement(n_ncr, n_et, n_ring, region_signals):  # analyze_contrast_enhancement, :179-252
    results = {'enhancement_present': bool(n_et > 0), 'pattern': None, 'heterogeneity': None, 'metrics': {}}
    if not results['enhancement_present']:
        results['pattern'] = 'Non-enhancing'
        results['heterogeneity'] = 'Not applicable'
        results['description'] = ('Non-enhancing pattern can be seen with lower-grade glioma, treatment effect, or other pathology; '
                                  'clinical and histopathological correlation required')
        return results
    et_signals = region_signals['regions'].get('et', {})
    if et_signals:
        enhancement_ratio = et_signals['T1ce'].get('enhancement_ratio', 1.0)
        results['metrics']['enhancement_ratio_T1ce_over_T1'] = enhancement_ratio
        results['metrics']['T1ce_ratio_to_normal'] = et_signals['T1ce']['ratio_to_normal']
        t1ce_mean = et_signals['T1ce']['mean_intensity']
        t1ce_std = et_signals['T1ce']['std']
        if t1ce_mean > 0:
            cv = t1ce_std / t1ce_mean
            results['metrics']['coefficient_of_variation'] = round(float(cv), 3)
            if cv > 0.35:
                results['heterogeneity'] = 'Markedly heterogeneous'
            elif cv > 0.25:
                results['heterogeneity'] = 'Heterogeneous'
            elif cv > 0.15:
                results['heterogeneity'] = 'Mildly heterogeneous'
            else:
                results['heterogeneity'] = 'Homogeneous'
    if n_ncr > 0 and n_et > 0 and n_ring > 0.3 * n_et:  # :223-236: enhancing voxels within two dilations of the necrotic core
        results['pattern'] = 'Ring-enhancing'
        results['description'] = 'Peripheral rim enhancement surrounding central non-enhancing core, characteristic of high-grade glioma or metastasis'
    else:
        results['pattern'] = 'Solid/nodular enhancing'
        results['description'] = 'Solid pattern of enhancement without central necrosis'
    if 'enhancement_ratio_T1ce_over_T1' in results['metrics']:
        ratio = results['metrics']['enhancement_ratio_T1ce_over_T1']
        if ratio > 2.0:
            results['enhancement_strength'] = 'Marked enhancement'
        elif ratio > 1.5:
            results['enhancement_strength'] = 'Strong enhancement'
        elif ratio > 1.2:
            results['enhancement_strength'] = 'Moderate enhancement'
        elif ratio > 1.05:
            results['enhancement_strength'] = 'Mild enhancement'
        else:
            results['enhancement_strength'] = 'Minimal/equivocal enhancement'
    return results


def _t2_flair_mismatch(region_signals):  # detect_t2_flair_mismatch, :255-284
    results = {'mismatch_detected': False, 'description': None}
    for key, region in region_signals['regions'].items():
        t2_ratio = region['T2']['ratio_to_normal']
        flair_ratio = region['FLAIR']['ratio_to_normal']
        if t2_ratio > 1.3 and flair_ratio < t2_ratio * 0.7:
            results['mismatch_detected'] = True
            results['region'] = key
            results['t2_ratio'] = t2_ratio
            results['flair_ratio'] = flair_ratio
            results['description'] = (f"Possible T2/FLAIR mismatch in {region['region']}: T2 hyperintense (ratio {t2_ratio:.2f}) with relatively "
                                      f"suppressed FLAIR (ratio {flair_ratio:.2f}). May suggest IDH-mutant lower-grade glioma.")
            break
    if not results['mismatch_detected']:
        results['description'] = "No T2/FLAIR mismatch detected. Signal intensity patterns concordant between T2 and FLAIR sequences."
    return results


def sequence_findings_from_stats(region_moments, voxel_dims):
    """The four dicts of step 1 from what the device delivers.  Pure host arithmetic in float64.

    region_moments  float64 [8, 4, 3], ``masked_moments`` of (T1, T1ce, T2, FLAIR) over the bits NCR (seg == 1), ED (seg == 2),
                    ET (seg == 3 or 4), NORMAL_T1 .. NORMAL_FLAIR (seg == 0 and the modality brighter than the 5th percentile of
                    its positive voxels; empty for a modality without a positive voxel) and RING (ET within two dilations of NCR)
    voxel_dims      voxel sizes along axis 0, 1, 2
    """
    m = np.asarray(region_moments, dtype=np.float64).reshape(NBITS, 4, 3)
    voxel_volume_cm3 = float(np.prod([float(v) for v in voxel_dims]) / 1000)  # utils.get_voxel_dimensions, utils.py:117-124
    n_ncr, n_ed, n_et, n_ring = (int(m[b][T1][0]) for b in (NCR, ED, ET, RING))
    region_signals = _all_region_signals(m)

    def volume(n):  # utils.calculate_volume, utils.py:181-183
        return float(np.int64(n) * voxel_volume_cm3)
    return {'region_signal_analysis': region_signals,
            'contrast_enhancement': _contrast_enhancement(n_ncr, n_et, n_ring, region_signals),
            't2_flair_mismatch': _t2_flair_mismatch(region_signals),
            'volumes': {'Whole Tumor (WT)': volume(n_ncr + n_ed + n_et), 'Tumor Core (TC)': volume(n_ncr + n_et), 'Enhancing Tumor (ET)': volume(n_et),
                        'Necrotic Core (NCR)': volume(n_ncr), 'Peritumoral Edema (ED)': volume(n_ed)}}  # :508-514


def region_flags(seg, chans, ctx=None):
    """The flag byte per voxel ``sequence_findings`` reduces over, from a CUDA uint8 label map with the labels 0..4 and the four
    CUDA float32 volumes in channel order.  ``ctx``: the ``features.CaseContext`` of these tensors, which has the four percentiles."""
    import torch
    from . import components
    flags = torch.zeros_like(seg)
    flag_from_labels(seg, (1,), NCR, flags)                               # utils.py:173-175
    flag_from_labels(seg, (2,), ED, flags)
    flag_from_labels(seg, (3, 4), ET, flags)
    for c, bit in enumerate(NORMAL):                                      # utils.py:57-58
        count, p = masked_percentiles(chans[c], 5, lo=0) if ctx is None else ctx.positive_percentiles(c, 5)
        if count:                                                         # (no positive voxel: `data > 0`, an empty mask)
            flag_from_flags(flags, bit, forbid=TUMOUR, x=chans[c], lo=float(p[0]))
    flag_from_labels(binary_dilation(components._indicator(seg, (1,)), 2), (1,), RING, flags)  # :225-226
    flag_from_flags(flags, RING, require=1 << RING | 1 << ET)
    return flags


def sequence_findings(seg, t1, t1ce, t2, flair, voxel_dims, ctx=None):
    """seg: CUDA uint8 label map [d0, d1, d2] (1 = ncr, 2 = ed, 3 / 4 = et, nothing above 4); t1, t1ce, t2, flair: CUDA float32
    volumes of that shape -> the dicts ``region_signal_analysis``, ``contrast_enhancement``, ``t2_flair_mismatch`` and ``volumes``
    of the reference's step 1.  ``ctx``: the ``features.CaseContext`` of these tensors (it has checked them), or None."""
    import torch
    if ctx is not None:
        seg, chans = ctx.volumes(seg, (t1, t1ce, t2, flair), "sequence_findings")
        return sequence_findings_from_stats(masked_moments(torch.stack(chans), region_flags(seg, chans, ctx)), voxel_dims)
    seg = check_volume(seg, torch.uint8, "sequence_findings")
    chans = [check_volume(v, torch.float32, "sequence_findings") for v in (t1, t1ce, t2, flair)]
    if any(v.shape != seg.shape for v in chans):
        raise ValueError("sequence_findings: the volumes and the label map differ in shape")
    if int(seg.max()) > 4:
        raise ValueError("sequence_findings: the label map holds values above 4 (0 = background, 1 = ncr, 2 = ed, 3 / 4 = et)")
    flags = region_flags(seg, chans)
    return sequence_findings_from_stats(masked_moments(torch.stack(chans), flags), voxel_dims)


# ---- the command ------------------------------------------------------------------------------------------------------
def _summary(res):
    ce = res['contrast_enhancement']
    return (f"{ce['pattern']}; {ce['heterogeneity']}; {ce.get('enhancement_strength', 'no enhancement strength')}; "
            f"T2/FLAIR mismatch {'detected' if res['t2_flair_mismatch']['mismatch_detected'] else 'not detected'}; "
            f"{len(res['region_signal_analysis']['regions'])} regions")


STEP_SPEC = StepSpec(key='step1_sequence_findings', title='Step 1 - Sequence-specific findings', description='Step 1: sequence-specific findings (MI355X)',
                     call=lambda seg, chans, zooms, ctx=None: sequence_findings(seg, chans['t1'], chans['t1ce'], chans['t2'], chans['flair'], zooms, ctx=ctx),
                     summary=_summary,
                     tail={'sequences_analyzed': ['T1', 'T1ce', 'T2', 'FLAIR'], 'diffusion_available': False,
                           'diffusion_note': 'DWI/ADC not available in standard BraTS dataset'})  # :531-533


def analyze(input_folder, segmentation_path, output_path=None):
    return run_step(STEP_SPEC, input_folder, segmentation_path, output_path)


def main(argv=None):
    return step_main(STEP_SPEC, argv)


if __name__ == '__main__':
    sys.exit(main())
