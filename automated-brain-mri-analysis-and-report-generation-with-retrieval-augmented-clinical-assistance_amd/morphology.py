"""Binary morphology, exact distance transform and the reference's tumour morphology (step 4) on the device.

``feature_extraction/step4_morphology.py`` erodes and dilates the whole-tumour mask with scipy (:42, :149, :227, :252, :254),
runs two ``distance_transform_edt`` and three whole-volume ``np.gradient`` calls for one coefficient of variation on the
tumour surface (:160-181), turns ``np.where(mask)`` into a covariance matrix (:84-100) and indexes the four modalities with
boolean masks (:231-262, :324-338).  Here the label map and the volumes stay on the device: erosion, dilation, the squared
distance transform, the gradient statistics at the surface voxels, the coordinate moments and the intensity moments of up to
eight overlapping regions are HIP kernels (csrc/morphology.hip), and everything step 4 reports is host arithmetic on their
integers and sums, in the reference's order of operations (``morphology_from_stats``: a pure function, testable without a
device).  The report prose of step 4 (``text_summary``) is out of scope.

As a command (the reference's arguments, :690-703):

    python -m brats_amd.morphology --input CASE_DIR --segmentation SEG.nii.gz [--output JSON]
"""
from __future__ import annotations

import sys
from fractions import Fraction

import numpy as np

from .case_io import FLAIR, T1, T1CE, T2, StepSpec, run_step, step_main
from .volume_ops import (NBITS, binary_dilation, binary_erosion, check_volume, distance_transform_edt_sq, flag_from_flags, flag_from_labels, masked_moments,
                         mean_std, second_moments, surface_gradient_stats)

#: region bits of the flag map ``tumor_morphology`` builds (one uint8 per voxel)
WT, BAND, INNER, OUTER, NCR, CYSTIC = 0, 1, 2, 3, 4, 5


# ---- step4_morphology.py:33-541 on the integers and sums --------------------------------------------------------------
def _shape_descriptors(n_wt, n_surface, moments, voxel_dims):  # calculate_shape_descriptors, :483-541
    if n_wt == 0:
        return {'volume_cm3': 0, 'surface_area_mm2': 0, 'sphericity': 0, 'compactness': 0, 'elongation': 1.0, 'principal_axes_mm': [0, 0, 0]}
    volume_mm3 = np.int64(n_wt) * np.prod(voxel_dims)
    volume_cm3 = volume_mm3 / 1000
    avg_face_area = (voxel_dims[0] * voxel_dims[1] + voxel_dims[1] * voxel_dims[2] + voxel_dims[0] * voxel_dims[2]) / 3
    surface_area = float(np.int64(n_surface) * avg_face_area)  # :33-55
    if surface_area == 0 or volume_mm3 == 0:  # :58-75
        sphericity = 0.0
    else:
        radius = (3 * volume_mm3 / (4 * np.pi)) ** (1 / 3)
        sphericity = float(min(1.0, max(0.0, 4 * np.pi * radius ** 2 / surface_area)))
    compactness = 0.0 if surface_area == 0 else float(min(1.0, (36 * np.pi * volume_mm3**2) / (surface_area**3)))  # :118-130
    if n_wt < 10:  # :78-115
        elongation, axes = 1.0, [1.0, 1.0, 1.0]
    else:
        n, s = int(moments[0]), [int(v) for v in moments[1:4]]
        second = {(0, 0): int(moments[4]), (1, 1): int(moments[5]), (2, 2): int(moments[6]), (0, 1): int(moments[7]), (0, 2): int(moments[8]),
                  (1, 2): int(moments[9])}
        cov = np.zeros((3, 3))
        for (a, b), sab in second.items():  # np.cov: sum of centred products / (n - 1), here from exact integers
            cov[a, b] = cov[b, a] = float(Fraction(n * sab - s[a] * s[b], n * (n - 1))) * voxel_dims[a] * voxel_dims[b]
        eigenvalues = np.sort(np.linalg.eigvalsh(cov))[::-1]
        elongation = float(np.sqrt(eigenvalues[0] / eigenvalues[-1])) if eigenvalues[-1] > 0 else 1.0
        axes = [float(np.sqrt(e) * 2) for e in eigenvalues]
    shape_class = ('Spherical/round' if sphericity > 0.8 else 'Ovoid' if sphericity > 0.6 else 'Irregular' if sphericity > 0.4
                   else 'Highly irregular/complex')
    elongation_class = 'Elongated' if elongation > 2.5 else ('Mildly elongated' if elongation > 1.5 else 'Roughly isotropic')
    return {'volume_cm3': float(volume_cm3), 'surface_area_mm2': float(surface_area), 'sphericity': float(sphericity),
            'compactness': float(compactness), 'elongation': float(elongation), 'principal_axes_mm': axes,
            'shape_classification': shape_class, 'elongation_classification': elongation_class}


def _border_regularity(n_wt, n_surface, gradient):  # analyze_border_regularity, :133-205
    if n_wt == 0:
        return {'regularity_score': 0, 'classification': 'No tumor', 'description': 'No tumor detected'}
    if n_surface < 10:
        return {'regularity_score': 1.0, 'classification': 'Too small to assess', 'description': 'Tumor too small for border analysis'}
    _, mean, std = gradient
    regularity = 1.0 / (1.0 + std / mean) if std > 0 else 1.0
    if regularity > 0.7:
        classification, description = 'Smooth contour', 'Smooth, regular outer contour (note: does not indicate margin sharpness)'
    elif regularity > 0.5:
        classification, description = 'Mildly lobulated', 'Some contour irregularity with mild lobulation'
    elif regularity > 0.3:
        classification, description = 'Lobulated', 'Lobulated/irregular outer contour'
    else:
        classification, description = 'Highly irregular', 'Highly irregular/spiculated outer contour'
    return {'regularity_score': float(regularity), 'classification': classification, 'description': description,
            'surface_voxel_count': int(n_surface), 'concept': 'contour_smoothness'}


def _margin_definition(region):  # analyze_margin_definition, :208-290; region[bit] = (n, sum, sum of squares) of T1ce
    if region[WT][0] == 0:
        return {'margin_sharpness': 0, 'classification': 'No tumor', 'description': 'No tumor detected'}
    if region[BAND][0] == 0:
        return {'margin_sharpness': 0.5, 'classification': 'Could not assess', 'description': 'Insufficient peritumoral tissue for analysis'}
    tumor_mean, _ = mean_std(region[WT])
    peritumoral_mean, _ = mean_std(region[BAND])
    contrast = abs(tumor_mean - peritumoral_mean) / peritumoral_mean if peritumoral_mean > 0 else 0
    if region[INNER][0] > 0 and region[OUTER][0] > 0:
        inner_mean, inner_std = mean_std(region[INNER])
        outer_mean, outer_std = mean_std(region[OUTER])
        border_gradient_normalized = abs(inner_mean - outer_mean) / (inner_std + outer_std + 1e-6)
    else:
        border_gradient_normalized = 0
    sharpness = min(1.0, (contrast + border_gradient_normalized) / 2)
    if sharpness > 0.6:
        classification, description = 'Sharp transition', 'Abrupt tumor-brain intensity transition, well-demarcated margin'
    elif sharpness > 0.4:
        classification, description = 'Moderate transition', 'Moderately distinct margin with some gradual transition zones'
    elif sharpness > 0.2:
        classification, description = 'Gradual transition', 'Indistinct margin with gradual intensity blending into brain'
    else:
        classification, description = 'Infiltrative transition', 'No clear intensity demarcation, tumor infiltrates surrounding parenchyma'
    return {'margin_sharpness': float(sharpness), 'contrast_ratio': float(contrast), 'border_gradient': float(border_gradient_normalized),
            'classification': classification, 'description': description, 'concept': 'intensity_transition'}


def _cystic_vs_solid(n_wt, region_moments, voxel_dims):  # analyze_cystic_vs_solid, :293-397
    if n_wt == 0:
        return {'classification': 'No tumor', 'cystic_percentage': 0, 'solid_percentage': 0, 'description': 'No tumor detected'}
    voxel_vol = np.prod(voxel_dims) / 1000
    n_ncr = int(region_moments[NCR][T2][0])
    if n_ncr > 0:
        cystic_fraction_in_ncr = np.int64(region_moments[CYSTIC][T2][0]) / n_ncr
        t2_mean, t2_std = mean_std(region_moments[NCR][T2])
        flair_mean, _ = mean_std(region_moments[NCR][FLAIR])
        t2_cv = t2_std / t2_mean if t2_mean > 0 else 0
        flair_t2_ratio = flair_mean / t2_mean if t2_mean > 0 else 1
    else:
        cystic_fraction_in_ncr, t2_cv, flair_t2_ratio = 0, 0, 1
    ncr_volume = np.int64(n_ncr) * voxel_vol
    wt_volume = np.int64(n_wt) * voxel_vol
    cystic_volume = ncr_volume * cystic_fraction_in_ncr
    cystic_percentage = (cystic_volume / wt_volume * 100) if wt_volume > 0 else 0
    solid_volume = wt_volume - cystic_volume
    solid_percentage = 100 - cystic_percentage
    if cystic_percentage > 70:
        classification, description = 'Predominantly cystic', 'Large cystic component with thin wall/rim'
    elif cystic_percentage > 40:
        classification, description = 'Cystic with solid component', 'Mixed cystic and solid tumor with significant cystic component'
    elif cystic_percentage > 15:
        classification, description = 'Solid with cystic component', 'Predominantly solid tumor with cystic/necrotic areas'
    elif n_ncr > 0:
        if t2_cv > 0.3:
            classification, description = 'Solid with necrosis', 'Solid tumor with central necrotic (non-cystic) component'
        else:
            classification, description = 'Solid with possible cyst', 'Solid tumor with possible small cystic component'
    else:
        classification, description = 'Solid', 'Homogeneous solid tumor without significant cystic component'
    signal_characteristics = {
        't2_homogeneity': 'Homogeneous' if t2_cv < 0.2 else ('Mildly heterogeneous' if t2_cv < 0.4 else 'Heterogeneous'),
        'flair_suppression': 'Present (suggests true cyst)' if flair_t2_ratio < 0.7 else 'Absent (suggests necrosis/protein)',
        'csf_like_signal_fraction': float(cystic_fraction_in_ncr)}
    return {'classification': classification, 'cystic_volume_cm3': float(cystic_volume), 'cystic_percentage': float(cystic_percentage),
            'solid_volume_cm3': float(solid_volume), 'solid_percentage': float(solid_percentage),
            'signal_characteristics': signal_characteristics, 'description': description}


def _necrosis_pattern(n_wt, label_stats, voxel_dims):  # analyze_necrosis_pattern, :400-480
    ncr = label_stats[1]
    tc = label_stats[[1, 3, 4]].sum(axis=0)   # utils.py:176; only the counts and coordinate sums of the union are used
    ncr_volume = ncr[0] * np.prod(voxel_dims) / 1000
    tc_volume = tc[0] * np.prod(voxel_dims) / 1000
    wt_volume = np.int64(n_wt) * np.prod(voxel_dims) / 1000
    if wt_volume == 0:
        return {'necrosis_present': False, 'pattern': 'No tumor', 'description': 'No tumor detected'}
    if ncr_volume == 0:
        return {'necrosis_present': False, 'necrosis_volume_cm3': 0, 'necrosis_percentage': 0, 'pattern': 'No necrosis',
                'description': 'No central necrosis identified, solid tumor'}
    necrosis_pct = (ncr_volume / wt_volume) * 100
    if ncr[0] > 0 and tc[0] > 0:
        ncr_centroid = np.array([np.float64(int(ncr[1 + i])) / int(ncr[0]) for i in range(3)])  # np.mean of integer coordinates
        tc_centroid = np.array([np.float64(int(tc[1 + i])) / int(tc[0]) for i in range(3)])
        dist = np.linalg.norm((ncr_centroid - tc_centroid) * voxel_dims)
        tc_radius = (3 * tc_volume * 1000 / (4 * np.pi)) ** (1 / 3)
        if dist < tc_radius * 0.3:
            location, location_description = 'Central', 'Necrosis centered within tumor'
        elif dist < tc_radius * 0.6:
            location, location_description = 'Eccentric', 'Necrosis somewhat offset from tumor center'
        else:
            location, location_description = 'Peripheral', 'Necrosis located eccentrically'
    else:
        location, location_description = 'Undetermined', 'Could not determine necrosis location'
    if necrosis_pct > 50:
        pattern = 'Extensive necrosis'
        description = f'Large central necrotic component ({necrosis_pct:.0f}% of tumor), characteristic of high-grade glioma'
    elif necrosis_pct > 25:
        pattern = 'Moderate necrosis'
        description = f'Moderate central necrosis ({necrosis_pct:.0f}% of tumor), suggests high-grade pathology'
    elif necrosis_pct > 10:
        pattern = 'Focal necrosis'
        description = f'Focal areas of necrosis ({necrosis_pct:.0f}% of tumor)'
    else:
        pattern = 'Minimal necrosis'
        description = f'Small necrotic foci ({necrosis_pct:.0f}% of tumor)'
    return {'necrosis_present': True, 'necrosis_volume_cm3': float(ncr_volume), 'necrosis_percentage': float(necrosis_pct), 'pattern': pattern,
            'location': location, 'location_description': location_description, 'description': description}


def morphology_from_stats(label_stats, moments, gradient, region_moments, voxel_dims):
    """The five dicts of step 4 from what the device delivers.  Pure host arithmetic in float64.

    label_stats     int64 [K >= 5, 10], ``mi355_label_stats`` of the label map (counts and coordinate sums per label value)
    moments         int64 [10], ``second_moments`` of the whole-tumour mask ``seg > 0``
    gradient        (n, mean, std) of ``surface_gradient_stats`` on the whole tumour's surface, or None when the surface has
                    fewer than 10 voxels (the reference does not look at the distance maps then)
    region_moments  float64 [8, 4, 3], ``masked_moments`` of (T1, T1ce, T2, FLAIR) over the bits WT (seg > 0), BAND (5 dilations
                    minus WT), INNER (WT minus its erosion: the surface), OUTER (1 dilation minus WT), NCR (seg == 1) and CYSTIC
                    (NCR voxels with the CSF-like signal of :329-333)
    voxel_dims      voxel sizes along axis 0, 1, 2 (called x, y, z as in the reference)
    """
    voxel_dims = [float(v) for v in voxel_dims]
    label_stats = np.asarray(label_stats, dtype=np.int64).reshape(-1, 10)
    moments = np.asarray(moments, dtype=np.int64).reshape(10)
    region_moments = np.asarray(region_moments, dtype=np.float64).reshape(NBITS, -1, 3)
    n_wt, n_surface = int(region_moments[WT][0][0]), int(region_moments[INNER][0][0])
    if n_wt != int(moments[0]):
        raise ValueError(f"morphology_from_stats: {n_wt} voxels carry the whole-tumour bit, the moments are of {int(moments[0])}")
    if n_surface >= 10 and gradient is None:
        raise ValueError("morphology_from_stats: a surface of 10 voxels or more needs its gradient statistics")
    return {'shape_descriptors': _shape_descriptors(n_wt, n_surface, moments, voxel_dims),
            'border_regularity': _border_regularity(n_wt, n_surface, gradient),
            'margin_definition': _margin_definition(region_moments[:, T1CE, :]),
            'necrosis_pattern': _necrosis_pattern(n_wt, label_stats, voxel_dims),
            'cystic_solid_classification': _cystic_vs_solid(n_wt, region_moments, voxel_dims)}


def csf_thresholds(t1, t2, flair):
    """(upper T1, lower T2, upper FLAIR) bounds of the CSF-like signal, :317-320 and the factors of :330-332, from float64 host
    arrays: ``np.percentile`` exactly as the reference calls it."""
    csf_t1_upper = np.percentile(t1[t1 > 0], 10)
    csf_t2_lower = np.percentile(t2[t2 > 0], 85)
    csf_flair_upper = np.percentile(flair[flair > 0], 20)
    return float(csf_t1_upper * 1.5), float(csf_t2_lower * 0.8), float(csf_flair_upper * 2)


def region_flags(seg, t1, t2, flair, ctx=None):
    """The flag byte per voxel ``tumor_morphology`` reduces over: bits WT, BAND, INNER, OUTER, NCR and CYSTIC of a CUDA uint8 label
    map and three CUDA float32 volumes (T1ce takes no part in any region).  Only the WT bit when there is no tumour.  ``ctx``: the
    ``features.CaseContext`` of these tensors, which has the erosion, the dilations and the three percentiles."""
    import torch
    flags = torch.zeros_like(seg)
    flag_from_labels(seg, range(1, 256), WT, flags)                      # utils.py:177, wt = seg > 0
    if not bool(seg.any()):                                              # :38, :141, :219, :305 return early
        return flags
    from .percentile import masked_percentiles
    if ctx is None:
        flag_from_labels(binary_erosion(seg), (1,), INNER, flags)        # :42, :149-150, :252-253: wt & ~eroded
        flag_from_flags(flags, INNER, require=1 << WT, forbid=1 << INNER)
        flag_from_labels(binary_dilation(seg), (1,), OUTER, flags)       # :254
        flag_from_flags(flags, OUTER, require=1 << OUTER, forbid=1 << WT)
        flag_from_labels(binary_dilation(seg, 5), (1,), BAND, flags)     # :227-228
        flag_from_flags(flags, BAND, require=1 << BAND, forbid=1 << WT)
        p_t1, p_t2, p_flair = masked_percentiles(t1, 10, lo=0)[1], masked_percentiles(t2, 85, lo=0)[1], masked_percentiles(flair, 20, lo=0)[1]
    else:
        ctx.eroded_into(flags, INNER, 1)
        flag_from_flags(flags, INNER, require=1 << WT, forbid=1 << INNER)
        ctx.dilated_into(flags, OUTER, 1, forbid=1 << WT)
        ctx.dilated_into(flags, BAND, 5, forbid=1 << WT)
        p_t1, p_t2, p_flair = ctx.positive_percentiles(T1, 10)[1], ctx.positive_percentiles(T2, 85)[1], ctx.positive_percentiles(FLAIR, 20)[1]
    flag_from_labels(seg, (1,), NCR, flags)                              # utils.py:173
    t1_hi = float(p_t1[0] * 1.5)                                         # :317-320 and the factors of :330-332, as csf_thresholds
    t2_lo = float(p_t2[0] * 0.8)
    flair_hi = float(p_flair[0] * 2)
    flag_from_flags(flags, CYSTIC, require=1 << NCR, x=t1, hi=t1_hi)     # :329-333
    flag_from_flags(flags, CYSTIC, require=1 << CYSTIC, x=t2, lo=t2_lo)
    flag_from_flags(flags, CYSTIC, require=1 << CYSTIC, x=flair, hi=flair_hi)
    return flags


def tumor_morphology(seg, t1, t1ce, t2, flair, voxel_dims, ctx=None):
    """seg: CUDA uint8 label map [d0, d1, d2] (1 = ncr, 2 = ed, 3 / 4 = et); t1, t1ce, t2, flair: CUDA float32 volumes of that
    shape -> the dicts ``shape_descriptors``, ``border_regularity``, ``margin_definition``, ``necrosis_pattern`` and
    ``cystic_solid_classification`` of the reference's step 4.

    Everything comes from device results, the three ``np.percentile`` thresholds of :317-320 included: ``masked_percentiles``
    selects their order statistics on the device and interpolates as numpy does, bit for bit (``csf_thresholds`` is the same
    on host arrays).  ``ctx``: the ``features.CaseContext`` of these tensors (it has checked them), or None."""
    import torch
    from . import components, evaluate
    if ctx is not None:
        seg, chans = ctx.volumes(seg, (t1, t1ce, t2, flair), "tumor_morphology")
    else:
        seg = check_volume(seg, torch.uint8, "tumor_morphology")
        chans = [check_volume(v, torch.float32, "tumor_morphology") for v in (t1, t1ce, t2, flair)]
        if any(v.shape != seg.shape for v in chans):
            raise ValueError("tumor_morphology: the volumes and the label map differ in shape")
    flags = region_flags(seg, chans[T1], chans[T2], chans[FLAIR], ctx)
    region_moments = masked_moments(torch.stack(chans), flags)
    gradient = None
    if region_moments[INNER][0][0] >= 10:                                # :152
        d2_in = distance_transform_edt_sq(seg)                           # :160-161
        d2_out = distance_transform_edt_sq(components._indicator(seg, (0,)))
        gradient = surface_gradient_stats(d2_in, d2_out, flags, 1 << INNER)
    return morphology_from_stats(evaluate.label_stats(seg, 8) if ctx is None else ctx.label_stats, second_moments(seg), gradient, region_moments, voxel_dims)


# ---- the command ------------------------------------------------------------------------------------------------------
def _summary(res):
    return (f"{res['shape_descriptors'].get('shape_classification', 'No tumor')}; {res['border_regularity']['classification']}; "
            f"{res['margin_definition']['classification']}; {res['necrosis_pattern']['pattern']}; {res['cystic_solid_classification']['classification']}")


STEP_SPEC = StepSpec(key='step4_morphology', title='Step 4 - Tumor morphology and margins', description='Step 4: tumor morphology and margins (MI355X)',
                     call=lambda seg, chans, zooms, ctx=None: tumor_morphology(seg, chans['t1'], chans['t1ce'], chans['t2'], chans['flair'], zooms, ctx=ctx),
                     summary=_summary)


def analyze(input_folder, segmentation_path, output_path=None):
    return run_step(STEP_SPEC, input_folder, segmentation_path, output_path)


def main(argv=None):
    return step_main(STEP_SPEC, argv)


if __name__ == '__main__':
    sys.exit(main())
