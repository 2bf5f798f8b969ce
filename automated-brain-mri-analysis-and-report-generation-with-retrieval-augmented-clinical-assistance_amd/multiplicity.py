"""Step 3 of the reference's feature extraction as a command (feature_extraction/step3_multiplicity.py:549-562):

    python -m brats_amd.multiplicity --input CASE_DIR --segmentation SEG.nii.gz [--output JSON]

The voxel sizes come from the segmentation's own header (the reference reads them from the case's T1 file, which lies on the
same grid); ``--input`` only names the case.  The JSON holds the numeric dicts of step 3, not its report prose.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np


def analyze(input_folder, segmentation_path, output_path=None):
    import torch
    from . import components, nifti
    img = nifti.load(segmentation_path)
    seg = np.ascontiguousarray(np.round(img.data).astype(np.uint8))  # (x, y, z) as nibabel hands it to the reference, :459-460
    zooms = [float(v) for v in img.zooms]
    res = {'case_id': Path(input_folder).name, 'step': 'Step 3 - Lesion multiplicity and distribution',
           'voxel_info': {'dimensions_mm': zooms, 'volume_mm3': float(np.prod(zooms)), 'volume_cm3': float(np.prod(zooms) / 1000)}}
    res.update(components.lesion_multiplicity(torch.from_numpy(seg).cuda(), zooms))
    if output_path:
        Path(output_path).parent.mkdir(parents=True, exist_ok=True)
        with open(output_path, 'w') as f:
            json.dump(res, f, indent=2)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description='Step 3: lesion multiplicity and distribution (MI355X)')
    ap.add_argument('--input', required=True, help='Input folder containing MRI sequences (names the case)')
    ap.add_argument('--segmentation', required=True, help='Path to segmentation mask (NIfTI)')
    ap.add_argument('--output', default=None, help='Output path for JSON results')
    args = ap.parse_args(argv)
    res = analyze(args.input, args.segmentation, args.output)
    print(f"{res['case_id']}: {res['component_analysis']['description']}; {res['distribution_pattern']['pattern']}; "
          f"{res['enhancing_analysis']['pattern']}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
