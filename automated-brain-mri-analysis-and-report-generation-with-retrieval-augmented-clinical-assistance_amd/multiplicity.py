"""Step 3 of the reference's feature extraction as a command (feature_extraction/step3_multiplicity.py:549-562):

    python -m brats_amd.multiplicity --input CASE_DIR --segmentation SEG.nii.gz [--output JSON]

The voxel sizes come from the segmentation's own header (the reference reads them from the case's T1 file, which lies on the
same grid); ``--input`` only names the case.  The JSON holds the numeric dicts of step 3, not its report prose.
"""
from __future__ import annotations

import sys

from . import components
from .case_io import StepSpec, run_step, step_main


def _summary(res):
    return f"{res['component_analysis']['description']}; {res['distribution_pattern']['pattern']}; {res['enhancing_analysis']['pattern']}"


STEP_SPEC = StepSpec(key='step3_multiplicity', title='Step 3 - Lesion multiplicity and distribution',
                     description='Step 3: lesion multiplicity and distribution (MI355X)', modalities=(), zooms='segmentation', case_id='folder',
                     call=lambda seg, chans, zooms, ctx=None: components.lesion_multiplicity(seg, zooms, ctx=ctx), summary=_summary,
                     input_help='Input folder containing MRI sequences (names the case)')


def analyze(input_folder, segmentation_path, output_path=None):
    return run_step(STEP_SPEC, input_folder, segmentation_path, output_path)


def main(argv=None):
    return step_main(STEP_SPEC, argv)


if __name__ == '__main__':
    sys.exit(main())
