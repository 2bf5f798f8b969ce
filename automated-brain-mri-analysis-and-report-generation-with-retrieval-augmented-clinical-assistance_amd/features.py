"""All six feature-extraction steps of one case from one set of resident tensors.

The reference's pipeline calls none of the six steps one by one: ``run_full_pipeline.py:274-293`` spawns
``feature_extraction/run_all.py --input --segmentation --output`` once, and the files of that output folder are what everything
downstream reads.  Here ``CaseContext`` holds the label map and the four modalities on the device and works out once, on first
use, what more than one step derives from them: the percentiles of each modality's positive voxels and of the brain's (two
batched selects, ``masked_percentiles_multi``, where the six steps alone make 22 calls), the brain mask's threshold, the label
statistics, the 26-neighbour labelling of the tumour, and one city-block distance transform of the tumour each way, whose
thresholds are every dilation and erosion steps 2, 4, 5 and 6 take of it.  Each step's resident function takes the context as
``ctx=``; without one it runs as it always has.  ``extract_all`` runs the six through one context, ``run_all_steps`` does so from
the files of a case folder, loading each of the five files once, and writes the reference's seven JSON files; its running half,
``run_steps_resident``, is what ``pipeline.analyze_resident`` calls on the tensors the inference driver holds.

The reference's compiled report (``comprehensive_report``, ``llm_summary``, ``llm_ready_summary.json``, ``radiology_report.txt``)
and the steps' ``text_summary`` / ``technique`` prose stay out: they are string templates of the reference's program text.

As a command (the reference's arguments, run_all.py:503-516, and the two of ``brats_amd.mass_effect``):

    python -m brats_amd.features --input CASE_DIR --segmentation SEG.nii.gz --output OUT_DIR [--distance sampled|exact] [--seed N]
"""
from __future__ import annotations

import argparse
import sys
from datetime import datetime
from pathlib import Path

import numpy as np

from . import mass_effect, morphology, multiplicity, normal_structures, percentile, quality, sequence_findings
from .case_io import FLAIR, MODALITIES, T1, T1CE, T2, case_id_and_paths, document, load_case, step_zooms, to_device, write_json
from .volume_ops import check_volume, cityblock_distance, flag_from_flags, flag_from_i32

#: the records of the six steps, in order: what each one's command loads and what its file holds (``case_io.StepSpec``)
SPECS = tuple(m.STEP_SPEC for m in (sequence_findings, mass_effect, multiplicity, morphology, quality, normal_structures))
STEP_KEYS = tuple(spec.key for spec in SPECS)
#: the percentiles the six steps take of a modality's positive voxels (``x[x > 0]``), per channel: utils.py:57 (5, steps 1, 2, 5, 6),
#: step5_quality.py:194 (10), step4_morphology.py:317-320 (T1 10, T2 85, FLAIR 20)
POSITIVE_QS = {T1: (5, 10), T1CE: (5, 10), T2: (5, 10, 85), FLAIR: (5, 10, 20)}
#: and of its values over the brain mask: step2_mass_effect.py:179 and step6_normal_structures.py:48-50 (T1 15, T2 85, FLAIR 25),
#: step5_quality.py:210-212 (1, 25, 75, 99 of all four)
BRAIN_QS = {T1: (15, 1, 25, 75, 99), T1CE: (1, 25, 75, 99), T2: (85, 1, 25, 75, 99), FLAIR: (25, 1, 75, 99)}
BRAIN = 0  # the one bit of the context's own flag byte


class CaseContext:
    """The five resident tensors of a case and what more than one step derives from them, each worked out on first use and kept.

    seg: CUDA uint8 label map [d0, d1, d2] (1 = ncr, 2 = ed, 3 / 4 = et, nothing above 4); t1, t1ce, t2, flair: CUDA float32
    volumes of that shape.  Nothing kept depends on which step asks first: every quantity is a function of the five tensors."""

    def __init__(self, seg, t1, t1ce, t2, flair):
        import torch
        self.seg = check_volume(seg, torch.uint8, "CaseContext")
        self.chans = [check_volume(v, torch.float32, "CaseContext") for v in (t1, t1ce, t2, flair)]
        if any(v.shape != self.seg.shape for v in self.chans):
            raise ValueError("CaseContext: the volumes and the label map differ in shape")
        if int(self.seg.max()) > 4:
            raise ValueError("CaseContext: the label map holds values above 4 (0 = background, 1 = ncr, 2 = ed, 3 / 4 = et)")
        self._given = (seg, t1, t1ce, t2, flair)
        self._kept = {}
        self.select_launches = {}   # 'positive' / 'brain' -> kernel launches of that batched select

    def _once(self, name, make):
        if name not in self._kept:
            self._kept[name] = make()
        return self._kept[name]

    def volumes(self, seg, chans, what):
        """The checked tensors for a step that was handed ``seg`` and ``chans`` (T1, T1ce, T2, FLAIR, or T1 alone) beside the context:
        they must be the context's own."""
        given = (self._given[0],) + tuple(self._given[1:1 + len(chans)])
        mine = (self.seg,) + tuple(self.chans[:len(chans)])
        for t, g, m in zip((seg,) + tuple(chans), given, mine):
            if t is not g and t is not m:
                raise ValueError(f"{what}: the tensors are not the ones the context holds")
        return self.seg, list(self.chans[:len(chans)])

    # ---- percentiles ---------------------------------------------------------------------------------------------------
    def _select(self, name, qs, flags, require, lo):
        def make():
            info = {}
            stats = percentile.masked_order_stats_multi([(self.chans[c], qs[c], require, 0, lo, np.inf) for c in (T1, T1CE, T2, FLAIR)], flags, info)
            self.select_launches[name] = info['launches']
            return {c: stats[c] for c in (T1, T1CE, T2, FLAIR)}
        return self._once(name, make)

    @staticmethod
    def _pick(stats, have, q):
        """``masked_percentiles(x, q, ...)`` from the order statistics of the batch: the count and the values of ``q`` (its NaN refusal
        and its NaN values for an empty selection included)"""
        count, nans, below, above = stats
        want = [have.index(v) for v in np.atleast_1d(q).tolist()]
        return percentile.percentiles_from_order_stats((count, nans, below[want], above[want]), [have[k] for k in want])

    def positive_percentiles(self, channel, q):
        """``masked_percentiles(chans[channel], q, lo=0)`` for ``q`` among ``POSITIVE_QS[channel]``; the first call selects all of them
        in all four modalities at once.  A modality without a positive voxel has count 0, and only who asks for it sees that."""
        return self._pick(self._select('positive', POSITIVE_QS, None, 0, 0.0)[channel], POSITIVE_QS[channel], q)

    @property
    def flags(self):
        """The context's flag byte: bit BRAIN = ``t1 > P5(t1[t1 > 0])`` (utils.get_brain_mask, utils.py:63-68); no bit without a
        positive T1 voxel."""
        def make():
            import torch
            flags = torch.zeros_like(self.seg)
            self.brain_into(flags, BRAIN)
            return flags
        return self._once('flags', make)

    def brain_into(self, flags, bit):
        """Sets bit ``bit`` of a step's own flag byte to the brain mask; False (and nothing set) when T1 has no positive voxel."""
        count, p5 = self.positive_percentiles(T1, 5)
        if count:
            flag_from_flags(flags, bit, x=self.chans[T1], lo=float(p5[0]))
        return bool(count)

    def brain_percentiles(self, channel, q):
        """``masked_percentiles(chans[channel], q, flags, require=brain)`` for ``q`` among ``BRAIN_QS[channel]``: the count of the brain
        mask (of its voxels that are no NaN in that channel) and the values; the first call selects all of them at once."""
        return self._pick(self._select('brain', BRAIN_QS, self.flags, 1 << BRAIN, -np.inf)[channel], BRAIN_QS[channel], q)

    # ---- the label map -------------------------------------------------------------------------------------------------
    @property
    def label_stats(self):
        """``evaluate.label_stats(seg, 8)``"""
        from . import evaluate
        return self._once('label_stats', lambda: evaluate.label_stats(self.seg, 8))

    @property
    def tumour_components(self):
        """``components.label_components(seg, 3)``: the 26-neighbour labelling of ``seg > 0`` and its component count"""
        from . import components
        return self._once('tumour_components', lambda: components.label_components(self.seg, 3))

    @property
    def tumour_distance(self):
        """City-block distance to the tumour: ``<= n`` is ``binary_dilation(seg, n)``"""
        return self._once('tumour_distance', lambda: cityblock_distance(self.seg, True))

    @property
    def background_distance(self):
        """City-block distance to the tumour's background: ``> n`` is ``binary_erosion(seg, n)``"""
        return self._once('background_distance', lambda: cityblock_distance(self.seg, False))

    def dilated_into(self, flags, bit, iterations, require=0, forbid=0):
        """Bit ``bit`` of a step's flag byte = ``binary_dilation(seg, iterations)`` and the byte's ``require`` / ``forbid`` test"""
        return flag_from_i32(flags, bit, self.tumour_distance, 0, iterations, require=require, forbid=forbid)

    def eroded_into(self, flags, bit, iterations, require=0, forbid=0):
        """Bit ``bit`` of a step's flag byte = ``binary_erosion(seg, iterations)`` and the byte's ``require`` / ``forbid`` test"""
        return flag_from_i32(flags, bit, self.background_distance, iterations + 1, require=require, forbid=forbid)


def _call(spec, ctx, zooms, rng, distance):
    """What the step's own resident function returns, on the context's tensors"""
    args = {'rng': rng, 'distance': distance}
    return spec.call(ctx.seg, dict(zip(MODALITIES, ctx.chans)), zooms, ctx=ctx, **{k: args[k] for k in spec.step_args})


def extract_all(seg, t1, t1ce, t2, flair, voxel_dims, rng=None, distance='sampled'):
    """The six steps on one resident case through one ``CaseContext`` -> ``{'step1_sequence_findings': ..., ...,
    'step6_normal_structures': ...}``, each value what the step's own resident function returns (``sequence_findings``,
    ``mass_effect`` with ``rng`` and ``distance``, ``lesion_multiplicity``, ``tumor_morphology``, ``quality_control``,
    ``normal_structures``).  Step 2 takes the voxel sizes as ``np.float32``, as its command does; the others as ``float``."""
    ctx = CaseContext(seg, t1, t1ce, t2, flair)
    return {spec.key: _call(spec, ctx, step_zooms(spec, voxel_dims, voxel_dims), rng, distance) for spec in SPECS}


# ---- the command ------------------------------------------------------------------------------------------------------
def _summary(key, res):
    """One line per step, in the style of the step commands"""
    if key == STEP_KEYS[0]:
        ce = res['contrast_enhancement']
        return (f"{ce['pattern']}; {ce['heterogeneity']}; T2/FLAIR mismatch {'detected' if res['t2_flair_mismatch']['mismatch_detected'] else 'not detected'}; "
                f"{len(res['region_signal_analysis']['regions'])} regions")
    if key == STEP_KEYS[1]:
        return (f"{res['anatomical_location']['laterality']}, {res['anatomical_location']['primary_lobe']}; midline shift {res['midline_shift']['severity']}; "
                f"herniation risk {res['herniation_risk']['risk_level']}")
    if key == STEP_KEYS[2]:
        return f"{res['component_analysis']['description']}; {res['distribution_pattern']['pattern']}; {res['enhancing_analysis']['pattern']}"
    if key == STEP_KEYS[3]:
        return (f"{res['shape_descriptors'].get('shape_classification', 'No tumor')}; {res['border_regularity']['classification']}; "
                f"{res['margin_definition']['classification']}; {res['necrosis_pattern']['pattern']}")
    if key == STEP_KEYS[4]:
        seg, art = res['segmentation_quality'], res['artifact_detection']
        return f"segmentation {seg['grade']} ({seg['quality_score']}/100); image quality {res['image_quality']['overall_quality']}; artifacts {art['severity']}"
    vent, par = res['ventricular_system'], res['parenchyma']
    return f"ventricles {vent['size_assessment']}; {vent['hydrocephalus_type']}; parenchyma {par.get('overall_assessment', par.get('assessment'))}"


def run_all_steps(input_folder, segmentation_path, output_dir, rng=None, distance='sampled', report=None):
    """run_all.py:379-476 without its compiled report: loads the four modalities and the segmentation once each, uploads each
    once, runs the six steps in order through one ``CaseContext`` and writes ``<key>.json`` into ``output_dir`` as each step
    finishes - byte for byte the file that step's own command writes - and ``comprehensive_analysis.json`` at the end.  A step
    that raises leaves the earlier files behind and the exception propagates (run_all.py:411-446).  ``report(key, result)`` is
    called after each step.  Returns the comprehensive dict."""
    Path(output_dir).mkdir(parents=True, exist_ok=True)
    case = load_case(input_folder, segmentation_path)
    ctx = CaseContext(to_device(case.labels, np.uint8), *[to_device(case.images[k].data, np.float32) for k in MODALITIES])
    return run_steps_resident(ctx, case.case_id, input_folder, segmentation_path, case.images['t1'].zooms, case.segmentation.zooms, output_dir,
                              rng, distance, report)


def run_steps_resident(ctx, case_id, input_folder, segmentation_path, t1_zooms, segmentation_zooms, output_dir, rng=None, distance='sampled',
                       report=None):
    """The running half of ``run_all_steps`` on a ``CaseContext`` that is already on the device, whoever put it there (the files of
    a case folder, or ``pipeline.analyze_resident`` with the tensors the inference driver holds): the six steps in order, each
    file written as its step finishes, ``comprehensive_analysis.json`` last.  ``input_folder`` and ``segmentation_path`` only name
    the case in the files; ``t1_zooms`` / ``segmentation_zooms`` are the voxel sizes of the two headers the step commands read."""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    all_results = {'case_id': case_id, 'analysis_timestamp': datetime.now().isoformat(), 'input_folder': str(input_folder),
                   'segmentation_path': str(segmentation_path)}          # run_all.py:453-464
    for spec in SPECS:
        zooms = step_zooms(spec, t1_zooms, segmentation_zooms)
        res = document(spec, case_id, input_folder, zooms, _call(spec, ctx, zooms, rng, distance))
        write_json(out / f"{spec.key}.json", res)
        all_results[spec.key] = res
        if report:
            report(spec.key, res)
    write_json(out / "comprehensive_analysis.json", all_results)
    return all_results


def main(argv=None):
    ap = argparse.ArgumentParser(description='All six feature-extraction steps of one case (MI355X)')
    ap.add_argument('--input', required=True, help='Input folder containing MRI sequences')
    ap.add_argument('--segmentation', required=True, help='Path to segmentation mask (NIfTI)')
    ap.add_argument('--output', required=True, help='Output folder for results')
    ap.add_argument('--distance', default='sampled', choices=mass_effect.DISTANCES, help='tumour-to-CSF distance of step 2: between sampled voxels as the reference, or exact')
    ap.add_argument('--seed', type=int, default=None, help='seed of the generator the sampled distance draws from (default: unseeded)')
    args = ap.parse_args(argv)
    case_id = case_id_and_paths(args.input)[0]
    res = run_all_steps(args.input, args.segmentation, args.output, None if args.seed is None else np.random.RandomState(args.seed), args.distance,
                        report=lambda key, r: print(f"{case_id}: {key}: {_summary(key, r)}", flush=True))
    print(f"{res['case_id']}: 7 files in {args.output}")
    return 0


if __name__ == '__main__':
    sys.exit(main())
