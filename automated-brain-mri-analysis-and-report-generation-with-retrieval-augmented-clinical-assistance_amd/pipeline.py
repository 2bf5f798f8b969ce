"""Evaluation and feature extraction on the case the inference driver holds.

The reference's orchestrator runs four programs per case - ``run_brats2021_inference_singlethread.py``, ``convert_labels_to_brats.py``,
``evaluate_segmentation.py`` and ``feature_extraction/run_all.py`` (run_full_pipeline.py:146-293, :516-565) - and each of the last
three reads back from disk what the first one had on the device a moment earlier.  ``driver.main --analyze`` joins them: after a
case's ensemble, ``analyze_resident`` takes the uploaded modalities and the ensemble's label map where they are and produces the
files of steps 3-5 with the same code that writes them at the file boundary (``evaluate``, ``features.run_steps_resident``).

The driver keeps a volume in file order, [Z, Y, X]; the evaluator and the feature steps take (x, y, z) volumes.  The hand-off is
``volume_ops.reverse_axes`` (csrc/resident_case.hip): one launch for the four modalities, one for the label map, nothing uploaded a
second time, no transpose on the host.  The only file read beside the four modalities is the ground truth, once.

As a command, a thin front of the drop-in with ``--analyze`` set (every other argument of ``brats_amd.driver`` passes through):

    python -m brats_amd.pipeline --input CASE_DIR --output OUT [--gt SEG.nii.gz] [--lesionwise] [--distance sampled|exact] [--seed N]
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

from . import evaluate, features, nifti
from .volume_ops import reverse_axes

LABEL_FORMAT = "brats2025"   # what convert_labels_to_brats.py writes by default and the evaluator and the feature steps read


def brats_path(output_folder, case_name):
    """The converted label map, where run_full_pipeline.py:532 puts it"""
    return Path(output_folder) / f"{case_name}_brats.nii.gz"


def evaluation_path(output_folder, case_name):
    return Path(output_folder) / f"{case_name}_evaluation.json"


def feature_dir(output_folder, case_name, n_cases):
    """``<output>/feature_extraction`` for an input folder that holds one case (run_full_pipeline.py:561); one folder per case beneath
    it when it holds several"""
    base = Path(output_folder) / "feature_extraction"
    return base if n_cases <= 1 else base / case_name


def find_ground_truth(input_folder, case_name, gt=None):
    """``gt`` when given, else ``<input>/<case>_seg.nii.gz``, else ``<input>/<case>-seg.nii.gz``, else None"""
    if gt is not None:
        return Path(gt)
    for name in (f"{case_name}_seg.nii.gz", f"{case_name}-seg.nii.gz"):
        if (Path(input_folder) / name).is_file():
            return Path(input_folder) / name
    return None


def analyze_resident(raw, ens, like, case_name, n_cases, submit, *, input_folder, output_folder, gt=None, lesionwise=False, distance="sampled",
                     seed=None):
    """raw: CUDA float32 [4, Z, Y, X], the modalities as uploaded (T1, T1ce, T2, FLAIR); ens: CUDA uint8 [Z, Y, X], the ensemble's
    labels in the nnU-Net convention; like: the case's geometry (the T1 image); ``submit(fn, *args)``: the driver's background
    writer pool.  Writes ``<case>_brats.nii.gz``, ``<case>_evaluation.json`` when there is a ground truth (and prints the report
    whose four Dice lines run_full_pipeline.py:252-269 parses), and the seven files of ``feature_dir``.  The voxel sizes are those of
    ``like``: the prediction, the file written from it and the ground truth of a case lie on one grid.  A feature step that raises
    leaves the files before it in place; the driver joins the pending writes and lets the exception through.

    Must run while nothing else is in flight on the device (``driver.run_both_models`` calls it after its synchronise): hole filling
    and the other primitives with library-owned scratch do not share the device with the side stream's preprocessing."""
    import torch
    if raw.dim() != 4 or raw.shape[0] != 4 or tuple(raw.shape[1:]) != tuple(ens.shape):
        raise ValueError(f"analyze_resident: modalities {tuple(raw.shape)} and labels {tuple(ens.shape)} (four channels of the label map's shape)")
    labels_xyz = reverse_axes(evaluate.convert_labels(ens, LABEL_FORMAT))
    chans_xyz = reverse_axes(raw.contiguous())
    seg_path = brats_path(output_folder, case_name)
    submit(nifti.save_like, seg_path, labels_xyz.cpu().numpy(), like)
    zooms = like.zooms[:3]
    gt_path = find_ground_truth(input_folder, case_name, gt)
    if gt_path is None:
        print(f"No ground truth for {case_name} ({case_name}_seg.nii.gz): evaluation skipped")
    else:
        gt_map = np.ascontiguousarray(np.round(nifti.load(gt_path).data).astype(np.uint8))   # (x, y, z), as case_io.load_case
        if gt_map.shape != tuple(labels_xyz.shape):
            raise ValueError(f"shape mismatch: prediction {tuple(labels_xyz.shape)}, ground truth {gt_map.shape} ({gt_path})")
        gt_dev = torch.from_numpy(gt_map).to(labels_xyz.device)
        res = (evaluate.evaluate_lesionwise if lesionwise else evaluate.evaluate_with_surfaces)(labels_xyz, gt_dev, zooms)
        print("\n".join(evaluate.report_lines(res, str(seg_path), str(gt_path))))
        with open(evaluation_path(output_folder, case_name), "w") as f:
            json.dump(res, f, indent=2)
        print(f"metrics written to {evaluation_path(output_folder, case_name)}")
    ctx = features.CaseContext(labels_xyz, *chans_xyz.unbind(0))
    out = feature_dir(output_folder, case_name, n_cases)
    features.run_steps_resident(ctx, case_name, input_folder, seg_path, like.zooms, like.zooms, out,
                                None if seed is None else np.random.RandomState(seed), distance,
                                report=lambda key, r: print(f"{case_name}: {key}: {features._summary(key, r)}", flush=True))
    print(f"{case_name}: 7 files in {out}")


def main(argv=None):
    from . import driver
    return driver.main(["--analyze"] + list(sys.argv[1:] if argv is None else argv))


if __name__ == "__main__":
    sys.exit(main())
