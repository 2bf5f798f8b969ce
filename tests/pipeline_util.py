"""The synthetic case and model folders of the resident-pipeline tests (tests/test_gpu_pipeline.py), and the seed search behind them.

One case of 40 x 48 x 44 voxels (Z, Y, X) with voxel sizes 1.0 x 0.9 x 1.2 mm: a ground truth from ``synthetic.label_map``, and four
modalities from ``synthetic.mri_for_normal_structures`` with a central ventricle, so that all six feature steps have what they read
(step 6 refuses a case in which no ventricle is found).  The plans of the model folders name the case's own spacing, so the
driver does not resample and ``oracle.driver_ref.predict_case`` restates it.

The ensemble's label map must hold background and each of the labels 1, 2 and 3 in at least 50 voxels.  The seeds below were
chosen on the CPU:

    python tests/pipeline_util.py          # prints the label counts of the oracle's ensemble for MODEL_SEEDS

Model seeds (A, B) = (21, 31), case seed 11: background 18082, label 1 6766, label 2 21903, label 3 37729 voxels (of 84480), the
tumour in 26 components.  (Of eighteen seed pairs tried most leave under 50 voxels of background - untrained networks call nearly
everything tumour - and one, (61, 71), gives a map on which the reference's step 6 raises.)
"""
import os
import sys

import numpy as np

CASE = "BraTS-GLI-00021-000"
SHAPE_XYZ = (44, 48, 40)
ZOOMS_XYZ = (1.0, 0.9, 1.2)
PATCH = (32, 32, 32)
CASE_SEED = 11
MODEL_SEEDS = (21, 31)          # synthetic.make_model("A", seed=...), ("B", seed=...), one fold each
MIN_VOXELS = 50
LESIONS = [((15.0, 30.0, 24.0), 7.0), ((31.0, 14.0, 12.0), 4.0)]
VENTRICLES = [["obox", (15, 16, 13), (29, 32, 27)]]
MODALITIES = ("t1", "t1ce", "t2", "flair")


def case_arrays(amd, seed=CASE_SEED):
    """(ground truth uint8 (x, y, z), modalities float32 [4, x, y, z] with integer values)"""
    seg = amd.synthetic.label_map(seed, SHAPE_XYZ, LESIONS)
    vols = amd.synthetic.mri_for_normal_structures(seed + 1, seg, ventricles=VENTRICLES, contrast=0.5, enhancement=1.8)
    return seg, vols


def write_case(amd, folder, case=CASE, seed=CASE_SEED, with_gt=True):
    """Writes ``<case>_{t1,t1ce,t2,flair}.nii.gz`` (int16) and ``<case>_seg.nii.gz`` into ``folder``; returns the raw [4, Z, Y, X]
    float32 array the driver reads from those files."""
    seg, vols = case_arrays(amd, seed)
    like = amd.nifti.make_header(SHAPE_XYZ, zooms=ZOOMS_XYZ, origin=(0.0, -239.0, 0.0))
    os.makedirs(folder, exist_ok=True)
    for c, mod in enumerate(MODALITIES):
        amd.nifti.save_like(os.path.join(folder, f"{case}_{mod}.nii.gz"), vols[c].astype(np.int16), like)
    if with_gt:
        amd.nifti.save_like(os.path.join(folder, f"{case}_seg.nii.gz"), seg, like)
    return np.ascontiguousarray(vols.transpose(0, 3, 2, 1))


def model_state_dicts(amd, seeds=MODEL_SEEDS):
    return [amd.synthetic.make_model(preset, seed=s, num_pool=2, max_feat=128)[0] for preset, s in zip("AB", seeds)]


def write_models(amd, results, seeds=MODEL_SEEDS):
    """The two model folders under ``results`` (one fold each), with plans at the case's spacing: no resampling"""
    base = os.path.join(results, "3d_fullres", "Task500_BraTS2021")
    plans = amd.checkpoint.default_brats_plans(PATCH)
    plans["plans_per_stage"][0]["current_spacing"] = np.array(ZOOMS_XYZ[::-1], dtype=np.float64)
    sds = model_state_dicts(amd, seeds)
    for name, sd in zip((amd.driver.MODEL1, amd.driver.MODEL2), sds):
        amd.checkpoint.save_model_folder(os.path.join(base, name), name.split("__")[0], [sd], plans)
    return sds


def oracle_ensemble(raw_zyx, sds):
    """The driver's final label map [Z, Y, X] as the CPU oracle computes it"""
    from oracle import driver_ref, unet_ref
    seg1 = driver_ref.predict_case(raw_zyx, [sds[0]], unet_ref.default_cfg("batch"), PATCH)[0]
    seg2 = driver_ref.predict_case(raw_zyx, [sds[1]], unet_ref.default_cfg("group", 16), PATCH)[0]
    return driver_ref.label_ensemble(seg1, seg2)


def label_counts(seg):
    return [int((seg == v).sum()) for v in range(4)]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import brats_amd
    _, vols = case_arrays(brats_amd)
    counts = label_counts(oracle_ensemble(np.ascontiguousarray(vols.transpose(0, 3, 2, 1)), model_state_dicts(brats_amd)))
    print(f"model seeds {MODEL_SEEDS}, case seed {CASE_SEED}: voxels of background, 1, 2, 3 = {counts}")
    sys.exit(0 if min(counts) >= MIN_VOXELS else 1)
