"""-m gpu: ``driver.main --analyze`` (brats_amd.pipeline) - evaluation and feature extraction on the case the driver holds - against
the same work done at the file boundary: ``driver.main`` without the flag into another folder, then ``evaluate.main`` and
``features.main`` on files.  The case, the model folders and the seeds: tests/pipeline_util.py.

The file-boundary commands are given the ``<case>_brats.nii.gz`` the analysing run wrote, after that file has been shown to hold
``convert_labels`` of the plain run's final map (and the two runs' final maps to be equal byte for byte): the segmentation's path is
part of ``comprehensive_analysis.json``, so only one path can make the two files equal."""
import contextlib
import dataclasses
import gzip
import importlib
import io
import json
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import pipeline_util as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("step1_sequence_findings", "step2_mass_effect", "step3_multiplicity", "step4_morphology", "step5_quality", "step6_normal_structures")
LABEL_FILES = (f"{pu.CASE}.nii.gz", f"temp_model1/{pu.CASE}.nii.gz", f"temp_model2/{pu.CASE}.nii.gz")
PHRASES = ("Mean Dice Score", "Whole Tumor", "Tumor Core", "Enhancing Tumor")


def _run(amd, world, argv):
    """driver.main in this process on the shared model cache -> (return value, stdout)"""
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = amd.driver.main([str(a) for a in argv] + ["--results_folder", str(world["results"]), "--folds", "0"], model_cache=world["cache"])
    return rc, out.getvalue()


def _captured(fn, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = fn([str(a) for a in argv])
    return rc, out.getvalue()


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def _json(path):
    with open(path, encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def world(amd, gpu, tmp_path_factory):
    """The model folders, the case folder, one model cache for every run of this module, and the two runs most checks look at:
    ``plain`` (no flag) and ``joined`` (--analyze --seed 3, with ``nifti.load`` counted)."""
    tmp = tmp_path_factory.mktemp("pipeline")
    w = {"tmp": tmp, "results": tmp / "nnUNet_results", "case_dir": tmp / pu.CASE, "cache": amd.driver.ModelCache()}
    w["sds"] = pu.write_models(amd, w["results"])
    w["raw"] = pu.write_case(amd, w["case_dir"])
    w["gt"] = w["case_dir"] / f"{pu.CASE}_seg.nii.gz"
    try:
        w["plain"] = tmp / "plain"
        rc, w["plain_stdout"] = _run(amd, w, ["--input", w["case_dir"], "--output", w["plain"]])
        assert rc == 0
        loaded, real_load = [], amd.nifti.load

        def counting_load(path):
            loaded.append(str(path))
            return real_load(path)
        w["joined"] = tmp / "joined"
        amd.nifti.load = counting_load
        try:
            rc, w["joined_stdout"] = _run(amd, w, ["--input", w["case_dir"], "--output", w["joined"], "--analyze", "--seed", "3"])
        finally:
            amd.nifti.load = real_load
        assert rc == 0
        w["loaded"] = loaded
        yield w
    finally:
        w["cache"].close()


def test_the_prediction_meets_the_condition_on_the_input(amd, world):
    """Background and each of the labels 1, 2 and 3 in at least 50 voxels of the ensemble, on the device as the CPU oracle found it
    for these seeds (pipeline_util.MODEL_SEEDS)"""
    final = amd.nifti.load(world["plain"] / LABEL_FILES[0]).as_zyx()
    counts = pu.label_counts(final)
    print("voxels of background, 1, 2, 3:", counts)
    assert min(counts) >= pu.MIN_VOXELS, counts
    assert final.size == sum(counts)


def test_label_files_do_not_change(amd, world):
    for rel in LABEL_FILES:
        assert _gunzip(world["plain"] / rel) == _gunzip(world["joined"] / rel), rel
    assert "Tumor Volume Analysis" in world["joined_stdout"] and "SEGMENTATION COMPLETE" in world["joined_stdout"]
    for mod in ("0000", "0003"):
        assert (world["joined"] / "temp_model2" / "temp_input" / f"{pu.CASE}_{mod}.nii.gz").exists()
    assert not (world["plain"] / f"{pu.CASE}_brats.nii.gz").exists() and not (world["plain"] / "feature_extraction").exists()


def test_converted_label_file(amd, gpu, world):
    final = amd.nifti.load(world["plain"] / LABEL_FILES[0])
    brats = amd.nifti.load(world["joined"] / f"{pu.CASE}_brats.nii.gz")
    want = amd.evaluate.convert_labels(torch.from_numpy(np.ascontiguousarray(final.data)).to(gpu), "brats2025").cpu().numpy()
    assert brats.data.dtype == np.uint8 and np.array_equal(brats.data, want)
    like = amd.nifti.load(world["case_dir"] / f"{pu.CASE}_t1.nii.gz")
    assert brats.data.shape == like.data.shape and brats.zooms == like.zooms and np.array_equal(brats.affine, like.affine)
    assert brats.header[76:108] == like.header[76:108] and brats.header[252:328] == like.header[252:328] and brats.header[123] == like.header[123]
    assert brats.header == final.header   # the same writer, the same geometry, the same dtype


def test_feature_files_equal_the_file_boundary(amd, world):
    features = importlib.import_module("brats_amd.features")
    out = world["tmp"] / "features_at_the_file_boundary"
    brats = world["joined"] / f"{pu.CASE}_brats.nii.gz"
    rc, _ = _captured(features.main, ["--input", world["case_dir"], "--segmentation", brats, "--output", out, "--seed", "3"])
    assert rc == 0
    got_dir = world["joined"] / "feature_extraction"
    assert sorted(p.name for p in got_dir.iterdir()) == sorted([f"{k}.json" for k in STEPS] + ["comprehensive_analysis.json"])
    for key in STEPS:
        assert (got_dir / f"{key}.json").read_bytes() == (out / f"{key}.json").read_bytes(), key
    got, want = _json(got_dir / "comprehensive_analysis.json"), _json(out / "comprehensive_analysis.json")
    assert got.pop("analysis_timestamp") and want.pop("analysis_timestamp")
    assert got == want
    assert list(got) == ["case_id", "input_folder", "segmentation_path"] + list(STEPS)
    for key in STEPS:
        assert f"{pu.CASE}: {key}: " in world["joined_stdout"]


def _check_evaluation(amd, world, joined_dir, joined_stdout, extra):
    brats, ref_json = joined_dir / f"{pu.CASE}_brats.nii.gz", world["tmp"] / f"evaluation{'_'.join(extra)}.json"
    rc, ref_stdout = _captured(amd.evaluate.main, ["--pred", brats, "--gt", world["gt"], "--output", ref_json] + extra)
    assert rc == 0
    got = _json(joined_dir / f"{pu.CASE}_evaluation.json")
    assert got == _json(ref_json)
    assert ("lesionwise" in got["WT"]) == bool(extra)
    # the report: the evaluator's own block, whole and in one piece, and in it one line per phrase the orchestrator looks for
    block = ref_stdout[:ref_stdout.index("metrics written to")]
    assert block.count("\n") > 10 and block in joined_stdout
    for phrase in PHRASES:
        hits = [ln for ln in block.splitlines() if phrase in ln]
        assert len(hits) == 1 and re.search(r"\d{1,3}\.\d\d%", hits[0]), (phrase, hits)
    assert 0.0 <= got["mean_dice"] <= 1.0 and got["WT"]["surface_voxels_gt"] > 0


def test_evaluation_equals_the_file_boundary(amd, world):
    _check_evaluation(amd, world, world["joined"], world["joined_stdout"], [])


def test_evaluation_with_lesionwise_scores(amd, world):
    out = world["tmp"] / "joined_lesionwise"
    rc, stdout = _run(amd, world, ["--input", world["case_dir"], "--output", out, "--analyze", "--lesionwise", "--distance", "exact", "--gt", world["gt"]])
    assert rc == 0
    _check_evaluation(amd, world, out, stdout, ["--lesionwise"])
    assert "Lesion-wise" in stdout


def test_nothing_it_wrote_is_read_back(amd, world):
    loaded = [Path(p) for p in world["loaded"]]
    inputs = sorted(str(world["joined"] / "temp_model1" / "temp_input" / f"{pu.CASE}_{i:04d}.nii.gz") for i in range(4))
    assert sorted(str(p) for p in loaded) == sorted(inputs + [str(world["gt"])]), loaded
    assert len(loaded) == 5


def test_two_cases_one_without_a_ground_truth(amd, world):
    """A folder of two cases: ``feature_extraction/<case>/`` each; the second has no ``_seg`` file, so it is not evaluated - and says
    so - while its features are written."""
    other = "BraTS-GLI-00022-000"
    folder = world["tmp"] / "two_cases"
    folder.mkdir()
    for path in world["case_dir"].iterdir():
        shutil.copy(path, folder / path.name)
        if not path.name.endswith("_seg.nii.gz"):
            shutil.copy(path, folder / path.name.replace(pu.CASE, other))
    out = world["tmp"] / "joined_two"
    rc, stdout = _run(amd, world, ["--input", folder, "--output", out, "--analyze", "--seed", "3"])
    assert rc == 0
    for case in (pu.CASE, other):
        names = sorted(p.name for p in (out / "feature_extraction" / case).iterdir())
        assert names == sorted([f"{k}.json" for k in STEPS] + ["comprehensive_analysis.json"]), (case, names)
        assert (out / f"{case}_brats.nii.gz").exists()
    assert not any(p.is_file() for p in (out / "feature_extraction").iterdir())
    assert (out / f"{pu.CASE}_evaluation.json").exists() and not (out / f"{other}_evaluation.json").exists()
    assert f"No ground truth for {other}" in stdout and f"No ground truth for {pu.CASE}" not in stdout
    # the same voxels under another name: the same numbers (step 2 draws from a generator seeded per case)
    for key in STEPS:
        a, b = _json(out / "feature_extraction" / pu.CASE / f"{key}.json"), _json(out / "feature_extraction" / other / f"{key}.json")
        ids = (a.pop("case_id"), b.pop("case_id"))   # step 3 names a case by its input folder, as its command does
        assert ids == ((folder.name, folder.name) if key == STEPS[2] else (pu.CASE, other)), (key, ids)
        assert a == b, key
        one = _json(world["joined"] / "feature_extraction" / f"{key}.json")
        one.pop("case_id")
        assert {k: v for k, v in a.items() if k != "input_folder"} == {k: v for k, v in one.items() if k != "input_folder"}, key


def test_a_step_that_raises_leaves_what_was_written(amd, world, monkeypatch):
    """No fixture of the steps has this case's shape, so step 5 is made to raise here: steps 1-4, the three label files and the
    converted map stay, and the error leaves ``driver.main`` after the writers have been joined."""
    pipeline = importlib.import_module(amd.__name__ + ".pipeline")
    features = pipeline.features

    def refuse(*args, **kwargs):
        raise ValueError("quality_control: made to fail")
    specs = tuple(dataclasses.replace(s, call=refuse) if s.key == STEPS[4] else s for s in features.SPECS)
    monkeypatch.setattr(features, "SPECS", specs)
    out = world["tmp"] / "joined_failing"
    with pytest.raises(ValueError, match="made to fail"):
        _run(amd, world, ["--input", world["case_dir"], "--output", out, "--analyze", "--seed", "3"])
    names = sorted(p.name for p in (out / "feature_extraction").iterdir())
    assert names == sorted(f"{k}.json" for k in STEPS[:4])
    for key in STEPS[:4]:
        assert (out / "feature_extraction" / f"{key}.json").read_bytes() == (world["joined"] / "feature_extraction" / f"{key}.json").read_bytes()
    for rel in LABEL_FILES + (f"{pu.CASE}_brats.nii.gz",):
        assert _gunzip(out / rel) == _gunzip(world["joined"] / rel), rel
    assert (out / f"{pu.CASE}_evaluation.json").exists()


def test_sequential_with_analyze_is_refused_before_any_work(amd, world, capsys):
    out = world["tmp"] / "never"
    with pytest.raises(SystemExit) as e:
        amd.driver.main(["--input", str(world["case_dir"]), "--output", str(out), "--sequential", "--analyze"])
    assert e.value.code == 2 and "--sequential" in capsys.readouterr().err
    assert not out.exists()


def test_dropin_script_with_analyze(amd, world):
    """One child: the repo-root drop-in, as run_full_pipeline.py starts it, with the flag.  (``python -m brats_amd.pipeline`` is the same
    call with the flag put in front: tests/test_pipeline_cpu.py.)"""
    out = world["tmp"] / "child"
    env = dict(os.environ, MI355_NO_WORKER="1")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "run_brats2021_inference_singlethread.py"), "--input", str(world["case_dir"]),
                          "--output", str(out), "--results_folder", str(world["results"]), "--folds", "0", "--analyze", "--seed", "3"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    for rel in LABEL_FILES + (f"{pu.CASE}_brats.nii.gz",):
        assert _gunzip(out / rel) == _gunzip(world["joined"] / rel), rel
    for key in STEPS:
        assert (out / "feature_extraction" / f"{key}.json").read_bytes() == (world["joined"] / "feature_extraction" / f"{key}.json").read_bytes(), key
    got, want = _json(out / f"{pu.CASE}_evaluation.json"), _json(world["joined"] / f"{pu.CASE}_evaluation.json")
    assert got == want
    assert "Mean Dice Score" in res.stdout and "SEGMENTATION COMPLETE" in res.stdout
