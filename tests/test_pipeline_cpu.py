"""No device: the host side of ``driver.main --analyze`` (brats_amd.pipeline) - the new symbol's declarations, the arguments and
their refusals, where the files go, and that nothing changes for a caller who does not ask for the analysis."""
import importlib
import inspect
import os
import re
from pathlib import Path

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: what ``driver.main``'s parser gave for ``--input a --output b`` before the analysis flags existed
BEFORE = {"input": "a", "output": "b", "results_folder": None, "folds": [0, 1, 2, 3, 4], "disable_tta": False, "step_size": 0.5, "dtype": "f32",
          "sequential": False, "label_format": "nnunet"}


def _pipeline(amd):
    return importlib.import_module(amd.__name__ + ".pipeline")


def test_the_symbol_is_declared_bound_and_in_the_build(amd):
    with open(os.path.join(ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    assert re.search(r"\bint mi355_reverse_axes\(const void \*src_dev, void \*dst_dev, int channels, int d0, int d1, int d2, int elem_bytes, void \*stream\);",
                     header)
    assert "mi355_reverse_axes" in amd._lib.EXPORTS
    with open(amd._lib.__file__, encoding="utf-8") as f:
        assert "lib.mi355_reverse_axes.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]" in f.read()
    assert "resident_case.hip" in amd._build.SOURCES and (amd._build.CSRC / "resident_case.hip").is_file()
    lib = amd._lib.load()   # (conftest's `amd` has built it)
    assert hasattr(lib, "mi355_reverse_axes")
    vo = importlib.import_module("brats_amd.volume_ops")
    assert callable(vo.reverse_axes)
    with pytest.raises(ValueError, match="uint8 or float32"):
        vo.reverse_axes(None)


def test_parser_without_the_new_flags_is_what_it_was(amd):
    args = vars(amd.driver.parse_args(["--input", "a", "--output", "b"]))
    assert {k: args[k] for k in BEFORE} == BEFORE
    assert {k: v for k, v in args.items() if k not in BEFORE} == {"analyze": False, "gt": None, "lesionwise": False, "distance": "sampled", "seed": None}
    args = vars(amd.driver.parse_args(["--input", "a", "--output", "b", "--folds", "0", "2", "--disable_tta", "--step_size", "0.75", "--dtype", "f16",
                                       "--sequential", "--label-format", "brats2021", "--results_folder", "r"]))
    assert {k: args[k] for k in BEFORE} == {"input": "a", "output": "b", "results_folder": "r", "folds": [0, 2], "disable_tta": True, "step_size": 0.75,
                                            "dtype": "f16", "sequential": True, "label_format": "brats2021"}
    assert args["analyze"] is False


def test_parser_takes_the_new_flags(amd, tmp_path):
    gt = tmp_path / "gt.nii.gz"
    gt.write_bytes(b"")
    args = amd.driver.parse_args(["--input", "a", "--output", "b", "--analyze"])
    assert (args.analyze, args.gt, args.lesionwise, args.distance, args.seed) == (True, None, False, "sampled", None)
    args = amd.driver.parse_args(["--input", "a", "--output", "b", "--analyze", "--gt", str(gt), "--lesionwise", "--distance", "exact", "--seed", "7"])
    assert (args.analyze, args.gt, args.lesionwise, args.distance, args.seed) == (True, str(gt), True, "exact", 7)
    features = importlib.import_module("brats_amd.features")
    assert amd.driver.build_parser().parse_args(["--input", "a", "--output", "b"]).distance in features.mass_effect.DISTANCES


@pytest.mark.parametrize("extra,word", [(["--analyze", "--sequential"], "--sequential"), (["--analyze", "--label-format", "brats2025"], "--label-format"),
                                        (["--analyze", "--label-format", "brats2021"], "--label-format"), (["--lesionwise"], "--analyze"),
                                        (["--analyze", "--gt", "/no/such/file.nii.gz"], "no such file"), (["--analyze", "--distance", "nearest"], "--distance"),
                                        (["--gt", "x"], "--analyze")])
def test_parser_refusals(amd, capsys, extra, word):
    with pytest.raises(SystemExit) as e:
        amd.driver.parse_args(["--input", "a", "--output", "b"] + extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_main_refuses_before_it_looks_at_anything(amd, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        amd.driver.main(["--input", str(tmp_path / "in"), "--output", str(tmp_path / "out"), "--sequential", "--analyze"])
    assert e.value.code == 2 and not (tmp_path / "out").exists()
    assert "BraTS 2021 TUMOR SEGMENTATION" not in capsys.readouterr().out


def test_where_the_files_go(amd, tmp_path):
    p = _pipeline(amd)
    assert p.brats_path("out", "c1") == Path("out/c1_brats.nii.gz")
    assert p.evaluation_path("out", "c1") == Path("out/c1_evaluation.json")
    assert p.feature_dir("out", "c1", 1) == Path("out/feature_extraction")
    assert p.feature_dir("out", "c1", 2) == Path("out/feature_extraction/c1")
    assert p.feature_dir(Path("out"), "c2", 5) == Path("out/feature_extraction/c2")
    assert p.LABEL_FORMAT == "brats2025"


def test_ground_truth_lookup(amd, tmp_path):
    p = _pipeline(amd)
    assert p.find_ground_truth(tmp_path, "c1") is None
    (tmp_path / "c1-seg.nii.gz").write_bytes(b"")
    assert p.find_ground_truth(tmp_path, "c1") == tmp_path / "c1-seg.nii.gz"
    (tmp_path / "c1_seg.nii.gz").write_bytes(b"")
    assert p.find_ground_truth(tmp_path, "c1") == tmp_path / "c1_seg.nii.gz"
    assert p.find_ground_truth(tmp_path, "c2") is None
    assert p.find_ground_truth(tmp_path, "c2", "elsewhere/gt.nii.gz") == Path("elsewhere/gt.nii.gz")


def test_defaults_keep_the_driver_as_it_was(amd):
    sig = inspect.signature(amd.preprocessing.preprocess_case)
    assert sig.parameters["return_raw"].default is False
    assert list(sig.parameters)[:4] == ["raw", "device", "plans", "spacing_zyx"]
    sig = inspect.signature(amd.driver.run_both_models)
    assert sig.parameters["analyze"].default is None and list(sig.parameters)[-1] == "analyze"
    features = importlib.import_module("brats_amd.features")
    assert list(inspect.signature(features.run_all_steps).parameters) == ["input_folder", "segmentation_path", "output_dir", "rng", "distance", "report"]
    assert callable(features.run_steps_resident)


def test_the_front_passes_its_arguments_on(amd, monkeypatch):
    p = _pipeline(amd)
    seen = []
    monkeypatch.setattr(amd.driver, "main", lambda argv=None, **kw: seen.append(list(argv)) or 0)
    assert p.main(["--input", "a", "--output", "b", "--seed", "3"]) == 0
    assert seen == [["--analyze", "--input", "a", "--output", "b", "--seed", "3"]]
