"""``brats_amd.features``: the six steps through one ``CaseContext`` return what they return alone, in any order, and the command
writes the files the six step commands write, loading each of the five files once."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import morphology_util as mu
import normal_structures_util as nu
import quality_util as qu
import sequence_findings_util as su

pytestmark = pytest.mark.gpu

SMALL = [48, 56, 40]
FIXTURES = (("normal_structures", nu.load_fixture, lambda amd, c: nu.fixture_data(c)), ("quality", qu.load_fixture, lambda amd, c: qu.fixture_data(c)),
            ("sequence_findings", su.load_fixture, lambda amd, c: su.fixture_data(c)), ("morphology", mu.load_fixture, mu.fixture_data))
CASES = [(name, c["name"]) for name, load, _ in FIXTURES for c in load()["cases"] if list(c["args"]["shape"]) == SMALL]
STEP_KEYS = ("step1_sequence_findings", "step2_mass_effect", "step3_multiplicity", "step4_morphology", "step5_quality", "step6_normal_structures")
STEP_COMMANDS = ("sequence_findings", "mass_effect", "multiplicity", "morphology", "quality", "normal_structures")
TOP_KEYS = ["case_id", "analysis_timestamp", "input_folder", "segmentation_path", *STEP_KEYS]


def _mod(name):
    return importlib.import_module("brats_amd." + name)


def _host_case(amd, fixture, case_name):
    load, data = [(l, d) for n, l, d in FIXTURES if n == fixture][0]
    case = [c for c in load()["cases"] if c["name"] == case_name][0]
    seg, vols = data(amd, case)
    return seg, vols, case["voxel_dims"]


def _device_case(amd, gpu, fixture, case_name):
    seg, vols, zooms = _host_case(amd, fixture, case_name)
    return torch.from_numpy(np.array(seg)).to(gpu), [torch.from_numpy(np.array(v)).to(gpu) for v in vols], zooms


def _calls(seg, chans, zooms, ctx, rng, distance, order=range(6)):
    """The six resident functions as ``features.extract_all`` calls them (step 2 with float32 zooms), each outcome either
    ('ok', json text) or ('raised', type, message)"""
    z, z2 = [float(v) for v in zooms], [np.float32(v) for v in zooms]
    kw = {} if ctx is None else {"ctx": ctx}
    steps = (lambda: _mod("sequence_findings").sequence_findings(seg, *chans, z, **kw),
             lambda: _mod("mass_effect").mass_effect(seg, chans[0], z2, rng, distance, **kw),
             lambda: _mod("components").lesion_multiplicity(seg, z, **kw),
             lambda: _mod("morphology").tumor_morphology(seg, *chans, z, **kw),
             lambda: _mod("quality").quality_control(seg, *chans, z, **kw),
             lambda: _mod("normal_structures").normal_structures(seg, *chans, z, **kw))
    out = {}
    for k in order:
        try:
            out[k] = ("ok", json.dumps(steps[k]()))
        except Exception as e:  # the same exception is expected from both ways of calling
            out[k] = ("raised", type(e).__name__, str(e))
    return [out[k] for k in range(6)]


def test_enough_small_cases_are_covered():
    assert len(CASES) >= 40 and len(set(CASES)) == len(CASES)
    names = {c for _, c in CASES}
    assert {"no_tumour", "tumour_covers_brain", "none_zero_t1", "zero_t1", "no_brain_mask", "empty_brain", "aniso", "solid_ncr"} <= names


@pytest.mark.parametrize("fixture,case_name", CASES, ids=[f"{f}-{c}" for f, c in CASES])
def test_sharing_changes_nothing(amd, gpu, fixture, case_name):
    seg, chans, zooms = _device_case(amd, gpu, fixture, case_name)
    plain = _calls(seg, chans, zooms, None, None, "exact")
    ctx = _mod("features").CaseContext(seg, *chans)
    shared = _calls(seg, chans, zooms, ctx, None, "exact")
    for k in range(6):
        assert shared[k] == plain[k], (STEP_KEYS[k], case_name)
    if all(p[0] == "ok" for p in plain):
        both = _mod("features").extract_all(seg, *chans, zooms, distance="exact")
        assert list(both) == list(STEP_KEYS) and [json.dumps(both[k]) for k in STEP_KEYS] == [p[1] for p in plain]


def test_sharing_changes_nothing_under_the_sampled_distance(amd, gpu):
    seg, chans, zooms = _device_case(amd, gpu, "normal_structures", "moderate_left_adjacent")
    plain = _calls(seg, chans, zooms, None, np.random.RandomState(7), "sampled")
    shared = _calls(seg, chans, zooms, _mod("features").CaseContext(seg, *chans), np.random.RandomState(7), "sampled")
    assert shared == plain and plain[1][0] == "ok"
    assert json.loads(plain[1][1])["ventricular_compression"]["tumor_to_ventricle_distance_mm"] is not None
    both = _mod("features").extract_all(seg, *chans, zooms, rng=np.random.RandomState(7))
    assert json.dumps(both["step2_mass_effect"]) == plain[1][1]


@pytest.mark.parametrize("fixture,case_name", [("normal_structures", "moderate_left_adjacent"), ("quality", "bias_severe_ghost"),
                                               ("sequence_findings", "no_brain_mask"), ("normal_structures", "empty_brain")])
def test_the_order_of_the_steps_does_not_matter(amd, gpu, fixture, case_name):
    seg, chans, zooms = _device_case(amd, gpu, fixture, case_name)
    forward = _calls(seg, chans, zooms, _mod("features").CaseContext(seg, *chans), None, "exact")
    backward = _calls(seg, chans, zooms, _mod("features").CaseContext(seg, *chans), None, "exact", order=(5, 4, 3, 2, 1, 0))
    assert backward == forward


def test_the_context_checks_its_tensors_once(amd, gpu):
    f = _mod("features")
    seg, chans, zooms = _device_case(amd, gpu, "sequence_findings", "ring")
    with pytest.raises(ValueError, match="values above 4"):
        f.CaseContext(seg + 5 * (seg == 1).to(torch.uint8), *chans)
    with pytest.raises(ValueError, match="differ in shape"):
        f.CaseContext(seg, chans[0], chans[1][:, :, :-1], chans[2], chans[3])
    with pytest.raises(ValueError, match="float32"):
        f.CaseContext(seg, chans[0].double(), *chans[1:])
    ctx = f.CaseContext(seg, *chans)
    with pytest.raises(ValueError, match="not the ones the context holds"):
        _mod("quality").quality_control(seg, chans[1], chans[0], chans[2], chans[3], zooms, ctx=ctx)
    with pytest.raises(ValueError, match="distance 'nearest'"):
        _mod("mass_effect").mass_effect(seg, chans[0], zooms, None, "nearest", ctx=ctx)


# ---- the command ------------------------------------------------------------------------------------------------------
def _write_case(amd, tmp_path, scheme, fixture, case_name):
    seg, vols, zooms = _host_case(amd, fixture, case_name)
    case_id = "BraTS2021_00042" if scheme == "brats2021" else "BraTS-GLI-00042-000"
    names = ("_t1", "_t1ce", "_t2", "_flair") if scheme == "brats2021" else ("-t1n", "-t1c", "-t2w", "-t2f")
    case_dir = tmp_path / "some_folder"
    case_dir.mkdir()
    for v, suffix in zip(vols, names):
        amd.nifti.save_like(case_dir / f"{case_id}{suffix}.nii.gz", v.astype(np.int16), amd.nifti.make_header(seg.shape, zooms=tuple(zooms), dtype=np.int16))
    amd.nifti.save_like(tmp_path / "seg.nii.gz", seg, amd.nifti.make_header(seg.shape, zooms=tuple(zooms), dtype=np.uint8))
    return case_id, case_dir, tmp_path / "seg.nii.gz"


def _run_command(case_dir, seg_path, out_dir, extra):
    env = dict(os.environ, PYTHONPATH=mu.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "brats_amd.features", "--input", str(case_dir), "--segmentation", str(seg_path), "--output", str(out_dir),
                           *extra], capture_output=True, text=True, env=env, cwd=mu.ROOT, timeout=300)


@pytest.mark.parametrize("extra", [("--distance", "exact"), ("--seed", "3")], ids=["exact", "seed3"])
@pytest.mark.parametrize("scheme,case_name", [("brats2021", "moderate_left_adjacent"), ("brats2025", "edge_joined_pair")])
def test_the_command_writes_the_files_of_the_six_step_commands(amd, gpu, tmp_path, capsys, scheme, case_name, extra):
    case_id, case_dir, seg_path = _write_case(amd, tmp_path, scheme, "normal_structures", case_name)
    out = tmp_path / "results"
    res = _run_command(case_dir, seg_path, out, extra)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 7 and all(line.startswith(case_id + ": ") for line in lines), res.stdout
    assert [line.split(": ")[1] for line in lines[:6]] == list(STEP_KEYS)
    assert sorted(p.name for p in out.iterdir()) == sorted([f"{k}.json" for k in STEP_KEYS] + ["comprehensive_analysis.json"])
    alone = tmp_path / "alone"
    for key, command in zip(STEP_KEYS, STEP_COMMANDS):   # the step's own command, in this process
        argv = ["--input", str(case_dir), "--segmentation", str(seg_path), "--output", str(alone / f"{key}.json")]
        assert _mod(command).main(argv + (list(extra) if command == "mass_effect" else [])) == 0
        assert (out / f"{key}.json").read_bytes() == (alone / f"{key}.json").read_bytes(), key
    capsys.readouterr()
    whole = json.loads((out / "comprehensive_analysis.json").read_text())
    assert list(whole) == TOP_KEYS
    assert whole["case_id"] == case_id and whole["input_folder"] == str(case_dir) and whole["segmentation_path"] == str(seg_path)
    assert isinstance(whole["analysis_timestamp"], str) and len(whole["analysis_timestamp"]) >= 19
    for key in STEP_KEYS:
        assert whole[key] == json.loads((out / f"{key}.json").read_text()), key
    assert whole["step3_multiplicity"]["case_id"] == "some_folder"   # step 3 names the case after its folder


def test_each_file_is_loaded_once(amd, gpu, tmp_path, monkeypatch):
    _, case_dir, seg_path = _write_case(amd, tmp_path, "brats2021", "normal_structures", "mild_symmetric")
    loaded = []
    load = amd.nifti.load
    monkeypatch.setattr(amd.nifti, "load", lambda path: (loaded.append(os.path.basename(str(path))), load(path))[1])
    seen = []
    res = _mod("features").run_all_steps(case_dir, seg_path, tmp_path / "results", distance="exact", report=lambda key, r: seen.append(key))
    assert len(loaded) == 5 and len(set(loaded)) == 5, loaded
    assert seen == list(STEP_KEYS) and list(res) == TOP_KEYS


def test_a_raising_step_leaves_the_earlier_files_and_no_compilation(amd, gpu, tmp_path):
    _, case_dir, seg_path = _write_case(amd, tmp_path, "brats2021", "normal_structures", "empty_brain")
    out = tmp_path / "results"
    res = _run_command(case_dir, seg_path, out, ("--distance", "exact"))
    assert res.returncode != 0 and "Traceback" in res.stderr and "a threshold is NaN" in res.stderr, res.stdout + res.stderr  # step 4, as alone
    written = sorted(p.name for p in out.iterdir())
    assert written == [f"{k}.json" for k in STEP_KEYS[:3]], written   # T1 is zero: steps 1 to 3 cope, step 4 takes a percentile of nothing
    assert len(res.stdout.strip().splitlines()) == len(written)
