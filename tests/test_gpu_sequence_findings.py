"""Sequence findings (the reference's step 1) on the MI355X: the flag byte equals its numpy restatement, the dicts
equal what the reference's step 1 returned (tests/golden/sequence_findings.json; a std within 1e-9 relative, everything else
exactly), and step 4's region flags are still those of the host percentiles.  The child processes this file starts run under a
time limit of their own; nothing is retried."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import morphology_util as mu
import sequence_findings_util as su

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sf(amd):
    return su.module("sequence_findings")


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)  # (a copy: the cached fixture arrays are read-only)


def _run_case(sf, gpu, case):
    seg, vols = su.fixture_data(case)
    return sf.sequence_findings(_dev(seg, gpu), *(_dev(v, gpu) for v in vols), case["voxel_dims"])


def test_flag_byte_equals_the_numpy_restatement(sf, gpu):
    for case in su.load_fixture()["cases"]:
        seg, vols = su.fixture_data(case)
        got = sf.region_flags(_dev(seg, gpu), [_dev(v, gpu) for v in vols]).cpu().numpy()
        want = su.flag_map(sf, seg, vols)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (case["name"], int((got != want).sum()))


def test_sequence_findings_equal_the_reference(sf, gpu):
    cmp = su.Comparer()
    for case in su.load_fixture()["cases"]:
        got = _run_case(sf, gpu, case)
        assert tuple(got) == su.SECTIONS
        cmp.same(got, case["expected"], case["name"])
    print(f"sequence_findings: largest relative error of a std {cmp.worst:.3g} at {cmp.where}")


def test_repeats_are_bit_equal_and_bad_label_maps_are_refused(sf, gpu):
    case = [c for c in su.load_fixture()["cases"] if c["name"] == "ring"][0]
    one, two = _run_case(sf, gpu, case), _run_case(sf, gpu, case)
    assert json.dumps(one, sort_keys=True) == json.dumps(two, sort_keys=True)  # every float bit for bit
    seg, vols = su.fixture_data(case)
    bad = seg.copy()
    bad[0, 0, 0] = 5
    with pytest.raises(ValueError, match="above 4"):
        sf.sequence_findings(_dev(bad, gpu), *(_dev(v, gpu) for v in vols), case["voxel_dims"])
    with pytest.raises(ValueError, match="differ in shape"):
        sf.sequence_findings(_dev(seg, gpu), *(_dev(v[:-1], gpu) for v in vols), case["voxel_dims"])


@pytest.mark.parametrize("scheme,case_name", [("brats2021", "solid_ncr"), ("brats2025", "label4_no_ncr")])
def test_sequence_findings_command_writes_the_json(amd, gpu, tmp_path, scheme, case_name):
    case = [c for c in su.load_fixture()["cases"] if c["name"] == case_name][0]
    seg, vols = su.fixture_data(case)
    zooms = tuple(case["voxel_dims"])
    case_id = "BraTS2021_00042" if scheme == "brats2021" else "BraTS-GLI-00042-000"
    names = ("_t1", "_t1ce", "_t2", "_flair") if scheme == "brats2021" else ("-t1n", "-t1c", "-t2w", "-t2f")
    case_dir = tmp_path / "some_folder"
    case_dir.mkdir()
    for v, suffix in zip(vols, names):
        amd.nifti.save_like(case_dir / f"{case_id}{suffix}.nii.gz", v.astype(np.int16), amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.int16))
    amd.nifti.save_like(tmp_path / "seg.nii.gz", seg, amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.uint8))
    out = tmp_path / "results" / "step1.json"
    env = dict(os.environ, PYTHONPATH=su.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "brats_amd.sequence_findings", "--input", str(case_dir), "--segmentation", str(tmp_path / "seg.nii.gz"),
                          "--output", str(out)], capture_output=True, text=True, env=env, cwd=su.ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert len(res.stdout.strip().splitlines()) == 1 and res.stdout.startswith(case_id + ": "), res.stdout
    got = json.loads(out.read_text())
    assert list(got) == ["case_id", "step", "voxel_info", *su.SECTIONS, "sequences_analyzed", "diffusion_available", "diffusion_note"]
    assert got["case_id"] == case_id and got["step"] == "Step 1 - Sequence-specific findings"
    assert got["voxel_info"]["dimensions_mm"] == case["voxel_dims"]
    assert got["sequences_analyzed"] == ["T1", "T1ce", "T2", "FLAIR"] and got["diffusion_available"] is False
    su.Comparer().same({k: got[k] for k in su.SECTIONS}, case["expected"], case_name)


def test_morphology_region_flags_still_equal_the_host_percentiles(amd, gpu):
    """step 4 takes its three thresholds from the device percentiles now: the flag byte must be the one csf_thresholds gives"""
    morph = mu.morphology_module()
    pct = su.module("percentile")
    for case in mu.load_fixture()["cases"]:
        if case["args"]["shape"] == [240, 240, 155]:
            continue  # (test_gpu_morphology.py's end-to-end test runs it through the same path; test_gpu_percentile.py has a volume of its size)
        seg, vols = mu.fixture_data(amd, case)
        t1, t2, flair = (_dev(vols[c], gpu) for c in (morph.T1, morph.T2, morph.FLAIR))
        got = (float(pct.masked_percentiles(t1, 10, lo=0)[1][0] * 1.5), float(pct.masked_percentiles(t2, 85, lo=0)[1][0] * 0.8),
               float(pct.masked_percentiles(flair, 20, lo=0)[1][0] * 2))
        assert got == morph.csf_thresholds(*(vols[c].astype(np.float64) for c in (morph.T1, morph.T2, morph.FLAIR))), case["name"]
        flags = morph.region_flags(_dev(seg, gpu), t1, t2, flair).cpu().numpy()
        assert np.array_equal(flags, mu.flag_map(morph, seg, vols)), case["name"]
