"""-m gpu: the drop-in with and without ``--uncertainty`` on the case and the model folders of tests/pipeline_util.py (driver.main in
this process, one model cache): every product of the plain run stays byte-identical after gunzip, the three new files appear, the
maps carry the input's geometry and are zero outside the crop box, and the JSON's counts are those of a recount from
predictor.predict_folds_moments on the same tensors."""
import contextlib
import gzip
import io
import json
import os

import numpy as np
import pytest
import torch

import pipeline_util as pu

pytestmark = pytest.mark.gpu
NEW = (f"{pu.CASE}_entropy.nii.gz", f"{pu.CASE}_std.nii.gz", f"{pu.CASE}_uncertainty.json")
REGIONS = ("whole_tumor", "tumor_core", "enhancing_tumor")


def _run(amd, world, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = amd.driver.main([str(a) for a in argv] + ["--results_folder", str(world["results"]), "--folds", "0"], model_cache=world["cache"])
    return rc, out.getvalue()


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _content(path):
    if str(path).endswith(".gz"):
        with gzip.open(path, "rb") as f:
            return f.read()
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def world(amd, gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("uncertainty")
    w = {"tmp": tmp, "results": tmp / "nnUNet_results", "case_dir": tmp / pu.CASE, "cache": amd.driver.ModelCache()}
    pu.write_models(amd, w["results"])
    w["raw"] = pu.write_case(amd, w["case_dir"])
    try:
        for tag, flags in (("plain", []), ("unc", ["--uncertainty"])):
            w[tag] = tmp / tag
            rc, w[tag + "_stdout"] = _run(amd, w, ["--input", w["case_dir"], "--output", w[tag]] + flags)
            assert rc == 0
        with open(w["unc"] / NEW[2], encoding="utf-8") as f:
            w["doc"] = json.load(f)
        yield w
    finally:
        w["cache"].close()


def test_every_plain_product_is_unchanged_and_three_files_are_new(world):
    plain, unc = _files(world["plain"]), _files(world["unc"])
    assert sorted(set(unc) - set(plain)) == sorted(NEW) and set(plain) <= set(unc), (plain, unc)
    for rel in plain:
        assert _content(world["plain"] / rel) == _content(world["unc"] / rel), rel
    strip = lambda s: [l for l in s.splitlines() if "cm3" in l]
    assert strip(world["plain_stdout"]) == strip(world["unc_stdout"]) and len(strip(world["plain_stdout"])) == 5


def test_the_maps_have_the_inputs_geometry_and_are_zero_outside_the_crop_box(amd, world):
    like = amd.nifti.load(world["case_dir"] / f"{pu.CASE}_t1.nii.gz")
    raw = world["raw"]
    base = world["results"] / "3d_fullres" / "Task500_BraTS2021"
    plans = world["cache"].get(base / amd.driver.MODEL1, (0,), "f32").folder.plans
    _, props = amd.preprocessing.preprocess_case(raw, plans=plans, spacing_zyx=tuple(reversed(like.zooms)))
    outside = np.ones(raw.shape[1:], bool)
    outside[tuple(slice(int(b[0]), int(b[1])) for b in props["crop_bbox"])] = False
    print("voxels outside the crop box:", int(outside.sum()))
    for name in NEW[:2]:
        img = amd.nifti.load(world["unc"] / name)
        assert img.data.shape == pu.SHAPE_XYZ and img.data.dtype == np.float32
        assert np.allclose(img.zooms, pu.ZOOMS_XYZ) and bytes(img.header[252:328]) == bytes(like.header[252:328])
        m = img.as_zyx()
        assert np.isfinite(m).all() and m.min() >= 0 and m.max() <= 1 and m.max() > 0
        assert (m[outside] == 0).all()


def test_the_json_counts_are_a_recount(amd, world):
    """mean of each member from predict_folds_moments on the tensor the driver preprocesses; the ensemble's is (a + b) / 2 in fp32;
    counts are exact integers"""
    doc = world["doc"]
    assert doc["thresholds"] == [0.25, 0.5, 0.75] and doc["regions"] == list(REGIONS) and doc["case"] == pu.CASE
    assert doc["samples"] == {"folds": [1, 1], "mirrors": 8, "models": 2}
    like = amd.nifti.load(world["case_dir"] / f"{pu.CASE}_t1.nii.gz")
    base = world["results"] / "3d_fullres" / "Task500_BraTS2021"
    models = [world["cache"].get(base / m, (0,), "f32") for m in (amd.driver.MODEL1, amd.driver.MODEL2)]
    data, props = amd.preprocessing.preprocess_case(world["raw"], plans=models[0].folder.plans, spacing_zyx=tuple(reversed(like.zooms)))
    means = []
    for m in models:
        mean, m2 = amd.predictor.predict_folds_moments(m.nets, data, m.patch_size, 0.5, True, (0, 1, 2), True, m.nonlin)
        assert torch.equal(mean, amd.predictor.predict_folds(m.nets, data, m.patch_size, 0.5, True, (0, 1, 2), True, m.nonlin))
        means.append(mean.cpu().numpy())
    cm3 = float(np.prod(like.zooms)) / 1000.0
    blocks = [doc["ensemble"]] + doc["members"]
    for block, mean in zip(blocks, [(means[0] + means[1]) / np.float32(2)] + means):
        for k, name in enumerate(REGIONS):
            n25, n50, n75 = (int((mean[k] > np.float32(t)).sum()) for t in (0.25, 0.5, 0.75))
            b = block[name]
            assert b["voxels"] == n50 and b["volume_cm3"] == n50 * cm3 and b["volume_interval_cm3"] == [n75 * cm3, n25 * cm3], (name, b)
            assert b["volume_interval_cm3"][0] <= b["volume_cm3"] <= b["volume_interval_cm3"][1]
            assert b["boundary_fraction"] == (n25 - n75) / max(n50, 1)
            assert abs(b["expected_volume_cm3"] - float(mean[k].astype(np.float64).sum()) * cm3) <= 1e-9 * mean[k].size * cm3
            if n50:
                assert 0.5 < b["mean_confidence"] <= 1 and 0 <= b["mean_entropy_bits"] <= 1 and 0 <= b["mean_std"] <= b["max_std"] <= 0.5
    assert sum(doc["ensemble"][r]["voxels"] for r in REGIONS) > 0
    assert all(0 <= doc["member_agreement"][r] <= 1 for r in REGIONS)


def test_uncertainty_with_sequential_is_refused_before_anything_is_loaded(amd, world):
    err = io.StringIO()
    with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(err):
        amd.driver.main(["--input", str(world["case_dir"]), "--output", str(world["tmp"] / "never"), "--uncertainty", "--sequential",
                         "--results_folder", str(world["tmp"] / "no_such_models")])
    assert e.value.code not in (0, None) and "--sequential" in err.getvalue()
    assert not (world["tmp"] / "never").exists()
