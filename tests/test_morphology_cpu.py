"""Tumour morphology (the reference's step 4) from integers and sums, without a device.

tests/golden/morphology.json holds what the reference's own step 4 (feature_extraction/step4_morphology.py, imported
unmodified by tools/gen_morphology_golden.py) returned for seeded synthetic cases.  Here what the device would deliver is
computed with scipy and numpy, so these tests pin the host arithmetic, the fixture and the interface declarations."""
import os
import re

import numpy as np
import pytest

import morphology_util as mu
from oracle import ref_shim

NEW_SYMBOLS = ("mi355_binary_morphology", "mi355_edt_squared", "mi355_surface_gradient_stats", "mi355_mask_second_moments",
               "mi355_masked_moments", "mi355_flag_from_labels", "mi355_flag_from_flags")


def test_morphology_from_stats_reproduces_the_reference(amd):
    morph = mu.morphology_module()
    fixture = mu.load_fixture()
    cmp = mu.Comparer()
    for case in fixture["cases"]:
        seg, vols = mu.fixture_data(amd, case)
        got = morph.morphology_from_stats(*mu.host_stats(morph, seg, vols), case["voxel_dims"])
        assert tuple(got) == mu.SECTIONS
        cmp.same(got, case["expected"], case["name"])
    print(f"largest relative error of a float: {cmp.worst:.3g} at {cmp.where}")


def test_fixture_reaches_the_branch_table():
    cases = {c["name"]: c for c in mu.load_fixture()["cases"]}
    exp = {k: c["expected"] for k, c in cases.items()}

    def values(section, key):
        return {e[section][key] for e in exp.values() if key in e[section]}

    assert values("shape_descriptors", "shape_classification") == {"Spherical/round", "Ovoid", "Irregular", "Highly irregular/complex"}
    assert values("shape_descriptors", "elongation_classification") == {"Elongated", "Mildly elongated", "Roughly isotropic"}
    assert values("border_regularity", "classification") >= {"No tumor", "Too small to assess", "Smooth contour", "Mildly lobulated", "Lobulated"}
    margin = values("margin_definition", "classification")
    assert "No tumor" in margin and len(margin & {"Sharp transition", "Moderate transition", "Gradual transition", "Infiltrative transition"}) >= 3
    necrosis = values("necrosis_pattern", "pattern")
    assert {"No tumor", "No necrosis"} <= necrosis
    assert len(necrosis & {"Extensive necrosis", "Moderate necrosis", "Focal necrosis", "Minimal necrosis"}) >= 2
    assert len(values("necrosis_pattern", "location") & {"Central", "Eccentric", "Peripheral"}) >= 2
    cystic = values("cystic_solid_classification", "classification")
    assert {"No tumor", "Solid"} <= cystic and len(cystic) >= 5
    # geometry: a lesion on the corner of the volume, anisotropic voxels, the BraTS grid
    corner = [c for c in cases.values() if any(p[0] == "ball" and all(v - p[3] < 0 for v in p[2]) for p in c["args"]["parts"])]
    assert corner, "no case touches the corner of its volume"
    assert [c for c in cases.values() if len(set(c["voxel_dims"])) > 1]
    assert [c for c in cases.values() if c["args"]["shape"] == [240, 240, 155]]
    for c in cases.values():  # voxel sizes exact in float32, product included (header zooms are float32)
        d = c["voxel_dims"]
        assert all(float(np.float32(v)) == v for v in d) and float(np.float32(np.prod(d))) == float(np.prod(d))
    # the no-tumour dicts with their fewer keys and their integer zeros
    none = exp["none"]
    assert none["shape_descriptors"] == {"volume_cm3": 0, "surface_area_mm2": 0, "sphericity": 0, "compactness": 0, "elongation": 1.0,
                                         "principal_axes_mm": [0, 0, 0]}
    assert set(none["necrosis_pattern"]) == {"necrosis_present", "pattern", "description"}


def test_fixture_keeps_clear_of_every_threshold():
    tool = mu.generator_tool()
    data = mu.load_fixture()
    assert tool.too_close(data) == []
    assert sum(len(tool.scores(c["expected"])) for c in data["cases"]) >= 40
    assert os.path.getsize(mu.FIXTURE) < 100 * 1024


def test_fixture_is_what_the_reference_returns_today():
    if not ref_shim.reference_available():
        pytest.skip("the reference tree is not on this machine")
    assert mu.generator_tool().generate() == mu.load_fixture()


def test_intensities_are_integers_below_2_24(amd):
    for case in mu.load_fixture()["cases"][:4]:
        _, vols = mu.fixture_data(amd, case)
        assert vols.dtype == np.float32 and np.array_equal(vols, np.rint(vols)) and 0 <= vols.min() and vols.max() < 2 ** 24


@pytest.mark.parametrize("iterations", [1, 2, 5, 10])
def test_iterated_morphology_is_the_repeated_single_step(iterations):
    """scipy switches algorithm for iterations > 1; the kernels repeat the single step, which must be the same thing"""
    mask = (np.random.RandomState(3).random_sample((12, 17, 23)) < 0.6)
    mask[0, :5, :] = True  # foreground on a face: border_value = 0 bites
    for op in (mu.erode, mu.dilate):
        step = mask.astype(np.uint8)
        for _ in range(iterations):
            step = op(step)
        assert np.array_equal(step, op(mask, iterations))


def test_new_symbols_are_declared_and_bound(amd):
    with open(os.path.join(mu.ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(amd._lib.__file__), "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym
        assert sym in amd._lib.EXPORTS, sym
        assert f"lib.{sym}.argtypes" in binding, sym
    morph = mu.morphology_module()
    for name in ("binary_erosion", "binary_dilation", "distance_transform_edt_sq", "surface_gradient_stats", "second_moments", "masked_moments",
                 "flag_from_labels", "flag_from_flags", "tumor_morphology", "morphology_from_stats"):
        assert callable(getattr(morph, name)), name
