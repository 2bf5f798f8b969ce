"""Lesion multiplicity from integer component tables, without a device.

tests/golden/multiplicity.json holds what the reference's own step 3 (feature_extraction/step3_multiplicity.py, imported
unmodified by tools/gen_multiplicity_golden.py) returned for seeded synthetic label maps.  Here the tables the device would
deliver are computed with scipy.ndimage.label + numpy, so these tests pin the host arithmetic and the fixture itself.
"""
import importlib.util
import os

import numpy as np
import pytest

import components_util as cu
from oracle import ref_shim

SECTIONS = ("component_analysis", "distance_analysis", "satellite_analysis", "enhancing_analysis", "distribution_pattern")


def _tables(seg):
    lab, n = cu.scipy_labels(seg > 0, 3)
    tumour = cu.numpy_stats(lab, n, seg)
    lab, n = cu.scipy_labels(seg == 3, 3)
    return tumour, cu.numpy_stats(lab, n)


def test_multiplicity_from_stats_reproduces_the_reference(amd):
    fixture = cu.load_fixture()
    assert len(fixture["cases"]) >= 9
    for case in fixture["cases"]:
        seg = cu.fixture_label_map(amd, case)
        tumour, enhancing = _tables(seg)
        got = amd.components.multiplicity_from_stats(tumour, enhancing, case["voxel_dims"])
        assert set(got) == set(SECTIONS)
        cu.assert_same(got, case["expected"], case["name"])


def test_fixture_reaches_every_branch_of_the_reference():
    cases = {c["name"]: c for c in cu.load_fixture()["cases"]}
    exp = {k: c["expected"] for k, c in cases.items()}
    n_lesions = {k: e["component_analysis"]["num_components"] for k, e in exp.items()}
    max_d = {k: e["distance_analysis"]["max_distance_mm"] for k, e in exp.items()}
    pattern = {k: e["distribution_pattern"]["pattern"] for k, e in exp.items()}
    sat = {k: e["satellite_analysis"]["has_satellites"] for k, e in exp.items()}
    foci = {k: e["enhancing_analysis"]["num_enhancing_foci"] for k, e in exp.items()}

    def some(pred):
        return [k for k in exp if pred(k)]

    assert some(lambda k: n_lesions[k] == 0 and pattern[k] == "No tumor")
    assert some(lambda k: n_lesions[k] == 1 and pattern[k] == "Solitary")
    assert some(lambda k: n_lesions[k] in (2, 3) and not sat[k] and max_d[k] < 40 and pattern[k] == "Regional multifocal")
    assert some(lambda k: n_lesions[k] in (2, 3) and not sat[k] and max_d[k] > 40 and pattern[k] == "Distant multifocal")
    assert some(lambda k: n_lesions[k] > 3 and pattern[k] == "Diffuse/scattered")
    assert some(lambda k: sat[k] and pattern[k] == "Primary with satellites"
                and all(s["distance_from_primary_mm"] < 20 for s in exp[k]["satellite_analysis"]["satellites"]))
    assert some(lambda k: exp[k]["component_analysis"].get("excluded_fragments", 0) > 0)
    ties = [k for k in exp if len({c["voxel_count"] for c in exp[k]["component_analysis"]["components"]}) < n_lesions[k]]
    assert ties, "no case with two lesions of equal voxel count"
    for k in ties:  # the stable sort keeps scipy's numbering among equals
        comps = exp[k]["component_analysis"]["components"]
        for a, b in zip(comps, comps[1:]):
            if a["voxel_count"] == b["voxel_count"]:
                assert a["id"] < b["id"]
    assert some(lambda k: foci[k] > n_lesions[k] > 0)
    assert some(lambda k: n_lesions[k] > 0 and foci[k] == 0)
    assert some(lambda k: len(set(cases[k]["voxel_dims"])) > 1)
    assert some(lambda k: cases[k]["args"]["shape"] == [240, 240, 155])
    # relationships of every kind, and the no-tumour dicts with their fewer keys
    rel = {d["relationship"] for e in exp.values() for d in e["distance_analysis"]["distances"]}
    assert rel == {"Satellite/adjacent", "Regional spread", "Distant/separate"}
    none = exp[some(lambda k: n_lesions[k] == 0)[0]]
    assert set(none["component_analysis"]) == {"num_components", "components", "is_single_lesion", "description"}
    assert set(none["distribution_pattern"]) == {"pattern", "classification"}
    # every float32-exact voxel size, product included (header zooms are float32)
    for c in cases.values():
        d = c["voxel_dims"]
        assert all(float(np.float32(v)) == v for v in d) and float(np.float32(np.prod(d))) == float(np.prod(d))


def test_fixture_is_what_the_reference_returns_today():
    if not ref_shim.reference_available():
        pytest.skip("the reference tree is not on this machine")
    spec = importlib.util.spec_from_file_location("_gen_multiplicity_golden", os.path.join(cu.ROOT, "tools", "gen_multiplicity_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.generate() == cu.load_fixture()


def test_largest_component_restatement_truth_table():
    img = np.zeros((6, 8, 20), dtype=np.uint8)
    img[1, 1, 0:5] = 1      # class 1, 5 voxels
    img[1, 3, 0:3] = 1      # class 1, 3 voxels
    img[1, 5, 0:2] = 1      # class 1, 2 voxels
    img[3, 1, 0:4] = 2      # class 2, 4 voxels
    img[3, 3, 0:4] = 2      # class 2, 4 voxels: equal maxima
    img[3, 5, 0] = 2        # class 2, 1 voxel
    img[4, 6, 1] = 2        # touches nothing of class 2 through a face ((3,5,0) is a diagonal neighbour): 6-connectivity
    img[5, 1, 0:3] = 3      # classes 3 + 4 form one region of 5 voxels
    img[5, 1, 3:5] = 4
    img[5, 4, 0:2] = 4      # and a second one of 2 voxels
    out, removed, kept = cu.largest_component_ref(img, [1], 2.0)
    assert (out == 1).sum() == 5 and removed == {1: 6.0} and kept == {1: 10.0}
    assert np.array_equal(out[img != 1], img[img != 1])
    out, removed, kept = cu.largest_component_ref(img, [2], 1.0)
    assert (out == 2).sum() == 8 and removed == {2: 1.0} and kept == {2: 4.0}          # both maxima stay
    out, removed, kept = cu.largest_component_ref(img, [1], 2.0, minimum_valid_object_size=6.0)
    assert (out == 1).sum() == 8 and removed == {1: 4.0} and kept == {1: 10.0}         # 3 voxels x 2.0 reaches 6.0
    out, removed, kept = cu.largest_component_ref(img, [1], 2.0, minimum_valid_object_size={1: 100.0})
    assert (out == 1).sum() == 5
    out, removed, kept = cu.largest_component_ref(img, [(3, 4)], 1.0)
    assert (out == 3).sum() == 3 and (out == 4).sum() == 2 and removed == {(3, 4): 2.0} and kept == {(3, 4): 5.0}
    out, removed, kept = cu.largest_component_ref(img, [1, 2, (3, 4)], 1.0)
    assert [(out == v).sum() for v in (1, 2, 3, 4)] == [5, 8, 3, 2]
    out, removed, kept = cu.largest_component_ref(np.zeros_like(img), [1], 1.0)
    assert not out.any() and removed == {1: None} and kept == {1: None}
