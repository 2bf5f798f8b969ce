"""Normal-structures assessment (the reference's step 6) from integers and sums, without a device.

tests/golden/normal_structures.json holds what the reference's own step 6 (feature_extraction/step6_normal_structures.py, imported
unmodified by tools/gen_normal_structures_golden.py) returned - or raised - for seeded synthetic cases.  Here what the device would
deliver is computed with scipy and numpy (tests/normal_structures_util.py), so these tests pin the host arithmetic and the dict
building, the two pure helpers (integer bounds on squared distances, a coordinate percentile from a histogram), the restatements
themselves, the fixture and the interface declarations.  Every value is compared exactly: step 6 has no standard deviation."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import normal_structures_util as nu
from oracle import ref_shim

NEW_SYMBOLS = ("mi355_cityblock_distance", "mi355_flag_from_i32", "mi355_flag_from_box", "mi355_masked_order_stats_i32", "mi355_column_count_max",
               "mi355_label_components_nb")


def test_normal_structures_from_stats_reproduces_the_reference(amd):
    ns = nu.module("normal_structures")
    seen = set()
    for case in nu.load_fixture()["cases"]:
        seg, vols = nu.fixture_data(case)
        nu.check_case(ns, case, lambda: ns.normal_structures_from_stats(nu.host_stats(ns, seg, vols), case["voxel_dims"]))
        seen.add(case.get("raises", "returns"))
    assert seen == {"returns", "UnboundLocalError", "IndexError"}


def test_normal_structures_from_stats_needs_neither_a_device_nor_the_library(amd):
    ns = nu.module("normal_structures")
    stats = {"shape": (10, 10, 9), "n_brain": 500, "n_normal": 400, "n_ventricle": 0, "n_ventricle_left": 0, "n_ventricle_right": 0, "n_obstructed": 0,
             "periventricular": (0, 0.0), "cortical": (150, 150000.0, 150000.0), "deep": (100, 120000.0), "n_inferior": 0, "n_flow_void": 0,
             "peritumoral": (0, 0.0, 0.0)}
    got = ns.normal_structures_from_stats(stats, (1.0, 1.0, 2.0))
    assert tuple(got) == nu.SECTIONS
    assert got["ventricular_system"]["size_assessment"] == "Normal" and got["ventricular_system"]["evans_index_estimate"] == 0.0
    assert got["parenchyma"]["periventricular_assessment"] == {"hyperintensity_ratio": 1.0, "white_matter_disease_present": False,
                                                               "description": "Periventricular region could not be assessed"}
    assert got["parenchyma"]["gray_white_differentiation"]["assessment"] == "Could not assess"
    assert got["parenchyma"]["total_brain_volume_cm3"] == 1.0
    assert got["major_vessels"]["flow_voids"] == {"assessment": "Could not assess", "note": "Insufficient inferior brain for vessel assessment", "volume_cm3": 0.0}
    assert got["major_vessels"]["vascular_involvement"]["assessment"] == "Could not assess"
    with pytest.raises(ValueError, match="UnboundLocalError"):  # 101 deep voxels and no periventricular one
        ns.normal_structures_from_stats(dict(stats, deep=(101, 120000.0)), (1.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="brain mask .* is empty"):
        ns.normal_structures_from_stats({"shape": (10, 10, 9), "n_brain": 0}, (1.0, 1.0, 2.0))
    assert ns.normal_structures_from_stats(dict(stats, n_normal=0), (1.0, 1.0, 1.0))["parenchyma"] == {
        "assessment": "Unable to assess", "note": "Insufficient normal brain tissue for analysis"}


def test_sqrt_bounds_classify_as_the_float_comparison_does(amd):
    ns = nu.module("normal_structures")
    top = 200000
    k = np.arange(top + 1, dtype=np.int64)
    roots = np.sqrt(k.astype(np.float64))
    d2 = np.arange(0, top + 40, dtype=np.int64)
    root_d2 = np.sqrt(d2.astype(np.float64))
    for name, thresholds in (("sqrt(k)", roots), ("just below", np.nextafter(roots, -np.inf)[1:]), ("just above", np.nextafter(roots, np.inf)),
                             ("midpoints", (roots[:-1] + roots[1:]) / 2)):
        bounds = np.array([ns.sqrt_bounds(t) for t in thresholds], dtype=np.int64)
        le, ge = bounds[:, 0], bounds[:, 1]
        # the defining property, against the float comparison over every integer that can lie near the threshold
        lo = np.maximum(np.floor(thresholds * thresholds).astype(np.int64) - 3, 0)
        for off in range(8):
            cand = np.minimum(lo + off, d2[-1])
            assert np.array_equal(cand > le, root_d2[cand] > thresholds), (name, off)   # brain_dist > threshold
            assert np.array_equal(cand < ge, root_d2[cand] < thresholds), (name, off)   # brain_dist < threshold
        assert np.all(np.sqrt(le.astype(np.float64)) <= thresholds) and np.all(np.sqrt((le + 1).astype(np.float64)) > thresholds), name
        assert np.all(np.sqrt(ge.astype(np.float64)) >= thresholds) and np.all((ge == 0) | (np.sqrt(np.maximum(ge - 1, 0).astype(np.float64)) < thresholds)), name
    assert ns.sqrt_bounds(0.0) == (0, 0) and ns.sqrt_bounds(2.0) == (4, 4) and ns.sqrt_bounds(2.5) == (6, 7)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sqrt_bounds"):
            ns.sqrt_bounds(bad)


def test_coordinate_percentile_from_a_histogram_is_numpy(amd):
    ns = nu.module("normal_structures")
    rs = np.random.RandomState(3)
    masks = [rs.random_sample((6, 17, 5)) < p for p in (0.05, 0.3, 0.9)] + [rs.random_sample((3, 40, 4)) < 0.5]
    single = np.zeros((4, 9, 3), bool)
    single[2, 7, 1] = True
    plane = np.zeros((4, 9, 3), bool)
    plane[:, 4, :] = True
    two = np.zeros((4, 9, 3), bool)
    two[0, 1, 0] = two[3, 8, 2] = True
    for m in masks + [single, plane, two]:
        counts = m.sum(axis=(0, 2))
        for q in (75, 0, 100, 50, 12.5, 99.9):
            want = np.percentile(np.where(m)[1], q)
            got = ns.coordinate_percentile(counts, q)
            assert isinstance(got, np.float64) and got == want, (q, got, want)
    assert ns.coordinate_percentile(np.zeros(9, np.int64), 75) is None


def test_keep_rule_is_the_reference_loop(amd):
    ns, cu = nu.module("normal_structures"), __import__("components_util")
    d0 = 20
    m = np.zeros((d0, 30, 40), np.uint8)
    m[0:4, 0:20, 0:20] = 1      # 1600 voxels, centred at 1.5: off-centre (|1.5 - 10| = 8.5 >= 6)
    m[8:12, 0:20, 0:20] = 1     # 1600 voxels, centred at 9.5: kept
    m[14:16, 0:25, 0:20] = 1    # exactly 1000 voxels: not more than 1000
    m[4:5, 22:30, 30:40] = 1    # small
    lab, n = cu.scipy_labels(m, 2)
    keep = ns.keep_ventricles(cu.numpy_stats(lab, n), d0)
    want = [False] + [bool((lab == i).sum() > 1000 and abs(np.mean(np.where(lab == i)[0]) - d0 / 2) < d0 * 0.3) for i in range(1, n + 1)]
    assert keep == want and sum(keep) == 1 and n == 4


def test_symbols_are_declared_exported_and_bound(amd):
    with open(os.path.join(nu.ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(amd._lib.__file__), "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    import ctypes
    lib = ctypes.CDLL(str(amd._lib.lib_path()))
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym
        assert sym in amd._lib.EXPORTS and f"lib.{sym}.argtypes" in binding, sym
        assert hasattr(lib, sym), sym
    for line in ("step6_normal_structures.py:152", ":345", ":215", "step6_normal_structures.py:306-308", "step6_normal_structures.py:207", "step6_normal_structures.py:130-131",
                 "step6_normal_structures.py:66-67"):
        assert line in header, line
    assert "normal_structures.hip" in amd._build.SOURCES
    with open(os.path.join(nu.ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        integration = f.read()
    for sym in NEW_SYMBOLS:
        assert sym in integration, sym
    ns = nu.module("normal_structures")
    for mod, names in ((ns, ("cityblock_distance", "flag_from_i32", "flag_from_box", "masked_order_stats_i32", "column_count_max", "sqrt_bounds",
                             "coordinate_percentile", "normal_structures", "normal_structures_from_stats", "normal_structures_stats", "analyze", "main")),
                       (nu.module("components"), ("label_components_neighbours", "label_components")), (nu.module("synthetic"), ("mri_for_normal_structures",))):
        for name in names:
            assert callable(getattr(mod, name)), name
    assert ns.SECTIONS == nu.SECTIONS and ns.STEP == "Step 6 - Normal structures assessment"


def test_new_module_does_not_import_the_oracle(amd):
    with open(nu.module("normal_structures").__file__, encoding="utf-8") as f:
        text = f.read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M)
    assert "reference" not in [m.group(1) for m in re.finditer(r"^\s*(?:from|import)\s+(\w+)", text, flags=re.M)]


def test_fixture_is_what_the_reference_returns_today_and_covers_the_branch_table():
    if not ref_shim.reference_available():
        pytest.skip("the reference tree is not on this machine")
    tool = nu.generator_tool()
    data, hits, bad = tool.generate()
    assert data == nu.load_fixture()
    assert bad == []
    missing = [b for b in tool.REQUIRED if not any(b in hit for hit in hits.values())]
    assert missing == []
    assert len(tool.REQUIRED) == 34


def test_fixture_shape_and_size(amd):
    cases = nu.load_fixture()["cases"]
    shapes = [tuple(c["args"]["shape"]) for c in cases]
    assert shapes.count((240, 240, 155)) == 1 and set(shapes) == {(48, 56, 40), (240, 240, 155)}
    assert os.path.getsize(nu.FIXTURE) <= os.path.getsize(os.path.join(nu.ROOT, "tests", "golden", "sequence_findings.json"))
    assert [c for c in cases if len(set(c["voxel_dims"])) > 1]
    for case in cases:
        assert ("expected" in case) != ("raises" in case)
        if "expected" in case:
            assert list(case["expected"]) == list(nu.SECTIONS)
        if case["args"]["shape"] == [240, 240, 155]:
            continue  # (regenerated and hashed by the comparison with the reference above)
        _, vols = nu.fixture_data(case)
        assert vols.dtype == np.float32 and np.array_equal(vols, np.rint(vols)) and 0 <= vols.min() and vols.max() < 2 ** 15


@pytest.mark.parametrize("name", list(nu.cityblock_cases()))
def test_cityblock_restatement_is_scipy(name):
    mask = nu.cityblock_cases()[name]
    fg = mask != 0
    to_fg, to_bg = nu.cityblock(mask, True), nu.cityblock(mask, False)
    want = nu.scipy_taxicab(mask, True)
    assert np.all(to_fg == nu.FAR) if want is None else np.array_equal(to_fg, want), name
    assert np.array_equal(to_bg, nu.scipy_taxicab(mask, False)), name
    for n in nu.ITERATIONS:
        assert np.array_equal(to_fg <= n, ndimage.binary_dilation(fg, iterations=n)), (name, n)
        assert np.array_equal(to_bg > n, ndimage.binary_erosion(fg, iterations=n)), (name, n)


def test_seam_pairs_are_what_they_say():
    for name, shape, a, b, kind in nu.seam_pairs():
        m = np.zeros(shape, np.uint8)
        m[a] = m[b] = 1
        counts = [ndimage.label(m, ndimage.generate_binary_structure(3, c))[1] for c in (1, 2, 3)]
        assert counts == ([2, 1, 1] if kind == "edge" else [2, 2, 1]), name
    assert len(nu.seam_pairs()) == 9
