"""Quality control (the reference's step 5) from integers and sums, without a device.

tests/golden/quality.json holds what the reference's own step 5 (feature_extraction/step5_quality.py, imported unmodified by
tools/gen_quality_golden.py) returned for seeded synthetic cases.  Here what the device would deliver is computed with scipy and
numpy (tests/quality_util.py), so these tests pin the host arithmetic and the dict building, the restatements themselves
(against scipy, on the shapes the GPU tests use), the fixture and the interface declarations."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import quality_util as qu
from oracle import ref_shim

NEW_SYMBOLS = ("mi355_binary_fill_holes", "mi355_sobel_magnitude_stats", "mi355_radial_shell_moments", "mi355_face_slab_counts")


def test_quality_from_stats_reproduces_the_reference(amd):
    q = qu.module("quality")
    cmp = qu.Comparer()
    for case in qu.load_fixture()["cases"]:
        seg, vols = qu.fixture_data(case)
        got = q.quality_from_stats(qu.host_stats(q, seg, vols), case["voxel_dims"])
        assert tuple(got) == qu.SECTIONS
        cmp.same(got, case["expected"], case["name"])
    print(f"largest relative error of a float that contains a std: {cmp.worst:.3g} at {cmp.where}")


def test_quality_from_stats_needs_neither_a_device_nor_the_library(amd):
    q = qu.module("quality")
    stats = {"shape": (8, 8, 8), "label_stats": np.zeros((8, 10), dtype=np.int64), "n_brain": 0, "face_counts": np.zeros(6, dtype=np.int64), "n_edge": 0,
             "sequences": {name: {"ghost": np.zeros(3)} for name in q.SEQUENCES}}
    got = q.quality_from_stats(stats, (1.0, 1.0, 1.0))
    assert got["segmentation_quality"] == {"quality_score": 50, "grade": "Poor", "issues": ["No tumor segmentation detected"], "warnings": [],
                                           "recommendation": "Manual review required - no segmentation found"}
    assert got["image_quality"]["sequences"]["T2"] == {"snr_estimate": 0, "issues": ["No brain tissue detected"], "quality": "Poor"}
    assert list(got["artifact_detection"]["details"]) == ["motion_ghosting", "susceptibility", "wrap_around", "gibbs_ringing"]
    stats["label_stats"][2] = [500, 0, 0, 0, 3, 3, 3, 4, 4, 4]
    stats.update(num_components=1, filled=0, n_edge=101)
    with pytest.raises(ValueError, match="gradient statistics"):
        q.quality_from_stats(stats, (1.0, 1.0, 1.0))


def test_symbols_are_declared_exported_and_bound(amd):
    with open(os.path.join(qu.ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(amd._lib.__file__), "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    import ctypes
    lib = ctypes.CDLL(str(amd._lib.lib_path()))
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym
        assert sym in amd._lib.EXPORTS and f"lib.{sym}.argtypes" in binding, sym
        assert hasattr(lib, sym), sym
    assert "step5_quality.py:103" in header and "step5_quality.py:413-416" in header and "step5_quality.py:280-300" in header
    assert "step5_quality.py:385-390" in header
    assert "quality.hip" in amd._build.SOURCES
    q = qu.module("quality")
    for mod, names in ((q, ("binary_fill_holes", "sobel_magnitude_stats", "radial_shell_moments", "face_slab_counts", "quality_control",
                            "quality_from_stats", "quality_stats", "analyze", "main")), (qu.module("synthetic"), ("mri_for_quality",))):
        for name in names:
            assert callable(getattr(mod, name)), name
    assert q.SECTIONS == qu.SECTIONS and q.STEP == "Step 5 - Quality control and confidence metrics"


def test_new_module_does_not_import_the_oracle(amd):
    with open(qu.module("quality").__file__, encoding="utf-8") as f:
        text = f.read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M)
    assert "reference" not in [m.group(1) for m in re.finditer(r"^\s*(?:from|import)\s+(\w+)", text, flags=re.M)]


def test_fixture_is_what_the_reference_returns_today_and_covers_the_branch_table():
    if not ref_shim.reference_available():
        pytest.skip("the reference tree is not on this machine")
    tool = qu.generator_tool()
    data, hits, bad = tool.generate()
    assert data == qu.load_fixture()
    assert bad == []
    missing = [b for b in tool.REQUIRED if not any(b in hit for hit in hits.values())]
    assert missing == []
    assert len(tool.REQUIRED) == 45


def test_fixture_shape_and_size(amd):
    cases = qu.load_fixture()["cases"]
    shapes = [tuple(c["args"]["shape"]) for c in cases]
    assert shapes.count((240, 240, 155)) == 1 and set(shapes) == {(48, 56, 40), (240, 240, 155)}
    assert os.path.getsize(qu.FIXTURE) <= os.path.getsize(os.path.join(qu.ROOT, "tests", "golden", "sequence_findings.json"))
    assert [c for c in cases if len(set(c["voxel_dims"])) > 1]
    for case in cases:
        assert list(case["expected"]) == list(qu.SECTIONS)
        if case["args"]["shape"] == [240, 240, 155]:
            continue  # (regenerated and hashed by the comparison with the reference above)
        _, vols = qu.fixture_data(case)
        assert vols.dtype == np.float32 and np.array_equal(vols, np.rint(vols)) and 0 <= vols.min() and vols.max() < 2 ** 15


@pytest.mark.parametrize("name", list(qu.fill_cases()))
def test_fill_holes_restatement_is_scipy(name):
    mask = qu.fill_cases()[name]
    want = ndimage.binary_fill_holes(mask)
    got, filled = qu.fill_holes(mask)
    assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)), name
    assert filled == int(want.sum()) - int((mask != 0).sum())
    if name == "diagonal gap":
        assert filled == 27 and ndimage.label(mask == 0, ndimage.generate_binary_structure(3, 3))[1] == 1  # a 26-neighbour flood would leak
    if name == "winding channel":
        assert filled == 0 and not got[5, 5, 5]
    if name == "ball inside a shell":
        assert filled > 0 and got[10, 10, 10] and got[10, 10, 15]
    if name == "5x6x7 one enclosed voxel":
        assert filled == 1
    if name == "1x7x9 all on a face":
        assert filled == 0


@pytest.mark.parametrize("shape", qu.SOBEL_SHAPES)
def test_sobel_restatement_is_scipy_bit_for_bit(shape):
    x = qu.integer_volume(shape)
    assert np.array_equal(qu.sobel_magnitude(x), qu.scipy_sobel_magnitude(x))


def test_face_slab_restatement_is_the_reference_expression():
    x = qu.integer_volume((7, 9, 4)) - 16000.0
    got = qu.face_slab_counts(x, 5)
    want = [x[:5, :, :].max() > 0, x[-5:, :, :].max() > 0, x[:, :5, :].max() > 0, x[:, -5:, :].max() > 0]  # step5_quality.py:386-389
    assert [bool(v > 0) for v in got[:4]] == [bool(v) for v in want]
    assert got[4] == got[5] == int((x > 0).sum())  # margin 5 on an axis of 4: the whole axis
