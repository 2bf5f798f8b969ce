"""Mass effect (the reference's step 2) from integers and sums, without a device.

tests/golden/mass_effect.json holds what the reference's own step 2 (feature_extraction/step2_mass_effect.py, imported unmodified
by tools/gen_mass_effect_golden.py) returned for seeded synthetic cases.  Here what the device would deliver is computed with
scipy and numpy (tests/mass_effect_util.py), so these tests pin the host arithmetic and the dict building, the fixture, the
interface declarations, and that the cases of the GPU tests tell the restatements from their listed wrong variants."""
import os
import re

import numpy as np
import pytest

import mass_effect_util as mx
from oracle import ref_shim

NEW_SYMBOLS = ("mi355_axis_counts", "mi355_box_counts", "mi355_select_ranked", "mi355_min_pair_dist2", "mi355_masked_min_i32")


def test_mass_effect_from_stats_reproduces_the_reference(amd):
    me = mx.module()
    cmp = mx.Comparer()
    for case in mx.load_fixture()["cases"]:
        seg, t1 = mx.fixture_data(case)
        np.random.seed(case["rng_seed"])
        got = me.mass_effect_from_stats(mx.host_stats(me, seg, t1), case["voxel_dims"])
        assert tuple(got) == mx.SECTIONS
        cmp.same(got, case["expected"], case["name"])
        assert type(got["midline_shift"]["is_significant"]) is bool
    print(f"largest relative error of a float that contains a std: {cmp.worst:.3g} at {cmp.where}")


def test_exact_distance_is_the_fixtures_and_never_above_the_sampled_one(amd):
    me = mx.module()
    larger = equal_small = 0
    for case in mx.load_fixture()["cases"]:
        if case["args"]["shape"] == [240, 240, 155]:
            continue  # (a distance transform of 8.9 M voxels on the host: the GPU test and the generator cover it)
        seg, t1 = mx.fixture_data(case)
        state = np.random.get_state()
        got = me.mass_effect_from_stats(mx.host_stats(me, seg, t1, distance="exact"), case["voxel_dims"])["ventricular_compression"]
        assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))  # nothing drawn
        exact, sampled = got.get("tumor_to_ventricle_distance_mm"), case["expected"]["ventricular_compression"].get("tumor_to_ventricle_distance_mm")
        assert exact == case["facts"]["exact_distance_mm"]
        if exact is None:
            assert sampled is None
            continue
        assert exact <= sampled
        larger += exact < sampled
        if case["facts"]["n_tumour"] <= 1000 and case["facts"]["n_csf"] <= 1000:
            assert exact == sampled
            equal_small += 1
    assert larger >= 1 and equal_small >= 1


def test_from_stats_needs_neither_a_device_nor_the_library(amd):
    me = mx.module()
    stats = {"shape": (8, 8, 8), "label_stats": np.zeros((8, 10), dtype=np.int64), "n_brain": 0, "dist2": None}
    got = me.mass_effect_from_stats(stats, (1.0, 1.0, 1.0))
    assert got["midline_shift"] == {"shift_mm": 0, "shift_direction": "Not applicable", "severity": "No tumor detected",
                                    "clinical_significance": "No tumor present to cause mass effect", "is_significant": False}
    assert type(got["midline_shift"]["shift_mm"]) is int and type(got["ventricular_compression"]["asymmetry_ratio"]) is int
    assert got["ventricular_compression"]["details"] == "Could not analyze - no brain tissue detected"
    assert got["anatomical_location"]["lobes"] == [] and got["herniation_risk"]["risk_level"] == "Low"
    assert me.lobe_boxes((48, 56, 40)) == [(0, 48, 0, 25, 12, 40), (0, 48, 16, 39, 20, 40), (0, 16, 11, 39, 0, 22), (31, 48, 11, 39, 0, 22),
                                           (0, 48, 36, 56, 0, 40), (14, 33, 16, 33, 10, 24)]


def test_voxel_volume_is_the_float32_product(amd):
    me = mx.module()
    stats = {"shape": (8, 8, 8), "label_stats": np.zeros((8, 10), dtype=np.int64), "n_brain": 0, "dist2": None,
             "tumour_counts0": np.array([0, 0, 0, 7, 0, 0, 0, 0]), "box_counts": np.zeros(6, dtype=np.int64), "peritumoral": np.zeros(3), "distant": np.zeros(3)}
    stats["label_stats"][2] = [7, 21, 21, 21, 3, 3, 3, 3, 3, 3]
    dims = (0.1, 0.7, 1.3)
    got = me.mass_effect_from_stats(stats, dims)["herniation_risk"]["tumor_volume_cm3"]
    assert got == float(np.int64(7) * np.prod([np.float32(v) for v in dims]) / 1000)
    assert got != float(7 * np.prod([float(np.float32(v)) for v in dims]) / 1000)  # the float64 product of the same zooms differs


def test_symbols_are_declared_exported_and_bound(amd):
    with open(os.path.join(mx.ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(amd._lib.__file__), "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    import ctypes
    lib = ctypes.CDLL(str(amd._lib.lib_path()))
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym
        assert sym in amd._lib.EXPORTS and f"lib.{sym}.argtypes" in binding, sym
        assert hasattr(lib, sym), sym
    for cited in ("step2_mass_effect.py:472-518", "step2_mass_effect.py:215-225", "step2_mass_effect.py:227-232", "step2_mass_effect.py:214-232"):
        assert cited in header, cited
    assert f"#define MI355_AXIS_COUNTS_MAX {mx.AXIS_MAX}" in header
    assert "mass_effect.hip" in amd._build.SOURCES
    me = mx.module()
    assert (me.AXIS_MAX, me.MAX_BOXES, me.MAX_POINTS) == (mx.AXIS_MAX, 16, 65536)
    for mod, names in ((me, ("axis_counts", "box_counts", "select_ranked", "min_pair_dist2", "masked_min", "mass_effect_stats", "mass_effect_from_stats",
                             "mass_effect", "analyze", "main")), (mx.module("synthetic"), ("mri_for_mass_effect",))):
        for name in names:
            assert callable(getattr(mod, name)), name
    assert me.SECTIONS == mx.SECTIONS and me.STEP == "Step 2 - Mass effect metrics"


def test_new_module_does_not_import_the_oracle(amd):
    with open(mx.module().__file__, encoding="utf-8") as f:
        text = f.read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M)
    assert "reference" not in [m.group(1) for m in re.finditer(r"^\s*(?:from|import)\s+(\w+)", text, flags=re.M)]


def test_fixture_is_what_the_reference_returns_today_and_covers_the_branch_table():
    if not ref_shim.reference_available():
        pytest.skip("the reference tree is not on this machine")
    tool = mx.generator_tool()
    data, hits, bad = tool.generate()
    assert data == mx.load_fixture()
    assert bad == []
    missing = [b for b in tool.REQUIRED if not any(b in hit for hit in hits.values())]
    assert missing == []
    assert len(tool.REQUIRED) == 61


def test_fixture_shape_and_size(amd):
    cases = mx.load_fixture()["cases"]
    shapes = [tuple(c["args"]["shape"]) for c in cases]
    assert shapes.count((240, 240, 155)) == 1 and set(shapes) == {(48, 56, 40), (240, 240, 155)}
    assert os.path.getsize(mx.FIXTURE) <= 128 * 1024
    assert [c for c in cases if len(set(c["voxel_dims"])) > 1]
    for case in cases:
        assert list(case["expected"]) == list(mx.SECTIONS)
        if case["args"]["shape"] == [240, 240, 155]:
            continue  # (regenerated and hashed by the comparison with the reference above)
        _, t1 = mx.fixture_data(case)
        assert t1.dtype == np.float32 and np.array_equal(t1, np.rint(t1)) and 0 <= t1.min() and t1.max() < 2 ** 15


# ---- the cases of the GPU tests tell the restatements from their wrong variants ----------------------------------------
def test_a_split_at_half_the_axis_is_told_from_the_split_at_the_midline(amd):
    told = 0
    for case in mx.load_fixture()["cases"]:
        want = case["expected"]["midline_shift"]
        if "brain_midline_x" not in want or case["args"]["shape"] == [240, 240, 155]:
            continue
        seg, t1 = mx.fixture_data(case)
        brain = mx.masks(seg, t1)[1]
        assert mx.shift_mm(brain, case["voxel_dims"][0]) == want["shift_mm"], case["name"]
        told += mx.shift_mm(brain, case["voxel_dims"][0], split="dims") != want["shift_mm"]
    assert told >= 10  # the brain spans the indices 1 .. 46 of 48: int(23.5) = 23 is not 48 // 2


def test_closed_boxes_are_told_from_half_open_ones():
    flags = mx.random_flags(mx.BOX_SHAPE)
    for name, boxes in mx.box_cases().items():
        right, wrong = mx.box_counts(flags, boxes, 1, 2), mx.box_counts(flags, boxes, 1, 2, closed=True)
        assert np.array_equal(right, wrong) == (name == "whole volume"), name  # (a closed whole-volume box has nothing left to add)
    assert mx.box_counts(flags, mx.box_cases()["empty"]).sum() == 0
    assert mx.box_counts(flags, mx.box_cases()["whole volume"])[0] == flags.size


@pytest.mark.parametrize("shape", mx.RANK_SHAPES)
def test_ranks_from_one_and_fortran_order_are_told_from_the_c_order_ranks(shape):
    for density in mx.RANK_DENSITIES:
        flags = mx.density_flags(shape, density)
        sel = mx.selected(flags, 4, 1)
        ranks = mx.rank_set(int(sel.sum()))
        right = mx.select_ranked(flags, ranks, 4, 1)
        assert sel.reshape(-1)[right].all() and np.array_equal(np.sort(np.flatnonzero(sel))[ranks], right)
        assert not np.array_equal(mx.select_ranked(flags, ranks, 4, 1, base=1), right), (shape, density)
        assert not np.array_equal(mx.select_ranked(flags, ranks, 4, 1, order="F"), right), (shape, density)


def test_an_unconditional_second_draw_is_told_by_the_generator_state():
    told = 0
    for case in mx.load_fixture()["cases"]:
        n_t, n_csf = case["facts"]["n_tumour"], case["facts"]["n_csf"]
        if not (n_t and n_csf):
            continue
        states = []
        for unconditional in (False, True):
            gen = np.random.RandomState(case["rng_seed"])
            mx.draws(n_t, n_csf, gen, unconditional)
            states.append(gen.get_state()[1:3])
        same = np.array_equal(states[0][0], states[1][0]) and states[0][1] == states[1][1]
        assert same == (n_csf > 1000), case["name"]
        told += not same
    assert told >= 3
