"""not gpu: the table of scratch users (scratch_util.py) is closed - every ``device_scratch(`` call site under csrc/ belongs to a
case, every case is complete, and every reference a case names exists - and its references are the util modules' own."""
import os
import re

import numpy as np
import pytest

import scratch_util as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "automated-brain-mri-analysis-and-report-generation-with-retrieval-augmented-clinical-assistance_amd")
CSRC = os.path.join(PKG, "csrc")


def declared_sites():
    sites = set()
    for c in sx.CASES:
        sites |= set(c.sites)
    for n in sx.NETWORK_SITES.values():
        sites |= set(n["sites"])
    return sites


def test_every_call_site_has_a_case_and_every_case_a_call_site():
    found = sx.call_sites(CSRC)
    assert sum(found.values()) >= 36, found
    actual = {(fn, i) for fn, n in found.items() for i in range(n)}
    declared = declared_sites()
    per_file = {fn: len({s for s in declared if s[0] == fn}) for fn in {s[0] for s in declared} | set(found)}
    assert per_file == {fn: found.get(fn, 0) for fn in per_file}, \
        f"device_scratch( call sites per file {found}, declared by scratch_util.CASES {per_file}: a new scratch user needs a case"
    assert declared == actual, (sorted(actual - declared), sorted(declared - actual))


def test_the_slot_names_are_the_librarys(amd):
    hdr = open(os.path.join(CSRC, "common.h"), encoding="utf-8").read()
    enum = re.search(r"enum ScratchSlot \{(.*?)\}", hdr, re.S).group(1)
    names = [n.split("=")[0].strip() for n in enum.split(",")]
    assert names[-1] == "SCR_COUNT" and tuple(names[:-1]) == amd.ops.SCRATCH_SLOTS
    assert amd.ops.scratch_slot_count() == len(amd.ops.SCRATCH_SLOTS)   # host code: mi355_scratch_sizes needs no device
    assert set(amd.ops.SCRATCH_SHARED) < set(amd.ops.SCRATCH_SLOTS)
    api = open(os.path.join(ROOT, "include", "mi355_nnunet.h"), encoding="utf-8").read()
    lanes = int(re.search(r"#define MI355_SCRATCH_LANES (\d+)", api).group(1))
    assert lanes == amd.ops.SCRATCH_LANES
    runtime = open(os.path.join(CSRC, "runtime.hip"), encoding="utf-8").read()
    assert "constexpr int MAX_LANES = MI355_SCRATCH_LANES;" in runtime
    binding = open(os.path.join(PKG, "_lib.py"), encoding="utf-8").read()
    for sym in ("mi355_scratch_sizes", "mi355_scratch_fill", "mi355_scratch_release", "mi355_scratch_zero_pages"):
        assert sym in amd._lib.EXPORTS and f"lib.{sym}.argtypes" in binding, sym


#: the entry points that reach device_scratch, by case name: several share a call site (the three neighbourhoods of the labelling, the
#: two callers of the radix select), so the call-site count alone would not miss one of them
ENTRY_POINTS = {
    "zscore_masked", "label_confusion", "label_stats", "cosine_topk", "crop_mask", "resize_axis_order3", "clip_to_range_of",
    "label_components_6", "label_components_18", "label_components_26", "component_stats", "largest_component",
    "binary_morphology", "edt_squared", "surface_gradient_stats", "second_moments", "masked_moments",
    "masked_percentiles", "masked_percentiles_multi", "masked_order_stats_i32", "column_count_max",
    "binary_fill_holes", "sobel_magnitude_stats", "radial_shell_moments", "face_slab_counts",
    "axis_counts", "box_counts", "select_ranked", "min_pair_dist2", "masked_min",
    "conv_splitk_f32", "conv_splitk_f16", "conv_wino3_f32", "conv_s2dma_f32", "conv_dma_f16", "conv_s2dma_f16",
}


def test_every_case_is_complete(amd):
    assert len({c.name for c in sx.CASES}) == len(sx.CASES)
    assert {c.name for c in sx.CASES} == ENTRY_POINTS, {c.name for c in sx.CASES} ^ ENTRY_POINTS
    assert set(sx.NETWORK_SITES) == {"unet_forward", "sw_predict"}
    used = set()
    for c in sx.CASES:
        assert c.sites and all(isinstance(f, str) and isinstance(i, int) for f, i in c.sites), c.name
        assert c.slots and set(c.slots) <= set(amd.ops.SCRATCH_SLOTS), c.name
        used |= set(c.slots)
        assert callable(c.inputs) and callable(c.call) and callable(c.reference), c.name
        assert isinstance(c.exact, bool) and (c.exact or c.gate is not None), f"{c.name}: a case that is not exact needs its test's gate"
        assert len(c.shapes) == 2 and c.shapes[0] != c.shapes[1], c.name
        if len(c.shapes[0]) == 3:   # volumes: the larger one is the larger one
            assert int(np.prod(c.shapes[0])) > int(np.prod(c.shapes[1])), c.name
        if c.shapes != (sx.LARGE, sx.SMALL):
            assert c.need, f"{c.name}: shapes other than the suite's odd sizes need a reason"
        assert c.patterns in (sx.NAN_WORDS, sx.INDEX_WORDS, (0x5A5A5A5A,)), c.name
        if c.patterns == (0x5A5A5A5A,):
            assert c.name.startswith("conv_") and sx.ALLOWED_STALE_READS, c.name
        assert callable(sx.resolve(c.reference_of)), c.reference_of
    for n in sx.NETWORK_SITES.values():
        used |= set(n["slots"])
        assert callable(sx.resolve(n["reference_of"]))
    assert used == set(amd.ops.SCRATCH_SLOTS), set(amd.ops.SCRATCH_SLOTS) - used
    # index and offset tables live in these slots: their cases never see a word that is no small index
    for c in sx.CASES:
        if set(c.slots) & {"SCR_COMPONENTS", "SCR_MASS_EFFECT", "SCR_TOPK"} or c.name == "binary_fill_holes":
            assert c.patterns == sx.INDEX_WORDS, c.name
    assert sx.ALLOWED_STALE_READS == ()


def test_reference_modules_are_the_existing_ones():
    allowed = ("components_util.", "morphology_util.", "quality_util.", "mass_effect_util.", "normal_structures_util.", "preprocess_util.",
               "plumbing_util.", "sequence_findings_util.", "test_gpu_ops.", "test_gpu_extras.", "oracle.")
    for c in sx.CASES:
        assert c.reference_of.startswith(allowed), (c.name, c.reference_of)


EXACT = [c.name for c in sx.CASES if c.exact]


def _leaves(x):
    if isinstance(x, (tuple, list)):
        for v in x:
            yield from _leaves(v)
    elif isinstance(x, dict):
        for v in x.values():
            yield from _leaves(v)
    elif isinstance(x, (np.ndarray, int, float, np.number)):
        yield np.asarray(x)


@pytest.mark.parametrize("name", EXACT)
def test_exact_references_give_what_the_util_modules_give(name):
    """For each exact case the reference applied to the smaller shape's inputs is the util module's function applied to them: the
    case adds no reference of its own (a case whose reference wraps several calls is compared part by part)."""
    c = sx.BY_NAME[name]
    inp = sx.inputs_of(name, 1)
    want = sx.reference_of(name, 1)
    fn = sx.resolve(c.reference_of)
    direct = {
        "crop_mask": lambda: tuple(fn(inp["vol"])),
        "label_stats": lambda: (fn(inp["seg"], 8),),
        "clip_to_range_of": lambda: (fn(inp["x"], inp["ref"], 2),),
        "label_components_6": lambda: fn(inp["mask"], 1),
        "label_components_18": lambda: fn(inp["mask"], 2),
        "label_components_26": lambda: fn(inp["mask"], 3),
        "component_stats": lambda: (lambda lab, n: (n, fn(lab, n, inp["seg"])))(*sx.cu.scipy_labels(inp["mask"], 3)),
        "largest_component": lambda: fn(inp["seg"], [1, (2, 3)], 1.0, {1: 3.0, (2, 3): 2.0}),
        "binary_morphology": lambda: (fn(inp["mask"], 3), sx.mu.dilate(inp["mask"], 2)),
        "edt_squared": lambda: (fn(inp["mask"]),),
        "second_moments": lambda: (fn(inp["mask"]),),
        "masked_moments": lambda: (fn(inp["vols"], inp["flags"]),),
        "masked_percentiles": lambda: (lambda sel: (int(sel.size), 0) + tuple(fn(sel, sx.QS8)[:2]))(sx._pct_selected(inp["x"], inp["flags"], 1, 4, lo=0.0)),
        "masked_percentiles_multi": lambda: tuple(tuple((lambda sel: (int(sel.size), 0) + tuple(fn(sel, qs)[:2]))(sx._pct_selected(inp[v], inp["flags"], req, forb))
                                                        for v, qs, req, forb in batch) for batch in (sx._MULTI_A, sx._MULTI_B)),
        "masked_order_stats_i32": lambda: fn(inp["values"][sx.nu.selected(inp["flags"], 2, 1)], sx.QS8),
        "column_count_max": lambda: (fn(inp["flags"], 3, 5, 2),),
        "binary_fill_holes": lambda: fn(inp["mask"]),
        "radial_shell_moments": lambda: fn(inp["x"], inp["selected"], inp["centre"]),
        "face_slab_counts": lambda: (fn(inp["x"], 3),),
        "axis_counts": lambda: fn(inp["flags"], 5, 2),
        "box_counts": lambda: (fn(inp["flags"], sx._boxes(inp["flags"].shape), 1, 4),),
        "select_ranked": lambda: (fn(inp["flags"], inp["ranks"], 4, 1), int(sx.mx.selected(inp["flags"], 4, 1).sum())),
        "min_pair_dist2": lambda: (fn(inp["a"], inp["b"], inp["shape"]),),
        "masked_min": lambda: fn(inp["values"], inp["flags"], 5, 2),
    }
    assert name in direct, f"{name}: say here how its util reference is called"
    sx.same(want, direct[name](), name)
    # and the inputs select something: an empty selection would make every later comparison vacuous
    assert any(np.any(v != 0) for v in _leaves(want)), name
