"""not gpu: the host half of lesion-wise scoring - the declarations of the four new entry points, lesionwise_from_tables against the
scipy restatement of lesionwise_util.py on small hand-made cases and on the scene, the integers and the two aggregates the issue
quotes for the scene, the refusals, and the command's arguments and report lines."""
import os
import re

import numpy as np
import pytest

import lesionwise_util as lu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mi355_binary_morphology_nb", "mi355_label_pair_counts", "mi355_label_lookup", "mi355_label_lookup_i32")
PHRASES = ("Mean Dice Score", "Whole Tumor", "Tumor Core", "Enhancing Tumor")


def test_new_symbols_are_declared_bound_and_built(amd):
    with open(os.path.join(ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    pkg = os.path.dirname(amd._lib.__file__)
    with open(os.path.join(pkg, "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    lib = amd._lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym
        assert sym in amd._lib.EXPORTS, sym
        assert f"lib.{sym}.argtypes" in binding, sym
        assert hasattr(lib, sym), sym
    assert "lesionwise.hip" in amd._build.SOURCES
    with open(os.path.join(pkg, "csrc", "lesionwise.hip"), encoding="utf-8") as f:
        assert "device_scratch(" not in f.read(), "the new file takes all working memory from its caller"
    assert int(re.search(r"#define MI355_PAIR_TABLE_MAX (\d+)", header).group(1)) == amd.components.PAIR_TABLE_MAX == 1 << 20
    assert int(re.search(r"#define MI355_MORPH_NB_LDS_STEPS (\d+)", header).group(1)) == amd.volume_ops.MORPH_NB_LDS_STEPS
    assert int(re.search(r"#define MI355_LOOKUP_MAX_LABEL (\d+)", header).group(1)) == amd.components.MAX_COMPONENTS
    for mod, names in ((amd.volume_ops, ("binary_dilation_nb", "binary_erosion_nb")), (amd.components, ("pair_counts", "lookup")),
                       (amd.evaluate, ("lesionwise_from_tables", "lesionwise_metrics", "evaluate_lesionwise"))):
        for name in names:
            assert callable(getattr(mod, name)), name


# ---------------------------------------------------------------------------------------------------------------- hand-made cases
def _blank():
    return np.zeros((12, 14, 30), dtype=np.uint8), np.zeros((12, 14, 30), dtype=np.uint8)


def merge_by_dilation():
    P, G = _blank()
    G[4:8, 4:8, 4:8] = 1
    G[4:8, 4:8, 11:15] = 1        # three voxels of background between the two: one lesion after three steps
    P[4:8, 4:8, 5:13] = 1
    return P, G


def shared_component():
    P, G = _blank()
    G[2:6, 2:6, 2:6] = 1
    G[2:6, 2:6, 20:24] = 1
    P[3, 3, 3:23] = 1             # one line through both
    return P, G


def matched_through_dilation_only():
    P, G = _blank()
    G[4:8, 4:8, 4:8] = 1
    P[5, 5, 9:11] = 1             # beside the lesion, inside its dilation, no common voxel
    return P, G


def sub_threshold_with_a_match():
    P, G = _blank()
    G[4:6, 4:6, 4:6] = 1          # 8 voxels
    P[4:6, 4:6, 5:8] = 1
    return P, G


def false_negative_and_false_positive():
    P, G = _blank()
    G[2:6, 2:6, 2:6] = 1          # 64 voxels, missed
    P[8:11, 8:11, 20:24] = 1      # far from it
    return P, G


CASES = {"merge_by_dilation": merge_by_dilation, "shared_component": shared_component, "matched_through_dilation_only": matched_through_dilation_only,
         "sub_threshold_with_a_match": sub_threshold_with_a_match, "false_negative_and_false_positive": false_negative_and_false_positive,
         "both_empty": _blank, "scene": lu.scene}


def from_tables(amd, P, G, spacing, **kw):
    gg, pd, pl, parts = lu.tables_of(P, G, kw.get("dilation", 3))
    return amd.evaluate.lesionwise_from_tables(gg, pd, pl, spacing, lu.distance_callback(P, G, spacing, parts), **kw)


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), (1.5, 1.0, 0.8)])
@pytest.mark.parametrize("name", list(CASES))
def test_from_tables_equals_the_restatement(amd, name, spacing):
    P, G = CASES[name]()
    got = from_tables(amd, P, G, spacing)
    worst = lu.same(got, lu.region_lesionwise(P, G, spacing), name)
    assert worst == 0.0, "the same distances and the same host arithmetic"
    import json
    assert json.loads(json.dumps(got)) == got, "plain ints, floats, bools and lists"


def test_hand_made_cases_show_what_they_are_named_for(amd):
    r = from_tables(amd, *merge_by_dilation(), (1, 1, 1))
    assert (r["num_lesions"], r["lesions"][0]["gt_components"], r["lesions"][0]["gt_voxels"], r["num_fp"]) == (1, 2, 128, 0)
    r = from_tables(amd, *shared_component(), (1, 1, 1))
    assert [row["pred_components"] for row in r["lesions"]] == [[1], [1]] and r["num_fp"] == 0 and r["num_tp"] == 2
    assert [row["pred_voxels"] for row in r["lesions"]] == [20, 20] and [row["intersection"] for row in r["lesions"]] == [3, 3]
    r = from_tables(amd, *matched_through_dilation_only(), (1, 1, 1))
    row = r["lesions"][0]
    assert row["pred_components"] == [1] and row["intersection"] == 0 and row["dice"] == 0.0 and 0 < row["hd95"] < 374.0
    assert (r["num_tp"], r["num_fn"], r["num_fp"]) == (1, 0, 0) and r["lesionwise_dice"] == 0.0 and r["lesionwise_hd95"] == row["hd95"]
    r = from_tables(amd, *sub_threshold_with_a_match(), (1, 1, 1))
    assert r["lesions"][0]["counted"] is False and r["lesions"][0]["pred_components"] == [1] and r["lesions"][0]["dice"] > 0
    assert (r["num_counted"], r["num_fp"], r["lesionwise_dice"], r["lesionwise_hd95"]) == (0, 0, 1.0, 0.0), "N == 0: only a sub-threshold lesion, no false positive"
    r = from_tables(amd, *false_negative_and_false_positive(), (1, 1, 1))
    assert (r["num_fn"], r["num_fp"], r["num_tp"]) == (1, 1, 0) and r["fp_components"] == [{"id": 1, "voxels": 36}]
    assert r["lesions"][0]["hd95"] == 374.0 and r["lesionwise_dice"] == 0.0 and r["lesionwise_hd95"] == 374.0
    r = from_tables(amd, *_blank(), (1, 1, 1))
    assert (r["num_lesions"], r["num_fp"], r["lesionwise_dice"], r["lesionwise_hd95"]) == (0, 0, 1.0, 0.0), "N == 0: both maps empty"
    r = from_tables(amd, *false_negative_and_false_positive(), (1, 1, 1), penalty_mm=100.0, min_volume_mm3=0.0)
    assert r["lesionwise_hd95"] == 100.0 and r["penalty_mm"] == 100.0


def test_the_threshold_is_strict(amd):
    P, G = _blank()
    G[2:7, 2:7, 2:4] = 1          # 50 voxels
    P[2:7, 2:7, 2:4] = 1
    for spacing, counted in (((1, 1, 1), False), ((1, 1, 1.02), True), ((2, 1, 0.5), False)):
        r = from_tables(amd, P, G, spacing)
        assert r["lesions"][0]["gt_voxels"] == 50 and r["lesions"][0]["counted"] is counted, spacing
        lu.same(r, lu.region_lesionwise(P, G, spacing), spacing)
    G[2, 2, 4] = P[2, 2, 4] = 1   # 51 voxels
    assert from_tables(amd, P, G, (1, 1, 1))["lesions"][0]["counted"] is True
    assert from_tables(amd, P, G, (1, 1, 1), min_volume_mm3=51.0)["lesions"][0]["counted"] is False


def test_literal_tables_and_a_mapping_of_distances(amd):
    """no scipy: two ground-truth components in one dilated component, a second lesion that nothing meets; predicted component 1
    overlaps the first lesion, component 2 lies in no dilated component"""
    gg = np.array([[900, 60, 30], [0, 40, 0], [0, 20, 0], [0, 0, 10]])   # rows: background, gcc 1..3; columns: outside, dilated 1, 2
    pd = np.array([[895, 95, 40], [0, 25, 0], [5, 0, 0]])
    pl = np.array([[975, 45, 10], [10, 15, 0], [5, 0, 0]])
    d = {1: (np.array([0.0, 1.0, 2.0]), np.array([0.0, 3.0]))}
    r = amd.evaluate.lesionwise_from_tables(gg, pd, pl, (1, 1, 1), d, min_volume_mm3=5.0)
    assert [(x["gt_voxels"], x["gt_components"], x["pred_components"], x["pred_voxels"], x["intersection"]) for x in r["lesions"]] == \
        [(60, 2, [1], 25, 15), (10, 1, [], 0, 0)]
    assert r["lesions"][0]["dice"] == 30 / 85 and r["lesions"][0]["hd95"] == np.percentile([0.0, 1.0, 2.0, 0.0, 3.0], 95)
    assert r["fp_components"] == [{"id": 2, "voxels": 5}] and (r["num_tp"], r["num_fn"], r["num_fp"]) == (1, 1, 1)
    assert r["lesionwise_dice"] == (30 / 85 + 0.0) / 3 and r["lesionwise_hd95"] == (r["lesions"][0]["hd95"] + 374.0 + 374.0) / 3
    bad = gg.copy()
    bad[1] = [0, 20, 20]    # a ground-truth component in two dilated components
    with pytest.raises(ValueError, match="dilat"):
        amd.evaluate.lesionwise_from_tables(bad, pd, pl, (1, 1, 1), d)
    with pytest.raises(ValueError, match="disagree"):
        amd.evaluate.lesionwise_from_tables(gg, pd, pl[:, ::-1], (1, 1, 1), d)


def test_the_scene_gives_the_quoted_integers(amd):
    P, G = lu.scene()
    for spacing in ((1.0, 1.0, 1.0), (1.5, 1.0, 0.8)):
        want, parts = lu.region_lesionwise(P, G, spacing, with_parts=True)
        assert (parts["n_gt"], parts["n_pred"], parts["n_les"]) == (5, 4, 4)
        rows = want["lesions"]
        assert [r["gt_voxels"] for r in rows] == [27, 523, 257, 64] and [r["gt_components"] for r in rows] == [1, 2, 1, 1]
        assert [r["pred_components"] for r in rows] == [[1], [2], [2, 3], []]
        assert [r["pred_voxels"] for r in rows] == [8, 548, 550, 0] and [r["intersection"] for r in rows] == [1, 406, 1, 0]
        assert [r["counted"] for r in rows] == [False, True, True, True]
        assert want["fp_components"] == [{"id": 4, "voxels": 27}]
        assert (want["num_lesions"], want["num_counted"], want["num_tp"], want["num_fn"], want["num_fp"]) == (4, 3, 2, 1, 1)
        assert want["lesionwise_dice"] == 0.1901620623466239
        got = from_tables(amd, P, G, spacing)
        assert got["lesionwise_dice"] == 0.1901620623466239
        if spacing == (1.0, 1.0, 1.0):
            assert want["lesionwise_hd95"] == 196.75935248845744 and got["lesionwise_hd95"] == 196.75935248845744
    labels_p, labels_g = lu.scene_labels()
    res = lu.case_lesionwise(labels_p, labels_g, (1, 1, 1))
    assert all(res[k]["lesionwise_dice"] == 0.1901620623466239 for k in ("WT", "TC", "ET"))


def test_the_dilation_reaches_what_the_issue_says():
    """k steps of the 18-neighbourhood from one seed: max(|a|, |b|, |c|) <= k and |a| + |b| + |c| <= 2 k"""
    for k, count in ((1, 19), (2, 93), (3, 263), (4, 569)):
        m = np.zeros((11, 11, 11), np.uint8)
        m[5, 5, 5] = 1
        out = lu.morph(m, True, 18, k)
        g = np.abs(np.indices(m.shape) - 5)
        assert int(out.sum()) == count and np.array_equal(out != 0, (g.max(axis=0) <= k) & (g.sum(axis=0) <= 2 * k))


# ---------------------------------------------------------------------------------------------------------------- refusals, command
def test_refusals_need_no_device(amd):
    import torch
    ev = amd.evaluate
    a = torch.zeros((3, 4, 5), dtype=torch.uint8)
    with pytest.raises(ValueError, match="shapes"):
        ev.lesionwise_metrics(a, torch.zeros((3, 4, 6), dtype=torch.uint8), (1, 1, 1))
    with pytest.raises(ValueError, match="uint8"):
        ev.lesionwise_metrics(a, a.to(torch.int16), (1, 1, 1))
    for bad in ((1, 1), (1, 1, 0), (1, float("nan"), 1), "abc", None):
        with pytest.raises(ValueError, match="spacing"):
            ev.lesionwise_metrics(a, a, bad)
    for bad in (0, 17, -1, 2.5, "x", None):
        with pytest.raises(ValueError, match="dilation"):
            ev.lesionwise_metrics(a, a, (1, 1, 1), dilation=bad)
    for bad in (-1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="min_volume_mm3"):
            ev.lesionwise_metrics(a, a, (1, 1, 1), min_volume_mm3=bad)
        with pytest.raises(ValueError, match="penalty_mm"):
            ev.lesionwise_metrics(a, a, (1, 1, 1), penalty_mm=bad)
    with pytest.raises(ValueError, match="CUDA"):
        ev.lesionwise_metrics(a, a, (1, 1, 1))
    with pytest.raises(ValueError, match="regions"):
        ev.lesionwise_metrics(a, a, (1, 1, 1), regions={str(k): (1,) for k in range(5)})


def test_parser_takes_the_new_flags_and_keeps_the_old_defaults(amd):
    ap = amd.evaluate.build_parser()
    args = ap.parse_args(["--pred", "p", "--gt", "g"])
    assert (args.lesionwise, args.dilation, args.min_lesion_mm3, args.lesion_penalty_mm) == (False, 3, 50.0, 374.0)
    assert (args.output, args.tolerance_mm, args.penalty_mm, args.no_surface) == (None, 1.0, None, False)
    args = ap.parse_args(["--pred", "p", "--gt", "g", "--lesionwise", "--dilation", "2", "--min-lesion-mm3", "10", "--lesion-penalty-mm", "100"])
    assert (args.lesionwise, args.dilation, args.min_lesion_mm3, args.lesion_penalty_mm) == (True, 2, 10.0, 100.0)
    with pytest.raises(SystemExit):
        ap.parse_args(["--pred", "p", "--gt", "g", "--dilation", "three"])


def check_lesionwise_lines(lines, res):
    """the new block comes last, names the regions by WT / TC / ET only and carries none of the four phrases the pipeline searches for"""
    start = [i for i, ln in enumerate(lines) if ln.startswith("Lesion-wise")]
    assert len(start) == 1
    block = lines[start[0]:]
    assert start[0] > max(i for i, ln in enumerate(lines) if any(p in ln for p in PHRASES))
    assert not any(p in ln for ln in block for p in PHRASES)
    for key in ("WT", "TC", "ET"):
        m = res[key]["lesionwise"]
        hits = [ln for ln in block if ln.split()[:1] == [key]]
        assert len(hits) == 1, (key, block)
        assert f"{m['lesionwise_dice']:.4f}" in hits[0] and f"{m['lesionwise_hd95']:.2f}" in hits[0]
        assert f"{m['num_lesions']} / {m['num_counted']} / {m['num_tp']} / {m['num_fn']} / {m['num_fp']}" in hits[0]


@pytest.mark.parametrize("surfaces", [True, False])
def test_report_lines_with_the_lesionwise_block(amd, surfaces):
    from test_surface_distance_cpu import check_report_contract, made_up_metrics
    plain = made_up_metrics(amd, surfaces)
    without = amd.evaluate.report_lines(plain, "pred.nii.gz", "gt.nii.gz")
    res = made_up_metrics(amd, surfaces)
    for key, (P, G) in zip(("WT", "TC", "ET"), (lu.scene(), false_negative_and_false_positive(), _blank())):
        res[key]["lesionwise"] = lu.region_lesionwise(P, G, (1, 1, 1))
    lines = amd.evaluate.report_lines(res, "pred.nii.gz", "gt.nii.gz")
    assert all("\n" not in ln for ln in lines)
    check_report_contract(lines, {"mean_dice": 0.59636, "WT": 0.91234, "TC": 0.80555, "ET": 0.0712})
    check_lesionwise_lines(lines, res)
    first = next(i for i, ln in enumerate(lines) if ln.startswith("Lesion-wise"))
    assert lines[:first - 1] == without[:-1] and lines[-1] == without[-1], "without the flag the report is what it was; the block is appended"
