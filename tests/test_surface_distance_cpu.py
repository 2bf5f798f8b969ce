"""not gpu: the host half of the surface-distance metrics (HD95, ASSD, surface Dice) - the declarations of the three
new entry points, the pure-numpy metrics against the oracle of surface_distance_util.py, the oracle's own box invariance, and the
command's arguments and report."""
import os
import re

import numpy as np
import pytest

import surface_distance_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mi355_region_surfaces", "mi355_edt_to_flagged_f64", "mi355_gather_flagged_f64")
FLOATS = ("hd", "hd95", "assd", "surface_dice")
INTEGERS = ("within_tolerance_pred", "within_tolerance_gt", "surface_voxels_pred", "surface_voxels_gt")


def test_new_symbols_are_declared_bound_and_built(amd):
    with open(os.path.join(ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(amd._lib.__file__), "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym
        assert sym in amd._lib.EXPORTS, sym
        assert f"lib.{sym}.argtypes" in binding, sym
    assert "surface_distance.hip" in amd._build.SOURCES
    limit = int(re.search(r"#define MI355_SURFACE_EDT_MAX_LINE (\d+)", header).group(1))
    assert limit >= 256, "a 240 x 240 x 155 box must fit the tile"
    assert int(re.search(r"#define MI355_GATHER_CHUNK (\d+)", header).group(1)) == amd.evaluate.GATHER_CHUNK
    with open(os.path.join(os.path.dirname(amd._lib.__file__), "csrc", "surface_distance.hip"), encoding="utf-8") as f:
        assert "device_scratch(" not in f.read(), "the new file takes all working memory from its caller"
    for name in ("surface_distances", "surface_metrics_from_distances", "surface_metrics", "evaluate_with_surfaces", "report_lines", "main"):
        assert callable(getattr(amd.evaluate, name)), name


def _same(got, want, what):
    for k in FLOATS:
        worst, ok = su.close(got[k], want[k])
        assert ok, (what, k, got[k], want[k], worst)
    for k in INTEGERS:
        assert got[k] == want[k] and isinstance(got[k], int), (what, k, got[k], want[k])


HAND_MADE = {
    # the pooled percentile is not the larger of the two per-direction percentiles, nor the 95th percentile of either
    "pooled_percentile": (np.arange(1, 41, dtype=np.float64), np.array([100.0, 0.25, 0.5])),
    "long_tail_in_one_direction": (np.array([0.0, 0.0, 1.0, 1.0, 1.0, 9.0]), np.array([0.0] * 30 + [2.0])),
    "one_element_each": (np.array([2.5]), np.array([0.75])),
    "one_element_against_many": (np.array([1.0]), np.linspace(0.0, 7.0, 23)),
    "all_zero": (np.zeros(5), np.zeros(7)),
    "exactly_at_tolerance": (np.array([1.0, 1.0, 2.0]), np.array([1.0, 0.5])),
}


@pytest.mark.parametrize("name", list(HAND_MADE))
@pytest.mark.parametrize("tolerance", [1.0, 2.0, 0.3])
def test_metrics_from_hand_made_distances(amd, name, tolerance):
    d_ab, d_ba = HAND_MADE[name]
    got = amd.evaluate.surface_metrics_from_distances(d_ab, d_ba, tolerance_mm=tolerance)
    _same(got, su.metrics(d_ab, d_ba, tolerance), name)
    assert got["hd"] == max(d_ab.max(), d_ba.max())
    assert got["hd95"] == np.percentile(np.hstack((d_ab, d_ba)), 95)


def test_pooled_percentile_differs_from_per_direction_maxima(amd):
    d_ab, d_ba = HAND_MADE["pooled_percentile"]
    got = amd.evaluate.surface_metrics_from_distances(d_ab, d_ba)
    per_direction = max(np.percentile(d_ab, 95), np.percentile(d_ba, 95))
    assert got["hd"] == 100.0 and got["hd95"] != per_direction and got["hd95"] < got["hd"]
    assert got["assd"] == (d_ab.mean() + d_ba.mean()) / 2
    assert got["surface_dice"] == (1 + 2) / 43 and (got["within_tolerance_pred"], got["within_tolerance_gt"]) == (1, 2)


@pytest.mark.parametrize("penalty", [None, 373.13])
def test_empty_masks(amd, penalty):
    f = amd.evaluate.surface_metrics_from_distances
    both = f(np.zeros(0), np.zeros(0), penalty_mm=penalty)
    assert (both["hd"], both["hd95"], both["assd"], both["surface_dice"]) == (0.0, 0.0, 0.0, 1.0)
    _same(both, su.metrics(np.zeros(0), np.zeros(0), 1.0, penalty), "both empty")
    for d_ab, d_ba in ((np.zeros(0), np.full(4, np.inf)), (np.full(3, np.inf), np.zeros(0)), (np.zeros(0), np.array([1.0, 2.0]))):
        one = f(d_ab, d_ba, penalty_mm=penalty)
        assert one["hd"] == penalty and one["hd95"] == penalty and one["assd"] == penalty and one["surface_dice"] == 0.0
        assert (one["surface_voxels_pred"], one["surface_voxels_gt"]) == (len(d_ab), len(d_ba))
        assert one["within_tolerance_pred"] == 0 and one["within_tolerance_gt"] == 0
        _same(one, su.metrics(d_ab, d_ba, 1.0, penalty), "one empty")


@pytest.mark.parametrize("shape", [(19, 23, 17), (9, 31, 40)])
@pytest.mark.parametrize("spacing", su.SPACINGS)
def test_oracle_is_box_invariant(shape, spacing):
    """surfaces first, crop second: every site and every query lies inside the joint box, so the distances do not change - bit for bit"""
    pred, gt = su.label_pair(41, shape)
    for name, labels in su.REGIONS.items():
        whole = su.region_distances(pred, gt, labels, spacing)
        boxed = su.region_distances(pred, gt, labels, spacing, crop=True)
        assert len(whole[0]) > 0 and len(whole[1]) > 0, name
        assert np.array_equal(whole[0], boxed[0]) and np.array_equal(whole[1], boxed[1]), (name, spacing)
    # cropping FIRST would change the surface: a mask that fills its box has no interior voxel on the box faces
    mask = np.zeros((8, 8, 8), bool)
    mask[2:6, 2:6, 2:6] = True
    assert su.surface(mask)[2:6, 2:6, 2:6].sum() == 64 - 8 and su.surface(mask[2:6, 2:6, 2:6]).sum() == 64 - 8
    mask[:, :, :] = True
    assert su.surface(mask).sum() == 512 - 216, "a position outside the volume counts as background"


def test_generators_are_nested_and_seeded():
    pred, gt = su.label_pair(7, (24, 40, 72))
    again, _ = su.label_pair(7, (24, 40, 72))
    assert np.array_equal(pred, again) and not np.array_equal(pred, gt)
    for seg in (pred, gt, su.nested_labels(3, (19, 23, 17))):
        assert seg.dtype == np.uint8 and set(np.unique(seg)) == {0, 1, 2, 3}


def test_refusals_need_no_device(amd):
    import torch
    ev = amd.evaluate
    a = torch.zeros((3, 4, 5), dtype=torch.uint8)
    with pytest.raises(ValueError, match="shapes"):
        ev.surface_distances(a, torch.zeros((3, 4, 6), dtype=torch.uint8), (1, 1, 1))
    with pytest.raises(ValueError, match="uint8"):
        ev.surface_distances(a, a.to(torch.int16), (1, 1, 1))
    for bad in ((1, 1), (1, 1, 0), (1, -1, 1), (1, float("nan"), 1), (1, float("inf"), 1), "abc", None):
        with pytest.raises(ValueError, match="spacing"):
            ev.surface_distances(a, a, bad)
    with pytest.raises(ValueError, match="regions"):
        ev.surface_distances(a, a, (1, 1, 1), regions={str(k): (1,) for k in range(5)})


def test_parser_accepts_the_reference_flags_alone(amd):
    ap = amd.evaluate.build_parser()
    args = ap.parse_args(["--pred", "P.nii.gz", "--gt", "G.nii.gz"])
    assert (args.pred, args.gt, args.output, args.tolerance_mm, args.penalty_mm, args.no_surface) == ("P.nii.gz", "G.nii.gz", None, 1.0, None, False)
    args = ap.parse_args(["--pred", "p", "--gt", "g", "--output", "o.json", "--tolerance-mm", "2", "--penalty-mm", "373.13", "--no-surface"])
    assert (args.output, args.tolerance_mm, args.penalty_mm, args.no_surface) == ("o.json", 2.0, 373.13, True)
    with pytest.raises(SystemExit):
        ap.parse_args(["--pred", "p"])


def made_up_metrics(amd, surfaces=True):
    overlap = {"iou": 0.5, "sensitivity": 0.75, "tp": 1.0, "fp": 1.0, "fn": 1.0}
    res = {lab: dict(overlap, dice=0.1 * lab) for lab in (1, 2, 3)}
    res.update(WT=dict(overlap, dice=0.91234), TC=dict(overlap, dice=0.80555), ET=dict(overlap, dice=0.0712), mean_dice=0.59636)
    if surfaces:
        res["WT"].update(amd.evaluate.surface_metrics_from_distances([1.0, 2.0, 3.5], [0.5, 12.25]))
        res["TC"].update(amd.evaluate.surface_metrics_from_distances([], []))
        res["ET"].update(amd.evaluate.surface_metrics_from_distances([], [np.inf, np.inf]))
    return res


def check_report_contract(lines, want):
    """what the pipeline's parser looks for: exactly one line per phrase, the score as NN.NN%, no 'Dice' / 'Label' in the last three"""
    for phrase, key in (("Mean Dice Score", "mean_dice"), ("Whole Tumor", "WT"), ("Tumor Core", "TC"), ("Enhancing Tumor", "ET")):
        hits = [ln for ln in lines if phrase in ln]
        assert len(hits) == 1, (phrase, hits)
        m = re.search(r"(\d+\.\d+)%", hits[0])
        assert m and re.fullmatch(r"\d{1,3}\.\d\d", m.group(1)), hits[0]
        assert float(m.group(1)) == pytest.approx(100 * want[key], abs=0.005 + 1e-9), hits[0]
        if phrase != "Mean Dice Score":
            assert "Dice" not in hits[0] and "Label" not in hits[0], hits[0]


@pytest.mark.parametrize("surfaces", [True, False])
def test_report_lines_meet_the_pipeline_contract(amd, surfaces):
    res = made_up_metrics(amd, surfaces)
    lines = amd.evaluate.report_lines(res, "pred.nii.gz", "gt.nii.gz")
    assert all("\n" not in ln for ln in lines)
    check_report_contract(lines, {"mean_dice": 0.59636, "WT": 0.91234, "TC": 0.80555, "ET": 0.0712})
    text = "\n".join(lines)
    assert ("HD95" in text and "ASSD" in text) == surfaces
    if surfaces:   # the surface rows come after the four lines and speak of the regions by their short names
        last = max(i for i, ln in enumerate(lines) if "Mean Dice Score" in ln or "Tumor" in ln)
        first = min(i for i, ln in enumerate(lines) if "HD95" in ln)
        assert first > last and "n/a" in text
