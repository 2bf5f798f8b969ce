"""Writes tests/golden/quality.json from the REFERENCE's own step 5 (development machine only: needs the reference tree).

    python tools/gen_quality_golden.py [--small-only]

``feature_extraction/step5_quality.py`` is imported unmodified from where it lies (its ``utils`` with an inert stand-in for the
absent nibabel package, as tools/gen_sequence_findings_golden.py does) and ``assess_segmentation_quality``,
``assess_image_quality``, ``detect_artifacts``, ``calculate_measurement_confidence`` and ``identify_limitations`` run over label
maps drawn by ``brats_amd.synthetic.shapes_map`` and volumes drawn by ``brats_amd.synthetic.mri_for_quality``.  Per case the
fixture holds the generator arguments, the voxel sizes, a sha256 of the label map and of the four volumes (all are regenerated
from the seeds, not stored) and the dicts the reference returned.  Intensities are integers below 2^15, as in BraTS files, so
the float32 copy the device works on equals the reference's float64 exactly and every Sobel magnitude is the root of an exact
integer.

The tool prints the branch table and refuses to write a fixture that misses one of the REQUIRED branches, or in which a
branching quantity lies within 1e-6 of its threshold, a value printed into a message within 1e-6 of the rounding boundary of
its format, or a brain voxel's distance within 1e-9 (relative) of a shell radius: such a case would pin rounding, not behaviour.
``--small-only`` leaves the 240 x 240 x 155 case out and writes nothing (for tuning the small cases).
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "quality.json")
SECTIONS = ("segmentation_quality", "image_quality", "artifact_detection", "measurement_confidence", "limitations_and_caveats")
SEQUENCES = ("T1", "T1ce", "T2", "FLAIR")
CLEARANCE, SHELL_CLEARANCE = 1e-6, 1e-9

S = (48, 56, 40)
C = (24, 28, 20)
TUMOUR = [["ball", 2, C, 10], ["ball", 3, C, 6], ["ball", 1, C, 3]]
FRAGMENTS = [["box", 2, (40, 10, 10), (41, 11, 11)], ["box", 2, (41, 11, 11), (42, 12, 12)], ["box", 2, (40, 20, 10), (41, 21, 11)],
             ["box", 2, (40, 30, 10), (41, 31, 11)], ["box", 2, (40, 40, 10), (41, 41, 11)], ["box", 2, (40, 45, 30), (41, 46, 31)],
             ["box", 2, (36, 50, 30), (37, 51, 31)]]
TIE = [[c, 0.12] for c in range(4)]  # the lowest 12 % of every channel tied: no background below the 10th percentile
CASES = [
    dict(name="clean", parts=TUMOUR, brain_axes=0.35),
    dict(name="none_zero_t1", parts=[], zero_channel=0),
    dict(name="tiny_tiny_brain", parts=[["ball", 3, C, 2]], brain_axes=0.15),
    dict(name="fair_segmentation", parts=[["ball", 2, (10, 28, 20), 13], ["ball", 0, (12, 28, 20), 7]] + FRAGMENTS, voxel_dims=(4.0, 4.0, 4.0)),
    dict(name="good_segmentation", parts=[["ball", 2, (42, 28, 20), 7], ["ball", 3, (42, 28, 20), 4], ["ball", 0, (42, 28, 20), 2]] + FRAGMENTS,
         voxel_dims=(1.0, 1.0, 1.5)),
    dict(name="fair_t2", parts=TUMOUR, plateau=TIE, levels=[[1000, 150], [1000, 150], [200, 3000], [1000, 150]]),
    dict(name="good_t2", parts=TUMOUR, plateau=TIE, levels=[[1000, 150], [1000, 150], [500, 1300], [1000, 150]]),
    dict(name="issues_poor_t2", parts=TUMOUR, plateau=[[2, 0.12]], dropout=[[1, (20, 36, 14), (30, 44, 24)]],
         spikes=[[3, 0.008, 5000, 0.008, 100], [2, 0.008, 8000, 0.0, 0]]),
    dict(name="bias_moderate", parts=TUMOUR, brain_axes=0.35, radial_gain=-0.5),
    dict(name="bias_severe_ghost", parts=TUMOUR, radial_gain=-0.62, ghost=[[1, 60, "exp"], [2, 90, "exp"], [3, 200, "flat"]]),
    dict(name="full_size", shape=(240, 240, 155), parts=[["ball", 2, (120, 130, 80), 22], ["ball", 3, (118, 126, 80), 13], ["ball", 1, (116, 124, 79), 7]],
         sigma=6.0, ghost=[[2, 40, "exp"]]),
]
SEED = 29
REQUIRED = (
    "seg/no_tumour", "seg/small", "seg/large", "seg/components>5", "seg/diagonal_fragments", "seg/holes_small", "seg/holes_large", "seg/boundary_low",
    "seg/boundary_high", "seg/grade/Excellent", "seg/grade/Good", "seg/grade/Fair", "seg/grade/Poor",
    "img/snr_background", "img/snr_proxy", "img/missing_non_t1", "img/outliers", "img/seq/Excellent", "img/seq/Good", "img/seq/Fair", "img/seq/Poor",
    "img/overall/Excellent", "img/overall/Good", "img/overall/Fair", "img/overall/Poor", "img/no_brain",
    "art/inhomogeneity/absent", "art/inhomogeneity/not_detected", "art/inhomogeneity/Moderate", "art/inhomogeneity/Severe", "art/motion/multi",
    "art/motion/absent", "art/wrap/true", "art/wrap/false", "art/gibbs/detected", "art/gibbs/not_detected", "art/gibbs/insufficient", "art/gibbs/no_tumour",
    "art/overall/None", "art/overall/Mild", "art/overall/Moderate to Severe",
    "cav/non_enhancing", "cav/boundary", "cav/t2_snr", "cav/suboptimal")


def _lists(v):
    return [_lists(x) for x in v] if isinstance(v, (list, tuple)) else v


def case_args(case):
    return {"seed": case.get("seed", SEED), "shape": list(case.get("shape", S)), "parts": _lists(case["parts"]), "levels": _lists(case.get("levels")),
            "brain_axes": case.get("brain_axes", 0.47), "radial_gain": float(case.get("radial_gain", 0.0)), "plateau": _lists(case.get("plateau", [])),
            "ghost": _lists(case.get("ghost", [])), "dropout": _lists(case.get("dropout", [])), "spikes": _lists(case.get("spikes", [])),
            "edge_noise": _lists(case.get("edge_noise")), "zero_channel": case.get("zero_channel"), "sigma": float(case.get("sigma", 3.0))}


def case_data(args):
    """(label map, [4, ...] volumes) of a fixture case from its stored arguments"""
    from brats_amd import synthetic
    seg = synthetic.shapes_map(args["seed"], tuple(args["shape"]), args["parts"])
    vols = synthetic.mri_for_quality(args["seed"] + 1, seg, levels=args["levels"], brain_axes=args["brain_axes"], radial_gain=args["radial_gain"],
                                     plateau=args["plateau"], ghost=args["ghost"], dropout=args["dropout"], spikes=args["spikes"],
                                     edge_noise=args["edge_noise"], zero_channel=args["zero_channel"], sigma=args["sigma"])
    return seg, vols


def load_step5():
    from oracle import gen_golden, ref_shim
    ref = os.path.join(ref_shim.REFERENCE_ROOT, "feature_extraction")
    utils = gen_golden._import_by_path("utils", os.path.join(ref, "utils.py"), {"nibabel": {}})
    saved = sys.modules.get("utils")
    sys.modules["utils"] = utils
    try:
        return utils, gen_golden._import_by_path("_reference_step5_quality", os.path.join(ref, "step5_quality.py"))
    finally:
        if saved is None:
            sys.modules.pop("utils", None)
        else:
            sys.modules["utils"] = saved


def _plain(o):
    if isinstance(o, np.generic):
        return o.item()
    raise TypeError(type(o))


def quantities(seg, vols, dims):
    """What step 5 branches on and prints, recomputed from the data without rounding: ``scores`` (name, value, thresholds),
    ``printed`` (name, value, decimals of its format), ``shell`` (the smallest relative gap between a brain voxel's distance and a
    shell radius, or None) and ``facts``, the branches that do not show in the returned dicts."""
    from scipy import ndimage
    scores, printed, facts, shell = [], [], set(), None
    wt = seg > 0
    if wt.any():
        volume = wt.sum() * (np.prod(dims) / 1000)
        scores.append(("wt_volume", volume, (0.5, 300.0)))
        if volume < 0.5:
            printed.append(("wt_volume", volume, 2))
        if volume > 300:
            printed.append(("wt_volume", volume, 0))
        hole_fraction = (ndimage.binary_fill_holes(wt) & ~wt).sum() / wt.sum()
        scores.append(("hole_fraction", hole_fraction, (0.1,)))
        if hole_fraction > 0.1:
            printed.append(("hole_percent", hole_fraction * 100, 0))
        if 0 < hole_fraction <= 0.1:
            facts.add("seg/holes_small")
        if hole_fraction > 0.1:
            facts.add("seg/holes_large")
        n26 = ndimage.label(wt, ndimage.generate_binary_structure(3, 3))[1]
        if n26 > 5 and ndimage.label(wt)[1] != n26:
            facts.add("seg/diagonal_fragments")
        if wt[:3].any() or wt[:, :3].any() or wt[:, :, :3].any():
            facts.add("seg/boundary_low")
        if wt[-3:].any() or wt[:, -3:].any() or wt[:, :, -3:].any():
            facts.add("seg/boundary_high")
    data = [v.astype(np.float64) for v in vols]
    t1 = data[0]
    brain = t1 > np.percentile(t1[t1 > 0], 5) if t1.max() > 0 else t1 > 0
    for name, x in zip(SEQUENCES, data):
        if brain.any():
            values = x[brain]
            background = ~brain & (x > 0) & (x < np.percentile(x[x > 0], 10))
            if background.sum() > 100:
                facts.add("img/snr_background")
                std = x[background].std()
            else:
                facts.add("img/snr_proxy")
                std = values.std()
            snr = values.mean() / std if std > 0 else 0
            scores.append((name + "/snr", snr, (5.0, 6.0, 10.0, 20.0)))
            if name == "T2" and snr < 6:
                printed.append(("T2/snr", snr, 1))
            zero_fraction = ((x == 0) & brain).sum() / brain.sum()
            iqr = np.percentile(values, 75) - np.percentile(values, 25)
            outliers = ((values > np.percentile(values, 99) + 3 * iqr).sum() + (values < np.percentile(values, 1) - 3 * iqr).sum()) / len(values)
            for what, fraction in (("zero", zero_fraction), ("outlier", outliers)):
                scores.append((f"{name}/{what}_fraction", fraction, (0.01,)))
                if fraction > 0.01:
                    printed.append((f"{name}/{what}_percent", fraction * 100, 1))
        ghost = ~brain & (x > 0)
        if ghost.sum() > 1000:
            scores.append((name + "/background_cv", x[ghost].std() / x[ghost].mean(), (0.5,)))
    if brain.any():
        coords = np.where(brain)
        centre = [np.mean(coords[i]) for i in range(3)]
        dist = np.sqrt((coords[0] - centre[0]) ** 2 + (coords[1] - centre[1]) ** 2 + (coords[2] - centre[2]) ** 2)
        top = dist.max()
        if top > 0:
            shell = float(min(np.abs(dist - top * f).min() / (top * f) for f in (0.3, 0.7)))
        inner, outer = t1[brain][dist < top * 0.3], t1[brain][dist > top * 0.7]
        if len(inner) > 100 and len(outer) > 100:
            scores.append(("inhomogeneity_ratio", outer.mean() / inner.mean(), (0.6, 0.7, 1.4, 1.6)))
        else:
            facts.add("art/inhomogeneity/absent")
    if wt.any():
        edge = wt & ~ndimage.binary_erosion(wt, iterations=2)
        if edge.sum() > 100:
            g = np.sqrt(sum(ndimage.sobel(t1, axis=a) ** 2 for a in range(3)))[edge]
            scores.append(("edge_gradient_cv", g.std() / g.mean() if g.mean() > 0 else 0, (1.5,)))
    return scores, printed, shell, facts


def branches(expected, facts):
    """the names of REQUIRED a case hits"""
    hit = set(facts)
    sq, iq, art, cav = (expected[k] for k in ("segmentation_quality", "image_quality", "artifact_detection", "limitations_and_caveats"))
    warnings = " | ".join(sq["warnings"])
    if "num_components" not in sq:
        hit.add("seg/no_tumour")
    for key, text in (("seg/small", "Very small"), ("seg/large", "Very large"), ("seg/components>5", "Multiple disconnected")):
        if text in warnings:
            hit.add(key)
    hit.add("seg/grade/" + sq["grade"])
    for m in iq["sequences"].values():
        hit.add("img/seq/" + m["quality"])
        if m["issues"] == ["No brain tissue detected"]:
            hit.add("img/no_brain")
        if any(i.startswith("Intensity outliers") for i in m["issues"]):
            hit.add("img/outliers")
    if any(i.startswith("Missing data") for k in SEQUENCES[1:] for i in iq["sequences"][k]["issues"]):
        hit.add("img/missing_non_t1")
    hit.add("img/overall/" + iq["overall_quality"])
    d = art["details"]
    if "intensity_inhomogeneity" in d:
        hit.add("art/inhomogeneity/" + (d["intensity_inhomogeneity"].get("severity", "?") if d["intensity_inhomogeneity"]["detected"] else "not_detected"))
    hit.add("art/motion/multi" if len(d["motion_ghosting"].get("affected_sequences", [])) >= 2 else
            ("art/motion/single" if d["motion_ghosting"]["detected"] else "art/motion/absent"))
    hit.add("art/wrap/true" if d["wrap_around"]["detected"] else "art/wrap/false")
    gibbs = d["gibbs_ringing"]
    hit.add("art/gibbs/detected" if gibbs["detected"] else "art/gibbs/insufficient" if "note" in gibbs else
            "art/gibbs/no_tumour" if "num_components" not in sq else "art/gibbs/not_detected")
    hit.add("art/overall/" + art["severity"])
    for key, text in (("cav/non_enhancing", "Non-enhancing"), ("cav/boundary", "Tumor at image boundary"), ("cav/t2_snr", "Low T2 SNR"),
                      ("cav/suboptimal", "Suboptimal image quality")):
        if any(c.startswith(text) for c in cav["caveats"]):
            hit.add(key)
    return hit


def too_close(name, scores, printed, shell):
    bad = []
    for what, value, thresholds in scores:
        for t in thresholds:
            if abs(value - t) <= CLEARANCE * max(1.0, abs(t)):
                bad.append(f"{name}: {what} = {value!r} within {CLEARANCE} of {t}")
    for what, value, decimals in printed:
        scaled = value * 10 ** decimals
        if abs(scaled - (math.floor(scaled) + 0.5)) <= CLEARANCE * 10 ** decimals:
            bad.append(f"{name}: {what} = {value!r} within {CLEARANCE} of a rounding boundary of :.{decimals}f")
    if shell is not None and shell <= SHELL_CLEARANCE:
        bad.append(f"{name}: a brain voxel's distance lies within {shell:.3g} (relative) of a shell radius")
    return bad


def generate(small_only=False, verbose=False):
    """(fixture, branches hit per case, complaints)"""
    utils, s5 = load_step5()
    cases, hits, bad = [], {}, []
    for case in CASES:
        if small_only and "shape" in case:
            continue
        args = case_args(case)
        seg, vols = case_data(args)
        assert vols.max() < 2 ** 15 and vols.min() >= 0 and np.array_equal(vols, np.rint(vols))
        dims = [float(v) for v in case.get("voxel_dims", (1.0, 1.0, 1.0))]
        seg_i = np.round(seg).astype(np.int32)  # step5_quality.py:626
        mri = {k: v.astype(np.float64) for k, v in zip(SEQUENCES, vols)}  # what nibabel's get_fdata hands the reference, :652
        masks = utils.get_tumor_masks(seg_i)
        brain = utils.get_brain_mask(mri["T1"])
        seg_quality = s5.assess_segmentation_quality(seg_i, masks, dims)
        image_quality = s5.assess_image_quality(mri, brain)
        expected = {"segmentation_quality": seg_quality, "image_quality": image_quality, "artifact_detection": s5.detect_artifacts(mri, brain, seg_i),
                    "measurement_confidence": s5.calculate_measurement_confidence({}),
                    "limitations_and_caveats": s5.identify_limitations(seg_quality, image_quality, masks)}
        expected = json.loads(json.dumps(expected, default=_plain))
        scores, printed, shell, facts = quantities(seg, vols, dims)
        hits[case["name"]] = branches(expected, facts)
        bad += too_close(case["name"], scores, printed, shell)
        if verbose:
            print(case["name"], " ".join(f"{n}={v:.6g}" for n, v, _ in scores), f"shell_gap={shell}")
        cases.append({"name": case["name"], "args": args, "voxel_dims": dims,
                      "sha256": {"seg": hashlib.sha256(seg.tobytes()).hexdigest(), "vols": hashlib.sha256(vols.tobytes()).hexdigest()},
                      "expected": expected})
    out = {"generator": "tools/gen_quality_golden.py (reference functions imported from feature_extraction/step5_quality.py)", "cases": cases}
    return out, hits, bad


def dumps(data):
    """one line per case: the fixture stays below the size of the step-1 fixture"""
    head = json.dumps({k: v for k, v in data.items() if k != "cases"}, ensure_ascii=False)[:-1]
    return head + ', "cases": [\n' + ",\n".join(json.dumps(c, ensure_ascii=False, separators=(",", ":")) for c in data["cases"]) + "\n]}\n"


if __name__ == "__main__":
    small_only = "--small-only" in sys.argv[1:]
    data, hits, bad = generate(small_only, verbose=True)
    for name, hit in hits.items():
        print(name, "|", ", ".join(sorted(hit)))
    missing = [b for b in REQUIRED if not any(b in hit for hit in hits.values())]
    if missing:
        bad.append("no case hits: " + ", ".join(missing))
    if bad or small_only:
        sys.exit("not written:\n" + "\n".join(bad or ["--small-only"]))
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(dumps(data))
    print(os.path.getsize(OUT), "bytes")
