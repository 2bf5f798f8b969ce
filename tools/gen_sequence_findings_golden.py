"""Writes tests/golden/sequence_findings.json from the REFERENCE's own step 1 (development machine only: needs the reference tree).

    python tools/gen_sequence_findings_golden.py

``feature_extraction/step1_sequence_findings.py`` is imported unmodified from where it lies (its ``utils`` with an inert
stand-in for the absent nibabel package, as tools/gen_morphology_golden.py does) and ``analyze_all_region_signals``,
``analyze_contrast_enhancement``, ``detect_t2_flair_mismatch`` and ``calculate_volume`` run over label maps drawn by
``brats_amd.synthetic.shapes_map`` and volumes drawn by ``brats_amd.synthetic.mri_with_region_gains``.  Per case the fixture
holds the generator arguments, the voxel sizes, a sha256 of the label map and of the four volumes (all are regenerated from the
seeds, not stored) and the dicts the reference returned.  Intensities are integers below 2^24, as in BraTS files, so the
float32 copy the device works on equals the reference's float64 exactly.

The tool prints the branch table and refuses to write a fixture in which a score lies within 1e-6 of a classification
threshold or a value handed to ``round(..., 3)`` within 1e-6 of a rounding boundary: such a case would pin rounding, not
behaviour.
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "sequence_findings.json")
SECTIONS = ("region_signal_analysis", "contrast_enhancement", "t2_flair_mismatch", "volumes")
CLEARANCE = 1e-6
RATIO_THRESHOLDS = (0.6, 0.85, 1.15, 1.5)
CV_THRESHOLDS = (0.15, 0.25, 0.35)
ENHANCEMENT_THRESHOLDS = (1.05, 1.2, 1.5, 2.0)

S = (48, 56, 40)
C = (24, 28, 20)
CASES = [
    dict(name="none", shape=S, parts=[], gains=[]),
    dict(name="ring", shape=S, parts=[["ball", 2, C, 13], ["ball", 3, C, 9], ["ball", 1, C, 6]],
         gains=[[1, 0.7, 0.5, 1.8, 1.0], [2, 0.9, 0.9, 1.4, 1.4], [3, 1.0, 2.4, 1.3, 1.3]], et_noise=0.35),
    dict(name="solid_ncr", shape=S, parts=[["ball", 3, C, 10], ["ball", 1, C, 2]], gains=[[1, 0.8, 0.8, 1.3, 1.25], [3, 1.0, 1.7, 1.2, 1.25]],
         et_noise=0.52, voxel_dims=(0.9375, 0.9375, 1.875)),
    dict(name="label4_no_ncr", shape=S, parts=[["ball", 2, C, 12], ["ball", 4, C, 8]], gains=[[2, 0.9, 0.9, 1.6, 1.0], [4, 1.0, 1.35, 1.25, 1.25]],
         et_noise=0.8),
    dict(name="non_enhancing", shape=S, parts=[["ball", 2, C, 12], ["ball", 1, C, 5]], gains=[[1, 0.5, 0.5, 1.6, 1.4], [2, 0.9, 0.9, 1.4, 1.6]]),
    dict(name="mild", shape=S, parts=[["ball", 3, (20, 30, 18), 9]], gains=[[3, 1.0, 1.12, 1.0, 1.0]]),
    dict(name="minimal", shape=S, parts=[["ball", 2, C, 13], ["ball", 3, C, 9], ["ball", 1, (24, 28, 14), 3]],
         gains=[[1, 0.75, 0.75, 1.3, 0.7], [2, 1.0, 1.0, 1.25, 1.3], [3, 1.0, 1.0, 1.1, 1.1]], et_noise=0.1),
    dict(name="zero_t1", shape=S, parts=[["ball", 3, C, 9], ["ball", 1, C, 5]], gains=[[1, 1.0, 0.7, 1.4, 1.2], [3, 1.0, 1.6, 1.2, 1.2]], zero_channel=0),
    dict(name="no_brain_mask", shape=S, parts=[["ball", 2, (4, 5, 3), 9], ["ball", 3, (4, 5, 3), 5]], gains=[[2, 0.9, 0.9, 1.4, 1.4], [3, 1.0, 1.3, 1.2, 1.2]],
         brain=False, et_noise=0.2),
    dict(name="full_size", shape=(240, 240, 155), parts=[["ball", 2, (120, 130, 80), 22], ["ball", 3, (118, 126, 80), 13], ["ball", 1, (116, 124, 79), 7]],
         gains=[[1, 0.7, 0.6, 1.7, 1.1], [2, 0.9, 0.9, 1.45, 1.5], [3, 1.0, 1.8, 1.25, 1.3]], et_noise=0.45, sigma=6.0),
]
SEED = 23


def case_args(case):
    return {"seed": case.get("seed", SEED), "shape": list(case["shape"]), "parts": [[list(v) if isinstance(v, tuple) else v for v in p] for p in case["parts"]],
            "gains": [[float(v) if i else int(v) for i, v in enumerate(row)] for row in case["gains"]], "et_noise": float(case.get("et_noise", 0.0)),
            "zero_channel": case.get("zero_channel"), "sigma": float(case.get("sigma", 3.0)), "brain": bool(case.get("brain", True))}


def case_data(args):
    """(label map, [4, ...] volumes) of a fixture case from its stored arguments"""
    from brats_amd import synthetic
    seg = synthetic.shapes_map(args["seed"], tuple(args["shape"]), args["parts"])
    vols = synthetic.mri_with_region_gains(args["seed"] + 1, seg, args["gains"], et_noise=args["et_noise"], zero_channel=args["zero_channel"],
                                           sigma=args["sigma"], brain=args["brain"])
    return seg, vols


def load_step1():
    from oracle import gen_golden, ref_shim
    ref = os.path.join(ref_shim.REFERENCE_ROOT, "feature_extraction")
    utils = gen_golden._import_by_path("utils", os.path.join(ref, "utils.py"), {"nibabel": {}})
    saved = sys.modules.get("utils")
    sys.modules["utils"] = utils
    try:
        return utils, gen_golden._import_by_path("_reference_step1_sequence_findings", os.path.join(ref, "step1_sequence_findings.py"))
    finally:
        if saved is None:
            sys.modules.pop("utils", None)
        else:
            sys.modules["utils"] = saved


def _plain(o):
    if isinstance(o, np.generic):
        return o.item()
    raise TypeError(type(o))


def scores(expected):
    """(name, value, thresholds) of every score of a case that a classification of step 1 branches on, recomputed without
    rounding from the means and deviations the reference returned"""
    out = []
    rs = expected["region_signal_analysis"]
    normal = rs["normal_brain_reference"]
    for key, region in rs["regions"].items():
        for seq in ("T1", "T2", "FLAIR", "T1ce"):
            nm = normal[seq + "_mean"]
            out.append((f"{key}/{seq}/ratio", region[seq]["mean_intensity"] / nm if nm and nm > 0 else 1.0, RATIO_THRESHOLDS))
        t1 = region["T1"]["mean_intensity"]
        out.append((f"{key}/enhancement_ratio", region["T1ce"]["mean_intensity"] / t1 if t1 and t1 > 0 else 1.0, ENHANCEMENT_THRESHOLDS))
        out.append((f"{key}/enhancement_ratio_rounded", region["T1ce"]["enhancement_ratio"], ENHANCEMENT_THRESHOLDS))
        out.append((f"{key}/T2_ratio_rounded", region["T2"]["ratio_to_normal"], (1.3,)))
        out.append((f"{key}/FLAIR_minus_0.7_T2", region["FLAIR"]["ratio_to_normal"] - region["T2"]["ratio_to_normal"] * 0.7, (0.0,)))
    et = rs["regions"].get("et")
    if et and et["T1ce"]["mean_intensity"] > 0:
        out.append(("et/cv", et["T1ce"]["std"] / et["T1ce"]["mean_intensity"], CV_THRESHOLDS))
    return out


def rounded(expected):
    """(name, value) of everything the reference hands to round(..., 3)"""
    return [(n, v) for n, v, _ in scores(expected) if n.endswith("/ratio") or n.endswith("/enhancement_ratio") or n == "et/cv"]


def branch_table(cases):
    rows = []
    for c in cases:
        e = c["expected"]
        ce, regions = e["contrast_enhancement"], e["region_signal_analysis"]["regions"]
        labels = sorted({regions[k][s]["signal_label"] for k in regions for s in ("T1", "T2", "FLAIR", "T1ce")})
        rows.append((c["name"], "+".join(regions) or "-", str(ce["pattern"]), str(ce["heterogeneity"]), ce.get("enhancement_strength", "-"),
                     "mismatch " + e["t2_flair_mismatch"].get("region", "no"), ", ".join(labels) or "-",
                     "T1 normal " + ("None" if e["region_signal_analysis"]["normal_brain_reference"]["T1_mean"] is None else "set")))
    return rows


def generate():
    utils, s1 = load_step1()
    cases = []
    for case in CASES:
        args = case_args(case)
        seg, vols = case_data(args)
        assert vols.max() < 2 ** 24 and vols.min() >= 0 and np.array_equal(vols, np.rint(vols))
        dims = tuple(float(v) for v in case.get("voxel_dims", (1.0, 1.0, 1.0)))
        seg_i = np.round(seg).astype(np.int32)  # step1_sequence_findings.py:401
        t1, t1ce, t2, flair = (v.astype(np.float64) for v in vols)  # what nibabel's get_fdata hands the reference
        masks = utils.get_tumor_masks(seg_i)
        volume_cm3 = float(np.prod(dims) / 1000)  # utils.get_voxel_dimensions
        signals = s1.analyze_all_region_signals(t1, t2, flair, t1ce, masks, seg_i)
        expected = {"region_signal_analysis": signals,
                    "contrast_enhancement": s1.analyze_contrast_enhancement(t1, t1ce, masks, signals),
                    "t2_flair_mismatch": s1.detect_t2_flair_mismatch(signals),
                    "volumes": {name: utils.calculate_volume(masks[key], volume_cm3) for name, key in
                                (("Whole Tumor (WT)", "wt"), ("Tumor Core (TC)", "tc"), ("Enhancing Tumor (ET)", "et"), ("Necrotic Core (NCR)", "ncr"),
                                 ("Peritumoral Edema (ED)", "ed"))}}  # :508-514
        cases.append({"name": case["name"], "args": args, "voxel_dims": list(dims),
                      "sha256": {"seg": hashlib.sha256(seg.tobytes()).hexdigest(), "vols": hashlib.sha256(vols.tobytes()).hexdigest()},
                      "expected": expected})
    out = {"generator": "tools/gen_sequence_findings_golden.py (reference functions imported from feature_extraction/step1_sequence_findings.py)",
           "cases": cases}
    return json.loads(json.dumps(out, default=_plain))


def too_close(data):
    bad = []
    for c in data["cases"]:
        for name, value, thresholds in scores(c["expected"]):
            for t in thresholds:
                if abs(value - t) <= CLEARANCE:
                    bad.append(f"{c['name']}: {name} = {value!r} within {CLEARANCE} of {t}")
        for name, value in rounded(c["expected"]):
            boundary = (math.floor(value * 1000) + 0.5) / 1000
            if abs(value - boundary) <= CLEARANCE:
                bad.append(f"{c['name']}: {name} = {value!r} within {CLEARANCE} of the rounding boundary {boundary}")
    return bad


if __name__ == "__main__":
    data = generate()
    for row in branch_table(data["cases"]):
        print(" | ".join(row))
    for c in data["cases"]:
        print(c["name"], " ".join(f"{n}={v:.6g}" for n, v, _ in scores(c["expected"]) if not n.endswith("rounded")))
    bad = too_close(data)
    if bad:
        sys.exit("not written:\n" + "\n".join(bad))
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(data, f, indent=1, ensure_ascii=False)
    print(os.path.getsize(OUT), "bytes")
