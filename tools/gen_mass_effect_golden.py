"""Writes tests/golden/mass_effect.json from the REFERENCE's own step 2 (development machine only: needs the reference tree).

    python tools/gen_mass_effect_golden.py [--small-only]

``feature_extraction/step2_mass_effect.py`` is imported unmodified from where it lies (its ``utils`` with an inert stand-in for the
absent nibabel package, as tools/gen_quality_golden.py does) and ``determine_anatomical_location``, ``calculate_midline_shift``,
``analyze_ventricular_compression``, ``analyze_sulcal_effacement`` and ``assess_herniation_risk`` run over label maps drawn by
``brats_amd.synthetic.shapes_map`` and T1 volumes drawn by ``brats_amd.synthetic.mri_for_mass_effect``.  The voxel sizes go in as
float32, as ``header.get_zooms()`` hands them to the reference, and ``np.random.seed(rng_seed)`` is called right before
``analyze_ventricular_compression``, which draws its samples from numpy's global generator.  Per case the fixture holds the
generator arguments, the voxel sizes, that seed, a sha256 of the label map and of the volume (both are regenerated from the
seeds, not stored), the dicts the reference returned, and three facts computed here with numpy and scipy: the number of tumour
and of CSF voxels and the exact tumour-to-CSF distance (a distance transform, the minimum over ALL pairs).  Intensities are
integers below 2^15, as in BraTS files, so the float32 copy the device works on equals the reference's float64 exactly.

The tool prints the branch table and refuses to write a fixture that misses one of the REQUIRED branches, or in which a
branching quantity lies within 1e-6 of its threshold or a value printed into a message within 1e-6 of the rounding boundary of
its format: such a case would pin rounding, not behaviour.  ``--small-only`` leaves the 240 x 240 x 155 case out and writes
nothing (for tuning the small cases).
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "mass_effect.json")
SECTIONS = ("anatomical_location", "midline_shift", "ventricular_compression", "sulcal_effacement", "herniation_risk")
CLEARANCE = 1e-6

S = (48, 56, 40)
C = (24, 28, 19)
LEFT, RIGHT = (14, 28, 19), (34, 28, 19)
OUTER_CUT = [[(4, 0, 0), (14, 56, 40)]]    # the left half loses its outer part: its centre of mass moves towards the midline
INNER_CUT = [[(14, 0, 0), (23, 56, 40)]]   # ... its inner part: away from the midline
SMALL = 0.15                               # a brain of about 1500 voxels: fewer than 1000 CSF-like ones


def _dark(left, right, factor=0.3):
    """CSF-like slabs `left` / `right` voxels thick on either side of the middle"""
    rows = []
    if left:
        rows.append([(22 - left, 8, 6), (22, 48, 34), factor])
    if right:
        rows.append([(26, 8, 6), (26 + right, 48, 34), factor])
    return rows


CASES = [
    dict(name="no_tumour", parts=[]),
    dict(name="no_brain", parts=[["ball", 2, C, 5]], zero=True),
    dict(name="shift_below", parts=[["ball", 2, LEFT, 5]], cuts=OUTER_CUT, voxel_dims=(0.5, 1.0, 1.0)),
    dict(name="shift_minimal", parts=[["ball", 2, LEFT, 5]], cuts=OUTER_CUT, voxel_dims=(1.5, 1.0, 1.0)),
    dict(name="shift_mild_right_tumour", parts=[["ball", 2, RIGHT, 7], ["ball", 3, RIGHT, 4]], cuts=OUTER_CUT, voxel_dims=(3.0, 1.0, 1.0)),
    dict(name="shift_moderate_negative", parts=[["ball", 2, LEFT, 7], ["ball", 1, LEFT, 3]], cuts=INNER_CUT, voxel_dims=(2.0, 1.0, 1.0)),
    dict(name="shift_severe", parts=[["ball", 2, LEFT, 7]], cuts=OUTER_CUT, voxel_dims=(12.0, 1.0, 1.0), noise=30.0, peri_scale=0.3),
    dict(name="shift_severe_negative_right", parts=[["ball", 2, RIGHT, 5]], cuts=INNER_CUT, voxel_dims=(4.0, 1.0, 1.0)),
    dict(name="csf_right_only", parts=[["ball", 2, (24, 29, 8), 4]], dark=_dark(0, 14)),
    dict(name="csf_left_only", parts=[["ball", 2, (38, 30, 15), 4]], dark=_dark(14, 0)),
    dict(name="csf_moderate", parts=[["ball", 2, (38, 30, 8), 4]], dark=_dark(6, 13)),
    dict(name="csf_mild", parts=[["ball", 2, (24, 30, 4), 3]], dark=_dark(12, 8)),
    dict(name="csf_even", parts=[["ball", 2, (24, 48, 19), 5]], dark=_dark(10, 10)),
    dict(name="small_brain_big_tumour", parts=[["ball", 2, C, 7], ["ball", 1, C, 3]], brain_axes=SMALL),
    dict(name="small_brain_small_tumour", parts=[["ball", 3, C, 3]], brain_axes=SMALL),
    dict(name="small_brain_far_tumour", parts=[["ball", 2, (6, 8, 6), 3]], brain_axes=SMALL),
    dict(name="effaced", parts=[["ball", 2, C, 7], ["ball", 3, C, 4]], noise=30.0, peri_scale=0.3),
    dict(name="partly_effaced", parts=[["ball", 2, (21, 28, 19), 7]], noise=30.0, peri_scale=0.68),
    dict(name="not_effaced", parts=[["ball", 2, (26, 28, 19), 7]], noise=30.0),
    dict(name="frontal_parietal_high", parts=[["ball", 2, (24, 20, 31), 5]]),
    dict(name="frontal_parietal_mid", parts=[["ball", 2, (24, 20, 23), 5]]),
    dict(name="frontal_temporal", parts=[["ball", 2, (10, 18, 19), 5]]),
    dict(name="large_tumour", parts=[["ball", 2, C, 6]], voxel_dims=(4.0, 4.0, 4.0)),
    dict(name="full_size", shape=(240, 240, 155), parts=[["ball", 2, (100, 130, 80), 22], ["ball", 3, (98, 126, 80), 13], ["ball", 1, (96, 124, 79), 7]],
         sigma=6.0, voxel_dims=(1.0, 1.0, 1.0)),
]
SEED = 31
GYRI = ("superior frontal gyrus region", "middle frontal gyrus region", "inferior frontal gyrus region", "superior parietal lobule region",
        "inferior parietal lobule region", "superior temporal gyrus region", "middle temporal gyrus region", "inferior temporal gyrus region",
        "occipital cortex region", "gyral localization not determined")
REQUIRED = (
    "mid/no_tumour", "mid/no_brain", "mid/below", "mid/Minimal", "mid/Mild", "mid/Moderate", "mid/Severe", "mid/shift_positive", "mid/shift_negative",
    "mid/tumour_left", "mid/tumour_right",
    "vent/no_brain", "vent/compressed_left", "vent/compressed_right", "vent/compressed_none", "vent/Severe", "vent/Moderate", "vent/Mild",
    "vent/None/Minimal", "vent/distance_none", "vent/tumour<=1000,csf>1000", "vent/tumour>1000,csf<=1000", "vent/tumour<=1000,csf<=1000",
    "vent/tumour>1000,csf>1000",
    "sulcal/no_tumour", "sulcal/no_peritumoral", "sulcal/no_distant", "sulcal/Moderate to Severe", "sulcal/Mild to Moderate", "sulcal/None/Minimal",
    "loc/left", "loc/right", "loc/left-predominant", "loc/right-predominant", "loc/bilateral", "loc/lobe/frontal", "loc/lobe/parietal",
    "loc/lobe/temporal", "loc/lobe/occipital", "loc/deep", "loc/indeterminate", "loc/depth/Deep", "loc/depth/Subcortical", "loc/depth/Cortical",
    *("loc/gyrus/" + g for g in GYRI),
    "hern/Low", "hern/Mild", "hern/Moderate", "hern/High", "hern/large_tumour",
    "cond/sampled>exact", "cond/small_sets_sampled==exact")


def _lists(v):
    return [_lists(x) for x in v] if isinstance(v, (list, tuple)) else v


def case_args(case):
    return {"seed": case.get("seed", SEED), "shape": list(case.get("shape", S)), "parts": _lists(case["parts"]), "brain_axes": case.get("brain_axes", 0.47),
            "cuts": _lists(case.get("cuts", [])), "dark": _lists(case.get("dark", [])), "noise": float(case.get("noise", 0.0)),
            "peri_scale": float(case.get("peri_scale", 1.0)), "zero": bool(case.get("zero", False)), "sigma": float(case.get("sigma", 3.0))}


def case_data(args):
    """(label map, T1 volume) of a fixture case from its stored arguments"""
    from brats_amd import synthetic
    seg = synthetic.shapes_map(args["seed"], tuple(args["shape"]), args["parts"])
    t1 = synthetic.mri_for_mass_effect(args["seed"] + 1, seg, brain_axes=args["brain_axes"], cuts=args["cuts"], dark=args["dark"], noise=args["noise"],
                                       peri_scale=args["peri_scale"], zero=args["zero"], sigma=args["sigma"])
    return seg, t1


def load_step2():
    from oracle import gen_golden, ref_shim
    ref = os.path.join(ref_shim.REFERENCE_ROOT, "feature_extraction")
    utils = gen_golden._import_by_path("utils", os.path.join(ref, "utils.py"), {"nibabel": {}})
    saved = sys.modules.get("utils")
    sys.modules["utils"] = utils
    try:
        return utils, gen_golden._import_by_path("_reference_step2_mass_effect", os.path.join(ref, "step2_mass_effect.py"))
    finally:
        if saved is None:
            sys.modules.pop("utils", None)
        else:
            sys.modules["utils"] = saved


def _plain(o):
    if isinstance(o, np.generic):
        return o.item()
    raise TypeError(type(o))


def masks(seg, t1):
    """(tumour, brain, csf) as step 2 forms them, utils.py:63-68 and step2_mass_effect.py:165-181"""
    x = t1.astype(np.float64)
    tumour = seg > 0
    brain = x > np.percentile(x[x > 0], 5) if x.max() > 0 else x > 0
    if not brain.any():
        return tumour, brain, np.zeros_like(brain)
    csf = (x < np.percentile(x[brain], 15)) & (x > 0) & ~tumour
    return tumour, brain, csf


def quantities(seg, t1, dims, expected, lobe_boxes):
    """What step 2 branches on and prints: ``scores`` (name, value, thresholds), ``printed`` (name, value, decimals of its
    format) and ``facts`` - the branches that do not show in the returned dicts, the set sizes and the exact distance."""
    from scipy import ndimage
    scores, printed, hit = [], [], set()
    tumour, brain, csf = masks(seg, t1)
    n_t, n_csf = int(tumour.sum()), int(csf.sum())
    facts = {"n_tumour": n_t, "n_csf": n_csf, "exact_distance_mm": None}
    x = t1.astype(np.float64)
    if x.max() > 0 and not brain.any():
        raise SystemExit("a plateau at the 5th percentile empties the brain mask: keep such volumes out of the fixture")
    loc, mid, vent, sul, hern = (expected[k] for k in SECTIONS)
    if n_t:
        shape = seg.shape
        left = tumour[:shape[0] // 2].sum() / n_t
        scores.append(("left_fraction", left, (0.9, 0.6, 0.4, 0.1)))
        b = [int(tumour[bx[0]:bx[1], bx[2]:bx[3], bx[4]:bx[5]].sum()) for bx in lobe_boxes(shape)]
        for name, n, t in (("frontal", b[0], 0.05), ("parietal", b[1], 0.05), ("temporal", b[2] + b[3], 0.05), ("occipital", b[4], 0.05), ("deep", b[5], 0.1)):
            scores.append((name + "_fraction", n / n_t, (t,)))
            if n / n_t > t:
                printed.append((name + "_percent", n / n_t * 100, 0))
        scores.append(("relative_depth", loc["relative_depth_score"], (0.7, 0.4)))
        scores.append(("centroid_z", loc["tumor_centroid"]["z"] / shape[2], (0.7, 0.5, 0.65, 0.45, 0.3)))
        volume = hern["tumor_volume_cm3"]
        scores.append(("tumour_volume", volume, (50.0,)))
        if any(s.startswith("Large tumor") for s in hern["herniation_signs"]):
            printed.append(("tumour_volume", volume, 1))
            hit.add("hern/large_tumour")
    if n_t and brain.any():
        scores.append(("shift_mm", mid["shift_mm"], (1.0, 3.0, 5.0, 10.0)))
        scores.append(("centroid_minus_midline", mid["tumor_centroid_x"] - mid["brain_midline_x"], (0.0,)))
        if mid["shift_mm"] >= 1:
            printed.append(("shift_mm", mid["shift_mm"], 1))
            positive = (mid["shift_direction"] == "Left to right") == (mid["tumor_hemisphere"] == "left")
            hit.add("mid/shift_positive" if positive else "mid/shift_negative")
    if brain.any():
        a, l, r = vent["asymmetry_ratio"], vent["left_ventricle_volume_cm3"], vent["right_ventricle_volume_cm3"]
        scores.append(("asymmetry_ratio", a, (0.15, 0.3, 0.5)))
        if l + r > 0:
            scores.append(("left_over_right", l / r if r else np.inf, (0.7,)))
            scores.append(("right_over_left", r / l if l else np.inf, (0.7,)))
        if a > 0.15:
            printed.append(("asymmetry_ratio", a, 2))
        if vent["tumor_to_ventricle_distance_mm"] is None:
            hit.add("vent/distance_none")
    if "variance_ratio" in sul:
        scores.append(("variance_ratio", sul["variance_ratio"], (0.6, 0.8)))
    if n_t and n_csf:
        hit.add(f"vent/tumour{'>' if n_t > 1000 else '<='}1000,csf{'>' if n_csf > 1000 else '<='}1000")
        exact = float(np.sqrt(np.rint(ndimage.distance_transform_edt(~csf) ** 2)[tumour].min()) * np.float32(dims[0]))
        facts["exact_distance_mm"] = exact
        sampled = vent["tumor_to_ventricle_distance_mm"]
        assert sampled >= exact, (sampled, exact)
        if sampled > exact:
            hit.add("cond/sampled>exact")
        if n_t <= 1000 and n_csf <= 1000:
            assert sampled == exact, (sampled, exact)
            hit.add("cond/small_sets_sampled==exact")
    return scores, printed, facts, hit


def branches(expected, hit):
    """the names of REQUIRED a case hits"""
    hit = set(hit)
    loc, mid, vent, sul, hern = (expected[k] for k in SECTIONS)
    if mid["severity"] == "No tumor detected":
        hit.add("mid/no_tumour")
    elif mid["severity"] == "Could not calculate":
        hit.add("mid/no_brain")
    else:
        hit.add("mid/below" if not mid["is_significant"] else "mid/" + mid["severity"])
        hit.add("mid/tumour_" + mid["tumor_hemisphere"])
    if vent["severity"] == "Could not analyze":
        hit.add("vent/no_brain")
    else:
        hit.add("vent/compressed_" + vent["compressed_side"])
        hit.add("vent/" + vent["severity"])
    hit.add({"No tumor detected": "sulcal/no_tumour", "Could not analyze": "sulcal/no_peritumoral"}.get(sul["severity"], "sulcal/" + sul["severity"]))
    if sul.get("details") == "Tumor occupies majority of brain volume":
        hit.discard("sulcal/Severe")
        hit.add("sulcal/no_distant")
    if loc["hemisphere"] != "None":
        hit.add("loc/" + loc["hemisphere"])
        for lobe in loc["lobes"]:
            hit.add("loc/deep" if lobe == "deep structures" else "loc/indeterminate" if lobe == "location indeterminate" else "loc/lobe/" + lobe)
        hit.add("loc/depth/" + loc["depth"].split()[0].split("/")[0])
        for g in loc["approximate_gyri"]:
            hit.add("loc/gyrus/" + g)
    hit.add("hern/" + hern["risk_level"])
    return hit


def too_close(name, scores, printed):
    bad = []
    for what, value, thresholds in scores:
        for t in thresholds:
            if abs(value - t) <= CLEARANCE * max(1.0, abs(t)):
                bad.append(f"{name}: {what} = {value!r} within {CLEARANCE} of {t}")
    for what, value, decimals in printed:
        scaled = value * 10 ** decimals
        if abs(scaled - (math.floor(scaled) + 0.5)) <= CLEARANCE * 10 ** decimals:
            bad.append(f"{name}: {what} = {value!r} within {CLEARANCE} of a rounding boundary of :.{decimals}f")
    return bad


def run_reference(s2, seg, t1, dims, rng_seed):
    """the five dicts, as ``analyze_mass_effect`` (:660-723) computes them from its loaded arrays"""
    seg_i = np.round(seg).astype(np.int32)   # :675
    x = t1.astype(np.float64)                # what nibabel's get_fdata hands the reference
    vd = [np.float32(v) for v in dims]       # list(header.get_zooms()[:3]), utils.py:119-121
    location = s2.determine_anatomical_location(seg_i, vd)
    midline = s2.calculate_midline_shift(x, seg_i, vd)
    np.random.seed(rng_seed)
    ventricle = s2.analyze_ventricular_compression(x, seg_i, vd)
    sulcal = s2.analyze_sulcal_effacement(x, seg_i, vd)
    volume = (seg_i > 0).sum() * np.prod(vd) / 1000
    expected = {"anatomical_location": location, "midline_shift": midline, "ventricular_compression": ventricle, "sulcal_effacement": sulcal,
                "herniation_risk": s2.assess_herniation_risk(midline, ventricle, sulcal, volume, location)}
    return json.loads(json.dumps(expected, default=_plain))


def generate(small_only=False, verbose=False):
    """(fixture, branches hit per case, complaints)"""
    from brats_amd.mass_effect import lobe_boxes
    _, s2 = load_step2()
    cases, hits, bad = [], {}, []
    for case in CASES:
        if small_only and "shape" in case:
            continue
        args = case_args(case)
        seg, t1 = case_data(args)
        assert t1.max() < 2 ** 15 and t1.min() >= 0 and np.array_equal(t1, np.rint(t1))
        dims = [float(v) for v in case.get("voxel_dims", (1.0, 1.0, 1.0))]
        rng_seed = int(case.get("rng_seed", args["seed"]))
        expected = run_reference(s2, seg, t1, dims, rng_seed)
        scores, printed, facts, hit = quantities(seg, t1, dims, expected, lobe_boxes)
        hits[case["name"]] = branches(expected, hit)
        bad += too_close(case["name"], scores, printed)
        if verbose:
            print(case["name"], " ".join(f"{n}={v:.6g}" for n, v, _ in scores), facts, expected["ventricular_compression"].get("tumor_to_ventricle_distance_mm"))
        cases.append({"name": case["name"], "args": args, "voxel_dims": dims, "rng_seed": rng_seed,
                      "sha256": {"seg": hashlib.sha256(seg.tobytes()).hexdigest(), "t1": hashlib.sha256(t1.tobytes()).hexdigest()},
                      "facts": facts, "expected": expected})
    out = {"generator": "tools/gen_mass_effect_golden.py (reference functions imported from feature_extraction/step2_mass_effect.py)", "cases": cases}
    return out, hits, bad


def dumps(data):
    """one line per case"""
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
