"""Writes tests/golden/morphology.json from the REFERENCE's own step 4 (development machine only: needs the reference tree).

    python tools/gen_morphology_golden.py

``feature_extraction/step4_morphology.py`` is imported unmodified from where it lies (its ``utils`` with an inert stand-in
for the absent nibabel package, as tools/gen_multiplicity_golden.py does) and its five analysis functions run over label maps
drawn by ``brats_amd.synthetic.shapes_map`` and volumes drawn by ``brats_amd.synthetic.mri_for_label_map``.  Per case the
fixture holds the generator arguments, the voxel sizes, a sha256 of the label map and of the four volumes (all are regenerated
from the seeds, not stored) and the dicts the reference returned.  Intensities are integers below 2^24, as in BraTS files, so
the float32 copy the device works on equals the reference's float64 exactly.  Voxel sizes are exact in float32 and so is
their product.

The tool prints the branch table and refuses to write a fixture in which a score lies within 1e-6 of a classification
threshold: such a case would pin rounding, not behaviour.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "morphology.json")
SECTIONS = ("shape_descriptors", "border_regularity", "margin_definition", "necrosis_pattern", "cystic_solid_classification")
CLEARANCE = 1e-6

S = (48, 56, 40)
C = (24, 28, 20)
CASES = [
    dict(name="none", shape=S, parts=[]),
    dict(name="ball", shape=S, parts=[["ball", 2, C, 13], ["ball", 3, C, 9], ["ball", 1, C, 4]], gain=0.15),
    dict(name="rod", shape=S, parts=[["box", 2, (22, 26, 0), (25, 29, 40)]], gain=0.6),
    dict(name="sheet", shape=S, parts=[["box", 2, (8, 10, 20), (40, 46, 21)]], gain=0.3),
    dict(name="slab", shape=S, parts=[["box", 3, (8, 10, 20), (40, 46, 22)], ["box", 1, (10, 12, 20), (38, 44, 22)]], cystic=1.0),
    dict(name="noise50", shape=S, parts=[["noise", 2, (10, 12, 8), (38, 44, 32), 0.5]]),
    dict(name="noise20", shape=S, parts=[["noise", 2, (10, 12, 8), (38, 44, 32), 0.2]]),
    dict(name="noise08", shape=S, parts=[["noise", 2, (10, 12, 8), (38, 44, 32), 0.08]]),
    dict(name="tiny", shape=S, parts=[["box", 3, (24, 28, 18), (25, 29, 22)]]),
    dict(name="eccentric", shape=S, parts=[["ball", 2, C, 14], ["ball", 3, C, 11], ["ball", 1, (24, 32, 20), 6]], gain=0.06, cystic=1.0),
    dict(name="peripheral", shape=S, parts=[["ball", 3, C, 12], ["ball", 1, (24, 35, 24), 4]], gain=0.05),
    dict(name="moderate", shape=S, parts=[["ball", 2, C, 12], ["ball", 4, C, 10], ["ball", 1, C, 8]], gain=0.3, cystic=0.9),
    dict(name="extensive", shape=S, parts=[["ball", 3, C, 12], ["ball", 1, C, 10]], gain=0.3, cystic=0.0),
    dict(name="corner", shape=S, parts=[["ball", 2, (2, 3, 2), 10], ["ball", 1, (2, 3, 2), 4]], gain=0.3, brain=False),
    dict(name="aniso", shape=S, parts=[["ball", 2, C, 12], ["ball", 3, (24, 30, 20), 7], ["ball", 1, (24, 30, 20), 3]], gain=0.2,
         voxel_dims=(0.9375, 0.9375, 1.875)),
    dict(name="full_size", shape=(240, 240, 155), parts=[["ball", 2, (120, 130, 80), 22], ["ball", 3, (118, 126, 80), 13], ["ball", 1, (116, 124, 79), 7]],
         gain=0.25, cystic=0.5, sigma=6.0),
]
SEED = 11


def case_args(case):
    return {"seed": case.get("seed", SEED), "shape": list(case["shape"]), "parts": [[list(v) if isinstance(v, tuple) else v for v in p] for p in case["parts"]],
            "gain": float(case.get("gain", 0.0)), "cystic": float(case.get("cystic", 0.0)), "sigma": float(case.get("sigma", 3.0)),
            "brain": bool(case.get("brain", True))}


def case_data(args):
    """(label map, [4, ...] volumes) of a fixture case from its stored arguments"""
    from brats_amd import synthetic
    seg = synthetic.shapes_map(args["seed"], tuple(args["shape"]), args["parts"])
    vols = synthetic.mri_for_label_map(args["seed"] + 1, seg, gain=args["gain"], cystic=args["cystic"], sigma=args["sigma"], brain=args["brain"])
    return seg, vols


def load_step4():
    from oracle import gen_golden, ref_shim
    ref = os.path.join(ref_shim.REFERENCE_ROOT, "feature_extraction")
    utils = gen_golden._import_by_path("utils", os.path.join(ref, "utils.py"), {"nibabel": {}})
    saved = sys.modules.get("utils")
    sys.modules["utils"] = utils
    try:
        return utils, gen_golden._import_by_path("_reference_step4_morphology", os.path.join(ref, "step4_morphology.py"))
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
    """(name, value, thresholds) of every score of a case that a classification of step 4 branches on"""
    out = []
    sd, br, md, nc, cy = (expected[k] for k in SECTIONS)
    if "shape_classification" in sd:
        out.append(("sphericity", sd["sphericity"], (0.8, 0.6, 0.4)))
        out.append(("elongation", sd["elongation"], (2.5, 1.5)))
    if "surface_voxel_count" in br:
        out.append(("regularity", br["regularity_score"], (0.7, 0.5, 0.3)))
    if "contrast_ratio" in md:
        out.append(("sharpness", md["margin_sharpness"], (0.6, 0.4, 0.2)))
    if nc["necrosis_present"]:
        out.append(("necrosis_pct", nc["necrosis_percentage"], (50, 25, 10)))
    if "cystic_volume_cm3" in cy:
        out.append(("cystic_pct", cy["cystic_percentage"], (70, 40, 15)))
    return out


def branch_table(cases):
    rows = []
    for c in cases:
        e = c["expected"]
        rows.append((c["name"], e["shape_descriptors"].get("shape_classification", "-"), e["shape_descriptors"].get("elongation_classification", "-"),
                     e["border_regularity"]["classification"], e["margin_definition"]["classification"], e["necrosis_pattern"]["pattern"],
                     e["necrosis_pattern"].get("location", "-"), e["cystic_solid_classification"]["classification"]))
    return rows


def generate():
    utils, s4 = load_step4()
    cases = []
    for case in CASES:
        args = case_args(case)
        seg, vols = case_data(args)
        assert vols.max() < 2 ** 24 and np.array_equal(vols, np.rint(vols))
        dims = tuple(float(v) for v in case.get("voxel_dims", (1.0, 1.0, 1.0)))
        seg_i = np.round(seg).astype(np.int32)  # step4_morphology.py:620
        t1, t1ce, t2, flair = (v.astype(np.float64) for v in vols)  # what nibabel's get_fdata hands the reference
        masks = utils.get_tumor_masks(seg_i)
        expected = {"shape_descriptors": s4.calculate_shape_descriptors(seg_i, masks, dims),
                    "border_regularity": s4.analyze_border_regularity(masks["wt"], dims),
                    "margin_definition": s4.analyze_margin_definition(t1ce, seg_i, masks, dims),
                    "necrosis_pattern": s4.analyze_necrosis_pattern(seg_i, masks, dims),
                    "cystic_solid_classification": s4.analyze_cystic_vs_solid(t1, t2, flair, seg_i, masks, dims)}
        cases.append({"name": case["name"], "args": args, "voxel_dims": list(dims),
                      "sha256": {"seg": hashlib.sha256(seg.tobytes()).hexdigest(), "vols": hashlib.sha256(vols.tobytes()).hexdigest()},
                      "expected": expected})
    out = {"generator": "tools/gen_morphology_golden.py (reference functions imported from feature_extraction/step4_morphology.py)", "cases": cases}
    return json.loads(json.dumps(out, default=_plain))


def too_close(data):
    bad = []
    for c in data["cases"]:
        for name, value, thresholds in scores(c["expected"]):
            for t in thresholds:
                if abs(value - t) <= CLEARANCE:
                    bad.append(f"{c['name']}: {name} = {value!r} within {CLEARANCE} of {t}")
    return bad


if __name__ == "__main__":
    data = generate()
    for row in branch_table(data["cases"]):
        print(" | ".join(row))
    for c in data["cases"]:
        print(c["name"], " ".join(f"{n}={v:.6g}" for n, v, _ in scores(c["expected"])))
    bad = too_close(data)
    if bad:
        sys.exit("not written:\n" + "\n".join(bad))
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(data, f, indent=1, ensure_ascii=False)
    print(os.path.getsize(OUT), "bytes")
