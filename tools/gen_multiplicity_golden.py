"""Writes tests/golden/multiplicity.json from the REFERENCE's own step 3 (development machine only: needs the reference tree).

    python tools/gen_multiplicity_golden.py

``feature_extraction/step3_multiplicity.py`` is imported unmodified from where it lies (its ``utils`` with an inert stand-in
for the absent nibabel package, which the functions used here never touch) and its functions run over label maps drawn by
``brats_amd.synthetic.label_map``.  Per case the fixture holds the generator arguments, the voxel sizes, a sha256 of the label
map (the maps are regenerated from the seed, not stored) and the dicts the reference returned, minus its report prose
(clinical_implication, differential_considerations, enhancement_note), which is out of scope.  Voxel sizes are exact in
float32 and so is their product, as header zooms are float32.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "multiplicity.json")
PROSE = ("clinical_implication", "differential_considerations", "enhancement_note")

S = (96, 112, 80)
CASES = [
    dict(name="none", shape=S, lesions=[], fragments=0),
    dict(name="single", shape=S, lesions=[((40, 50, 40), 12)], fragments=0),
    dict(name="regional", shape=S, lesions=[((30, 40, 40), 10), ((30, 70, 40), 6)], fragments=0),
    dict(name="distant", shape=S, lesions=[((20, 20, 20), 10), ((75, 90, 60), 7)], fragments=0),
    dict(name="diffuse", shape=S, lesions=[((20, 20, 20), 8), ((75, 90, 60), 7), ((20, 90, 20), 6), ((75, 20, 60), 5)], fragments=0),
    dict(name="satellite", shape=S, lesions=[((40, 50, 40), 10), ((40, 66, 40), 4)], fragments=40),
    dict(name="tie", shape=S, lesions=[((60, 80, 50), 6), ((25, 30, 30), 6)], fragments=0, enhancing=False),
    dict(name="aniso", shape=S, lesions=[((40, 50, 40), 12), ((70, 90, 60), 5)], fragments=25, voxel_dims=(0.9375, 0.9375, 1.25)),
    dict(name="full_size", shape=(240, 240, 155), lesions=[((120, 130, 80), 16), ((60, 70, 40), 9), ((180, 170, 110), 7)], fragments=60),
]
SEED = 7


def case_label_map(case):
    from brats_amd import synthetic
    return synthetic.label_map(case.get("seed", SEED), case["shape"], case["lesions"], case["fragments"], enhancing=case.get("enhancing", True))


def load_step3():
    from oracle import gen_golden, ref_shim
    ref = os.path.join(ref_shim.REFERENCE_ROOT, "feature_extraction")
    utils = gen_golden._import_by_path("utils", os.path.join(ref, "utils.py"), {"nibabel": {}})
    saved = sys.modules.get("utils")
    sys.modules["utils"] = utils
    try:
        return gen_golden._import_by_path("_reference_step3_multiplicity", os.path.join(ref, "step3_multiplicity.py"))
    finally:
        if saved is None:
            sys.modules.pop("utils", None)
        else:
            sys.modules["utils"] = saved


def _plain(o):
    if isinstance(o, np.generic):
        return o.item()
    raise TypeError(type(o))


def generate():
    s3 = load_step3()
    cases = []
    for case in CASES:
        seg = case_label_map(case)
        dims = tuple(float(v) for v in case.get("voxel_dims", (1.0, 1.0, 1.0)))
        seg_i = seg.astype(np.int32)  # step3_multiplicity.py:460
        ca = s3.detect_connected_components(seg_i, dims)
        da = s3.calculate_inter_lesion_distances(ca["components"], dims)
        if ca["components"]:
            sa = s3.detect_satellite_lesions(ca["components"], ca["components"][0], dims)
        else:  # what analyze_multiplicity puts there when nothing was found (:500-505)
            sa = {"satellite_count": 0, "satellites": [], "has_satellites": False, "description": ca["description"]}
        ea = s3.analyze_enhancing_components(seg_i, dims)
        dp = {k: v for k, v in s3.classify_distribution_pattern(ca, da, sa, ea).items() if k not in PROSE}
        cases.append({"name": case["name"],
                      "args": {"seed": case.get("seed", SEED), "shape": list(case["shape"]), "lesions": [[list(c), r] for c, r in case["lesions"]],
                               "fragments": case["fragments"], "enhancing": case.get("enhancing", True)},
                      "voxel_dims": list(dims), "sha256": hashlib.sha256(seg.tobytes()).hexdigest(),
                      "expected": {"component_analysis": ca, "distance_analysis": da, "satellite_analysis": sa, "enhancing_analysis": ea,
                                   "distribution_pattern": dp}})
    out = {"generator": "tools/gen_multiplicity_golden.py (reference functions imported from feature_extraction/step3_multiplicity.py)",
           "cases": cases}
    return json.loads(json.dumps(out, default=_plain))


if __name__ == "__main__":
    data = generate()
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(data, f, indent=1, ensure_ascii=False)
    for c in data["cases"]:
        e = c["expected"]
        print(c["name"], e["component_analysis"]["description"], "| max", e["distance_analysis"]["max_distance_mm"], "| sat",
              e["satellite_analysis"]["satellite_count"], "| foci", e["enhancing_analysis"]["num_enhancing_foci"], "|", e["distribution_pattern"]["pattern"])
    print(os.path.getsize(OUT), "bytes")
