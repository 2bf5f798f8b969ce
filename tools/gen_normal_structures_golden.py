"""Writes tests/golden/normal_structures.json from the REFERENCE's own step 6 (development machine only: needs the reference tree).

    python tools/gen_normal_structures_golden.py [--small-only]

``feature_extraction/step6_normal_structures.py`` is imported unmodified from where it lies (its ``utils`` with an inert stand-in
for the absent nibabel package, as tools/gen_quality_golden.py does) and ``analyze_ventricular_system``, ``analyze_parenchyma`` and
``analyze_major_vessels`` run over label maps drawn by ``brats_amd.synthetic.shapes_map`` and volumes drawn by
``brats_amd.synthetic.mri_for_normal_structures``.  Per case the fixture holds the generator arguments, the voxel sizes, a sha256 of
the label map and of the four volumes (all are regenerated from the seeds, not stored) and the three dicts the reference
returned - or, where it raised, ``"raises"`` with the name of the exception in place of ``"expected"``.  Intensities are integers
below 2^15, as in BraTS files, so every sum is exact in float64 and every float of step 6 can be compared exactly.

The tool prints the branch table and refuses to write a fixture that misses one of the REQUIRED branches, or in which a
branching quantity lies within 1e-6 of its threshold: such a case would pin rounding, not behaviour.  ``--small-only`` leaves the
240 x 240 x 155 case out and writes nothing (for tuning the small cases).

Flow voids 'Prominent' has a narrow way in.  The reference counts the inferior-brain voxels strictly below their own 5th
percentile, so the fraction it tests is at most (floor(0.05 (n - 1)) + 1) / n: it passes 0.05 by less than 1 / n, and only while the
values around that rank are all different (the ``"ramp"`` case: 0.05 + 5.5e-5 here, clear of the threshold by more than the
rule asks).  The other way in, a fraction of 0.001 to the last bit, lies on a threshold and is what the clearance rule refuses.
No branch of step 6 is unreachable under the rule.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "normal_structures.json")
SECTIONS = ("ventricular_system", "parenchyma", "major_vessels")
CLEARANCE = 1e-6

S = (48, 56, 40)
SMALL_TUMOUR = [["ball", 2, (10, 28, 28), 5], ["ball", 3, (10, 28, 28), 3]]
CENTRAL = ["obox", (18, 20, 16), (30, 36, 24)]                                        # 1408 voxels, six rows on either side of d0 // 2
EDGE_PAIR = [["obox", (16, 18, 15), (24, 29, 24)], ["obox", (24, 27, 15), (32, 38, 24)]]    # 696 + 696 voxels, joined across an edge only
CORNER_PAIR = [["obox", (14, 14, 8), (22, 25, 17)], ["obox", (22, 23, 15), (30, 34, 24)]]   # 696 + 696 voxels, joined across a corner only
COVER_DEEP = [["box", 2, (5, 6, 5), (43, 50, 35)]]                                    # a tumour over everything deeper than the 60th percentile
CASES = [
    dict(name="mild_symmetric", parts=SMALL_TUMOUR, ventricles=[CENTRAL], contrast=0.5, voids="step"),
    dict(name="moderate_left_adjacent", parts=[["ball", 2, (8, 28, 20), 6]], ventricles=[["obox", (14, 16, 15), (26, 40, 24)]], contrast=0.38, pv_gain=0.2,
         voids="tie", voxel_dims=(1.0, 1.0, 1.5)),
    dict(name="marked_right_communicating", parts=SMALL_TUMOUR, ventricles=[["obox", (20, 16, 14), (38, 40, 25)]], contrast=-0.1, pv_gain=0.6, voids="ramp",
         enhancement=1.8),
    dict(name="ventriculomegaly_narrow", parts=SMALL_TUMOUR, ventricles=[["obox", (18, 12, 14), (30, 44, 26)]], contrast=0.5, voxel_dims=(0.9, 0.9, 1.2)),
    dict(name="edge_joined_pair", parts=SMALL_TUMOUR, ventricles=EDGE_PAIR, contrast=0.5, voids="step"),
    dict(name="corner_joined_pair", parts=SMALL_TUMOUR, ventricles=[["obox", (18, 20, 26), (30, 36, 34)]] + CORNER_PAIR, contrast=0.5),
    dict(name="off_centre_component", parts=SMALL_TUMOUR, ventricles=[CENTRAL, ["box", (4, 17, 13), (12, 39, 27)]], contrast=0.5),
    dict(name="tumour_covers_brain", parts=[["box", 2, (0, 0, 0), S]], ventricles=[CENTRAL]),
    dict(name="no_tumour", parts=[], ventricles=[CENTRAL], contrast=0.5),
    dict(name="no_ventricle_deep_tumour", parts=COVER_DEEP, ventricles=[], cuts=[[(0, 0, 0), (48, 56, 13)]]),
    dict(name="unbound_cortical_mask", parts=SMALL_TUMOUR, ventricles=[]),
    dict(name="empty_brain", parts=SMALL_TUMOUR, ventricles=[CENTRAL], zero=True),
    dict(name="full_size", shape=(240, 240, 155), parts=[["ball", 2, (70, 130, 90), 22], ["ball", 3, (68, 126, 90), 13], ["ball", 1, (66, 124, 89), 7]],
         ventricles=[["obox", (95, 90, 62), (118, 150, 92)], ["obox", (122, 90, 62), (150, 150, 92)]], contrast=0.5, pv_gain=0.2, voids="step",
         enhancement=1.8, sigma=6.0),
]
SEED = 61
REQUIRED = (
    "size/Normal", "size/Mildly prominent", "size/Moderately dilated", "size/Markedly dilated",
    "hydrocephalus/Communicating hydrocephalus suggested", "hydrocephalus/Ventriculomegaly noted", "hydrocephalus/No hydrocephalus",
    "obstruction/adjacent", "obstruction/none", "symmetry/symmetric", "symmetry/left", "symmetry/right",
    "components/off_centre_rejected", "components/edge_only_kept", "components/corner_only_rejected",
    "parenchyma/unable", "wm/chronic", "wm/mild", "wm/none", "wm/could_not", "gw/Preserved", "gw/Mildly reduced", "gw/Reduced", "gw/Could not assess",
    "flow/Present", "flow/Not well visualized", "flow/Prominent", "flow/Could not assess", "vascular/Possible", "vascular/Not evident", "vascular/Could not assess",
    "vascular/no_tumour", "raises/UnboundLocalError", "raises/empty_brain")


def _lists(v):
    return [_lists(x) for x in v] if isinstance(v, (list, tuple)) else v


def case_args(case):
    return {"seed": case.get("seed", SEED), "shape": list(case.get("shape", S)), "parts": _lists(case["parts"]), "ventricles": _lists(case["ventricles"]),
            "brain_axes": float(case.get("brain_axes", 0.47)), "outside": float(case.get("outside", 60.0)), "contrast": float(case.get("contrast", 0.0)),
            "pv_gain": float(case.get("pv_gain", 0.0)), "voids": case.get("voids"), "enhancement": float(case.get("enhancement", 1.0)),
            "cuts": _lists(case.get("cuts", [])), "zero": bool(case.get("zero", False)), "sigma": float(case.get("sigma", 3.0))}


def case_data(args):
    """(label map, [4, ...] volumes) of a fixture case from its stored arguments"""
    from brats_amd import synthetic
    seg = synthetic.shapes_map(args["seed"], tuple(args["shape"]), args["parts"])
    vols = synthetic.mri_for_normal_structures(args["seed"] + 1, seg, ventricles=args["ventricles"], brain_axes=args["brain_axes"], outside=args["outside"],
                                               contrast=args["contrast"], pv_gain=args["pv_gain"], voids=args["voids"], enhancement=args["enhancement"],
                                               cuts=args["cuts"], zero=args["zero"], sigma=args["sigma"])
    return seg, vols


def load_step6():
    from oracle import gen_golden, ref_shim
    ref = os.path.join(ref_shim.REFERENCE_ROOT, "feature_extraction")
    utils = gen_golden._import_by_path("utils", os.path.join(ref, "utils.py"), {"nibabel": {}})
    saved = sys.modules.get("utils")
    sys.modules["utils"] = utils
    try:
        return utils, gen_golden._import_by_path("_reference_step6_normal_structures", os.path.join(ref, "step6_normal_structures.py"))
    finally:
        if saved is None:
            sys.modules.pop("utils", None)
        else:
            sys.modules["utils"] = saved


def _plain(o):
    if isinstance(o, np.generic):
        return o.item()
    raise TypeError(type(o))


def quantities(s6, seg, vols, dims):
    """What step 6 branches on, recomputed from the data without rounding: ``scores`` (name, value, thresholds) and ``facts``, the
    branches that do not show in the returned dicts.  Nothing when the brain mask is empty."""
    from scipy import ndimage
    scores, facts = [], set()
    t1, t1ce, t2, flair = (v.astype(np.float64) for v in vols)
    d0, d1, d2 = seg.shape
    brain = t1 > np.percentile(t1[t1 > 0], 5) if t1.max() > 0 else t1 > 0
    if not brain.any():
        return scores, facts
    tumour = seg > 0
    normal = brain & ~tumour
    vent, csf = s6.identify_ventricles(t1, t2, flair, brain, tumour)
    kept = {}
    for conn in (1, 2, 3):  # what the keep rule would make of the CSF mask with 6, 18 and 26 neighbours
        labeled, n = ndimage.label(csf, structure=ndimage.generate_binary_structure(3, conn))
        rows = [(int((labeled == i).sum()), float(np.mean(np.where(labeled == i)[0]))) for i in range(1, n + 1)]
        kept[conn] = sum(c for c, x in rows if c > 1000 and abs(x - d0 / 2) < d0 * 0.3)
        if conn == 2:
            for c, x in rows:
                scores.append(("component_voxels", float(c), (1000.0,)))
                if c > 1000:
                    scores.append(("component_offset", abs(x - d0 / 2), (d0 * 0.3,)))
                    if not abs(x - d0 / 2) < d0 * 0.3:
                        facts.add("components/off_centre_rejected")
    assert kept[2] == int(vent.sum())
    if kept[2] > kept[1]:
        facts.add("components/edge_only_kept")
    if kept[3] > kept[2]:
        facts.add("components/corner_only_rejected")
    if normal.any():
        vbr = vent.sum() / normal.sum() * 100
        scores.append(("vbr", vbr, (2.0, 4.0, 5.0, 6.0, 7.0)))
    if vent.any():
        left, right = vent[:d0 // 2].sum(), vent[d0 // 2:].sum()
        scores.append(("asymmetry", abs(int(left) - int(right)) / (left + right), (0.15,)))
        facts.add("symmetry/" + ("left" if left > right else "right" if right > left else "symmetric"))
        frontal_y = np.percentile(np.where(vent)[1], 75)
        scores.append(("evans", np.max(np.sum(vent[:, int(frontal_y):, :], axis=0)) / d0, (0.3,)))
        scores.append(("obstruction", (vent & ndimage.binary_dilation(tumour, iterations=5)).sum() / vent.sum(), (0.1,)))
    if normal.any():
        dist = ndimage.distance_transform_edt(brain)
        deep = normal & (dist > np.percentile(dist[brain], 60))
        cortical = normal & (dist < np.percentile(dist[brain], 40))
        pv = ndimage.binary_dilation(vent, iterations=10) & normal & ~vent
        scores.append(("deep_voxels", float(deep.sum()), (100.0,)))
        if pv.any():
            scores.append(("cortical_voxels", float(cortical.sum()), (100.0,)))
            if cortical.any():
                scores.append(("pv_ratio", flair[pv].mean() / flair[cortical].mean(), (1.15, 1.3)))
            if deep.sum() > 100 and cortical.sum() > 100:
                scores.append(("gw_ratio", t1[deep].mean() / t1[cortical].mean(), (1.0, 1.1)))
    inferior = brain.copy()
    inferior[:, :, d2 // 3:] = False
    if inferior.any():
        fraction = (inferior & (t1 < np.percentile(t1[inferior], 5)) & ~tumour).sum() / inferior.sum()
        scores.append(("flow_void_fraction", fraction, (0.001, 0.05)))
    peri = ndimage.binary_dilation(tumour, iterations=10) & ~tumour & brain
    if peri.any():
        scores.append(("enhancement_ratio", t1ce[peri].mean() / t1[peri].mean(), (1.5,)))
    if not tumour.any():
        facts.add("vascular/no_tumour")
    return scores, facts


def branches(result, facts):
    """the names of REQUIRED (and the optional flow/Prominent) a case hits"""
    hit = set(facts)
    if "raises" in result:
        hit.add("raises/" + ("UnboundLocalError" if result["raises"] == "UnboundLocalError" else "empty_brain"))
        return hit
    vent, par, ves = (result["expected"][k] for k in SECTIONS)
    hit.add("size/" + vent["size_assessment"])
    hit.add("hydrocephalus/" + vent["hydrocephalus_type"])
    hit.add("obstruction/adjacent" if vent["obstruction_risk"] > 0.1 else "obstruction/none")
    if "assessment" in par:
        hit.add("parenchyma/unable")
    else:
        text = par["periventricular_assessment"]["description"]
        hit.add("wm/" + ("chronic" if text.startswith("FLAIR hyperintensities") else "mild" if text.startswith("Mild") else
                         "none" if text.startswith("No significant") else "could_not"))
        hit.add("gw/" + par["gray_white_differentiation"]["assessment"])
    hit.add("flow/" + ves["flow_voids"]["assessment"])
    hit.add("vascular/" + ves["vascular_involvement"]["assessment"])
    return hit


def too_close(name, scores):
    bad = []
    for what, value, thresholds in scores:
        for t in thresholds:
            if abs(value - t) <= CLEARANCE * max(1.0, abs(t)):
                bad.append(f"{name}: {what} = {value!r} within {CLEARANCE} of {t}")
    return bad


def generate(small_only=False, verbose=False):
    """(fixture, branches hit per case, complaints)"""
    utils, s6 = load_step6()
    cases, hits, bad = [], {}, []
    for case in CASES:
        if small_only and "shape" in case:
            continue
        args = case_args(case)
        seg, vols = case_data(args)
        assert vols.max() < 2 ** 15 and vols.min() >= 0 and np.array_equal(vols, np.rint(vols))
        dims = [float(v) for v in case.get("voxel_dims", (1.0, 1.0, 1.0))]
        seg_i = np.round(seg).astype(np.int32)  # step6_normal_structures.py:444
        t1, t1ce, t2, flair = (v.astype(np.float64) for v in vols)  # what nibabel's get_fdata hands the reference
        tumour = utils.get_tumor_masks(seg_i)["wt"]
        brain = utils.get_brain_mask(t1)
        try:
            with np.errstate(all="ignore"):
                expected = {"ventricular_system": s6.analyze_ventricular_system(t1, t2, flair, brain, tumour, dims),
                            "parenchyma": s6.analyze_parenchyma(t1, t2, flair, brain, tumour, dims),
                            "major_vessels": s6.analyze_major_vessels(t1, t1ce, brain, tumour, dims)}
            result = {"expected": json.loads(json.dumps(expected, default=_plain))}
        except (UnboundLocalError, IndexError, ValueError) as e:
            result = {"raises": type(e).__name__}
        scores, facts = quantities(s6, seg, vols, dims)
        hits[case["name"]] = branches(result, facts)
        bad += too_close(case["name"], scores)
        if verbose:
            print(case["name"], " ".join(f"{n}={v:.6g}" for n, v, _ in scores), result.get("raises", ""))
        cases.append({"name": case["name"], "args": args, "voxel_dims": dims,
                      "sha256": {"seg": hashlib.sha256(seg.tobytes()).hexdigest(), "vols": hashlib.sha256(vols.tobytes()).hexdigest()}, **result})
    out = {"generator": "tools/gen_normal_structures_golden.py (reference functions imported from feature_extraction/step6_normal_structures.py)",
           "cases": cases}
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
