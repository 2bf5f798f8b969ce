#!/usr/bin/env python3
"""Time of the six feature-extraction steps of one case, run one by one and through ``brats_amd.features``, on the 240 x 240 x 155
`full_size` case of tests/golden/normal_structures.json.

    python tools/features_time.py [--part files|resident|all] [--runs 3] [--repeats 15] [--out profiles/features_time.json] [--profile]

(a) ``files``: wall time at the file boundary, in one warm process.  The case is written as five .nii.gz files (int16 volumes, uint8
    labels); ``six_analyze`` runs the six ``analyze`` functions of the step commands in sequence, each loading its own files,
    ``run_all_steps`` the one command of ``brats_amd.features``.  One untimed round first, then --runs timed rounds, the two
    interleaved; step 2 under ``distance='exact'`` on both sides, so that no generator is involved.
(b) ``resident``: on resident tensors, between stream events, median of --repeats after a warm round: ``six_plain``, the six resident
    functions in sequence, and ``extract_all``.

A tree without ``brats_amd.features`` (the parent commit, for an interleaved comparison from a shell loop) reports ``six_analyze`` and
``six_plain`` only.  --profile: one warm and one measured round of each resident variant and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/features_time.py --profile` (launch counts per kernel; no counters in that run).
"""
import argparse
import importlib
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

STEP_MODULES = ("sequence_findings", "mass_effect", "multiplicity", "morphology", "quality", "normal_structures")


def mod(name):
    return importlib.import_module("brats_amd." + name)


def have_features():
    try:
        mod("features")
        return True
    except ImportError:
        return False


def write_case(folder, seg, vols):
    nifti = mod("nifti")
    case_dir = Path(folder) / "BraTS2021_00042"
    case_dir.mkdir()
    for v, suffix in zip(vols, ("_t1", "_t1ce", "_t2", "_flair")):
        nifti.save_like(case_dir / f"BraTS2021_00042{suffix}.nii.gz", v.astype(np.int16), nifti.make_header(seg.shape, dtype=np.int16))
    nifti.save_like(Path(folder) / "seg.nii.gz", seg, nifti.make_header(seg.shape, dtype=np.uint8))
    return case_dir, Path(folder) / "seg.nii.gz"


def six_analyze(case_dir, seg_path, out_dir):
    out = {}
    for name in STEP_MODULES:   # each writes its JSON, as its command does
        out[name] = mod(name).analyze(case_dir, seg_path, Path(out_dir) / f"{name}.json", **({"distance": "exact"} if name == "mass_effect" else {}))
    return out


def six_plain(seg, chans, zooms, ctx=None):
    kw = {} if ctx is None else {"ctx": ctx}
    z = [float(v) for v in zooms]
    return (mod("sequence_findings").sequence_findings(seg, *chans, z, **kw),
            mod("mass_effect").mass_effect(seg, chans[0], [np.float32(v) for v in zooms], None, "exact", **kw),
            mod("components").lesion_multiplicity(seg, z, **kw),
            mod("morphology").tumor_morphology(seg, *chans, z, **kw),
            mod("quality").quality_control(seg, *chans, z, **kw),
            mod("normal_structures").normal_structures(seg, *chans, z, **kw))


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 2)


def event_ms(fn, repeats):
    import torch
    fn()
    times = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(float(np.min(times)), 3), "max_ms": round(float(np.max(times)), 3),
            "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("files", "resident", "all"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    import brats_amd  # noqa: F401
    import gen_normal_structures_golden as gen
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    assert torch.cuda.is_available(), "needs the GPU"
    with open(ROOT / "tests" / "golden" / "normal_structures.json") as f:
        case = [c for c in json.load(f)["cases"] if c["name"] == "full_size"][0]
    seg, vols = gen.case_data(case["args"])
    vols = [np.ascontiguousarray(v.astype(np.int16).astype(np.float32)) for v in vols]   # what the files hold
    features = have_features()
    result = {"tool": "tools/features_time.py", "shape": list(seg.shape), "device": torch.cuda.get_device_name(0), "has_features": features}
    dseg = torch.from_numpy(np.ascontiguousarray(seg)).cuda()
    chans = [torch.from_numpy(v).cuda() for v in vols]
    zooms = case["voxel_dims"]

    if args.profile:
        six_plain(dseg, chans, zooms)
        six_plain(dseg, chans, zooms)
        if features:
            mod("features").extract_all(dseg, *chans, zooms, distance="exact")
            mod("features").extract_all(dseg, *chans, zooms, distance="exact")
        torch.cuda.synchronize()
        print(json.dumps({"profile_rounds": {"six_plain": 2, "extract_all": 2 if features else 0}}))
        return 0

    if args.part in ("resident", "all"):
        plain = six_plain(dseg, chans, zooms)
        rows = {"six_plain": event_ms(lambda: six_plain(dseg, chans, zooms), args.repeats)}
        if features:
            f = mod("features")
            both = f.extract_all(dseg, *chans, zooms, distance="exact")
            assert [json.dumps(both[k]) for k in f.STEP_KEYS] == [json.dumps(p) for p in plain], "extract_all differs from the six plain calls"
            rows["extract_all"] = event_ms(lambda: f.extract_all(dseg, *chans, zooms, distance="exact"), args.repeats)
            rows["six_plain_again"] = event_ms(lambda: six_plain(dseg, chans, zooms), args.repeats)
            ctx = f.CaseContext(dseg, *chans)
            ctx.positive_percentiles(0, 5)
            ctx.brain_percentiles(0, 15)
            result["select_launches"] = dict(ctx.select_launches)
        result["resident"] = rows

    if args.part in ("files", "all"):
        with tempfile.TemporaryDirectory() as tmp:
            case_dir, seg_path = write_case(tmp, seg, vols)
            out = Path(tmp) / "out"
            runs = {"six_analyze": []}
            six_analyze(case_dir, seg_path, Path(tmp) / "alone")
            if features:
                runs["run_all_steps"] = []
                mod("features").run_all_steps(case_dir, seg_path, out, distance="exact")
            for _ in range(args.runs):
                runs["six_analyze"].append(wall_ms(lambda: six_analyze(case_dir, seg_path, Path(tmp) / "alone")))
                if features:
                    runs["run_all_steps"].append(wall_ms(lambda: mod("features").run_all_steps(case_dir, seg_path, out, distance="exact")))
            result["files_ms"] = runs
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
