#!/usr/bin/env python3
"""Time of the morphology primitives and of the whole of ``tumor_morphology`` on the device against the reference-equivalent
scipy + numpy sequence on the same node's host, for the `full_size` (240 x 240 x 155) case of tests/golden/morphology.json.

    python tools/morphology_time.py [--out profiles/morphology_time.json] [--repeats 30] [--profile]

Device times: HIP events around warm calls (one warm-up call first, then the median and the minimum of --repeats timed
calls); the entry points that return numbers to the host synchronise themselves, which the events include.  The end-to-end
figure is also taken WITH the upload of the label map and the four volumes.  Host times: the calls step 4 makes - binary
erosion and dilations, two distance transforms, three whole-volume gradients, np.where + np.cov, the boolean-mask statistics
and the three percentiles (which the device path takes with masked_percentiles) - threads capped at 16 as tests/conftest.py does.  --profile: a short device-only run, for
`rocprofv3 --kernel-trace --stats -- python tools/morphology_time.py --profile`.
"""
import argparse
import json
import os
import platform
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def device_ms(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(float(np.min(times)), 4), "repeats": repeats}


def host_sequence(seg, vols, dims):
    """what step4_morphology.py computes for one case, call for call, without its dict building"""
    from scipy.ndimage import binary_dilation, binary_erosion, distance_transform_edt
    t = {}

    def lap(name, t0):
        t[name] = round((time.perf_counter() - t0) * 1e3, 2)

    t1, t1ce, t2, flair = (v.astype(np.float64) for v in vols)
    wt, ncr = seg > 0, seg == 1
    t0 = time.perf_counter()
    eroded = binary_erosion(wt)
    surface = wt & ~eroded
    dil5, dil1 = binary_dilation(wt, iterations=5), binary_dilation(wt)
    lap("erosion_and_dilations", t0)
    t0 = time.perf_counter()
    signed = distance_transform_edt(wt) - distance_transform_edt(~wt)
    lap("two_distance_transforms", t0)
    t0 = time.perf_counter()
    grad = np.sqrt(sum(np.gradient(signed, axis=k) ** 2 for k in range(3)))[surface]
    cv = grad.std() / grad.mean()
    lap("three_gradients", t0)
    t0 = time.perf_counter()
    coords = np.where(wt)
    points = np.array([coords[k] * dims[k] for k in range(3)]).T
    eig = np.linalg.eigvalsh(np.cov((points - points.mean(axis=0)).T))
    lap("where_and_cov", t0)
    t0 = time.perf_counter()
    stats = [t1ce[m].mean() for m in (wt, dil5 & ~wt)] + [f(t1ce[m]) for m in (surface, dil1 & ~wt) for f in (np.mean, np.std)]
    stats += [t2[ncr].std(), t2[ncr].mean(), flair[ncr].mean()]
    lap("masked_statistics", t0)
    t0 = time.perf_counter()
    pct = [np.percentile(t1[t1 > 0], 10), np.percentile(t2[t2 > 0], 85), np.percentile(flair[flair > 0], 20)]
    lap("three_percentiles", t0)
    t["total"] = round(sum(t.values()), 2)
    return t, (cv, eig, stats, pct)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    import brats_amd  # noqa: F401
    from brats_amd import components, morphology as mo
    import gen_morphology_golden as gen
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    assert torch.cuda.is_available(), "needs the GPU"
    with open(ROOT / "tests" / "golden" / "morphology.json") as f:
        case = [c for c in json.load(f)["cases"] if c["name"] == "full_size"][0]
    seg, vols = gen.case_data(case["args"])
    dims = case["voxel_dims"]
    repeats = 2 if args.profile else args.repeats
    dseg = torch.from_numpy(seg).cuda()
    dvols = torch.from_numpy(vols).cuda()
    inv = components._indicator(dseg, (0,))
    flags = mo.region_flags(dseg, dvols[mo.T1], dvols[mo.T2], dvols[mo.FLAIR])
    d2_in, d2_out = mo.distance_transform_edt_sq(dseg), mo.distance_transform_edt_sq(inv)
    rows = {
        "binary_erosion_1": device_ms(lambda: mo.binary_erosion(dseg), repeats),
        "binary_dilation_1": device_ms(lambda: mo.binary_dilation(dseg), repeats),
        "binary_dilation_5": device_ms(lambda: mo.binary_dilation(dseg, 5), repeats),
        "binary_dilation_10": device_ms(lambda: mo.binary_dilation(dseg, 10), repeats),
        "edt_squared_inside": device_ms(lambda: mo.distance_transform_edt_sq(dseg), repeats),
        "edt_squared_outside": device_ms(lambda: mo.distance_transform_edt_sq(inv), repeats),
        "surface_gradient_stats": device_ms(lambda: mo.surface_gradient_stats(d2_in, d2_out, flags, 1 << mo.INNER), repeats),
        "second_moments": device_ms(lambda: mo.second_moments(dseg), repeats),
        "masked_moments_4_channels": device_ms(lambda: mo.masked_moments(dvols, flags), repeats),
        "region_flags_with_device_percentiles": device_ms(lambda: mo.region_flags(dseg, dvols[mo.T1], dvols[mo.T2], dvols[mo.FLAIR]), repeats),
        "tumor_morphology": device_ms(lambda: mo.tumor_morphology(dseg, *dvols, dims), repeats),
    }
    state = {}

    def with_upload():
        state["res"] = mo.tumor_morphology(torch.from_numpy(seg).cuda(), *torch.from_numpy(vols).cuda(), dims)

    rows["tumor_morphology_with_upload"] = device_ms(with_upload, repeats)
    out = {"tool": "tools/morphology_time.py", "case": "full_size", "shape": list(seg.shape), "tumour_voxels": int((seg > 0).sum()),
           "surface_voxels": state["res"]["border_regularity"]["surface_voxel_count"], "device": torch.cuda.get_device_name(0), "device_ms": rows}
    if not args.profile:
        host, _ = host_sequence(seg, vols, dims)      # warm
        runs = [host_sequence(seg, vols, dims)[0] for _ in range(3)]
        best = min(runs, key=lambda r: r["total"])
        out["host"] = {"cpu": cpu_model(), "threads": int(os.environ.get("OMP_NUM_THREADS", torch.get_num_threads())), "best_of": 3, "ms": best}
        out["device_with_upload_faster_than_host"] = rows["tumor_morphology_with_upload"]["median_ms"] < best["total"]
    for k, v in rows.items():
        print(f"{k:40s} {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f})")
    if "host" in out:
        print("host:", json.dumps(out["host"]))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
