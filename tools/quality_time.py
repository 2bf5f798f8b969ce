#!/usr/bin/env python3
"""Time of ``quality_control`` (the reference's step 5) on the device against its scipy + numpy restatement on the same node's
host, on the 240 x 240 x 155 case of tests/golden/quality.json.

    python tools/quality_time.py [--out profiles/quality_time.json] [--repeats 15] [--profile]

Device times: warm calls on resident tensors between two stream events (every call synchronises itself: it returns host
values), median and minimum of --repeats, for the
whole of ``quality_control`` and for each of the four entry points of csrc/quality.hip by itself.  Host time: ``host_stats`` of
tests/quality_util.py (the scipy / numpy calls step 5 makes: label, binary_fill_holes by labelling, erosion, three Sobel
passes, percentiles, boolean-mask reductions) plus ``quality_from_stats``, best of 2, threads capped at 16 as
tests/conftest.py does.  --profile: a short device-only run, for
`rocprofv3 --kernel-trace --stats -- python tools/quality_time.py --profile` (per-kernel times; no counters in that run).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    import brats_amd  # noqa: F401
    from brats_amd import quality as q
    import quality_util as qu
    from morphology_time import cpu_model, device_ms
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    assert torch.cuda.is_available(), "needs the GPU"
    case = qu.case("full_size")
    seg, vols = qu.fixture_data(case)
    dseg = torch.from_numpy(np.array(seg)).cuda()
    dvols = [torch.from_numpy(np.array(v)).cuda() for v in vols]
    got = q.quality_control(dseg, *dvols, case["voxel_dims"])
    qu.Comparer().same(got, case["expected"], "full_size")
    repeats = 3 if args.profile else args.repeats
    flags = (dvols[0] > 0).to(torch.uint8)
    centre = [v / 2.0 for v in seg.shape]
    rows = {"quality_control": device_ms(lambda: q.quality_control(dseg, *dvols, case["voxel_dims"]), repeats),
            "binary_fill_holes": device_ms(lambda: q.binary_fill_holes(dseg), repeats),
            "sobel_magnitude_stats_all_positive_voxels": device_ms(lambda: q.sobel_magnitude_stats(dvols[0], flags, 1), repeats),
            "radial_shell_moments_all_positive_voxels": device_ms(lambda: q.radial_shell_moments(dvols[0], flags, 1, centre), repeats),
            "face_slab_counts": device_ms(lambda: q.face_slab_counts(dvols[0], 5), repeats)}
    for k, v in rows.items():
        print(f"{k:44s} device {v['median_ms']:9.3f} ms (min {v['min_ms']:.3f})")
    out = {"tool": "tools/quality_time.py", "shape": list(seg.shape), "device": torch.cuda.get_device_name(0), "cpu": cpu_model(),
           "host_threads": int(torch.get_num_threads()), "rows": rows}
    if not args.profile:
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            q.quality_from_stats(qu.host_stats(q, seg, vols), case["voxel_dims"])
            times.append((time.perf_counter() - t0) * 1e3)
        out["host_scipy_numpy_ms"] = round(min(times), 1)
        print(f"host scipy + numpy restatement: {out['host_scipy_numpy_ms']} ms")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
