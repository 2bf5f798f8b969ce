#!/usr/bin/env python3
"""Time of ``masked_percentiles`` on the device against ``np.percentile`` on the same node's host, on 240 x 240 x 155 volumes.

    python tools/percentile_time.py [--out profiles/percentile_time.json] [--repeats 30] [--profile]

Volumes: (a) the MR-like T1 of the `full_size` case of tests/golden/morphology.json, selected with lo = 0 (``data[data > 0]``),
(b) uniform random finite bit patterns, (c) a constant volume; 1 and 8 percentiles per call.  Device times: warm calls with a
device synchronise on both sides (the call synchronises itself: it returns host values), median and minimum of --repeats.
Host times: ``np.percentile`` of the float64 copy of the same selected values (the copy and the selection are not timed), best
of 3, threads capped at 16 as tests/conftest.py does.  --profile: a short device-only run, for
`rocprofv3 --kernel-trace --stats -- python tools/percentile_time.py --profile` (per-kernel times; no counters in that run).
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

Q1, Q8 = (10,), (0, 5, 10, 25, 50, 85, 99, 100)


def device_ms(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(float(np.min(times)), 4), "repeats": repeats}


def host_ms(values, qs):
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        np.percentile(values, qs)
        times.append((time.perf_counter() - t0) * 1e3)
    return round(min(times), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    import brats_amd  # noqa: F401
    from brats_amd import percentile as pc
    import gen_morphology_golden as gen
    from morphology_time import cpu_model
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    assert torch.cuda.is_available(), "needs the GPU"
    with open(ROOT / "tests" / "golden" / "morphology.json") as f:
        case = [c for c in json.load(f)["cases"] if c["name"] == "full_size"][0]
    _, vols = gen.case_data(case["args"])
    rs = np.random.RandomState(5)
    bits = rs.randint(0, 2 ** 32, vols[0].size, dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] &= np.uint32(0xFF7FFFFF)
    volumes = {"a_mr_like_lo_0": (vols[0], 0.0), "b_random_bits": (bits.view(np.float32).reshape(vols[0].shape), -np.inf),
               "c_constant": (np.full(vols[0].shape, 1234.5, np.float32), -np.inf)}
    repeats = 3 if args.profile else args.repeats
    rows = {}
    for name, (x, lo) in volumes.items():
        dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        selected = x[(x > lo) & np.isfinite(x)].astype(np.float64)
        for label, qs in (("1_percentile", Q1), ("8_percentiles", Q8)):
            count, got = pc.masked_percentiles(dx, qs, lo=lo)
            assert count == selected.size and np.array_equal(got, np.percentile(selected, qs)), (name, label)
            row = {"selected": int(count), "device": device_ms(lambda: pc.masked_percentiles(dx, qs, lo=lo), repeats)}
            if not args.profile:
                row["host_np_percentile_ms"] = host_ms(selected, qs)
            rows[f"{name}/{label}"] = row
            print(f"{name + '/' + label:36s} device {row['device']['median_ms']:8.3f} ms (min {row['device']['min_ms']:.3f})"
                  + (f"   host {row['host_np_percentile_ms']:8.2f} ms" if "host_np_percentile_ms" in row else ""))
    out = {"tool": "tools/percentile_time.py", "shape": list(vols[0].shape), "device": torch.cuda.get_device_name(0), "cpu": cpu_model(),
           "host_threads": int(torch.get_num_threads()), "rows": rows,
           "constant_over_mr_like": {k: round(rows[f"c_constant/{k}"]["device"]["median_ms"] / rows[f"a_mr_like_lo_0/{k}"]["device"]["median_ms"], 3)
                                     for k in ("1_percentile", "8_percentiles")}}
    print("constant / MR-like:", out["constant_over_mr_like"])
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
