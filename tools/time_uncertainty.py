#!/usr/bin/env python3
"""What keeping the second moment costs: config 3 of bench.py (both ensemble members, 8 tiles x 8 mirrors of 128^3 each, one
synthetic case) predicted with predictor.predict_folds against predictor.predict_folds_moments, fp16 and fp32.

HIP events around each prediction on the caller's stream (the lanes join it before the event), the two variants ALTERNATING
within one process so that clock and thermal drift fall on both alike, the median and the quartiles of each.  Prints one JSON line.

    python tools/time_uncertainty.py [--steps 9] [--warmup 2] [--dtypes f16 f32]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PATCH = (128, 128, 128)
MODELS = (("A", 7), ("B", 8))   # bench.py WORKLOADS[3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", nargs="+", default=["f16", "f32"], choices=("f16", "f32"))
    args = ap.parse_args()
    import torch
    import brats_amd
    from brats_amd import predictor, preprocessing, synthetic
    dev = torch.device("cuda", 0)
    data, _ = preprocessing.preprocess_case(synthetic.make_volume(seed=1000), dev)
    out = {"workload": "bench.py config 3: 2 members x 8 tiles x 8 mirrors, patch 128^3", "crop": list(data.shape[1:]), "steps": args.steps,
           "lanes": predictor.default_lanes()}
    for dt in args.dtypes:
        members = []
        for name, seed in MODELS:
            sd, meta = synthetic.make_model(name, seed=seed)
            members.append([brats_amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"], dtype=dt)])
            del sd
        call = (PATCH, 0.5, True, (0, 1, 2), True, "sigmoid")
        variants = {"predict_folds": lambda: [predictor.predict_folds(m, data, *call) for m in members],
                    "predict_folds_moments": lambda: [predictor.predict_folds_moments(m, data, *call) for m in members]}
        ms = {k: [] for k in variants}
        for i in range(args.warmup + args.steps):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = fn()
                e1.record()
                e1.synchronize()
                del res
                if i >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        row = {}
        for k, v in ms.items():
            q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
            row[k] = {"median_ms": round(statistics.median(v), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3), "min_ms": round(min(v), 3)}
        row["overhead_percent"] = round(100.0 * (row["predict_folds_moments"]["median_ms"] / row["predict_folds"]["median_ms"] - 1.0), 2)
        out[dt] = row
        for m in members:
            for n in m:
                n.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
