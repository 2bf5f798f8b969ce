#!/usr/bin/env python3
"""Time of connected-component labelling + per-component statistics on the device against scipy + numpy on the same node's
host, for the two full-size (240 x 240 x 155) volumes DESIGN.md quotes: the `full_size` case of tests/golden/multiplicity.json
(tumour mask, 26 neighbours) and Bernoulli noise at p = 0.31 (6 neighbours: the percolation threshold, the hardest case
for union-find).

    python tools/components_time.py [--out FILE.json] [--min-seconds 0.5] [--profile]

Device times: host clock around warm calls between device synchronises, enough repeats to fill --min-seconds.  Host times:
scipy.ndimage.label plus a bincount-based table, threads capped at 16 as tests/conftest.py does.  --profile: a short run
without the host side, for `rocprofv3 --kernel-trace --stats -- python tools/components_time.py --profile`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def host_table(lab, n, seg):
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    comp = flat[idx] - 1
    out = np.zeros((n, 14), dtype=np.int64)
    out[:, 0] = np.bincount(comp, minlength=n)
    for k, c in enumerate(np.unravel_index(idx, lab.shape)):
        out[:, 1 + k] = np.round(np.bincount(comp, weights=c, minlength=n)).astype(np.int64)  # (exact: the sums stay below 2^53)
        lo, hi = np.full(n, 1 << 40, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        np.minimum.at(lo, comp, c)
        np.maximum.at(hi, comp, c)
        out[:, 4 + k], out[:, 7 + k] = lo, hi
    s = seg.ravel()[idx]
    for v in (1, 2, 3, 4):
        out[:, 9 + v] = np.bincount(comp[s == v], minlength=n)
    return out


def timed(fn, min_seconds, sync=None):
    """mean seconds per call over enough warm calls to fill min_seconds (at least 3), and the number of calls"""
    fn()
    reps, t = 0, 0.0
    while t < min_seconds or reps < 3:
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        t += time.perf_counter() - t0
        reps += 1
    return t / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    from scipy import ndimage
    import brats_amd
    from brats_amd import components
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    assert torch.cuda.is_available(), "needs the GPU"
    with open(ROOT / "tests" / "golden" / "multiplicity.json") as f:
        case = [c for c in json.load(f)["cases"] if c["name"] == "full_size"][0]["args"]
    seg = brats_amd.synthetic.label_map(case["seed"], tuple(case["shape"]), [(tuple(c), r) for c, r in case["lesions"]], case["fragments"],
                                        enhancing=case["enhancing"])
    noise = (np.random.RandomState(26).random_sample((240, 240, 155)) < 0.31).astype(np.uint8)
    min_seconds = 0.05 if args.profile else args.min_seconds
    rows = []
    for name, vol, conn in (("full_size fixture case, tumour mask", seg, 3), ("Bernoulli noise p = 0.31", noise, 1)):
        dev = torch.from_numpy(vol).cuda()
        state, host = {}, {}

        def label_only():
            state["labels"], state["n"] = components.label_components(dev, conn)

        def label_and_stats():
            label_only()
            state["stats"] = components.component_stats(state["labels"], state["n"], dev)

        label_only()
        n = state["n"]
        with_stats = n <= components.MAX_COMPONENTS
        row = {"volume": name, "shape": list(vol.shape), "connectivity": conn, "components": n, "foreground_voxels": int((vol != 0).sum())}
        sec, reps = timed(label_only, min_seconds, torch.cuda.synchronize)
        row["device_label_ms"], row["device_label_reps"] = round(sec * 1e3, 4), reps
        if with_stats:
            sec, reps = timed(label_and_stats, min_seconds, torch.cuda.synchronize)
            row["device_label_and_stats_ms"], row["device_label_and_stats_reps"] = round(sec * 1e3, 4), reps
        else:
            row["device_label_and_stats_ms"] = None
            row["note"] = f"{n} components exceed the {components.MAX_COMPONENTS}-row statistics table: labelling only"
        if not args.profile:
            structure = ndimage.generate_binary_structure(3, conn)

            def host_label():
                host["lab"], host["n"] = ndimage.label(vol != 0, structure=structure)

            def host_all():
                host_label()
                host["stats"] = host_table(host["lab"], host["n"], vol)

            sec, reps = timed(host_label, args.min_seconds)
            row["host_label_ms"], row["host_label_reps"] = round(sec * 1e3, 2), reps
            sec, reps = timed(host_all, args.min_seconds)
            row["host_label_and_table_ms"], row["host_label_and_table_reps"] = round(sec * 1e3, 2), reps
            assert host["n"] == n and np.array_equal(state["labels"].cpu().numpy(), host["lab"])
            if with_stats:
                assert np.array_equal(state["stats"], host["stats"])
            row["outputs_equal"] = True
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/components_time.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
