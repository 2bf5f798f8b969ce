#!/usr/bin/env python3
"""Time of ``mass_effect`` (the reference's step 2) on the device, in both distance modes, against its scipy + numpy restatement
on the same node's host, on the 240 x 240 x 155 case of tests/golden/mass_effect.json.

    python tools/mass_effect_time.py [--out profiles/mass_effect_time.json] [--repeats 15] [--profile]

Device times: warm calls on resident tensors between two stream events (every call synchronises itself: it returns host
values), median and minimum of --repeats, for the whole of ``mass_effect`` with ``distance='sampled'`` and ``'exact'`` and for
each of the five entry points of csrc/mass_effect.hip by itself.  Host times: ``host_stats`` of tests/mass_effect_util.py (the
scipy / numpy calls step 2 makes: percentiles, np.where profiles, ten dilations, boolean-mask reductions, the two draws and the
1000 x 1000 distances; the reference tree itself is not on the GPU node) plus ``mass_effect_from_stats``, best of 2, threads
capped at 16 as tests/conftest.py does; and, by themselves, the two ``np.random.choice(n, 1000, replace=False)`` draws, which
permute the whole population (44 473 tumour and 569 315 CSF voxels here) - they run on the host in the device path too.
--profile: a short device-only run, for `rocprofv3 --kernel-trace --stats -- python tools/mass_effect_time.py --profile`
(per-kernel times; no counters in that run).
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
    from brats_amd import mass_effect as me
    from brats_amd.morphology import distance_transform_edt_sq
    import mass_effect_util as mx
    from morphology_time import cpu_model, device_ms
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    assert torch.cuda.is_available(), "needs the GPU"
    case = mx.case("full_size")
    seg, t1 = mx.fixture_data(case)
    dseg, dt1 = torch.from_numpy(np.array(seg)).cuda(), torch.from_numpy(np.array(t1)).cuda()
    np.random.seed(case["rng_seed"])
    mx.Comparer().same(me.mass_effect(dseg, dt1, case["voxel_dims"]), case["expected"], "full_size")
    repeats = 3 if args.profile else args.repeats
    n_t, n_csf = case["facts"]["n_tumour"], case["facts"]["n_csf"]
    flags = (dt1 > 0).to(torch.uint8) | ((dseg > 0).to(torch.uint8) << 1)  # bit 0: about 40 % of the volume, bit 1: the tumour
    n_pos = int((t1 > 0).sum())
    ranks = np.random.RandomState(1).choice(n_pos, 1000, replace=False)
    a = me.select_ranked(flags, np.random.RandomState(2).choice(n_t, 1000, replace=False), 2)[0]
    b = me.select_ranked(flags, ranks, 1)[0]
    d2 = distance_transform_edt_sq((dt1 > 0).to(torch.uint8))
    rows = {"mass_effect_sampled": device_ms(lambda: me.mass_effect(dseg, dt1, case["voxel_dims"], rng=np.random.RandomState(1)), repeats),
            "mass_effect_exact": device_ms(lambda: me.mass_effect(dseg, dt1, case["voxel_dims"], distance="exact"), repeats),
            "axis_counts_all_positive_voxels": device_ms(lambda: me.axis_counts(flags, 1), repeats),
            "axis_counts_tumour": device_ms(lambda: me.axis_counts(flags, 2), repeats),
            "box_counts_6_boxes_tumour": device_ms(lambda: me.box_counts(flags, me.lobe_boxes(seg.shape), 2), repeats),
            "select_ranked_1000_of_all_positive_voxels": device_ms(lambda: me.select_ranked(flags, ranks, 1), repeats),
            "min_pair_dist2_1000x1000": device_ms(lambda: me.min_pair_dist2(a, b, seg.shape), repeats),
            "masked_min_tumour": device_ms(lambda: me.masked_min(d2, flags, 2), repeats)}
    for k, v in rows.items():
        print(f"{k:44s} device {v['median_ms']:9.3f} ms (min {v['min_ms']:.3f})")
    out = {"tool": "tools/mass_effect_time.py", "shape": list(seg.shape), "device": torch.cuda.get_device_name(0), "cpu": cpu_model(),
           "host_threads": int(torch.get_num_threads()), "n_tumour": n_t, "n_csf": n_csf, "rows": rows}
    if not args.profile:
        for mode in me.DISTANCES:
            times = []
            for _ in range(2):
                t0 = time.perf_counter()
                me.mass_effect_from_stats(mx.host_stats(me, seg, t1, np.random.RandomState(1), mode), case["voxel_dims"])
                times.append((time.perf_counter() - t0) * 1e3)
            out[f"host_scipy_numpy_{mode}_ms"] = round(min(times), 1)
            print(f"host scipy + numpy restatement, {mode}: {out[f'host_scipy_numpy_{mode}_ms']} ms")
        times = []
        for _ in range(5):
            gen = np.random.RandomState(1)
            t0 = time.perf_counter()
            me.sample_ranks(n_t, n_csf, gen)
            times.append((time.perf_counter() - t0) * 1e3)
        out["host_two_draws_ms"] = round(min(times), 3)
        print(f"the two np.random.choice draws on the host: {out['host_two_draws_ms']} ms")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
