#!/usr/bin/env python3
"""Time of the surface-distance path (brats_amd.evaluate.surface_metrics: HD95, ASSD, surface Dice of WT, TC and ET) on the device, end
to end and stage by stage, beside the scipy oracle of tests/surface_distance_util.py on the same node's host, for one synthetic
240 x 240 x 155 case of brats_amd.synthetic and a second label map that differs from it.

    python tools/surface_distance_time.py [--out profiles/surface_distance_time.json] [--repeats 20] [--profile]

Device times: HIP events around warm calls (one warm-up call first, then the median and the minimum of --repeats timed calls).  The
end-to-end calls return numbers to the host and so synchronise themselves (the distance transform once per direction for its site
count, the gather once for its count, the copy of the distances), which the events include; the stage rows are the three entry points
alone on buffers that stay allocated: `region_surfaces` is asynchronous (the closing event waits for it), the other two synchronise as
said.  The end-to-end figure is also taken WITH the upload of the two label maps.  Host times: binary_erosion and
distance_transform_edt(sampling=...) per region and direction plus the numpy metrics, best of 3, threads capped at 16 as
tests/conftest.py does.  --profile: a short device-only run, for `rocprofv3 --kernel-trace --stats -- python tools/surface_distance_time.py --profile`.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

from morphology_time import cpu_model, device_ms  # noqa: E402

SHAPE = (240, 240, 155)
SPACING = (1.0, 1.0, 1.0)


def label_maps():
    from brats_amd import synthetic
    gt = synthetic.label_map(5, SHAPE, [((120, 110, 80), 34), ((70, 150, 60), 13)])
    pred = synthetic.label_map(6, SHAPE, [((122, 108, 81), 31), ((70, 151, 62), 15)])
    return pred, gt


def host_sequence(pred, gt):
    import surface_distance_util as su
    t = {}
    t0 = time.perf_counter()
    surfaces = {name: (su.surface(su.region_mask(pred, labels)), su.surface(su.region_mask(gt, labels))) for name, labels in su.REGIONS.items()}
    t["six_erosions"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    dist = {name: (su.directed(sa, sb, SPACING), su.directed(sb, sa, SPACING)) for name, (sa, sb) in surfaces.items()}
    t["six_distance_transforms_and_indexing"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    res = {name: su.metrics(*d) for name, d in dist.items()}
    t["metrics"] = round((time.perf_counter() - t0) * 1e3, 2)
    t["total"] = round(sum(t.values()), 2)
    return t, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    import brats_amd  # noqa: F401
    from brats_amd import _lib, evaluate as ev
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    assert torch.cuda.is_available(), "needs the GPU"
    pred, gt = label_maps()
    repeats = 2 if args.profile else args.repeats
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    # the stages alone, on the whole tumour's joint box
    u8p, i32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    table = ev._region_table(ev.SURFACE_REGIONS)
    flags = torch.empty(dp.numel(), dtype=torch.uint8, device="cuda")
    stats = [ev.label_stats(t, 8)[[1, 2, 3]] for t in (dp, dg)]
    present = np.concatenate([s[s[:, 0] > 0] for s in stats])
    lo, hi = present[:, 4:7].min(axis=0).astype(np.int32), (present[:, 7:10].max(axis=0) + 1).astype(np.int32)
    n = int(np.prod((hi - lo).astype(np.int64)))
    words = (n + ev.GATHER_CHUNK - 1) // ev.GATHER_CHUNK + 1
    dist2 = torch.empty(n, dtype=torch.float64, device="cuda")
    picked = torch.empty(int(stats[0][:, 0].sum()), dtype=torch.float64, device="cuda")
    blocks, word = torch.empty(words, dtype=torch.int32, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda")
    sp, count = np.array(SPACING, dtype=np.float64), np.zeros(1, dtype=np.int64)
    box = (lo.ctypes.data_as(i32p), hi.ctypes.data_as(i32p))

    def surfaces():
        _lib.check(lib.mi355_region_surfaces(dp.data_ptr(), dg.data_ptr(), *SHAPE, table.ctypes.data_as(u8p), table.ctypes.data_as(u8p), flags.data_ptr(),
                                             flags.numel(), stream))

    def transform():
        _lib.check(lib.mi355_edt_to_flagged_f64(flags.data_ptr(), *SHAPE, *box, 0x10, sp.ctypes.data_as(f64p), dist2.data_ptr(), n, word.data_ptr(), stream))

    def gather():
        _lib.check(lib.mi355_gather_flagged_f64(dist2.data_ptr(), flags.data_ptr(), *SHAPE, *box, 0x01, picked.data_ptr(), picked.numel(), blocks.data_ptr(),
                                                words, count.ctypes.data_as(C.POINTER(C.c_int64)), stream))

    surfaces()
    rows = {
        "region_surfaces_both_maps_all_regions": device_ms(surfaces, repeats),
        "edt_to_flagged_f64_wt_box": device_ms(transform, repeats),
        "gather_flagged_f64_wt_box": device_ms(gather, repeats),
        "label_stats_one_map": device_ms(lambda: ev.label_stats(dp, 8), repeats),
        "surface_metrics_wt_tc_et": device_ms(lambda: ev.surface_metrics(dp, dg, SPACING), repeats),
        "evaluate_with_surfaces": device_ms(lambda: ev.evaluate_with_surfaces(dp, dg, SPACING), repeats),
    }
    state = {}

    def with_upload():
        state["res"] = ev.surface_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), SPACING)

    rows["surface_metrics_with_upload"] = device_ms(with_upload, repeats)
    res = state["res"]
    out = {"tool": "tools/surface_distance_time.py", "shape": list(SHAPE), "spacing": list(SPACING), "device": torch.cuda.get_device_name(0),
           "wt_box": [int(v) for v in hi - lo], "wt_box_voxels": n,
           "surface_voxels": {k: [m["surface_voxels_pred"], m["surface_voxels_gt"]] for k, m in res.items()},
           "hd95": {k: m["hd95"] for k, m in res.items()}, "device_ms": rows}
    if not args.profile:
        runs = [host_sequence(pred, gt) for _ in range(3)]
        best, host_res = min(runs, key=lambda r: r[0]["total"])
        out["host"] = {"cpu": cpu_model(), "threads": int(os.environ.get("OMP_NUM_THREADS", torch.get_num_threads())), "best_of": 3, "ms": best}
        out["agrees_with_host"] = all(abs(res[k][f] - host_res[k][f]) <= 1e-12 * abs(host_res[k][f]) for k in res for f in ("hd", "hd95", "assd", "surface_dice"))
    for k, v in rows.items():
        print(f"{k:44s} {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f})")
    print("WT box", out["wt_box"], "surface voxels", out["surface_voxels"])
    if "host" in out:
        print("host:", json.dumps(out["host"]), "agrees:", out["agrees_with_host"])
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
