#!/usr/bin/env python3
"""Time of lesion-wise scoring (brats_amd.evaluate.lesionwise_metrics: lesion-wise Dice and HD95 of WT, TC and ET) on the device, end
to end and for the three entry points of csrc/lesionwise.hip alone, beside the scipy restatement of tests/lesionwise_util.py on the same
node's host, for one synthetic 240 x 240 x 155 pair (lesionwise_util.blob_case: four ball lesions, one of them missed by the
prediction, and 300 specks in the prediction).

    python tools/lesionwise_time.py [--out profiles/lesionwise_time.json] [--repeats 20] [--no-host]

Device times: HIP events around warm calls (one warm-up call first, then the median and the minimum of --repeats timed calls).  The
dilation rows are asynchronous calls on buffers that stay allocated (the closing event waits for them); `mi355_binary_morphology`
beside them is the existing one-launch-per-step cross stencil, for the same three steps.  The histogram and the lookup return or
check numbers on the host and synchronise themselves, which the events include; so does the end-to-end call, many times.  Host
times: the restatement per region, best of 2, threads capped at 16 as tests/conftest.py does.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy side (over half a minute)")
    args = ap.parse_args()
    import torch
    import brats_amd  # noqa: F401
    import lesionwise_util as lu
    from brats_amd import _lib, components as cc, evaluate as ev, volume_ops as vo
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    assert torch.cuda.is_available(), "needs the GPU"
    pred, gt = lu.blob_case(SHAPE)
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    repeats = args.repeats

    # the stages alone, on the whole tumour
    g_mask, p_mask = cc._indicator(dg, (1, 2, 3)), cc._indicator(dp, (1, 2, 3))
    out, tmp = torch.empty_like(g_mask), torch.empty_like(g_mask)

    def dilate_nb(neighbours, iterations):
        _lib.check(lib.mi355_binary_morphology_nb(g_mask.data_ptr(), *SHAPE, 1, neighbours, iterations, out.data_ptr(), tmp.data_ptr(), tmp.numel(), stream))

    rows = {
        "binary_morphology_nb_dilate_18_3_steps_one_launch": device_ms(lambda: dilate_nb(18, 3), repeats),
        "binary_morphology_nb_dilate_18_1_step": device_ms(lambda: dilate_nb(18, 1), repeats),
        "binary_morphology_nb_dilate_6_3_steps_one_launch": device_ms(lambda: dilate_nb(6, 3), repeats),
        "binary_morphology_cross_3_steps_three_launches": device_ms(lambda: vo.binary_dilation(g_mask, 3), repeats),
        "binary_morphology_nb_dilate_18_9_steps_three_launches": device_ms(lambda: dilate_nb(18, 9), repeats),
    }
    pcc, n_pred = cc.label_components(p_mask, 3)
    gcc, n_gt = cc.label_components(g_mask, 3)
    gdcc, n_les = cc.label_components(vo.binary_dilation_nb(g_mask, 18, 3), 3)
    rows["label_pair_counts_lds_path"] = device_ms(lambda: cc.pair_counts(gcc, n_gt, gdcc, n_les), repeats)
    rows["label_pair_counts_lds_path_pred"] = device_ms(lambda: cc.pair_counts(pcc, n_pred, gdcc, n_les), repeats)
    rows["label_pair_counts_global_path"] = device_ms(lambda: cc.pair_counts(pcc, n_pred, pcc, n_pred), repeats)
    table8 = (np.arange(n_pred + 1) % 16).astype(np.uint8)
    table32 = np.arange(n_pred + 1, dtype=np.int32)
    rows["label_lookup_u8"] = device_ms(lambda: cc.lookup(pcc, n_pred, table8), repeats)
    rows["label_lookup_i32"] = device_ms(lambda: cc.lookup(pcc, n_pred, table32), repeats)
    rows["label_components_26_one_map"] = device_ms(lambda: cc.label_components(p_mask, 3), repeats)
    rows["lesionwise_metrics_wt_tc_et"] = device_ms(lambda: ev.lesionwise_metrics(dp, dg, SPACING), repeats)
    rows["evaluate_lesionwise"] = device_ms(lambda: ev.evaluate_lesionwise(dp, dg, SPACING), repeats)
    res = ev.lesionwise_metrics(dp, dg, SPACING)
    out_json = {"tool": "tools/lesionwise_time.py", "shape": list(SHAPE), "spacing": list(SPACING), "device": torch.cuda.get_device_name(0),
                "components_wt": {"pred": n_pred, "gt": n_gt, "lesions": n_les},
                "pair_table_entries": {"lds_path": (n_gt + 1) * (n_les + 1), "lds_path_pred": (n_pred + 1) * (n_les + 1), "global_path": (n_pred + 1) ** 2},
                "counts": {k: [m["num_lesions"], m["num_counted"], m["num_tp"], m["num_fn"], m["num_fp"]] for k, m in res.items()},
                "lesionwise_dice": {k: m["lesionwise_dice"] for k, m in res.items()}, "lesionwise_hd95": {k: m["lesionwise_hd95"] for k, m in res.items()},
                "device_ms": rows}
    if not args.no_host:
        best, host_res = None, None
        for _ in range(2):
            t0 = time.perf_counter()
            host_res = lu.case_lesionwise(pred, gt, SPACING)
            ms = round((time.perf_counter() - t0) * 1e3, 1)
            best = ms if best is None else min(best, ms)
        t0 = time.perf_counter()
        lu.morph(gt > 0, True, 18, 3)
        out_json["host"] = {"cpu": cpu_model(), "threads": int(os.environ.get("OMP_NUM_THREADS", torch.get_num_threads())), "best_of": 2,
                            "restatement_wt_tc_et_ms": best, "scipy_dilation_18_3_steps_ms": round((time.perf_counter() - t0) * 1e3, 1)}
        out_json["agrees_with_host"] = all(lu.same(res[k], host_res[k], k) <= 1e-12 for k in res)
    for k, v in rows.items():
        print(f"{k:56s} {v['median_ms']:10.3f} ms (min {v['min_ms']:.3f})")
    print("WT components", out_json["components_wt"], "counts", out_json["counts"])
    if "host" in out_json:
        print("host:", json.dumps(out_json["host"]), "agrees:", out_json["agrees_with_host"])
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out_json, f, indent=1)


if __name__ == "__main__":
    main()
