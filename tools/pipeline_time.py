#!/usr/bin/env python3
"""What the join of prediction, evaluation and feature extraction saves per case, on one
240 x 240 x 155 synthetic case with the two full-size ensemble members (models A + B, one fold each, 8-way mirror TTA).

    python tools/pipeline_time.py --parent-tree DIR [--runs 3] [--repeats 20] [--out profiles/pipeline_time.json] [--workdir DIR]

(a) ``files`` - the tree at DIR, a checkout of the parent commit with its library built: ``driver.main --label-format brats2025``, then
    ``evaluate.main`` and ``features.main`` on the files it wrote, in one warm process (what a pipeline pays when interpreter,
    library and checkpoints are already there; three cold processes cost more).
(b) ``joined`` - this tree: ``driver.main --analyze``.
Each run is a child process of its own that loads its models, runs once untimed and then once timed; the children alternate
a, b, a, b, ... so both sides see the same machine, one at a time (two resident drivers do not fit one device: each side's
activation arena wants the memory to itself).  Per run: the wall time of the whole call and the time from the end of the
prediction (the driver's ``[OK] Completed`` line, printed after its device synchronise) to the end of the last step, with the
moments at which the evaluation and the features were done.  Step 2 runs under ``--distance exact`` on both sides: no generator.

Then, in this process: ``mi355_reverse_axes`` between stream events, median of --repeats after a warm call, for the four float32
modalities [4, 155, 240, 240] and for the uint8 label map [155, 240, 240], with the bytes it reads and writes over that time as a
share of the 8.0 TB/s HBM peak (MI355X) and of the 6.29 TB/s a float4 copy reaches.  Both volumes fit the 256 MiB Infinity Cache
beside their outputs only in part (285 MB) or whole (18 MB): the share is of HBM's rate, the traffic need not all be HBM's.

The case: ``synthetic.mri_for_normal_structures`` with the two ventricles of the `full_size` fixture case, so that all six steps have
what they read, and a ground truth from ``synthetic.label_map``.  A run that raises is reported as such, not retried.
"""
import argparse
import contextlib
import json
import shutil
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CASE = "BraTS-GLI-00042-000"
SHAPE_XYZ = (240, 240, 155)
VENTRICLES = [["obox", (95, 90, 62), (118, 150, 92)], ["obox", (122, 90, 62), (150, 150, 92)]]
LESIONS = [((70.0, 130.0, 90.0), 22.0), ((160.0, 100.0, 60.0), 9.0)]
MARKS = (("prediction_done", "[OK] Completed:"), ("evaluation_done", "metrics written to"), ("features_done", ": 7 files in"))
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


class Marked:
    """A stdout that notes when each of MARKS first passes through it"""

    def __init__(self):
        self.at, self.text = {}, []

    def write(self, s):
        now = time.perf_counter()
        for name, phrase in MARKS:
            if name not in self.at and phrase in s:
                self.at[name] = now
        self.text.append(s)
        return len(s)

    def flush(self):
        pass


def prepare(amd, work, shape_xyz, patch):
    """The case folder and the two model folders (written once; both children read them)"""
    results = work / "nnUNet_results"
    base = results / "3d_fullres" / "Task500_BraTS2021"
    plans = amd.checkpoint.default_brats_plans(patch)
    small = {} if patch[0] >= 128 else {"num_pool": 2, "max_feat": 128}
    for name, preset, seed in ((amd.driver.MODEL1, "A", 7), (amd.driver.MODEL2, "B", 8)):
        if not (base / name).exists():
            amd.checkpoint.save_model_folder(base / name, name.split("__")[0], [amd.synthetic.make_model(preset, seed=seed, **small)[0]], plans)
    case_dir = work / CASE
    if not (case_dir / f"{CASE}_seg.nii.gz").exists():
        case_dir.mkdir(parents=True, exist_ok=True)
        scale = [s / f for s, f in zip(shape_xyz, SHAPE_XYZ)]
        seg = amd.synthetic.label_map(42, shape_xyz, [(tuple(c * k for c, k in zip(centre, scale)), r * min(scale)) for centre, r in LESIONS])
        vent = [[kind, [int(v * k) for v, k in zip(lo, scale)], [int(v * k) for v, k in zip(hi, scale)]] for kind, lo, hi in VENTRICLES]
        vols = amd.synthetic.mri_for_normal_structures(43, seg, ventricles=vent, contrast=0.5, pv_gain=0.2, voids="step", enhancement=1.8, sigma=6.0)
        like = amd.nifti.make_header(shape_xyz, zooms=(1.0, 1.0, 1.0), origin=(0.0, -239.0, 0.0))
        for v, mod in zip(vols, ("t1", "t1ce", "t2", "flair")):
            amd.nifti.save_like(case_dir / f"{CASE}_{mod}.nii.gz", v.astype(np.int16), like)
        amd.nifti.save_like(case_dir / f"{CASE}_seg.nii.gz", seg, like)
    return results, case_dir


def serve(tree, mode, work):
    """The child: the package of `tree`, models kept in a cache, one run per "run" line on stdin, one RESULT line per run."""
    sys.path.insert(0, str(tree))
    import importlib
    import torch
    import brats_amd as amd
    if torch.get_num_threads() > 16:
        torch.set_num_threads(16)
    real = sys.stdout
    results, case_dir = work / "nnUNet_results", work / CASE
    gt = case_dir / f"{CASE}_seg.nii.gz"
    cache = amd.driver.ModelCache()
    common = ["--input", str(case_dir), "--results_folder", str(results), "--folds", "0"]

    def one(tag):
        out = work / f"out_{mode}_{tag}"
        shutil.rmtree(out, ignore_errors=True)
        marked = Marked()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(marked):
            if mode == "joined":
                amd.driver.main(common + ["--output", str(out), "--analyze", "--distance", "exact"], model_cache=cache)
            else:
                amd.driver.main(common + ["--output", str(out), "--label-format", "brats2025"], model_cache=cache)
                marked.at["driver_returned"] = time.perf_counter()
                final = out / f"{CASE}.nii.gz"
                if amd.evaluate.main(["--pred", str(final), "--gt", str(gt), "--output", str(out / f"{CASE}_evaluation.json")]) != 0:
                    raise RuntimeError("evaluate.main failed")
                importlib.import_module("brats_amd.features").main(["--input", str(case_dir), "--segmentation", str(final),
                                                                    "--output", str(out / "feature_extraction"), "--distance", "exact"])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        p = marked.at["prediction_done"]
        res = {"total_s": round(t1 - t0, 3), "post_prediction_ms": round((t1 - p) * 1e3, 1)}
        res.update({f"{k}_ms": round((v - p) * 1e3, 1) for k, v in marked.at.items() if k != "prediction_done"})
        res["files_written"] = sum(1 for q in out.rglob("*") if q.is_file() and "temp_" not in str(q))
        return res

    def guarded(tag):
        try:
            return one(tag)
        except BaseException as e:   # (SystemExit of an argparse error included: the parent of this process wants a line either way)
            return {"error": f"{type(e).__name__}: {e}"[:600]}

    warm = guarded("warm")
    print("READY " + json.dumps(warm), file=real, flush=True)
    n = 0
    for line in sys.stdin:
        if line.strip() == "run":
            print("RESULT " + json.dumps(guarded(f"run{n}")), file=real, flush=True)
            n += 1
        elif line.strip() == "quit":
            break
    cache.close()
    return 0


def answer(child, word):
    """The child's next line that starts with `word` (the runtime may print lines of its own)"""
    while True:
        line = child.stdout.readline()
        if not line:
            raise RuntimeError(f"a child ended without a {word} line (exit status {child.poll()})")
        if line.startswith(word + " "):
            return json.loads(line[len(word) + 1:])


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
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(float(np.min(times)), 4), "max_ms": round(float(np.max(times)), 4), "repeats": repeats}


def kernel_rows(repeats, shape_zyx):
    import importlib
    import torch
    reverse_axes = importlib.import_module("brats_amd.volume_ops").reverse_axes
    rows = {}
    for name, t in (("float32_4ch", torch.randn((4,) + shape_zyx, device="cuda")), ("uint8_1ch", torch.randint(0, 4, shape_zyx, dtype=torch.uint8, device="cuda"))):
        row = event_ms(lambda: reverse_axes(t), repeats)   # (the output's allocation comes from torch's cache after the warm call)
        moved = 2 * t.numel() * t.element_size()
        row.update(shape=list(t.shape), bytes_read_plus_written=moved, tb_per_s=round(moved / (row["median_ms"] * 1e-3) / 1e12, 3),
                   share_of_hbm_peak=round(moved / (row["median_ms"] * 1e-3) / HBM_PEAK, 3), share_of_float4_copy=round(moved / (row["median_ms"] * 1e-3) / HBM_COPY, 3))
        rows[name] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--workdir", default="/tmp/pipeline_timing")
    ap.add_argument("--shape", type=int, nargs=3, default=list(SHAPE_XYZ), help="(x, y, z); smaller than the default only to rehearse")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--serve", nargs=2, metavar=("TREE", "MODE"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    work = Path(args.workdir)
    if args.serve:
        return serve(Path(args.serve[0]), args.serve[1], work)
    if not args.parent_tree:
        ap.error("--parent-tree is needed: the comparison is with the parent commit's file boundary")
    sys.path.insert(0, str(ROOT))
    import torch
    import brats_amd as amd
    assert torch.cuda.is_available(), "needs the GPU"
    work.mkdir(parents=True, exist_ok=True)
    t0 = time.perf_counter()
    prepare(amd, work, tuple(args.shape), (args.patch,) * 3)
    result = {"tool": "tools/pipeline_time.py", "device": torch.cuda.get_device_name(0), "shape_xyz": list(args.shape), "patch": args.patch,
              "models": "A + B, one fold each, 8-way mirror TTA, f32", "setup_s": round(time.perf_counter() - t0, 1), "runs": {}}
    print(f"case and models ready in {result['setup_s']} s", file=sys.stderr, flush=True)
    trees = (("files", Path(args.parent_tree).resolve()), ("joined", ROOT))
    for mode, tree in trees:
        result["runs"][mode] = {"tree": "the parent commit" if mode == "files" else "this tree", "warm": [], "timed": []}
    for _ in range(args.runs):
        for mode, tree in trees:   # one child at a time: each side's activation arena wants the device's memory to itself
            child = subprocess.Popen([sys.executable, str(Path(__file__).resolve()), "--workdir", str(work), "--serve", str(tree), mode],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=str(tree))
            try:
                result["runs"][mode]["warm"].append(answer(child, "READY"))
                child.stdin.write("run\n")
                child.stdin.flush()
                result["runs"][mode]["timed"].append(answer(child, "RESULT"))
                print(f"{mode}: warm {result['runs'][mode]['warm'][-1]}\n{mode}: timed {result['runs'][mode]['timed'][-1]}", file=sys.stderr, flush=True)
            finally:
                with contextlib.suppress(OSError):
                    child.stdin.write("quit\n")
                    child.stdin.flush()
                try:
                    child.wait(timeout=120)
                except subprocess.TimeoutExpired:
                    child.kill()
    for mode, rows in result["runs"].items():
        post = [r["post_prediction_ms"] for r in rows["timed"] if "post_prediction_ms" in r]
        if post:
            rows["post_prediction_ms"] = {"median": float(np.median(post)), "min": min(post), "max": max(post), "spread": round(max(post) - min(post), 1)}
    a, b = (result["runs"][m].get("post_prediction_ms") for m in ("files", "joined"))
    if a and b:
        result["gap_ms"] = {"median_files_minus_median_joined": round(a["median"] - b["median"], 1), "parent_spread": a["spread"],
                            "beyond_parent_spread": bool(a["min"] - b["max"] > a["spread"])}
    result["reverse_axes"] = kernel_rows(args.repeats, tuple(args.shape[::-1]))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
