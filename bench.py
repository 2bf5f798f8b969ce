#!/usr/bin/env python
"""bench.py - BraTS volumes/s of the MI355X-native nnU-Net sliding-window predictor.

One "step" = one pass of the hot path over one synthetic BraTS-shaped volume that is already
preprocessed and resident in HBM: tile gather -> U-Net forwards -> sigmoid -> Gaussian-weighted
aggregation -> probabilities -> region labels pasted into the full 155x240x240 uint8 volume.
Default workload = BASELINE.json configs[1]: one 4x240x240x155 volume, 128^3 patches, step 0.5,
model A (base 32, BatchNorm), 1 fold, fp32, no TTA -> 8 forwards per volume.  A plain run sets up, warms up
(W steps), times exactly K steps, writes the outputs of the last timed step if --dump-outputs is given, and prints
the JSON line.  With --full the line also carries the CPU baseline and the parity blocks against the CPU oracle,
the per-kernel HIP-event profile and roofline, and (config 2) `secondary` blocks for BASELINE.json configs[2]
(8-way TTA, models A + B, label ensemble) in fp16 and fp32, an `end_to_end` block (host volume -> H2D ->
crop -> z-score -> predict -> labels -> D2H) and a `reference_setting` block: the reference's own per-case setting
(5 folds x 2 models x 8-way TTA) in fp16 and fp32, three timed steps each.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config 2|3|4] [--dtype f32|f16] [--shard cases|tiles] [--folds F]
                    [--dump-outputs DIR] [--full [--no-cpu-baseline] [--no-secondary] [--no-reference-setting]]

--dump-outputs DIR: after the timed steps, what the last timed step computed, as float32 DIR/<name>.npy (at most 64 MB in
all; inputs and weights are seeded, so the same arguments give the same inputs on every run): configs 2 / 3 `labels`
(the full 155x240x240 label volume the step returns) and `probabilities_<model>` (a fixed, seeded sample of each ensemble
member's probabilities); config 4 `labels_case<i>` (a fixed, seeded sample of each case's label volume, written by the rank
that owns the case).

--config 3 --shard tiles = SURVEY.md 8e partitioning B (single-case latency): every rank works on the SAME volume, the
(fold, tile) work list of each ensemble member is dealt round-robin over the ranks (mi355_sw_partial_folds), the partial
aggregates travel through ONE RCCL all_gather per member and are summed in rank order; a step = that one volume, so this
mode scales strongly ("scaling": "strong").

--config 4 = BASELINE.json configs[3]: a batch of 32 synthetic volumes (seeds 1000..1031), config-3
settings, CASES dealt longest-first by tile count over the ranks (SURVEY.md 8e partitioning A, no
data-path collective); one step = the whole batch, so this workload scales strongly.

For N > 1 the driver launches this file under torch.distributed.run; when it is started plainly
with --gpus N > 1 it starts that launcher itself as a child process BEFORE anything touches the
GPU and relays the child's output and exit code.  Timing is barrier + synchronize bracketed and the
maximum over ranks.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md "Peak FP32 (matrix)"
PEAK_F16_MFMA_TFLOPS = 2500.0  # dense fp16/bf16 MFMA, same guide
NOMINAL_CLOCK_GHZ = 2.4        # the engine clock those peaks are quoted at (same guide)
PEAK_HBM_GBS = 8000.0
PATCH = (128, 128, 128)
DICE_GATE = 0.999  # BASELINE.json north_star: Dice against the reference CPU output >= 0.999
# Winograd kernels execute fewer multiplies than the algorithmic (direct-convolution) count that `achieved` uses:
# F(2,3) along y issues 2/3 of the direct MFMAs, F(2x2,3x3) over (z,y) 4/9, F(2x2x2,3x3x3) 8/27; frac can therefore exceed 1 and
# frac_executed = matrix-pipe utilisation is reported beside it.
EXECUTED_RATIO = {"conv3_f32_wino_kernel": 2.0 / 3.0, "conv3_f32_wino2_kernel<0>": 4.0 / 9.0, "conv3_f32_wino2_kernel<1>": 4.0 / 9.0,
                  "conv3_f32_wino2_kernel<2>": 4.0 / 9.0,
                  # F(2x2x2,3x3x3): 64 multiplies per 2x2x2 outputs and (cin, cout) instead of 8 * 27
                  "conv3_f32_wino3_kernel<0, false>": 8.0 / 27.0, "conv3_f32_wino3_kernel<1, false>": 8.0 / 27.0, "conv3_f32_wino3_kernel<2, false>": 8.0 / 27.0,
                  "conv3_f32_wino3_kernel<2, true>": 8.0 / 27.0}

WORKLOADS = {
    2: dict(models=[("A", 7)], tta=False, dtype="f32",
            name="BASELINE.json configs[1]: 1 volume 4x240x240x155, 128^3 patches, step 0.5, model A, 1 fold, no TTA"),
    3: dict(models=[("A", 7), ("B", 8)], tta=True, dtype="f16",
            name="BASELINE.json configs[2]: 1 volume, 8-way mirror TTA, models A+B, 1 fold each, label-round ensemble"),
    4: dict(models=[("A", 7), ("B", 8)], tta=True, dtype="f16", n_cases=32,
            name="BASELINE.json configs[3]: batch of 32 synthetic volumes (seeds 1000-1031), 8-way mirror TTA, models A+B, "
                 "1 fold each, label-round ensemble, cases sharded over the ranks"),
}


def _at_least(lo):
    def parse(v):
        n = int(v)
        if n < lo:
            raise argparse.ArgumentTypeError(f"must be >= {lo}")
        return n
    return parse


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=_at_least(1), default=10, help="timed steps")
    ap.add_argument("--warmup", type=_at_least(0), default=2, help="untimed steps before them")
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 4), help="BASELINE.json config (1-based)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: CPU baseline and parity against the CPU oracle, "
                         "per-kernel profile and roofline, and (config 2) the config-3, end-to-end and reference-setting blocks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline and the parity blocks")
    ap.add_argument("--no-secondary", action="store_true", help="skip the config-3 and end-to-end blocks of a --full run")
    ap.add_argument("--no-reference-setting", action="store_true", help="skip the 5-fold x 2-model x TTA block of a --full run")
    ap.add_argument("--batch-tiles", type=int, default=0)
    ap.add_argument("--cases", type=int, default=0, help="config 4: number of volumes in the batch (default 32)")
    ap.add_argument("--shard", choices=("cases", "tiles"), default="cases",
                    help="config 3 with N > 1: 'cases' = one volume per rank per step (weak scaling, no data-path collective); 'tiles' = "
                         "ONE volume per step for all ranks, its (fold, tile) work list dealt over the ranks and one RCCL all_gather of "
                         "the partial aggregates per ensemble member (SURVEY.md 8e partitioning B, strong scaling)")
    ap.add_argument("--lanes", type=int, default=0, help="HIP streams one predict_folds call spreads its (fold, tile) list over (0: the product's default, MI355_LANES or 2)")
    ap.add_argument("--folds", type=int, default=1, help="folds per ensemble member (the reference runs 5: driver :161)")
    ap.add_argument("--dtype", choices=("f32", "f16"), default=None, help="default: f32 for config 2, f16 for configs 3 and 4")
    # rehearsal of the N > 1 launch path on a box with fewer GPUs than ranks: ranks share device 0 and synchronise
    # over gloo (RCCL refuses two ranks on one device); never used by the driver
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help=argparse.SUPPRESS)
    ap.add_argument("--share-gpu", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def launch_command(n_gpus, argv, port=None):
    """The command the driver itself uses for N > 1 (one rank per GPU over RCCL)."""
    if port is None:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr",
            "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def maybe_self_launch(args, argv):
    """--gpus N > 1 without a launcher: become the launcher's parent.  Nothing in this process has touched HIP yet
    (torch is not even imported), so starting children is safe; we never exec."""
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
        proc = subprocess.run(launch_command(args.gpus, argv), env=env)
        sys.exit(proc.returncode)


class Ctx:
    """Process-level state of one bench run (rank, device, collective helpers)."""

    def __init__(self, args):
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={self.world}")
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
        dev_index = 0 if args.share_gpu else self.local_rank
        torch.cuda.set_device(dev_index)
        self.device = torch.device("cuda", dev_index)
        self.use_dist = "RANK" in os.environ and "MASTER_ADDR" in os.environ  # launched by torch.distributed.run (any N)
        self.backend = args.backend
        if self.use_dist:
            if self.backend == "nccl":
                dist.init_process_group("nccl", device_id=self.device)
            else:
                dist.init_process_group("gloo")

    def sync_all(self):
        self.torch.cuda.synchronize(self.device)
        if self.use_dist:
            if self.backend == "nccl":
                self.dist.barrier(device_ids=[self.device.index])
            else:
                self.dist.barrier()
            self.torch.cuda.synchronize(self.device)

    def max_over_ranks(self, seconds):
        if not self.use_dist:
            return seconds
        dev = self.device if self.backend == "nccl" else "cpu"
        t = self.torch.tensor([seconds], dtype=self.torch.float64, device=dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def close(self):
        if self.use_dist:
            self.dist.destroy_process_group()


def build_nets(models, dtype):
    import brats_amd
    from brats_amd import synthetic
    nets = []
    for name, seed in models:
        sd, meta = synthetic.make_model(name, seed=seed)
        nets.append(brats_amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"], dtype=dtype))
        del sd
    return nets


def lib_source_digest():
    """Digest of csrc/ + headers + flags the in-tree library is built from (the same one lib/libmi355_nnunet.so.digest records)."""
    try:
        from brats_amd import _build
        return _build._library_digest()
    except Exception:
        return None


def committed_counter(fname, section, kernel, field):
    """One figure from a committed rocprofv3 --pmc pass (profiles/pmc_traffic.json, profiles/kernel_clocks.json): the value, and
    whether the pass was taken on a library built from other sources than the one running now (`stale`)."""
    path = os.path.join(ROOT, "profiles", fname)
    if not os.path.exists(path):
        return None, None
    try:
        doc = json.load(open(path))
    except Exception:
        return None, None
    entry = (doc.get(section) or {}).get(kernel) if section else None
    if entry is None:
        entry = doc.get(kernel) if isinstance(doc.get(kernel), dict) else None
    if not entry or entry.get(field) is None:
        return None, None
    have, now = doc.get("_source_digest"), lib_source_digest()
    return entry[field], (have is None or now is None or have != now)


def timed_region(ctx, step, steps, warmup, nets, profile=True, capture=None):
    """W untimed steps, then exactly K steps between two barrier + synchronize brackets; with `profile` (--full) the per-kernel
    HIP-event profile (events recorded by the library on the launch stream) of the timed steps - or, when the step runs on more
    than one lane (predictor.predict_folds(lanes > 1): kernels of two streams overlap, so an event pair around one of them also
    times its neighbours), of ONE extra, untimed step on a single lane after the timed region; without it `prof` is None.
    `capture` (--dump-outputs): a dict whose "on" is True during the last timed step only, for the step to keep what it computed."""
    from brats_amd import predictor
    lanes = predictor.default_lanes()
    out = None
    for _ in range(warmup):
        out = step()
    if profile and lanes == 1:
        for net in nets:
            net.profile(True)
    ctx.sync_all()
    t0 = time.perf_counter()
    for i in range(steps):
        if capture is not None and i == steps - 1:
            capture["on"] = True
        out = step()
    ctx.sync_all()
    elapsed = ctx.max_over_ranks(time.perf_counter() - t0)
    if capture is not None:
        capture["on"] = False
    if not profile:
        return elapsed, None, out
    if lanes > 1:
        os.environ["MI355_LANES"] = "1"
        try:
            step()   # (arena of the caller's stream grows here, outside any timed region)
            for net in nets:
                net.profile(True)
            ctx.sync_all()
            step()
            ctx.sync_all()
        finally:
            os.environ["MI355_LANES"] = str(lanes)
    prof = {}
    for net in nets:
        for e in net.read_profile():
            p = prof.setdefault(e["name"], dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            for k in ("launches", "ms", "flops", "bytes"):
                p[k] += e[k]
        net.profile(False)
    return elapsed, prof, out


def roofline_of(prof, dtype, section):
    """Roofline of the kernel with the largest summed HIP-event time over the timed region.  `section`: the workload key of
    the committed counter passes ("config2_f32", "config3_f16", "config3_f32") or None when no pass exists for this workload."""
    dom_name, dom = max(prof.items(), key=lambda kv: kv[1]["ms"])
    avg_ms = dom["ms"] / dom["launches"]
    achieved = dom["flops"] / dom["launches"] / (avg_ms * 1e-3) / 1e12
    traffic = traffic_source = traffic_stale = None
    clock = clock_source = clock_stale = None
    if section:
        # (not measured in this run: the committed rocprofv3 --pmc passes of the same command on the same launch sizes)
        traffic, traffic_stale = committed_counter("pmc_traffic.json", section, dom_name, "hbm_bytes_per_launch")
        if traffic is not None:
            traffic_source = ("profiles/pmc_traffic.json (committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload, "
                              "tools/collect_profiles.sh; traffic_stale = the pass was taken on a library built from other sources)")
        # The clock the chip granted this kernel (DVFS), from the committed GRBM_GUI_ACTIVE passes of the same command: the nominal
        # peaks are quoted at 2.4 GHz, a power-limited MFMA kernel runs well below it.
        clock, clock_stale = committed_counter("kernel_clocks.json", section, dom_name, "shader_clock_ghz")
        if clock is not None:
            clock_source = "profiles/kernel_clocks.json (committed rocprofv3 --pmc GRBM_GUI_ACTIVE pass of this workload / dispatch durations, tools/kernel_clocks.py)"
    peak = PEAK_F32_MFMA_TFLOPS if dtype == "f32" else PEAK_F16_MFMA_TFLOPS
    ratio = EXECUTED_RATIO.get(dom_name, 1.0)
    conv_ms = sum(v["ms"] for k, v in prof.items() if v["flops"] > 0)
    conv_flops = sum(v["flops"] for v in prof.values())
    # `achieved` = algorithmic flops per launch / measured launch time (the contract's definition).  A Winograd kernel EXECUTES
    # fewer multiplies than that count (executed_flop_ratio < 1), so achieved / peak can exceed 1: the fraction the line leads with
    # (`frac`) is the executed one - what the matrix pipe actually did against its peak - and the algorithmic ratio is kept as
    # `frac_algorithmic`.
    return dict(bound="mfma", kernel=dom_name, achieved=round(achieved, 2), peak=peak, unit="TFLOP/s",
                frac=round(achieved * ratio / peak, 4), frac_algorithmic=round(achieved / peak, 4),
                achieved_executed=round(achieved * ratio, 2),
                traffic=traffic, traffic_source=traffic_source, traffic_stale=traffic_stale,
                executed_flop_ratio=round(ratio, 4),
                frac_executed=round(achieved * ratio / peak, 4), launches=dom["launches"], avg_launch_ms=round(avg_ms, 4),
                shader_clock_ghz=clock, shader_clock_source=clock_source, shader_clock_stale=clock_stale,
                frac_executed_at_that_clock=round(achieved * ratio / (peak * clock / NOMINAL_CLOCK_GHZ), 4) if clock else None,
                algorithmic_gflop_per_launch=round(dom["flops"] / dom["launches"] / 1e9, 3),
                algorithmic_mb_per_launch=round(dom["bytes"] / dom["launches"] / 1e6, 2),
                time_share=round(dom["ms"] / sum(p["ms"] for p in prof.values()), 4),
                # all conv / transposed-conv launches of the timed region together: algorithmic flops / their summed time
                conv_stages_frac=round(conv_flops / (conv_ms * 1e-3) / 1e12 / peak, 4) if conv_ms > 0 else None)


def kernel_table(prof):
    return {k: dict(launches=v["launches"], ms_total=round(v["ms"], 3),
                    tflops=round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 else None,
                    gbs=round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) if v["ms"] > 0 else None)
            for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}


PROB_SAMPLE = 1 << 20           # --dump-outputs: probabilities kept per ensemble member (configs 2 / 3)
CASE_LABEL_BUDGET = 12 << 20    # --dump-outputs: label voxels kept over all cases of config 4
DUMP_LIMIT_BYTES = 64 << 20


def seeded_sample(t, k, seed):
    """A fixed, seeded sample of k entries of the flattened tensor `t` (positions drawn without replacement and sorted), float32."""
    import torch
    n = t.numel()
    idx = np.sort(np.random.RandomState(seed).choice(n, min(k, n), replace=False))
    return t.reshape(-1)[torch.from_numpy(idx).to(t.device)].float().cpu().numpy()


def dump_outputs(dirname, arrays):
    """--dump-outputs: each array as float32 DIR/<name>.npy."""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(dirname, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), a)


def first_tile(data, steps_tbl):
    """The first 128^3 tile of the sliding window (zero-padded like the tiler pads), [1, C, 128, 128, 128]."""
    import torch
    z0, y0, x0 = steps_tbl[0][0], steps_tbl[1][0], steps_tbl[2][0]
    tile = data[:, z0:z0 + PATCH[0], y0:y0 + PATCH[1], x0:x0 + PATCH[2]]
    pad = [PATCH[i] - tile.shape[1 + i] for i in range(3)]
    return torch.nn.functional.pad(tile, (0, pad[2], 0, pad[1], 0, pad[0]))[None].contiguous()


class CpuOracle:
    """The CPU oracle (oracle/unet_ref.py, torch-CPU fp32) on a real tile of the timed volume: its timed forwards are
    the `cpu_baseline`, their outputs the parity reference for every GPU configuration of this run."""

    def __init__(self, tile):
        self.x = tile.cpu()
        self.logits = {}     # (name, seed) -> logits of the first tile
        self.seconds = {}    # name -> (seconds per forward on all cores, forwards timed)
        self.seconds_8t = None
        self.cores = None

    def forward(self, name, seed, min_forwards=1, budget_s=0.0):
        import torch
        from brats_amd import synthetic
        from oracle import unet_ref
        if (name, seed) in self.logits:
            return self.logits[(name, seed)]
        sd, meta = synthetic.make_model(name, seed=seed)
        cfg = unet_ref.default_cfg(norm=meta["norm"], num_groups=meta["num_groups"])
        if not self.logits:
            unet_ref.unet_forward(sd, self.x[:, :, :64, :64, :64], cfg)  # page in
        timed = min_forwards > 1 or budget_s > 0
        all_threads = torch.get_num_threads()
        if self.cores is None:
            self.cores = all_threads
        # the TIMED forwards (cpu_baseline) use every core the host gives torch, as SURVEY.md 8d asks; the forwards that only serve
        # as parity references run with 16 threads - on the 128-core GPU box torch's conv3d is faster that way (2.1 s against 3.9 s)
        if not timed and all_threads > 16:
            torch.set_num_threads(16)
        try:
            n, t0 = 0, time.perf_counter()
            while n < min_forwards or (time.perf_counter() - t0 < budget_s and n < 6):
                out = unet_ref.unet_forward(sd, self.x, cfg)
                n += 1
            if timed:
                self.seconds[name] = ((time.perf_counter() - t0) / n, n)
            elif name not in self.seconds:
                self.seconds[name] = ((time.perf_counter() - t0) / n, 0)   # (0 timed forwards: a parity run, 16 threads)
        finally:
            torch.set_num_threads(all_threads)
        self.logits[(name, seed)] = out
        return out

    def time_threads(self, name, seed, threads):
        """The same forward with torch.set_num_threads(threads): 8 relates the GPU box's host to the survey box (4.72 s
        per model-A patch at 8 threads), 16 is where torch's conv3d is fastest on the 128-core GPU box."""
        import torch
        from brats_amd import synthetic
        from oracle import unet_ref
        sd, meta = synthetic.make_model(name, seed=seed)
        cfg = unet_ref.default_cfg(norm=meta["norm"], num_groups=meta["num_groups"])
        before = torch.get_num_threads()
        torch.set_num_threads(threads)
        try:
            unet_ref.unet_forward(sd, self.x[:, :, :64, :64, :64], cfg)
            t0 = time.perf_counter()
            unet_ref.unet_forward(sd, self.x, cfg)
            dt = time.perf_counter() - t0
        finally:
            torch.set_num_threads(before)
        if threads == 8:
            self.seconds_8t = dt
        return dt


def cpu_model_string():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def parity_block(got_logits, ref_logits, sample):
    import torch
    from oracle import tiler_ref
    pr, pg = torch.sigmoid(ref_logits)[0].numpy(), torch.sigmoid(got_logits)[0].numpy()
    d = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(pg), tiler_ref.regions_to_labels(pr))
    return dict(sample=sample, max_abs_prob_err=float(np.abs(pg - pr).max()),
                max_abs_logit_err=float((got_logits - ref_logits).abs().max()), logit_std=float(ref_logits.std()),
                dice_wt_tc_et_mean=round(d["mean"], 6))


def parity_probs_block(got, ref, sample):
    from oracle import tiler_ref
    lg, lr = tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(ref)
    d = tiler_ref.brats_region_dice(lg, lr)
    return dict(sample=sample, max_abs_prob_err=float(np.abs(got - ref).max()), labels_differ=int((lg != lr).sum()),
                voxels=int(lr.size), dice_wt_tc_et_mean=round(d["mean"], 6))


def run_single_volume(ctx, args, config, dtype, steps, warmup, data, props, steps_tbl, oracle=None, folds=1, tiles_mode=False,
                      profile=True, dump=False):
    """configs 2 / 3: one volume per rank per step.  Returns the result dict (without the top-level contract keys); with `dump`,
    "_outputs" holds the arrays of the last timed step (--dump-outputs)."""
    from brats_amd import predictor, ops, parallel
    wl = WORKLOADS[config]
    members = [build_nets([(name, seed + k) for k in range(folds)], dtype) for name, seed in wl["models"]]   # [member][fold]
    nets = [n for m in members for n in m]
    full = props["original_size_of_raw_data"]
    lo = [b[0] for b in props["crop_bbox"]]
    n_tiles = int(np.prod([len(s) for s in steps_tbl]))
    n_mirrors = 8 if wl["tta"] else 1
    flops_per_volume = sum(n.flops(PATCH) for n in nets) * n_tiles * n_mirrors
    capture = {"on": False} if dump else None

    def step():
        if tiles_mode:   # partitioning B: this rank's (fold, tile) items, ONE exchange per member, identical result on every rank
            all_probs = [parallel.predict_case_tile_sharded(fold_nets, data, PATCH, 0.5, wl["tta"], (0, 1, 2), True, "sigmoid") for fold_nets in members]
        else:            # (the ensemble members of one case: the lanes of predictor.predict_members take them in staggered order)
            all_probs = predictor.predict_members(members, data, PATCH, 0.5, wl["tta"], (0, 1, 2), True, "sigmoid", batch_tiles=args.batch_tiles)
        if capture is not None and capture["on"]:
            capture["probs"] = all_probs
        segs = [ops.regions_to_labels(probs, (1, 2, 3), lo, full) for probs in all_probs]
        return segs[0] if len(segs) == 1 else ops.label_ensemble(segs[0], segs[1])

    elapsed, prof, seg = timed_region(ctx, step, steps, warmup, nets, profile, capture)
    res = dict(dtype=dtype, steps=steps, warmup=warmup, ms_per_step=round(elapsed / steps * 1e3, 3),
               volumes_per_s=round((1 if tiles_mode else ctx.world) * steps / elapsed, 4),
               config={"workload": wl["name"] + (f" [{folds} folds per member]" if folds != 1 else ""), "patch": list(PATCH),
                       "tiles_per_volume": n_tiles, "mirrors": n_mirrors, "folds_per_member": folds,
                       "models": [m[0] for m in wl["models"]], "crop": list(data.shape[1:]),
                       "lanes": (1 if tiles_mode else predictor.default_lanes()),   # HIP streams per predict_folds call (predictor.py)
                       "sharding": ("tiles: ONE volume per step, the (fold, tile) work list of each ensemble member dealt round-robin over the "
                                    "ranks, one RCCL all_gather of the partial aggregates per member, rank-ordered sum (SURVEY.md 8e B)")
                                   if tiles_mode else "cases (one volume per rank per step)",
                       "tflop_per_volume": round(flops_per_volume / 1e12, 3)},
               sustained_tflops_per_gpu=round(flops_per_volume * steps / elapsed / 1e12 / (ctx.world if tiles_mode else 1), 2),
               roofline=None if prof is None else
               roofline_of(prof, dtype, None if (args.batch_tiles or args.folds != 1 or tiles_mode) else f"config{config}_{dtype}"),
               kernels=None if prof is None else kernel_table(prof),
               label_histogram=ctx.torch.bincount(seg.flatten().to(ctx.torch.int64), minlength=4).tolist(),
               speedup_vs_nominal_5min=round(300.0 / (elapsed / steps), 1))
    res["_flops_per_volume"] = flops_per_volume
    res["_elapsed"] = elapsed
    if dump:
        res["_outputs"] = dict(labels=seg.cpu().numpy())
        for (name, _), probs in zip(wl["models"], capture["probs"]):
            res["_outputs"][f"probabilities_{name}"] = seeded_sample(probs, PROB_SAMPLE, seed=0)
    if oracle is not None and ctx.rank == 0:
        tile = first_tile(data, steps_tbl)
        par = {}
        for (name, seed), fold_nets in zip(wl["models"], members):
            ref = oracle.forward(name, seed)
            par[name] = parity_block(fold_nets[0](tile).cpu(), ref, f"first 128^3 tile of the timed volume, model {name} {dtype} GPU forward vs the CPU oracle forward")
        res["parity_vs_cpu_ref"] = par if len(par) > 1 else next(iter(par.values()))
    for n in nets:
        n.close()
    return res


REFERENCE_FOLDS = 5  # run_brats2021_inference_singlethread.py:161 folds=(0, 1, 2, 3, 4)


def run_reference_setting(ctx, dtype, data, props, steps_tbl, oracle=None, steps=3):
    """The reference's own per-case setting as ONE workload (run_brats2021_inference_singlethread.py:161,208-211,263-264):
    two models x five folds x 8-way mirror TTA, fold-mean probabilities per model (:128), region labels, label-round
    ensemble (:305).  Synthetic folds: seeds 7..11 (model A) and 8..12 (model B).  One untimed step (arena growth, first
    launches), then `steps` timed steps.  Parity leg (rank 0, when the CPU oracle runs): per ensemble member the FOLD MEAN on
    the first 128^3 tile of the timed volume (predict_folds on that tile, the five folds, no mirrors) against np.mean of the
    five CPU-oracle forwards (driver :128), under the same exit-3 gate as every other parity block."""
    from brats_amd import predictor, ops
    torch = ctx.torch
    models = [[("A", 7 + k) for k in range(REFERENCE_FOLDS)], [("B", 8 + k) for k in range(REFERENCE_FOLDS)]]
    nets = [build_nets(m, dtype) for m in models]
    full = props["original_size_of_raw_data"]
    lo = [b[0] for b in props["crop_bbox"]]
    n_tiles = int(np.prod([len(s) for s in steps_tbl]))
    flops = sum(n.flops(PATCH) for folds in nets for n in folds) * n_tiles * 8

    def step():
        segs = [ops.regions_to_labels(probs, (1, 2, 3), lo, full)
                for probs in predictor.predict_members(nets, data, PATCH, 0.5, True, (0, 1, 2), True, "sigmoid")]
        return ops.label_ensemble(segs[0], segs[1])

    step()
    torch.cuda.synchronize(ctx.device)
    t0 = time.perf_counter()
    for _ in range(steps):
        seg = step()
    torch.cuda.synchronize(ctx.device)
    dt = (time.perf_counter() - t0) / steps
    res = dict(workload="the reference's per-case setting: models A + B x 5 folds each x 8-way mirror TTA, fold mean, region "
                        "labels, label-round ensemble (run_brats2021_inference_singlethread.py:161,208-211,263-264)",
               dtype=dtype, steps=steps, warmup=1, forwards_per_volume=2 * REFERENCE_FOLDS * n_tiles * 8,
               seconds_per_volume=round(dt, 3), volumes_per_s=round(1.0 / dt, 4), tflop_per_volume=round(flops / 1e12, 1),
               sustained_tflops_per_gpu=round(flops / dt / 1e12, 1), speedup_vs_nominal_5min=round(300.0 / dt, 1),
               label_histogram=torch.bincount(seg.flatten().to(torch.int64), minlength=4).tolist())
    if oracle is not None:
        tile = first_tile(data, steps_tbl)
        par = {}
        for member, folds in zip(models, nets):
            ref = np.mean([torch.sigmoid(oracle.forward(name, seed))[0].numpy() for name, seed in member], axis=0)   # driver :128
            got = predictor.predict_folds(folds, tile[0], PATCH, 0.5, False, (0, 1, 2), True, "sigmoid").cpu().numpy()
            par[member[0][0]] = parity_probs_block(got, ref, f"fold mean of the {REFERENCE_FOLDS} model-{member[0][0]} folds on the first 128^3 tile of the "
                                                             f"timed volume (no mirrors), {dtype} GPU vs np.mean of {REFERENCE_FOLDS} CPU-oracle forwards")
        res["parity_vs_cpu_ref"] = par
    res["_seg"] = seg
    for folds in nets:
        for n in folds:
            n.close()
    return res


def run_end_to_end(ctx, raw, steps=3):
    """Host float32 volume -> H2D -> crop mask + bbox -> masked z-score -> sliding window (config 2) -> labels -> D2H."""
    from brats_amd import preprocessing, predictor, ops
    nets = build_nets(WORKLOADS[2]["models"], "f32")
    torch = ctx.torch

    def once():
        t = [time.perf_counter()]
        data, props = preprocessing.preprocess_case(raw, ctx.device)
        torch.cuda.synchronize(ctx.device)
        t.append(time.perf_counter())
        probs = predictor.predict_folds(nets, data, PATCH, 0.5, False, (0, 1, 2), True, "sigmoid")
        seg = ops.regions_to_labels(probs, (1, 2, 3), [b[0] for b in props["crop_bbox"]], props["original_size_of_raw_data"])
        torch.cuda.synchronize(ctx.device)
        t.append(time.perf_counter())
        host = seg.cpu()
        t.append(time.perf_counter())
        return [b - a for a, b in zip(t[:-1], t[1:])], host

    once()
    parts = np.array([once()[0] for _ in range(steps)])
    m = parts.mean(0)
    for n in nets:
        n.close()
    return dict(workload="config 2 from a host fp32 [4,155,240,240] array to a host uint8 label volume (PCIe-inclusive; never `value`)",
                steps=steps, ms_total=round(float(m.sum()) * 1e3, 2), ms_h2d_crop_zscore=round(float(m[0]) * 1e3, 2),
                ms_predict_labels=round(float(m[1]) * 1e3, 2), ms_labels_d2h=round(float(m[2]) * 1e3, 2),
                volumes_per_s=round(1.0 / float(m.sum()), 3))


def run_config4(ctx, args, dtype):
    """BASELINE.json configs[3]: the batch is fixed (32 volumes), ranks take cases round-robin; a step = the batch."""
    from brats_amd import synthetic, preprocessing, parallel
    wl = WORKLOADS[4]
    n_cases = args.cases or wl["n_cases"]
    nets = build_nets(wl["models"], dtype)
    # cost of every case in tiles (host-side bounding box of the raw volume; each rank looks at a round-robin share and the
    # counts are exchanged - bookkeeping outside the timed region), then longest-first assignment (parallel.shard_cases)
    raws = {i: synthetic.make_volume(seed=1000 + i) for i in parallel.shard_cases(n_cases, ctx.rank, ctx.world)}
    weights = [0.0] * n_cases
    for i, raw in raws.items():
        weights[i] = float(parallel.tiles_of_shape(preprocessing.nonzero_crop_shape(raw), PATCH, 0.5))
    if ctx.use_dist:
        dev = ctx.device if ctx.backend == "nccl" else "cpu"
        wt = ctx.torch.tensor(weights, dtype=ctx.torch.float64, device=dev)
        ctx.dist.all_reduce(wt)
        weights = [float(v) for v in wt.tolist()]
    mine = parallel.shard_cases(n_cases, ctx.rank, ctx.world, weights)
    cases = [None] * n_cases
    for i in mine:  # every rank generates and preprocesses only its own shard, outside the timed region
        raw = raws.pop(i) if i in raws else synthetic.make_volume(seed=1000 + i)
        cases[i] = preprocessing.preprocess_case(raw, ctx.device)
    raws.clear()
    tiles = mirrors = 0
    flops_batch = 0
    from brats_amd import ops
    for i in range(n_cases):
        if cases[i] is None:
            continue
        shp = cases[i][0].shape[1:]
        nt = int(np.prod([len(ops.compute_steps(PATCH[a], max(PATCH[a], shp[a]), 0.5)) for a in range(3)]))
        flops_batch += sum(n.flops(PATCH) for n in nets) * nt * 8
        tiles += nt
    if ctx.use_dist:  # host-side bookkeeping only (not in the timed region, not on the data path)
        dev = ctx.device if ctx.backend == "nccl" else "cpu"
        t = ctx.torch.tensor([float(flops_batch), float(tiles)], dtype=ctx.torch.float64, device=dev)
        ctx.dist.all_reduce(t)
        flops_batch, tiles = float(t[0].item()), int(t[1].item())

    def step():
        return parallel.predict_cases_sharded([[n] for n in nets], cases, ctx.rank, ctx.world, PATCH, 0.5, True, weights=weights)

    elapsed, prof, segs = timed_region(ctx, step, args.steps, args.warmup, nets, args.full)
    if args.dump_outputs:   # (each rank writes the cases it owns)
        k = CASE_LABEL_BUDGET // n_cases
        dump_outputs(args.dump_outputs, {f"labels_case{i:03d}": seeded_sample(seg, k, seed=i) for i, seg in segs.items()})
    hist = None
    if segs:
        first = segs[min(segs)]
        hist = ctx.torch.bincount(first.flatten().to(ctx.torch.int64), minlength=4).tolist()
    return dict(value=n_cases * args.steps / elapsed, elapsed=elapsed, scaling="strong", dtype=dtype,
                config={"workload": wl["name"], "patch": list(PATCH), "cases": n_cases, "cases_per_rank": len(mine),
                        "tiles_in_batch": tiles, "mirrors": 8, "models": [m[0] for m in wl["models"]],
                        "sharding": "cases longest-first (tile count) onto the least loaded rank, no data-path collective",
                        "tflop_per_batch": round(flops_batch / 1e12, 2)},
                sustained=flops_batch * args.steps / elapsed / 1e12 / ctx.world,
                roofline=None if prof is None else roofline_of(prof, dtype, None), kernels=None if prof is None else kernel_table(prof),
                label_histogram=hist)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.lanes > 0:
        os.environ["MI355_LANES"] = str(args.lanes)   # (before the self-launch: the ranks inherit it)
    maybe_self_launch(args, argv)

    import torch  # noqa: F401  (first GPU-capable import happens only here, after the self-launch decision)
    from brats_amd import synthetic, preprocessing, ops

    ctx = Ctx(args)
    dtype = args.dtype or WORKLOADS[args.config]["dtype"]

    if args.config == 4:
        r = run_config4(ctx, args, dtype)
        if ctx.rank == 0:
            print(json.dumps({
                "metric": "BraTS volumes/sec (4-modality 240x240x155)", "value": round(r["value"], 4), "unit": "volumes/s",
                "n_gpus": ctx.world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(r["elapsed"] / args.steps * 1e3, 3), "higher_is_better": True, "scaling": r["scaling"],
                "vs_baseline": None, "dtype": dtype, "data": "synthetic", "config": r["config"],
                "sustained_tflops_per_gpu": round(r["sustained"], 2), "roofline": r["roofline"], "cpu_baseline": None,
                "kernels": r["kernels"], "label_histogram": r["label_histogram"]}))
        ctx.close()
        return

    tiles_mode = args.shard == "tiles"
    if tiles_mode and args.config != 3:
        raise SystemExit("--shard tiles is the single-case latency mode of config 3 (SURVEY.md 8e partitioning B)")
    raw = synthetic.make_volume(seed=1000 + (0 if tiles_mode else ctx.rank))   # tiles mode: every rank works on the SAME case
    data, props = preprocessing.preprocess_case(raw, ctx.device)
    steps_tbl = [ops.compute_steps(PATCH[a], max(PATCH[a], data.shape[1 + a]), 0.5) for a in range(3)]
    want_cpu = args.full and not args.no_cpu_baseline and ctx.world == 1
    oracle = CpuOracle(first_tile(data, steps_tbl)) if (want_cpu and ctx.rank == 0) else None
    cpu = None
    if oracle is not None:
        name, seed = WORKLOADS[args.config]["models"][0]
        oracle.forward(name, seed, min_forwards=2, budget_s=10.0)  # >= 2 timed forwards, about 10 s of CPU work

    main_res = run_single_volume(ctx, args, args.config, dtype, args.steps, args.warmup, data, props, steps_tbl, oracle,
                                 folds=args.folds, tiles_mode=tiles_mode, profile=args.full,
                                 dump=bool(args.dump_outputs) and ctx.rank == 0)
    flops_per_volume, elapsed = main_res.pop("_flops_per_volume"), main_res.pop("_elapsed")
    if "_outputs" in main_res:   # (rank 0: in cases mode every rank has a volume of its own, in tiles mode they all hold the same)
        dump_outputs(args.dump_outputs, main_res.pop("_outputs"))

    secondary = None
    if args.full and args.config == 2 and dtype == "f32" and ctx.world == 1 and not args.no_secondary and not args.batch_tiles and args.folds == 1:
        # BASELINE.json configs[2] under the same clock and the same oracle tile (3 steps each), and the PCIe-inclusive leg
        secondary = {}
        for dt in ("f16", "f32"):
            r = run_single_volume(ctx, args, 3, dt, 3, 1, data, props, steps_tbl, oracle)
            r.pop("_flops_per_volume"); r.pop("_elapsed")
            secondary[f"config3_{dt}"] = r
        secondary["end_to_end"] = run_end_to_end(ctx, raw)
        if not args.no_reference_setting:
            ref = {dt: run_reference_setting(ctx, dt, data, props, steps_tbl, oracle) for dt in ("f16", "f32")}
            # the fp16 label volume against the fp32 label volume of the same run, all 155 x 240 x 240 voxels (a consistency check of
            # the two paths of this library through its own evaluator kernel; the oracle's verdict on each is the fold-mean parity
            # block above).  Raw nnU-Net labels: WT = {1, 2, 3}, TC = {2, 3}, ET = {3}.
            from brats_amd import evaluate
            seg16, seg32 = ref["f16"].pop("_seg"), ref["f32"].pop("_seg")
            cm = evaluate.confusion(seg16, seg32, 5).astype(np.float64)   # rows = fp16 label, columns = fp32 label
            dices = []
            for members in ((1, 2, 3), (2, 3), (3,)):
                m = list(members)
                tp = cm[np.ix_(m, m)].sum()
                dices.append((2 * tp + 1e-8) / (cm[m, :].sum() + cm[:, m].sum() + 1e-8))
            ref["f16"]["consistency_vs_f32_labels"] = dict(sample="ensembled label volume of the timed case, fp16 path vs fp32 path of this run, all voxels",
                                                            labels_differ=int(cm.sum() - np.trace(cm)), voxels=int(cm.sum()),
                                                            dice_wt_tc_et_mean=round(float(np.mean(dices)), 6))
            secondary["reference_setting"] = ref

    if ctx.rank != 0:
        ctx.close()
        return

    if oracle is not None:
        from brats_amd import network as _net
        name, seed = WORKLOADS[args.config]["models"][0]
        per_fw, n_fw = oracle.seconds[name]
        sd, _ = synthetic.make_model(name, seed=seed)
        flops_model0 = _net.topology_from_state_dict(sd).conv_flops(PATCH)
        cfgd = main_res["config"]
        # cpu_baseline.value = the BEST CPU configuration timed (all 128 cores of the GPU box are slower than 8 or 16
        # threads for torch's conv3d), with the all-core figure SURVEY.md 8d asks for beside it as flat keys
        timed = {int(oracle.cores): per_fw}
        for th in (8, 16):
            if th < oracle.cores:
                timed[th] = oracle.time_threads(name, seed, th)
        best = min(timed, key=timed.get)
        scale = flops_per_volume / flops_model0
        est_volume_s = timed[best] * scale
        cpu = dict(value=round(1.0 / est_volume_s, 6), unit="volumes/s", cores=best, kind="port", cpu_model=cpu_model_string(),
                   host_logical_cpus=os.cpu_count(), forward_s=round(timed[best], 2),
                   all_cores=int(oracle.cores), all_cores_forward_s=round(per_fw, 2), all_cores_value=round(1.0 / (per_fw * scale), 6),
                   sample=f"model {name} on the first 1x4x128^3 tile of the timed volume with the torch-CPU fp32 oracle: {n_fw} forwards on all "
                          f"{oracle.cores} threads ({per_fw:.2f} s each)" + "".join(f", one on {th} threads ({timed[th]:.2f} s)" for th in sorted(timed) if th != oracle.cores) +
                          f"; value = the fastest of these ({best} threads), scaled by flops to the "
                          f"{cfgd['tiles_per_volume'] * cfgd['mirrors'] * len(cfgd['models'])} forwards of one volume",
                   seconds_per_volume_est=round(est_volume_s, 2))
        for th in (8, 16):
            if th in timed:
                cpu[f"threads_{th}_forward_s"] = round(timed[th], 2)
                cpu[f"threads_{th}_value"] = round(1.0 / (timed[th] * scale), 6)
        if "B" in oracle.seconds:
            cpu["model_B_forward_s_16_threads"] = round(oracle.seconds["B"][0], 2)

    out = {
        "metric": "BraTS volumes/sec (4-modality 240x240x155)", "value": main_res["volumes_per_s"], "unit": "volumes/s",
        "n_gpus": ctx.world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": main_res["ms_per_step"],
        "higher_is_better": True, "scaling": "strong" if tiles_mode else "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
        "config": main_res["config"], "sustained_tflops_per_gpu": main_res["sustained_tflops_per_gpu"],
        "roofline": main_res["roofline"], "cpu_baseline": cpu, "parity_vs_cpu_ref": main_res.get("parity_vs_cpu_ref"),
        "kernels": main_res["kernels"], "label_histogram": main_res["label_histogram"],
        "speedup_vs_nominal_5min": main_res["speedup_vs_nominal_5min"],
    }
    if secondary is not None:
        out["secondary"] = secondary
    print(json.dumps(out))
    ctx.close()
    # north_star gate: Dice of the GPU label map against the CPU oracle's on the same tile >= 0.999, for every parity block of
    # this run; the line above is printed either way, a miss makes the run fail (the bench asserted nothing)
    misses = []

    def gate(where, node):
        """Every dict that carries `dice_wt_tc_et_mean` anywhere below a parity / consistency key is gated."""
        if not isinstance(node, dict):
            return
        if "dice_wt_tc_et_mean" in node:
            if node["dice_wt_tc_et_mean"] < DICE_GATE:
                misses.append(f"{where}: Dice {node['dice_wt_tc_et_mean']} < {DICE_GATE}")
            return
        for k, v in node.items():
            gate(f"{where}/{k}", v)

    def walk(where, node):
        if not isinstance(node, dict):
            return
        for k, v in node.items():
            if k in ("parity_vs_cpu_ref", "consistency_vs_f32_labels"):
                gate(f"{where}/{k}", v)
            elif isinstance(v, dict) and k in ("secondary", "reference_setting", "config3_f16", "config3_f32", "f16", "f32"):
                walk(f"{where}/{k}", v)

    walk("", out)
    if misses:
        print("PARITY GATE MISSED: " + "; ".join(misses), file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
