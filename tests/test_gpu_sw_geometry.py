"""-m gpu: the sliding window off the cube and off step 0.5 - patches of three different extents, steps 0.25, 0.3, 0.75 and 1.0 -
through every sharing layer (csrc/sw_share_plan.hip, csrc/sliding_window.hip), against the per-tile path and the CPU oracle.  The
plans of these geometries are proved exactly in tests/test_*_plan_cpu.py and their tile tables in tests/test_sw_geometry_cpu.py;
here the kernels run on them.

The switches are read once per process, so each setting runs in a child process of its own, one after the other, each with its own
timeout, and its return code is asserted before the next one starts; the children write an .npz the parent compares.  The network
is the reduced model A of the sibling files (num_pool = 2, max_feat = 128, BatchNorm, fp32).

Gates - the project's own, none new:
  * against oracle/tiler_ref.predict_3d_tiled at the same patch, step and mirror axes: probabilities within 1e-3, region Dice >= 0.999
    (BASELINE.json north_star; test_gpu_stage0_sharing.py);
  * a sharing switch on against off: 5e-5 on probabilities, all values finite (test_gpu_stage0_sharing.py, test_gpu_skip_sharing.py,
    test_gpu_level1_sharing.py); the stage-0 views on against off: the same bits (test_gpu_stage0_views.py);
  * three ranks tile-sharded against unsharded, one tile per forward on both sides: 2e-6 (test_gpu_stage0_sharing.py);
  * batch_tiles = 1 against the default: 5e-5 (test_gpu_network.py);
  * fp16: the gates of test_gpu_network._check_logits_f16, on the aggregated logits (nonlin = identity).

Cases - the name says which axis order or step a failure belongs to:
  * small_zyx_32_48_64: patch (32, 48, 64) on (41, 100, 75), 2 x 4 x 2 tiles, odd origins, middle tiles along y;
    small_zyx_64_32_48_mirror_zx: the permuted patch on the permuted volume (75, 41, 100), mirror axes (0, 2);
  * step_025 / step_075 / step_100 / step_030: patch 32^3 on (41, 57, 43); step_025_mirror_zyx: 3 x 5 x 3 = 45 tiles x 8 mirrors,
    several forwards per lane and more merged-slab keys per launch group than any other test runs; step_025_f16;
  * mid: patch (48, 64, 96) on (59, 77, 107), 2 x 2 x 2 tiles at odd origins (11, 13, 11): 1152 conv tiles per sample, where the shared
    skip half and the views turn on (asserted through ops.skip_share_plan / ops.stage0_view_plan);
  * level1: patch (128, 128, 160) on (139, 172, 200): z per-origin (0, 11), y and x merged, MI355_SHARE_LEVEL1 = 2 against 0 only.  No
    CPU oracle here (eight 128 x 128 x 160 forwards take about a minute on the CPU): the off path is held to the oracle by the
    smaller cases, the plan by the exact proof in tests/test_level1_share_plan_cpu.py.
  * The weight map: cnt of predictor.predict_tile_sharded against the sum of tiler_ref.get_gaussian(patch) placed at the tile
    origins - the only direct check of gaussian_map off the cube."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import tiler_ref, unet_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER = "stage0_gather_kernel"
LEVEL1 = "stage0_gather_kernel level 1"   # the profile entry of the level-1 hand-off gather
P32 = (32, 32, 32)
V32 = (41, 57, 43)
# name: (patch, volume, step, mirror axes or None, seed of the volume)
SMALL = {"small_zyx_32_48_64": ((32, 48, 64), (41, 100, 75), 0.5, None, 80),
         "small_zyx_64_32_48_mirror_zx": ((64, 32, 48), (75, 41, 100), 0.5, (0, 2), 81)}
STEP = {"step_025": (P32, V32, 0.25, None, 82), "step_025_mirror_zyx": (P32, V32, 0.25, (0, 1, 2), 82), "step_075": (P32, V32, 0.75, None, 83),
        "step_100": (P32, V32, 1.0, None, 84), "step_030": (P32, V32, 0.3, None, 85)}
MID = {"mid": ((48, 64, 96), (59, 77, 107), 0.5, None, 86)}
L1 = {"level1": ((128, 128, 160), (139, 172, 200), 0.5, None, 87)}
TILES = {"small_zyx_32_48_64": (2, 4, 2), "small_zyx_64_32_48_mirror_zx": (2, 2, 4), "step_025": (3, 5, 3), "step_025_mirror_zyx": (3, 5, 3),
         "step_075": (2, 3, 2), "step_100": (2, 2, 2), "step_030": (2, 4, 3), "mid": (2, 2, 2), "level1": (2, 2, 2)}
# what the default-switch child runs on top of the plain prediction
EXTRA = {"sharded": ["small_zyx_32_48_64"], "batch1": ["small_zyx_32_48_64", "step_025"], "cnt": ["small_zyx_32_48_64", "step_025"],
         "f16": ["step_025"]}

CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
from brats_amd import predictor
path, cases, extra = sys.argv[1], eval(sys.argv[2]), eval(sys.argv[3])
out = {}
def vol_of(shape, seed):
    return np.random.RandomState(seed).standard_normal((4,) + tuple(shape)).astype(np.float32)
def run(net, vol, patch, step, axes, nonlin="sigmoid", **kw):
    return predictor.predict_folds([net], vol, patch, step, axes is not None, axes or (0, 1, 2), True, nonlin, **kw)
sd, meta = brats_amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
net = brats_amd.UNet(sd, norm="batch")
for name, (patch, shape, step, axes, seed) in sorted(cases.items()):
    vol = vol_of(shape, seed)
    net.profile(True)
    out[name] = run(net, vol, patch, step, axes).cpu().numpy()
    prof = net.read_profile()
    net.profile(False)
    out[name + "_kernels"] = np.array([e["name"] for e in prof])
    out[name + "_bytes"] = np.array([e["bytes"] for e in prof])
    if name in extra.get("batch1", ()) or name in extra.get("sharded", ()):
        out[name + "_b1"] = run(net, vol, patch, step, axes, batch_tiles=1).cpu().numpy()
    if name in extra.get("sharded", ()):   # one tile per forward on both sides, as tests/test_gpu_stage0_sharing.py
        parts = [predictor.predict_tile_sharded(net, vol, r, 3, patch, step, False, batch_tiles=1) for r in range(3)]
        agg = parts[0][0].clone()
        for r in (1, 2):
            agg += parts[r][0]
        out[name + "_sharded"] = predictor.finish_sharded(agg, parts[0][1], vol.shape[1:], patch).cpu().numpy()
    if name in extra.get("cnt", ()):
        out[name + "_cnt"] = predictor.predict_tile_sharded(net, vol, 0, 1, patch, step, False)[1].cpu().numpy()
if extra.get("f16"):
    net16 = brats_amd.UNet(sd, norm="batch", dtype="f16")
    for name in extra["f16"]:
        patch, shape, step, axes, seed = cases[name]
        out[name + "_f16"] = run(net16, vol_of(shape, seed), patch, step, axes, nonlin="identity").cpu().numpy()
np.savez(path, **out)
"""


def _child(td, tag, cases, env, extra=None):
    path = os.path.join(td, tag + ".npz")
    res = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, repr(cases), repr(extra or {})], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(amd, gpu):
    """(default switches, MI355_SHARE_STAGE0 = 0): the small and the step cases; the default child also runs mid and the extras."""
    with tempfile.TemporaryDirectory() as td:
        on = _child(td, "on", {**SMALL, **STEP, **MID}, {}, EXTRA)
        off = _child(td, "off", {**SMALL, **STEP}, {"MI355_SHARE_STAGE0": "0"})
    return on, off


@pytest.fixture(scope="module")
def mid_runs(amd, gpu, runs):
    with tempfile.TemporaryDirectory() as td:
        no_skip = _child(td, "noskip", MID, {"MI355_SHARE_SKIP_CONV": "0"})
        no_views = _child(td, "noviews", MID, {"MI355_STAGE0_VIEWS": "0"})
    return runs[0], no_skip, no_views


@pytest.fixture(scope="module")
def level1_runs(amd, gpu):
    with tempfile.TemporaryDirectory() as td:
        on = _child(td, "l2", L1, {"MI355_SHARE_LEVEL1": "2"})
        off = _child(td, "l0", L1, {"MI355_SHARE_LEVEL1": "0"})
    return on, off


def _volume(shape, seed):
    return np.random.RandomState(seed).standard_normal((4,) + tuple(shape)).astype(np.float32)


@pytest.fixture(scope="module")
def oracle(amd):
    """One oracle prediction per case, shared by every comparison of that case."""
    sd, meta = amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
    fn = tiler_ref.make_net_fn(sd, unet_ref.default_cfg("batch"))
    refs = {}
    for name, (patch, shape, step, axes, seed) in {**SMALL, **STEP, **MID}.items():
        refs[name] = tiler_ref.predict_3d_tiled(fn, _volume(shape, seed), patch, 3, step, axes is not None, axes or (0, 1, 2), True, "sigmoid")
    for name in EXTRA["f16"]:
        patch, shape, step, axes, seed = STEP[name]
        refs[name + "_logits"] = tiler_ref.predict_3d_tiled(fn, _volume(shape, seed), patch, 3, step, axes is not None, axes or (0, 1, 2), True, "identity")
    return refs


def _kernels(run, name):
    return [str(k) for k in run[name + "_kernels"]]


def _against_oracle(tag, name, got, ref):
    err = float(np.abs(got - ref).max())
    dice = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(ref))["mean"]
    print(f"PARITY sw-geometry {name} {tag} vs oracle: max |dprob| {err:.2e}, Dice {dice:.6f}")
    assert err <= 1e-3 and dice >= 0.999, (name, tag)


def test_the_geometry_of_the_cases(amd):
    """The tile counts the names promise, odd origins, and the plans the cases are meant to run on."""
    for name, (patch, shape, step, axes, _) in {**SMALL, **STEP, **MID, **L1}.items():
        p = amd.ops.stage0_plan(shape, patch, step, axes or (), 2)
        origins = [sorted({s["origin"][a] for s in p["samples"] if s["mirror"] == ()}) for a in range(3)]
        assert tuple(len(o) for o in origins) == TILES[name] and p["shared"], (name, origins)
        assert any(o % 2 for a in range(3) for o in origins[a]), (name, origins)
        assert np.prod(shape) < (6e6 if name == "level1" else 1.2e6)
    patch, shape, step, axes, _ = MID["mid"]
    assert (patch[0] // 4) * (patch[1] // 8) * (patch[2] // 8) == 1152
    assert amd.ops.skip_share_plan(shape, patch, step)["skip_shared"] and amd.ops.stage0_view_plan(shape, patch, step)["half_viewed"]
    for name in list(SMALL) + list(STEP):   # below the threshold of the addend kernel: the shared stage 0 and the merged slabs alone
        patch, shape, step, axes, _ = {**SMALL, **STEP}[name]
        assert not amd.ops.skip_share_plan(shape, patch, step, axes or ())["skip_shared"], name
    m = amd.ops.stage0_merge_plan(V32, P32, 0.25, (0, 1, 2), 2, False)
    assert m["n_tiles"] == 45 and m["n_mirrors"] == 8 and m["n_slabs"][1] == 8 * 2 * 4 * 3 and m["n_slabs"][2] == 8 * 2 * 2
    patch, shape, step, axes, _ = L1["level1"]
    l1 = amd.ops.level1_share_plan(shape, patch, step, mode=2, num_pool=2)
    assert l1["on"] and l1["merged"] == (False, True, True) and len(l1["regions"]) == 2


@pytest.mark.parametrize("name", sorted({**SMALL, **STEP}))
def test_shared_stage0_matches_per_tile_and_oracle(runs, oracle, name):
    on, off = runs
    assert GATHER in _kernels(on, name) and GATHER not in _kernels(off, name), _kernels(on, name)
    d = float(np.abs(on[name] - off[name]).max())
    print(f"PARITY sw-geometry {name}: sharing on vs off {d:.2e}")
    assert np.isfinite(on[name]).all() and np.isfinite(off[name]).all() and d <= 5e-5
    _against_oracle("on", name, on[name], oracle[name])
    _against_oracle("off", name, off[name], oracle[name])


def test_tile_sharded_matches_unsharded(runs):
    for name in EXTRA["sharded"]:
        d = float(np.abs(runs[0][name + "_sharded"] - runs[0][name + "_b1"]).max())
        print(f"PARITY sw-geometry {name}: 3 ranks vs unsharded {d:.2e}")
        assert d <= 2e-6, name


@pytest.mark.parametrize("name", EXTRA["batch1"])
def test_one_tile_per_forward_matches_the_default(runs, name):
    d = float(np.abs(runs[0][name + "_b1"] - runs[0][name]).max())
    print(f"PARITY sw-geometry {name}: batch_tiles=1 vs default {d:.2e}")
    assert d <= 5e-5


def test_step_025_f16(runs, oracle):
    from test_gpu_network import _check_logits_f16
    _check_logits_f16(runs[0]["step_025_f16"][None], oracle["step_025_logits"][None])


@pytest.mark.parametrize("name", EXTRA["cnt"])
def test_weight_map(runs, name):
    """cnt = the sum over the tiles of the Gaussian map of the patch, placed at the tile origins.  The bound is derived: each term
    is the fp32 rounding of a double computed two ways that agree far below an fp32 ulp, so the terms differ by at most one
    rounding, 2^-23 relative; the device sums the k terms that cover a voxel in fp32, k - 1 more roundings of at most 2^-24 of a
    partial sum that never exceeds cnt: together at most (k + 1) * 2^-23 * cnt per voxel."""
    patch, shape, step, axes, _ = {**SMALL, **STEP}[name]
    padded = tuple(max(s, p) for s, p in zip(shape, patch))
    steps = tiler_ref.compute_steps_for_sliding_window(patch, padded, step)
    g = tiler_ref.get_gaussian(patch, 1.0 / 8).astype(np.float64)
    want, k = np.zeros(padded, np.float64), np.zeros(padded, np.int64)
    for z in steps[0]:
        for y in steps[1]:
            for x in steps[2]:
                sl = (slice(z, z + patch[0]), slice(y, y + patch[1]), slice(x, x + patch[2]))
                want[sl] += g
                k[sl] += 1
    got = runs[0][name + "_cnt"].astype(np.float64)
    assert got.shape == padded and k.min() >= 1 and k.max() > 8   # (the rounded origins lie closer than the nominal step: 12 and 45 tiles on one voxel)
    excess = np.abs(got - want) / ((k + 1) * 2.0 ** -23 * want)
    print(f"PARITY sw-geometry {name}: weight map, worst error {float(excess.max()):.3f} of the bound (k + 1) 2^-23 cnt, k up to {int(k.max())}")
    assert np.isfinite(got).all() and float(excess.max()) <= 1.0


def test_mid_skip_half_and_views(mid_runs, oracle):
    on, no_skip, no_views = mid_runs
    k_on, k_ns, k_nv = (_kernels(r, "mid") for r in mid_runs)
    assert [k for k in k_on if k.endswith(" up-half")] and [k for k in k_on if k.endswith(" skip-half")], k_on
    assert not [k for k in k_ns if k.endswith("-half")], k_ns
    d = float(np.abs(on["mid"] - no_skip["mid"]).max())
    print(f"PARITY sw-geometry mid: shared skip half on vs off {d:.2e}")
    assert np.isfinite(on["mid"]).all() and np.isfinite(no_skip["mid"]).all() and d <= 5e-5
    # views move where bytes are read and nothing else: the gather writes the shells alone, the result keeps its bits
    b_on, b_nv = (float(r["mid_bytes"][k.index(GATHER)]) for r, k in ((on, k_on), (no_views, k_nv)))
    print(f"PARITY sw-geometry mid: views on vs off max |dprob| {float(np.abs(on['mid'] - no_views['mid']).max()):.2e}, gather bytes {b_nv:.3e} -> {b_on:.3e}")
    assert b_on < b_nv and not [k for k in k_nv if "_view" in k]
    assert np.array_equal(on["mid"], no_views["mid"])
    for tag, run in (("on", on), ("skip-half off", no_skip), ("views off", no_views)):
        _against_oracle(tag, "mid", run["mid"], oracle["mid"])


def test_level1_on_against_off(level1_runs):
    """MI355_SHARE_LEVEL1 = 2 against 0 at a patch whose y and x extents differ, one per-origin and two merged axes.  On against off
    only - see the module docstring for what holds the off path and the plan."""
    on, off = level1_runs
    assert LEVEL1 in _kernels(on, "level1") and LEVEL1 not in _kernels(off, "level1"), _kernels(on, "level1")
    d = float(np.abs(on["level1"] - off["level1"]).max())
    print(f"PARITY sw-geometry level1: shared level 1 on vs off {d:.2e}")
    assert np.isfinite(on["level1"]).all() and np.isfinite(off["level1"]).all() and d <= 5e-5
