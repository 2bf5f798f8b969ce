"""-m gpu: the shared level 1 of the sliding window (MI355_SHARE_LEVEL1, csrc/sw_share_plan.hip "shared level 1").

The path needs the shared skip half, and its per-tile launch over the upsampled half of dec[np - 2][0] is the kernel with the addend
epilogue, which the dispatch gives a single sample of the half patch only from 1024 (tile, cout block) units on: 64 -> 64 over 64^3,
i.e. patch 128^3.  So the network cases run the reduced model A of the other sharing tests (num_pool = 2, max_feat = 128) at patch
128^3, where the CPU oracle still takes about 5 s per tile; the patch-32 volumes of those tests pin that the forced setting leaves
them alone, bit for bit.  The plan itself is proved exactly in tests/test_level1_share_plan_cpu.py.

* "bench": 139 x 172 x 138, z per-origin (0, 11), y and x merged - the default rule turns it on.
* "three": 128 x 200 x 128 with the x mirror: one tile along z and x, three along y (the middle one with two faces inside the
  region), a region that is no whole number of conv tiles at level 1 (100 rows) - forced (`2`); the default rule refuses it.
* `2` against `0`: 5e-5 on probabilities, the suite's bound for another summation order; both against oracle/tiler_ref: 1e-3 and
  Dice >= 0.999; three ranks tile-sharded against unsharded: 2e-6; a run on an arena filled with 0xFFFFFFFF returns the bits of the
  clean run; an InstanceNorm net at the bench geometry and the patch-32 cases are untouched.
* Single op: the addend epilogue at Cout = 64 (two cout blocks), N = 2, 8 x 16 x 16, against fp64 with the fp32 conv gate of
  test_gpu_skip_sharing.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tiler_ref, unet_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL1 = "stage0_gather_kernel level 1"   # the profile entry of the hand-off gather
REGIONS = "extract_tiles_kernel region-slabs"   # and of the region pass's stage-0 slabs (only where a region has a face inside the volume)

# name: (volume, mirror axes or None, patch)
BIG = {"bench": ((139, 172, 138), None, (128, 128, 128)), "three": ((128, 200, 128), (2,), (128, 128, 128))}
SMALL = {"y3": ((41, 56, 44), None, (32, 32, 32)), "mirror": ((40, 56, 44), (0, 1, 2), (32, 32, 32)), "odd": ((41, 57, 43), None, (32, 32, 32)),
         "single": ((32, 32, 32), None, (32, 32, 32))}

CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
from brats_amd import predictor
path, big, small = sys.argv[1], eval(sys.argv[2]), eval(sys.argv[3])
out = {}
def vol_of(i, shape):
    return np.random.RandomState(70 + i).standard_normal((4,) + tuple(shape)).astype(np.float32)
def run(net, vol, patch, axes, **kw):
    return predictor.predict_folds([net], vol, patch, 0.5, axes is not None, axes or (0, 1, 2), True, "sigmoid", **kw)
def profiled(net, key, *args):
    net.profile(True)
    out[key] = run(net, *args).cpu().numpy()
    out[key + "_kernels"] = np.array(sorted(e["name"] for e in net.read_profile()))
    net.profile(False)
sd, meta = brats_amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
net = brats_amd.UNet(sd, norm="batch")
for i, (name, (shape, axes, patch)) in enumerate(sorted(big.items())):
    vol = vol_of(i, shape)
    profiled(net, name, vol, patch, axes)
    filled = brats_amd.ops.scratch_fill("SCR_ARENA", 0xFFFFFFFF)
    assert filled > 0
    out[name + "_poisoned"] = run(net, vol, patch, axes).cpu().numpy()
    if axes is None:
        parts = [predictor.predict_tile_sharded(net, vol, r, 3, patch, 0.5, False, batch_tiles=1) for r in range(3)]
        agg = parts[0][0].clone()
        for r in (1, 2):
            agg += parts[r][0]
        out[name + "_sharded"] = predictor.finish_sharded(agg, parts[0][1], vol.shape[1:], patch).cpu().numpy()
        out[name + "_whole"] = run(net, vol, patch, axes, batch_tiles=1).cpu().numpy()
for i, (name, (shape, axes, patch)) in enumerate(sorted(small.items())):
    profiled(net, "batch_" + name, vol_of(10 + i, shape), patch, axes)
net = brats_amd.UNet(sd, norm="instance")
shape, axes, patch = big["bench"]
profiled(net, "instance_bench", vol_of(0, shape), patch, axes)
shape, axes, patch = small["y3"]
profiled(net, "instance_y3", vol_of(10, shape), patch, axes)
np.savez(path, **out)
"""


@pytest.fixture(scope="module")
def runs(amd, gpu):
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for flag in ("2", "0"):
            path = os.path.join(td, f"l{flag}.npz")
            res = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, repr(BIG), repr(SMALL)], env=dict(os.environ, MI355_SHARE_LEVEL1=flag),
                                 capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
            with np.load(path) as z:
                outs[flag] = {k: z[k] for k in z.files}
    return outs["2"], outs["0"]


@pytest.fixture(scope="module")
def oracle(amd):
    sd, meta = amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
    fn = tiler_ref.make_net_fn(sd, unet_ref.default_cfg("batch"))
    refs = {}
    for i, (name, (shape, axes, patch)) in enumerate(sorted(BIG.items())):
        vol = np.random.RandomState(70 + i).standard_normal((4,) + shape).astype(np.float32)
        refs[name] = tiler_ref.predict_3d_tiled(fn, vol, patch, 3, 0.5, axes is not None, axes or (0, 1, 2), True, "sigmoid")
    return refs


def test_the_plan_of_the_cases(amd):
    kw = dict(num_pool=2)
    bench = amd.ops.level1_share_plan(BIG["bench"][0], BIG["bench"][2], **kw)
    assert bench["on"] and bench["merged"] == (False, True, True)
    three = {m: amd.ops.level1_share_plan(BIG["three"][0], BIG["three"][2], mirror_axes=(2,), mode=m, **kw) for m in (1, 2)}
    assert three[2]["on"] and not three[1]["on"] and three[2]["merged"] == (False, True, False) and three[2]["region"] == (128, 200, 128)
    assert any({2, 3} <= set(s["slabs"]) for s in three[2]["samples"])
    for shape, axes, patch in SMALL.values():
        assert not amd.ops.level1_share_plan(shape, patch, mirror_axes=axes or (), mode=2, **kw)["on"]


@pytest.mark.parametrize("name", sorted(BIG))
def test_on_against_off_and_oracle(runs, oracle, name):
    on, off = runs
    assert LEVEL1 in list(on[name + "_kernels"]) and LEVEL1 not in list(off[name + "_kernels"]), list(on[name + "_kernels"])
    assert (REGIONS in list(on[name + "_kernels"])) == (name == "bench") and REGIONS not in list(off[name + "_kernels"])
    d = float(np.abs(on[name] - off[name]).max())
    e_on, e_off = (float(np.abs(x[name] - oracle[name]).max()) for x in (on, off))
    print(f"level-1 sharing {name}: on vs off {d:.2e}, on vs oracle {e_on:.2e}, off vs oracle {e_off:.2e}")
    assert np.isfinite(on[name]).all() and 0 < d <= 5e-5
    for got, err in ((on[name], e_on), (off[name], e_off)):
        assert err <= 1e-3
        dice = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(oracle[name]))
        assert dice["mean"] >= 0.999


@pytest.mark.parametrize("name", sorted(BIG))
def test_poisoned_arena_gives_the_same_bits(runs, name):
    for run in runs:
        assert np.array_equal(run[name], run[name + "_poisoned"])


def test_tile_sharded_matches_unsharded(runs):
    """Every rank computes all regions; the slabs run in launches of eight whatever tiles a rank holds."""
    for run, sw in zip(runs, ("on", "off")):
        d = float(np.abs(run["bench_sharded"] - run["bench_whole"]).max())
        print(f"level-1 sharing {sw}: 3 ranks vs unsharded {d:.2e}")
        assert d <= 2e-6, sw


@pytest.mark.parametrize("key", ["instance_bench", "instance_y3"] + ["batch_" + n for n in sorted(SMALL)])
def test_untouched(runs, key):
    """An InstanceNorm net - at the bench geometry, where the BatchNorm net takes the path - and patch 32^3 (the addend kernel does
    not take a 16^3 sample): the forced setting changes nothing."""
    on, off = runs
    assert LEVEL1 not in list(on[key + "_kernels"])
    assert np.array_equal(on[key], off[key]) and list(on[key + "_kernels"]) == list(off[key + "_kernels"])


def test_addend_epilogue_two_cout_blocks(amd, gpu):
    """The up-half launch of dec[np - 2][0]: 64 -> 64 with the addend, N = 2, 8 x 16 x 16."""
    rs = np.random.RandomState(6)
    n, d, h, w = 2, 8, 16, 16
    x = rs.standard_normal((n, d, h, w, 64)).astype(np.float32)
    wt = (rs.standard_normal((64, 64, 3, 3, 3)) / np.sqrt(64 * 27)).astype(np.float32)
    b = (0.1 * rs.standard_normal(64)).astype(np.float32)
    addend = rs.standard_normal((n, d, h, w, 64)).astype(np.float32)
    y = F.conv3d(torch.from_numpy(x).double().permute(0, 4, 1, 2, 3), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    ref = F.leaky_relu(y.permute(0, 2, 3, 4, 1) + torch.from_numpy(addend).double(), 0.01)
    got = amd.ops.conv3d_wino3_ndhwc(torch.from_numpy(x).to(gpu), wt, b, addend=torch.from_numpy(addend).to(gpu), act=1, slope=0.01)
    assert amd.ops.last_conv_kernel() == "conv3_f32_wino3_kernel<3, false>"
    err = float((got.double().cpu() - ref).abs().max())
    gate = 2e-5 * max(1.0, float(ref.abs().max()))
    print(f"addend epilogue, Cout 64: max error {err:.2e}, gate {gate:.2e}")
    assert torch.isfinite(got).all() and err <= gate
