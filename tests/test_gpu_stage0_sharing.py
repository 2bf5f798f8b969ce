"""-m gpu: the shared stage 0 of the sliding window (MI355_SHARE_STAGE0, csrc/sw_share_plan.hip "shared stage 0") against today's
per-tile path and the CPU oracle.

The switch is read once per process, so each setting runs in a child process of its own (one per setting for the small cases,
one per setting for the bench geometry); the children and the oracle predictions run once per module.

Bounds: sharing on against off within 5e-5 on probabilities - what the suite gives to "same tiles, other summation order"
(test_sliding_window_matches_oracle, batch_tiles); both against the oracle within 1e-3 and Dice >= 0.999 (BASELINE.json
north_star); tile-sharded against unsharded within 2e-6 (test_fold_list_tile_sharding).  A wrong shell or origin moves stage-0
features by O(1) within the receptive field of the deeper levels and misses the first bound by orders of magnitude."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import tiler_ref, unet_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = (32, 32, 32)
# name: (volume, mirrors).  (41, 57, 43): steps (0, 9) x (0, 12, 25) x (0, 11) - odd offsets and a middle tile with two interior
# faces on y; (20, 40, 30): padded in z and x, one tile along z; (40, 56, 44): 8-way mirrors; (32, 32, 32): one tile, path off.
CASES = {"odd": ((41, 57, 43), False), "padded": ((20, 40, 30), False), "mirror": ((40, 56, 44), True), "single": ((32, 32, 32), False)}

CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
from brats_amd import predictor
mode, path = sys.argv[1], sys.argv[2]
out = {}
def volume(shape, seed):
    return np.random.RandomState(seed).standard_normal((4,) + tuple(shape)).astype(np.float32)
if mode == "small":
    cases = eval(sys.argv[3])
    patch = (32, 32, 32)
    sd, meta = brats_amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
    net = brats_amd.UNet(sd, norm="batch")
    for i, (name, (shape, mirror)) in enumerate(sorted(cases.items())):
        vol = volume(shape, 40 + i)
        net.profile(True)
        out[name] = predictor.predict_folds([net], vol, patch, 0.5, mirror, (0, 1, 2), True, "sigmoid").cpu().numpy()
        out[name + "_kernels"] = np.array(sorted(e["name"] for e in net.read_profile()))
        net.profile(False)
        # one tile per forward on both sides: see test_tile_sharded_matches_unsharded
        parts = [predictor.predict_tile_sharded(net, vol, r, 3, patch, 0.5, False, batch_tiles=1) for r in range(3)]
        agg = parts[0][0].clone()
        for r in (1, 2):
            agg += parts[r][0]
        out[name + "_sharded"] = predictor.finish_sharded(agg, parts[0][1], vol.shape[1:], patch).cpu().numpy()
        out[name + "_whole"] = predictor.predict_folds([net], vol, patch, 0.5, False, (0, 1, 2), True, "sigmoid", batch_tiles=1).cpu().numpy()
    sd, meta = brats_amd.synthetic.make_model("A_in", seed=22, num_pool=2, max_feat=128)
    net_in = brats_amd.UNet(sd, norm="instance")
    out["instnorm"] = predictor.predict_folds([net_in], volume(cases["odd"][0], 40), patch, 0.5, False, (0, 1, 2), True, "sigmoid").cpu().numpy()
else:
    sd, meta = brats_amd.synthetic.make_model("A", seed=23, num_pool=2, max_feat=128)
    net = brats_amd.UNet(sd, norm="batch")
    net.profile(True)
    out["bench"] = predictor.predict_folds([net], volume((139, 172, 138), 50), (128, 128, 128), 0.5, False, (0, 1, 2), True, "sigmoid").cpu().numpy()
    out["bench_kernels"] = np.array(sorted(e["name"] for e in net.read_profile()))
np.savez(path, **out)
"""


def _children(mode, *extra):
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for flag in ("1", "0"):
            path = os.path.join(td, f"s{flag}.npz")
            res = subprocess.run([sys.executable, "-c", CHILD % ROOT, mode, path, *extra], env=dict(os.environ, MI355_SHARE_STAGE0=flag),
                                 capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
            with np.load(path) as z:
                outs[flag] = {k: z[k] for k in z.files}
    return outs["1"], outs["0"]


@pytest.fixture(scope="module")
def small(amd, gpu):
    return _children("small", repr(CASES))


@pytest.fixture(scope="module")
def oracle(amd):
    sd, meta = amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
    fn = tiler_ref.make_net_fn(sd, unet_ref.default_cfg("batch"))
    refs = {}
    for i, (name, (shape, mirror)) in enumerate(sorted(CASES.items())):
        vol = np.random.RandomState(40 + i).standard_normal((4,) + shape).astype(np.float32)
        refs[name] = tiler_ref.predict_3d_tiled(fn, vol, PATCH, 3, 0.5, mirror, (0, 1, 2), True, "sigmoid")
    return refs


@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_matches_per_tile_and_oracle(small, oracle, name):
    on, off = small
    shared = "stage0_gather_kernel" in list(on[name + "_kernels"])
    assert shared == (name != "single"), list(on[name + "_kernels"])
    assert "stage0_gather_kernel" not in list(off[name + "_kernels"])
    d = float(np.abs(on[name] - off[name]).max())
    e_on, e_off = (float(np.abs(x[name] - oracle[name]).max()) for x in (on, off))
    print(f"stage-0 sharing {name}: on vs off {d:.2e}, on vs oracle {e_on:.2e}, off vs oracle {e_off:.2e}")
    assert d <= 5e-5
    for got, err in ((on[name], e_on), (off[name], e_off)):
        assert err <= 1e-3
        dice = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(oracle[name]))
        assert dice["mean"] >= 0.999


def test_tile_sharded_matches_unsharded(small):
    """Every rank computes a tile's features the same way: the decision does not depend on rank, world or batch size, the
    whole-volume pass has the same shape on every rank and the slab convs run in launches of a fixed size.  Three ranks against
    the unsharded call, every volume of the file, within the 2e-6 of test_fold_list_tile_sharding.  Both sides run one tile per
    forward (batch_tiles = 1): the levels BEHIND stage 0 pick their kernels by the samples of a forward, and at these geometries
    a rank's 1 - 4 tiles per forward against the unsharded 2 - 12 send them to other kernels, which moves the PER-TILE path by
    2.9e-5 - 4.9e-5 as well (measured with the switch off; the 8-tile geometry of test_fold_list_tile_sharding happens not to
    cross such a threshold).  With equal forwards what is left is the rank-ordered sum, and the switch must not add to it."""
    for run, sw in zip(small, ("on", "off")):
        for name in sorted(CASES):
            d = float(np.abs(run[name + "_sharded"] - run[name + "_whole"]).max())
            print(f"stage-0 sharing {sw} {name}: 3 ranks vs unsharded {d:.2e}")
            assert d <= 2e-6, (sw, name)


def test_instance_norm_is_untouched(small):
    """Instance/GroupNorm statistics are per tile: the path is not taken and the switch changes nothing."""
    on, off = small
    assert np.array_equal(on["instnorm"], off["instnorm"])


def test_bench_geometry(amd, gpu):
    """139 x 172 x 138, patch 128^3, eight tiles: the only place the F(2x2x2,3x3x3) kernel meets the whole-volume (140 x 176 x 144,
    N = 1) and slab (N = 8 of 4 x 128 x 128, 128 x 8 x 128, 128 x 128 x 8) shapes.  No CPU oracle: on against off."""
    on, off = _children("bench")
    kernels = list(on["bench_kernels"])
    assert "stage0_gather_kernel" in kernels and "stage0_gather_kernel" not in list(off["bench_kernels"]), kernels
    assert "conv3_f32_wino3_kernel<0, false>" in kernels
    d = float(np.abs(on["bench"] - off["bench"]).max())
    print(f"stage-0 sharing, bench geometry: on vs off {d:.2e}")
    assert np.isfinite(on["bench"]).all() and d <= 5e-5
