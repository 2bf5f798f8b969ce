"""-m gpu: the two launch changes of the shared level 1 - MI355_S2_LEAST_PADDING, MI355_SUBBOX_GATHER (csrc/sw_share_plan.hip "shared
level 1") - end to end: they change how two pieces of the pass are launched, never a value.

The reduced model A of tests/test_gpu_level1_sharing.py (num_pool = 2, max_feat = 128) at patch 128^3 - smaller patches cannot take
the path - over 128 x 172 x 138: one tile along z, two along y and x, one region of 128 x 176 x 144 whose stride-2 launch is Wo = 72
wide.  One child process per setting (the switches are read once per process): both on (the default) against both `0`.
  * the probabilities are EQUAL, bit for bit;
  * the profile of the default run has conv3_f32_s2dma_kernel_view<4>, the other has not; both have the <5> launches of the y sub-boxes
    and of the per-tile levels below;
  * the hand-offs keep their profile entries (the sub-box gather and the level-1 hand-off are there in both)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("MI355_S2_LEAST_PADDING", "MI355_SUBBOX_GATHER")
VOLUME, PATCH = (128, 172, 138), (128, 128, 128)
VIEW4, VIEW5 = "conv3_f32_s2dma_kernel_view<4>", "conv3_f32_s2dma_kernel_view<5>"

CHILD = """
import sys, numpy as np
sys.path.insert(0, %r)
import brats_amd
from brats_amd import predictor
path, shape, patch = sys.argv[1], eval(sys.argv[2]), eval(sys.argv[3])
sd, meta = brats_amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
net = brats_amd.UNet(sd, norm="batch")
vol = np.random.RandomState(70).standard_normal((4,) + tuple(shape)).astype(np.float32)
net.profile(True)
probs = predictor.predict_folds([net], vol, patch, 0.5, False, (0, 1, 2), True, "sigmoid").cpu().numpy()
np.savez(path, probs=probs, kernels=np.array(sorted(e["name"] for e in net.read_profile())))
"""


@pytest.fixture(scope="module")
def runs(amd, gpu):
    assert amd.ops.level1_share_plan(VOLUME, PATCH, num_pool=2)["on"]
    outs = []
    with tempfile.TemporaryDirectory() as td:
        for flag in (None, "0"):
            env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            if flag:
                env.update({k: flag for k in SWITCHES})
            path = os.path.join(td, f"trim{flag}.npz")
            res = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, repr(VOLUME), repr(PATCH)], env=env, capture_output=True, text=True, timeout=300)
            assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
            with np.load(path) as z:
                outs.append({k: z[k] for k in z.files})
    return outs


def test_switches_on_equal_switches_off_bit_for_bit(runs):
    on, off = runs
    assert np.isfinite(on["probs"]).all() and on["probs"].std() > 0
    assert np.array_equal(on["probs"], off["probs"])


def test_the_region_launch_runs_the_16_wide_tile(runs):
    on, off = (list(r["kernels"]) for r in runs)
    assert any(VIEW4 in k for k in on) and not any(VIEW4 in k for k in off), on
    assert any(VIEW5 in k for k in on) and any(VIEW5 in k for k in off)
    for entry in ("stage0_gather_kernel sub-boxes", "stage0_gather_kernel level 1", "stage0_gather_kernel"):
        assert entry in on and entry in off, entry
    # nothing else moved: the same profile entries (one per name), the region's stride-2 conv apart
    assert set(on) - {VIEW4} == set(off)
