"""-m gpu: the shared skip half of the last decoder stage's concat conv (MI355_SHARE_SKIP_CONV, csrc/sw_share_plan.hip "shared skip half").

Single op: conv3_f32_wino3_kernel<0, false> with the epilogue addend - its twin instantiation <3, false>, which differs from it in that
epilogue only, so that launches without an addend run the code they ran before -, and the 64 -> 32 concat conv once as one launch and once as a
skip-half launch followed by an up-half launch that adds it, both against an fp64 CPU evaluation.
  * addend launch: |y - y_ref| <= 2e-5 * max(1, max|y_ref|), the fp32 conv gate of test_gpu_conv_fused.py;
  * split against whole: the split's maximum error at most twice the unsplit launch's (changed summation grouping and the one
    extra rounding of S).

Sliding window: the switch on against off within 5e-5 on probabilities, the bound tests/test_gpu_stage0_sharing.py uses for
"same tiles, other summation order".  The switch is read once per process, so each setting runs in one child process; the children
run once per module.  Patch 64^3: one sample of it is the smallest launch the dispatch sends to the kernel with the addend epilogue
(tests/test_skip_share_plan_cpu.py)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINO3 = "conv3_f32_wino3_kernel<0, false>"
WINO3_ADD = "conv3_f32_wino3_kernel<3, false>"  # the same kernel with the addend epilogue
PATCH = (64, 64, 64)
# name: (volume, mirrors, world).  faces: steps (0, 18, 36) x (0, 16) x (0, 8) - tiles with two interior faces on z, one on y and
# x, whole 4 x 8 x 8 conv tiles; odd: padded size (81, 77, 90) is extended to (84, 80, 96), which runs the mask in front of the
# skip-half conv; mirror: 8-way mirrors; ranks: dealt over world = 2.
CASES = {"faces": ((100, 80, 72), False, 1), "odd": ((81, 77, 90), False, 1), "mirror": ((72, 80, 72), True, 1), "ranks": ((81, 77, 90), False, 2)}

CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
from brats_amd import predictor
path, cases = sys.argv[1], eval(sys.argv[2])
patch = (64, 64, 64)
out = {}
def volume(shape, seed):
    return np.random.RandomState(seed).standard_normal((4,) + tuple(shape)).astype(np.float32)
sd, meta = brats_amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
net = brats_amd.UNet(sd, norm="batch")
for i, (name, (shape, mirror, world)) in enumerate(sorted(cases.items())):
    vol = volume(shape, 60 + i)
    net.profile(True)
    if world == 1:
        out[name] = predictor.predict_folds([net], vol, patch, 0.5, mirror, (0, 1, 2), True, "sigmoid").cpu().numpy()
    else:
        parts = [predictor.predict_tile_sharded(net, vol, r, world, patch, 0.5, mirror) for r in range(world)]
        agg = parts[0][0].clone()
        for r in range(1, world):
            agg += parts[r][0]
        out[name] = predictor.finish_sharded(agg, parts[0][1], vol.shape[1:], patch).cpu().numpy()
    prof = net.read_profile()
    net.profile(False)
    out[name + "_kernels"] = np.array([e["name"] for e in prof])
    out[name + "_flops"] = np.array([e["flops"] for e in prof])
    out[name + "_launches"] = np.array([e["launches"] for e in prof])
sd, meta = brats_amd.synthetic.make_model("A_in", seed=22, num_pool=2, max_feat=128)
net_in = brats_amd.UNet(sd, norm="instance")
out["instnorm"] = predictor.predict_folds([net_in], volume(cases["odd"][0], 60), patch, 0.5, False, (0, 1, 2), True, "sigmoid").cpu().numpy()
np.savez(path, **out)
"""


@pytest.fixture(scope="module")
def runs(amd, gpu):
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for flag in ("1", "0"):
            path = os.path.join(td, f"s{flag}.npz")
            res = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, repr(CASES)], env=dict(os.environ, MI355_SHARE_SKIP_CONV=flag),
                                 capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
            with np.load(path) as z:
                outs[flag] = {k: z[k] for k in z.files}
    return outs["1"], outs["0"]


def _conv_ref(x, w, b, addend=None, slope=0.01):
    """fp64 on the CPU: lrelu(bias + conv(x) + addend); x [N,D,H,W,C] -> [N,D,H,W,Cout]"""
    y = F.conv3d(torch.from_numpy(x).double().permute(0, 4, 1, 2, 3), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)
    y = y.permute(0, 2, 3, 4, 1)
    if addend is not None:
        y = y + torch.from_numpy(addend).double()
    return F.leaky_relu(y, slope)


@pytest.fixture(scope="module")
def single_op():
    rs = np.random.RandomState(5)
    n, d, h, w = 2, 8, 16, 16
    x_up = rs.standard_normal((n, d, h, w, 32)).astype(np.float32)
    x_skip = rs.standard_normal((n, d, h, w, 32)).astype(np.float32)
    wt = (rs.standard_normal((32, 64, 3, 3, 3)) / np.sqrt(64 * 27)).astype(np.float32)
    b = (0.1 * rs.standard_normal(32)).astype(np.float32)
    addend = rs.standard_normal((n, d, h, w, 32)).astype(np.float32)
    return x_up, x_skip, wt, b, addend


def test_addend_epilogue(amd, gpu, single_op):
    """N = 2, 8 x 16 x 16, 32 -> 32: 16 tiles on 16 workgroups, both samples, every wave's eight addend pieces."""
    x_up, _, wt, b, addend = single_op
    w32 = np.ascontiguousarray(wt[:, :32]) * np.float32(np.sqrt(2.0))
    ref = _conv_ref(x_up, w32, b, addend)
    y = amd.ops.conv3d_wino3_ndhwc(torch.from_numpy(x_up).to(gpu), w32, b, addend=torch.from_numpy(addend).to(gpu), act=1, slope=0.01)
    assert amd.ops.last_conv_kernel() == WINO3_ADD
    err = float((y.double().cpu() - ref).abs().max())
    gate = 2e-5 * max(1.0, float(ref.abs().max()))
    print(f"addend epilogue: max error {err:.2e}, gate {gate:.2e}")
    assert torch.isfinite(y).all() and err <= gate
    # without the addend the same call is the plain conv
    y0 = amd.ops.conv3d_wino3_ndhwc(torch.from_numpy(x_up).to(gpu), w32, b, act=1, slope=0.01)
    assert amd.ops.last_conv_kernel() == WINO3
    assert float((y0.double().cpu() - _conv_ref(x_up, w32, b)).abs().max()) <= gate


def test_split_against_whole(amd, gpu, single_op):
    """64 -> 32 over (up, skip): one launch, and S = conv(W[:, 32:], skip) with zero bias and no activation followed by
    lrelu(bias + conv(W[:, :32], up) + S)."""
    x_up, x_skip, wt, b, _ = single_op
    ref = _conv_ref(np.concatenate([x_up, x_skip], axis=-1), wt, b)
    up, skip = torch.from_numpy(x_up).to(gpu), torch.from_numpy(x_skip).to(gpu)
    whole = amd.ops.conv3d_wino3_ndhwc(up, wt, b, x1=skip, act=1, slope=0.01)
    assert amd.ops.last_conv_kernel() == WINO3
    s = amd.ops.conv3d_wino3_ndhwc(skip, np.ascontiguousarray(wt[:, 32:]), None, act=0)
    split = amd.ops.conv3d_wino3_ndhwc(up, np.ascontiguousarray(wt[:, :32]), b, addend=s, act=1, slope=0.01)
    assert amd.ops.last_conv_kernel() == WINO3_ADD
    e_whole = float((whole.double().cpu() - ref).abs().max())
    e_split = float((split.double().cpu() - ref).abs().max())
    print(f"64 -> 32 concat conv: one launch {e_whole:.3e}, split {e_split:.3e}, ratio {e_split / e_whole:.2f}")
    assert e_whole <= 2e-5 * max(1.0, float(ref.abs().max()))
    assert e_split <= 2.0 * e_whole


@pytest.mark.parametrize("name", sorted(CASES))
def test_on_matches_off(runs, name):
    on, off = runs
    d = float(np.abs(on[name] - off[name]).max())
    print(f"skip-half sharing {name}: on vs off {d:.2e}")
    assert np.isfinite(on[name]).all() and d <= 5e-5


@pytest.mark.parametrize("name", sorted(CASES))
def test_profile_shows_the_split(amd, runs, name):
    on, off = runs
    shape, mirror, world = CASES[name]
    kernels = [str(k) for k in on[name + "_kernels"]]
    skip = [k for k in kernels if k.endswith(" skip-half")]
    up = [k for k in kernels if k.endswith(" up-half")]
    assert skip and up == [WINO3_ADD + " up-half"], kernels
    assert not [k for k in off[name + "_kernels"] if str(k).endswith("-half")]
    # the shortened concat launch reports Cin = C0 = 32: 2 * samples * voxels * Cout * C0 * 27, over every (tile, mirror) once
    plan = amd.ops.skip_share_plan(shape, PATCH, 0.5, (0, 1, 2) if mirror else ())
    assert plan["skip_shared"]
    samples = plan["n_tiles"] * plan["n_mirrors"]
    got = float(on[name + "_flops"][kernels.index(up[0])])
    assert got == 2.0 * samples * 64 ** 3 * 32 * 32 * 27, (got, samples)


def test_instance_norm_is_untouched(runs):
    """Run-time statistics are per tile: the path is not taken and the switch changes nothing."""
    on, off = runs
    assert np.array_equal(on["instnorm"], off["instnorm"])
