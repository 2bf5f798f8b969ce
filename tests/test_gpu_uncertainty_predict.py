"""-m gpu: predictor.predict_folds_moments - the second moment through the whole sliding window - against predict_folds (the mean,
bit for bit) and against the float64 restatement uncertainty_util.predict_moments (the variance).

One child process with its own timeout runs everything on the device and writes an .npz (test_gpu_sw_geometry.py's pattern); the
CPU oracle is computed once per case and shared.

Network: the reduced model A (num_pool = 2, max_feat = 128, BatchNorm), two folds (seeds 21 and 22).  Geometry: patch 32^3 on
(41, 57, 43), step 0.5 (2 x 3 x 2 tiles, odd origins), mirrors (0, 1, 2): 2 folds x 12 tiles x 8 mirrors = 192 samples, which
predict_folds spreads over two lanes (192 >= 64) and, with lanes = 1, sends through mi355_sw_predict; and the single tile 32^3,
where cnt = 1 and the variance is that over folds and mirrors alone.

Gates:
  * mean BIT EQUAL to predict_folds at lanes = 1 and at lanes = 2;
  * var = max(m2 - mean^2, 0) within 2 sigma_ref eps + eps^2 + 64 x 2^-24 of the oracle's, eps = 1e-3 the project's probability gate
    (fp16: 0.05, the probability allowance of test_gpu_network._check_logits_f16).  DERIVED: with |dp_s| <= eps for every sample,
    var' - var = sum w (p' - mean')^2 - sum w (p - mean)^2 and Cauchy-Schwarz on the cross term give 2 sigma eps + eps^2; 64 x 2^-24
    covers the fp32 roundings of m2 - mean^2 of numbers <= 1 (the sums of up to 8 x 16 weighted terms and the subtraction);
  * everything finite; var > 1e-6 on at least 1 % of the voxels - of the ORACLE's variance too, so the test cannot pass on zeros
    (checked on the CPU for these seeds: test_the_oracle_has_spread)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import uncertainty_util as uu
from oracle import tiler_ref, unet_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = (32, 32, 32)
CASES = {"tiled": ((41, 57, 43), 82), "single": ((32, 32, 32), 88)}
FOLD_SEEDS = (21, 22)
EPS = {"f32": 1e-3, "f16": 0.05}

CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
from brats_amd import predictor
path, cases, seeds, patch = sys.argv[1], eval(sys.argv[2]), eval(sys.argv[3]), eval(sys.argv[4])
out = {}
sds = [brats_amd.synthetic.make_model("A", seed=s, num_pool=2, max_feat=128)[0] for s in seeds]
nets = {dt: [brats_amd.UNet(sd, norm="batch", dtype=dt) for sd in sds] for dt in ("f32", "f16")}
args = (patch, 0.5, True, (0, 1, 2), True, "sigmoid")
for name, (shape, seed) in sorted(cases.items()):
    vol = np.random.RandomState(seed).standard_normal((4,) + tuple(shape)).astype(np.float32)
    for dt in ("f32", "f16"):
        for lanes in (1, 2):
            mean, m2 = predictor.predict_folds_moments(nets[dt], vol, *args, lanes=lanes)
            key = "%%s_%%s_l%%d" %% (name, dt, lanes)
            out[key + "_mean"], out[key + "_m2"] = mean.cpu().numpy(), m2.cpu().numpy()
            out[key + "_probs"] = predictor.predict_folds(nets[dt], vol, *args, lanes=lanes).cpu().numpy()
np.savez(path, **out)
"""


@pytest.fixture(scope="module")
def run(amd, gpu):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "moments.npz")
        res = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, repr(CASES), repr(FOLD_SEEDS), repr(PATCH)], capture_output=True, text=True,
                             timeout=300)
        assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def oracle(amd):
    """(mean, m2) float64 per case, computed once."""
    fns = [tiler_ref.make_net_fn(amd.synthetic.make_model("A", seed=s, num_pool=2, max_feat=128)[0], unet_ref.default_cfg("batch")) for s in FOLD_SEEDS]
    refs = {}
    for name, (shape, seed) in CASES.items():
        vol = np.random.RandomState(seed).standard_normal((4,) + tuple(shape)).astype(np.float32)
        refs[name] = uu.predict_moments(fns, vol, PATCH, 0.5, (0, 1, 2), "sigmoid")
    return refs


def _var(mean, m2):
    mean, m2 = mean.astype(np.float64), m2.astype(np.float64)
    return np.maximum(m2 - mean * mean, 0.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_oracle_has_spread(oracle, name):
    """The restatement's own variance exceeds 1e-6 on at least 1 % of the voxels, and its mean is the tiler oracle's."""
    mean, m2 = oracle[name]
    var = _var(mean, m2)
    share = float((var > 1e-6).mean())
    print(f"oracle {name}: var > 1e-6 on {100 * share:.1f} % of the voxels, max std {float(np.sqrt(var.max())):.3f}")
    assert share >= 0.01 and (m2 >= mean * mean - 1e-15).all() and (mean >= 0).all() and (mean <= 1).all()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_mean_is_predict_folds_bit_for_bit(run, name, dtype):
    for lanes in (1, 2):
        key = f"{name}_{dtype}_l{lanes}"
        got, want = run[key + "_mean"], run[key + "_probs"]
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{key}: {int((got != want).sum())} voxels differ from predict_folds"


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_variance_against_the_oracle(run, oracle, name, lanes, dtype):
    key = f"{name}_{dtype}_l{lanes}"
    mean, m2 = run[key + "_mean"], run[key + "_m2"]
    assert np.isfinite(mean).all() and np.isfinite(m2).all()
    var, ref = _var(mean, m2), _var(*oracle[name])
    eps = EPS[dtype]
    bound = 2 * np.sqrt(ref) * eps + eps * eps + 64 * 2.0 ** -24
    err = np.abs(var - ref)
    share = float((var > 1e-6).mean())
    print(f"PARITY uncertainty {key}: max |dvar| {float(err.max()):.3e}, worst {float((err / bound).max()):.3f} of its bound, "
          f"max |dmean| {float(np.abs(mean - oracle[name][0]).max()):.2e}, var > 1e-6 on {100 * share:.1f} %")
    assert (err <= bound).all(), f"{key}: {int((err > bound).sum())} voxels beyond the bound"
    assert share >= 0.01
    if dtype == "f32":
        assert float(np.abs(mean - oracle[name][0]).max()) <= 1e-3
