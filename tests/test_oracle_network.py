"""not gpu: pins the oracle's network restatement (oracle/unet_ref.py) to the reference.

1. against golden vectors produced by importing the reference's own Generic_UNet
   (oracle/gen_golden.py -> tests/golden/net_*.npz);
2. against what the reference module itself builds and computes on a second seed (its
   state_dict keys / shapes and full logits, oracle/gen_golden.py -> tests/golden/net_module_*.npz)."""
import os

import numpy as np
import pytest
import torch

from oracle import gen_golden, unet_ref

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _moments(t):
    t = t.double()
    return np.array([t.mean().item(), t.std(unbiased=False).item(), t.norm().item(), t.abs().max().item()])


@pytest.mark.parametrize("name", ["A", "A_in", "B"])
def test_oracle_matches_reference_golden_64(amd, name):
    g = np.load(os.path.join(GOLD, f"net_{name}.npz"))
    sd, meta = amd.synthetic.make_model(name, seed=int(g["weight_seed"]))
    x = np.random.RandomState(int(g["input_seed"])).standard_normal((1, 4, 64, 64, 64)).astype(np.float32)
    y, stages = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm=meta["norm"], num_groups=16), return_stages=True)
    # same torch ops in the same order: the restatement is bit-identical on the generating machine,
    # allow a few ulp of the logit scale for other CPUs / oneDNN kernels
    tol = 1e-5 * float(g["logits_moments"][1])
    assert np.abs(y[:, :, ::8, ::8, ::8].numpy() - g["logits_sub"]).max() <= tol
    assert np.allclose(_moments(y), g["logits_moments"], rtol=1e-5)
    for k in ("ctx0", "ctx3", "loc4"):
        assert np.allclose(_moments(stages[k]), g[f"stage_{k}"], rtol=1e-5), k
    assert np.allclose(_moments(stages["bottleneck"]), g["stage_ctx5"], rtol=1e-5)


@pytest.mark.parametrize("norm", ["batch", "instance", "group"])
@pytest.mark.parametrize("nonlin_first", [False, True])
def test_oracle_matches_reference_golden_small(amd, norm, nonlin_first):
    g = np.load(os.path.join(GOLD, f"net_small_{norm}_{int(nonlin_first)}.npz"))
    sd, _ = amd.synthetic.make_model("A", seed=5, num_pool=2, max_feat=64, norm=norm)
    x = np.random.RandomState(6).standard_normal((2, 4, 16, 16, 32)).astype(np.float32)
    y = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm=norm, num_groups=8, nonlin_first=nonlin_first)).numpy()
    assert y.shape == g["logits"].shape
    assert np.abs(y - g["logits"]).max() <= 1e-5 * max(1.0, float(np.abs(g["logits"]).max()))


@pytest.mark.parametrize("cfg", gen_golden.MODULE_CFGS)
def test_oracle_matches_live_reference_module(amd, cfg):
    g = np.load(os.path.join(GOLD, gen_golden.module_fixture_name(cfg)))
    sd = amd.synthetic.make_state_dict(seed=int(g["weight_seed"]), all_heads=True, **cfg)
    # every key / shape the synthetic generator emits is what the reference constructor builds
    ref_shapes = {str(k): tuple(int(d) for d in s if d >= 0) for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    assert set(sd.keys()) == set(ref_shapes)
    for k in sd:
        assert tuple(sd[k].shape) == ref_shapes[k], k
    x = torch.from_numpy(np.random.RandomState(int(g["input_seed"])).standard_normal((2, 4, 32, 32, 32)).astype(np.float32))
    got = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm=cfg["norm"], num_groups=16))
    want = torch.from_numpy(g["logits"])
    assert got.shape == want.shape
    # same torch ops in the same order as the reference module: bit-identical on the CPU the fixture was made on; oneDNN picks
    # other kernels on other instruction sets (AVX2 / SSE4.1 against AVX-512: up to 3.7e-6 of max |logit|)
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()


def test_flop_count_matches_survey(amd):
    """model A = 965.6 GFLOP per 128^3 patch (all five seg heads), model B = 3342."""
    sd = amd.synthetic.make_state_dict(seed=1, norm="none", all_heads=True)
    assert abs(unet_ref.conv_flops(sd, (128, 128, 128)) / 1e9 - 965.6) < 0.1
    sd_b = amd.synthetic.make_state_dict(seed=1, norm="none", all_heads=True, max_feat=512, encoder_scale=2)
    assert abs(unet_ref.conv_flops(sd_b, (128, 128, 128)) / 1e9 - 3342.4) < 1.0
