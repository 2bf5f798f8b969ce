"""-m gpu: whole-network and sliding-window parity of the HIP path against the CPU oracle
(oracle/unet_ref.py is itself pinned to the reference module, see tests/test_oracle_*.py).

Tolerances (BASELINE.json north_star): probabilities within 1e-3 of the fp32 CPU path, Dice of
the label maps >= 0.999.  Logits are also bounded relative to their spread, a much tighter check."""
import numpy as np
import pytest
import torch

from oracle import tiler_ref, unet_ref

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-3


LOGIT_REL_TOL = 6e-5   # x logit spread.  Measured on MI355X (round 2): 0.7-4.7e-5 over every fp32 case of this file
                       # (worst: InstanceNorm 64^3 4.65e-5; the Winograd F(2x2,3x3) path at 128^3 3.8e-5), so a
                       # regression of the Winograd numerics by 1.6x already fails


ABS_LOGIT_TOL = 1e-3   # north_star, read literally: "softmax logits within 1e-3 fp32"


def _check_logits(got, ref, what="", rel_tol=None, abs_tol=ABS_LOGIT_TOL):
    """Which reading of the north_star's "logits within 1e-3" the suite enforces: ALL of them.  SURVEY.md 8d
    reads it as class PROBABILITIES within 1e-3 (what decides a label; gated here); the logits are gated relative to their spread
    (a regression detector: 6e-5 x spread is 1.6 x the worst fp32 case measured) AND, read literally, at 1e-3 absolute - for the
    synthetic heads with a logit spread above 16.7 the absolute bound is the tighter of the two (model A at 128^3: spread 24,
    measured 9.2e-4)."""
    rel_tol = LOGIT_REL_TOL if rel_tol is None else rel_tol
    spread = float(ref.std())
    err = float(np.abs(got - ref).max())
    perr = float(np.abs(1 / (1 + np.exp(-got.astype(np.float64))) - 1 / (1 + np.exp(-ref.astype(np.float64)))).max())
    print(f"PARITY {what}: logit max abs err {err:.3e} = {err / max(spread, 1.0):.2e} x spread ({spread:.2f}), prob err {perr:.2e}")
    assert err <= rel_tol * max(spread, 1.0), f"logit max abs err {err} (spread {spread})"
    if abs_tol is not None:
        assert err <= abs_tol, f"logit max abs err {err} > {abs_tol} (spread {spread})"
    assert perr <= PROB_TOL, f"sigmoid prob err {perr}"


@pytest.mark.parametrize("name", ["A", "A_in", "B"])
def test_forward_64_matches_oracle(amd, gpu, name):
    sd, meta = amd.synthetic.make_model(name, seed=7)
    net = amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"])
    x = np.random.RandomState(1).standard_normal((1, 4, 64, 64, 64)).astype(np.float32)
    ref = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm=meta["norm"], num_groups=meta["num_groups"])).numpy()
    got = net(torch.from_numpy(x).to(gpu)).cpu().numpy()
    _check_logits(got, ref, f"64^3 {name}")
    net.close()


def test_forward_batch_and_ragged_patch(amd, gpu):
    """Batch of 3 with a non-cubic patch (32 x 64 x 96): per-sample InstanceNorm statistics."""
    sd, meta = amd.synthetic.make_model("A_in", seed=3, num_pool=3, max_feat=128)
    net = amd.UNet(sd, norm="instance")
    x = np.random.RandomState(4).standard_normal((3, 4, 32, 64, 96)).astype(np.float32)
    ref = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm="instance")).numpy()
    got = net(torch.from_numpy(x).to(gpu)).cpu().numpy()
    _check_logits(got, ref)


def test_instance_and_group_norm_forwards_are_bit_reproducible(amd, gpu):
    """the Instance/GroupNorm sums are accumulated with atomics in arrival order; every partial is rounded to a
    fixed quantum first, which makes the fp64 additions exact and the result independent of that order (common.h:
    quantise_partial).  Five forwards of each model, fp32 and fp16, must agree bit for bit."""
    x = torch.from_numpy(np.random.RandomState(9).standard_normal((2, 4, 64, 64, 64)).astype(np.float32)).to(gpu)
    for name, dtype in (("A_in", "f32"), ("B", "f32"), ("A_in", "f16"), ("B", "f16")):
        sd, meta = amd.synthetic.make_model(name, seed=7)
        net = amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"], dtype=dtype)
        first = net(x).clone()
        for _ in range(4):
            assert torch.equal(net(x), first), (name, dtype)
        net.close()


SMALL_ACT_TOL = {"A_in": 1.5e-4, "B": 2.5e-5}


@pytest.mark.parametrize("name", ["A_in", "B"])
def test_norm_statistics_of_small_activations(amd, gpu, name):
    """the Instance/GroupNorm partial sums are rounded to a fixed quantum before the atomic add (common.h,
    quantise_partial).  Round 2's quantum for sum x^2 was 2e-3 at a 128^3 patch: with every conv weight scaled by 2e-3 the
    pre-norm activations have rms ~1e-3..1e-2, a workgroup's partial (128-512 voxels) lies at or below that quantum and
    the variance came out coarse or zero, i.e. a wrong 1/sqrt(var + eps) where var ~ eps.  The reference computes exact
    fp32 statistics (generic_UNet.py:43,62-65).  With var ~ eps the normalisation no longer restores unit scale, the logits of
    the scaled net are small (spread 1.3-2.1 for A_in, 1.9-8.1 for B) and ordinary fp32 summation noise is a larger fraction of
    it than in the other cases of this file.  Gates re-derived in round 4 from 3 model seeds x 3 input seeds each
    (tests/diagnostics/gate_seeds.py, profiles/r04_gate_seeds.txt): A_in 3.8e-5 .. 9.2e-5 x spread (this case: 6.7e-5), B
    2.3e-6 .. 1.07e-5; gate = 1.6 x / 2.3 x the largest of the nine.  A statistics error of the kind guarded against moves
    1 / sqrt(var + eps) by 2-50 % and the logits by > 1e-2 of their spread."""
    sd, meta = amd.synthetic.make_model(name, seed=7)
    sd = {k: (v * 2e-3 if k.endswith(".conv.weight") else v) for k, v in sd.items()}
    net = amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"])
    x = np.random.RandomState(12).standard_normal((1, 4, 64, 64, 64)).astype(np.float32)
    ref = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm=meta["norm"], num_groups=meta["num_groups"])).numpy()
    got = net(torch.from_numpy(x).to(gpu)).cpu().numpy()
    assert float(ref.std()) > 1e-3, "the scaled net must still produce a signal"
    _check_logits(got, ref, f"64^3 {name} with pre-norm rms ~1e-3", rel_tol=SMALL_ACT_TOL[name])
    net.close()


def test_forward_nonlin_first_variants(amd, gpu):
    """ConvDropoutNonlinNorm ordering (generic_UNet.py:75-80) with GroupNorm and BatchNorm."""
    for norm in ("group", "batch"):
        sd, _ = amd.synthetic.make_model("A", seed=5, num_pool=2, max_feat=64, norm=norm)
        net = amd.UNet(sd, norm=norm, num_groups=8, nonlin_first=True)
        x = np.random.RandomState(6).standard_normal((2, 4, 16, 16, 32)).astype(np.float32)
        ref = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm=norm, num_groups=8, nonlin_first=True)).numpy()
        got = net(torch.from_numpy(x).to(gpu)).cpu().numpy()
        _check_logits(got, ref)


def test_forward_128_model_a(amd, gpu):
    """Full-size patch of the bench model (BASELINE.json configs[1]); flop count cross-check."""
    sd, meta = amd.synthetic.make_model("A", seed=7)
    net = amd.UNet(sd, norm="batch")
    assert net.flops((128, 128, 128)) == unet_ref.conv_flops(sd, (128, 128, 128)) == net.topology.conv_flops((128, 128, 128))
    x = np.random.RandomState(2).standard_normal((1, 4, 128, 128, 128)).astype(np.float32)
    ref = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm="batch")).numpy()
    net.profile(True)
    got = net(torch.from_numpy(x).to(gpu)).cpu().numpy()
    kernels = {e["name"] for e in net.read_profile()}
    net.profile(False)
    _check_logits(got, ref)
    # the large stride-1 layers of this forward run on the Winograd kernel F(2x2x2,3x3x3) (whole 4 x 8 x 8 tiles and enough of them:
    # levels 0 and 1 here), the last conv on its fused-head instantiation: the tolerance above is therefore the Winograd path's
    # tolerance, not only the direct kernels'
    import os
    if os.environ.get("MI355_WINOGRAD") != "0" and os.environ.get("MI355_CONV_IMPL") is None and os.environ.get("MI355_WINO3", "1") != "0":
        assert "conv3_f32_wino3_kernel<0, false>" in kernels and "conv3_f32_wino3_kernel<1, false>" in kernels, sorted(kernels)


def _small_net(amd, norm="batch", seed=21):
    sd, _ = amd.synthetic.make_model("A", seed=seed, num_pool=2, max_feat=128, norm=norm)
    return sd


@pytest.mark.parametrize("cfg", [
    dict(shape=(40, 56, 44), mirror=True, gaussian=True, nonlin="sigmoid"),    # 2x2x2 tiles, 8-way TTA
    dict(shape=(32, 70, 32), mirror=False, gaussian=True, nonlin="sigmoid"),   # 1x4x1 tiles, no TTA
    dict(shape=(20, 40, 30), mirror=True, gaussian=True, nonlin="softmax"),    # padded in z and x; softmax head
    dict(shape=(32, 32, 32), mirror=True, gaussian=True, nonlin="sigmoid"),    # single tile -> no gaussian
    dict(shape=(48, 33, 47), mirror=True, gaussian=False, nonlin="sigmoid", axes=(0, 2)),  # 4-way TTA subset
])
def test_sliding_window_matches_oracle(amd, gpu, cfg):
    sd = _small_net(amd)
    net = amd.UNet(sd, norm="batch")
    patch = (32, 32, 32)
    rs = np.random.RandomState(31)
    vol = rs.standard_normal((4,) + cfg["shape"]).astype(np.float32)
    axes = cfg.get("axes", (0, 1, 2))
    ref = tiler_ref.predict_3d_tiled(tiler_ref.make_net_fn(sd, unet_ref.default_cfg("batch")), vol, patch, 3, 0.5,
                                     cfg["mirror"], axes, cfg["gaussian"], cfg["nonlin"])
    got = amd.predictor.predict_folds([net], vol, patch, 0.5, cfg["mirror"], axes, cfg["gaussian"], cfg["nonlin"])
    got = got.cpu().numpy()
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= PROB_TOL
    if cfg["nonlin"] == "sigmoid":
        d = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(ref))
        assert d["mean"] >= 0.999
    # batching tiles differently must not change the result beyond fp32 noise (the launcher may pick another
    # kernel / channel-chunk size for another batch size, i.e. another summation order)
    got2 = amd.predictor.predict_folds([net], vol, patch, 0.5, cfg["mirror"], axes, cfg["gaussian"], cfg["nonlin"],
                                       batch_tiles=1).cpu().numpy()
    assert np.abs(got2 - got).max() <= 5e-5


def test_fold_mean_and_tile_sharding(amd, gpu):
    sds = [_small_net(amd, seed=s) for s in (21, 22, 23)]
    nets = [amd.UNet(sd, norm="batch") for sd in sds]
    patch = (32, 32, 32)
    vol = np.random.RandomState(8).standard_normal((4, 40, 48, 36)).astype(np.float32)
    per_fold = [tiler_ref.predict_3d_tiled(tiler_ref.make_net_fn(sd, unet_ref.default_cfg("batch")), vol, patch, 3)
                for sd in sds]
    ref = np.mean(per_fold, axis=0)  # driver :128
    got = amd.predictor.predict_folds(nets, vol, patch).cpu().numpy()
    assert np.abs(got - ref).max() <= PROB_TOL
    # tile-sharded path (what N ranks would do), summed in rank order
    world = 3
    parts = [amd.predictor.predict_tile_sharded(nets[0], vol, r, world, patch) for r in range(world)]
    agg = parts[0][0].clone()
    for r in range(1, world):
        agg += parts[r][0]
    probs = amd.predictor.finish_sharded(agg, parts[0][1], vol.shape[1:], patch).cpu().numpy()
    assert np.abs(probs - per_fold[0]).max() <= PROB_TOL
    for r in range(1, world):
        assert torch.equal(parts[r][1], parts[0][1])  # every rank holds the same normaliser


def test_fold_list_tile_sharding(amd, gpu):
    """mi355_sw_partial_folds (SURVEY.md 8e partitioning B over the reference's fold list, driver :161): the (fold, tile) work
    list of three folds x 2x2x2 tiles dealt over 1, 3 and 5 ranks; the rank-ordered sum of the partial aggregates, normalised
    once and divided by the fold count, equals the fold mean of mi355_sw_predict (up to the fp32 rounding of the division
    order) and the oracle's np.mean of per-fold predictions (driver :128)."""
    sds = [_small_net(amd, seed=s) for s in (21, 22, 23)]
    nets = [amd.UNet(sd, norm="batch") for sd in sds]
    patch = (32, 32, 32)
    vol = np.random.RandomState(8).standard_normal((4, 40, 48, 36)).astype(np.float32)
    ref = np.mean([tiler_ref.predict_3d_tiled(tiler_ref.make_net_fn(sd, unet_ref.default_cfg("batch")), vol, patch, 3) for sd in sds], axis=0)
    want = amd.predictor.predict_folds(nets, vol, patch)
    assert amd.parallel.shard_fold_tiles(3, 8, 1, 5) == [(0, 1), (0, 6), (1, 3), (2, 0), (2, 5)]
    for world in (1, 3, 5):
        parts = [amd.predictor.predict_tile_sharded(nets, vol, r, world, patch) for r in range(world)]
        agg = parts[0][0].clone()
        for r in range(1, world):
            agg += parts[r][0]
            assert torch.equal(parts[r][1], parts[0][1])  # every rank holds the same one-fold normaliser
        probs = amd.predictor.finish_sharded(agg, parts[0][1], vol.shape[1:], patch, n_folds=3)
        assert float((probs - want).abs().max()) <= 2e-6, world
        assert np.abs(probs.cpu().numpy() - ref).max() <= PROB_TOL
    for n in nets:
        n.close()


def test_lanes_agree_with_the_single_stream_path(amd, gpu):
    """Round 5: predict_folds / predict_members over two (three) HIP streams of one GPU - the library keeps an activation arena and
    scratch per stream - against the single-stream mi355_sw_predict: 2 folds x 2x2x2 tiles x 8 mirrors = 128 samples (enough
    for the sample rule of the lane split), fp32.  The lane-ordered sum of the partial aggregates differs from the in-order sum
    by fp32 rounding only; predict_members (staggered member order) equals per-member predict_folds on lanes bit for bit; two
    DIFFERENT networks run on two user streams at once and give what they give one after the other."""
    sds = [_small_net(amd, seed=s) for s in (21, 22)]
    nets = [amd.UNet(sd, norm="batch") for sd in sds]
    other = [amd.UNet(_small_net(amd, seed=s), norm="batch") for s in (23, 24)]
    patch = (32, 32, 32)
    vol = torch.from_numpy(np.random.RandomState(8).standard_normal((4, 40, 48, 36)).astype(np.float32)).to(gpu)
    one = amd.predictor.predict_folds(nets, vol, patch, lanes=1)
    for lanes in (2, 3):
        got = amd.predictor.predict_folds(nets, vol, patch, lanes=lanes)
        assert float((got - one).abs().max()) <= 5e-6, lanes   # (measured 2.3e-6 at three lanes: sum-then-normalise against normalise-then-mean)
    both = amd.predictor.predict_members([nets, other], vol, patch, lanes=2)
    assert torch.equal(both[0], amd.predictor.predict_folds(nets, vol, patch, lanes=2))
    assert torch.equal(both[1], amd.predictor.predict_folds(other, vol, patch, lanes=2))
    # two user streams, one network each, enqueued back to back: separate arenas, no interference
    want = [amd.predictor.predict_folds(n, vol, patch, lanes=1) for n in (nets, other)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [None, None]
    for _ in range(3):
        for i, (st, n) in enumerate(zip(streams, (nets, other))):
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                outs[i] = amd.predictor.predict_folds(n, vol, patch, lanes=1)
        for st in streams:
            torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])
    # more streams than the library has lanes (4): the sixth takes over the least recently used lane after a device synchronise
    for k in range(6):
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            got = amd.predictor.predict_folds(nets if k % 2 == 0 else other, vol, patch, lanes=1)
        torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        assert torch.equal(got, want[k % 2]), k
    for n in nets + other:
        n.close()


# --------------------------------------------------------------------------- fp16 storage (BASELINE configs[2])
# Tolerance for the fp16 path, stated here as the north_star asks: activations are rounded to fp16 (2^-11 relative)
# after every block, accumulation stays fp32.  Against the fp32 CPU oracle we require the north_star's gate, Dice >= 0.999
# of the label maps on ALL voxels, logits within 3 % of their spread and probabilities within 0.05 (0.08 for the one case
# below whose InstanceNorm statistics at the bottleneck are taken over 2^3 = 8 voxels, which amplifies any perturbation;
# the reference's 128^3 patches have 64).  Measured on MI355X (round 2): logits 0.5-2.1 % of the spread, probabilities
# 0.016-0.063, Dice 0.99943-0.99976; with 8-way TTA at 128^3 probabilities 3.8e-3 / 4.5e-3, Dice 0.99984 / 0.99959.
def _check_logits_f16(got, ref, dice_all=0.999, prob_tol=0.05):
    spread = float(ref.std())
    err = float(np.abs(got - ref).max())
    assert err <= 3e-2 * max(spread, 1.0), f"fp16 logit max abs err {err} (spread {spread})"
    pg = 1 / (1 + np.exp(-got.astype(np.float64)))
    pr = 1 / (1 + np.exp(-ref.astype(np.float64)))
    assert float(np.abs(pg - pr).max()) <= prob_tol
    lg, lr = tiler_ref.regions_to_labels(pg[0].astype(np.float32)), tiler_ref.regions_to_labels(pr[0].astype(np.float32))
    d_all = tiler_ref.brats_region_dice(lg, lr)["mean"]
    print(f"PARITY f16: logit err {err / max(spread, 1.0):.2e} x spread, prob err {float(np.abs(pg - pr).max()):.3f}, Dice {d_all:.6f}")
    assert d_all >= dice_all
    sure = (np.abs(ref[0]) >= 1.0).all(0)
    assert tiler_ref.brats_region_dice(lg[sure], lr[sure])["mean"] >= 0.999
    return err / spread


@pytest.mark.parametrize("name", ["A", "A_in", "B"])
def test_forward_f16_64_matches_oracle(amd, gpu, name):
    sd, meta = amd.synthetic.make_model(name, seed=7)
    net = amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"], dtype="f16")
    x = np.random.RandomState(1).standard_normal((1, 4, 64, 64, 64)).astype(np.float32)
    ref = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm=meta["norm"], num_groups=meta["num_groups"])).numpy()
    net.profile(True)
    got = net(torch.from_numpy(x).to(gpu)).cpu().numpy()
    kernels = {e["name"] for e in net.read_profile()}
    net.profile(False)
    rel = _check_logits_f16(got, ref, prob_tol=0.08 if name == "A_in" else 0.05)
    print(f"fp16 {name}: max logit err / spread = {rel:.2e}")
    # round 5: the Cout = 32 layers of the full-resolution level (512 tiles of 8^3 at 64^3) run on the LDS-DMA kernel with two
    # workgroups per CU - model A incl. its fused-head instantiation, the Instance/GroupNorm models incl. the one that normalises
    # its producer's output in LDS and carries the statistics epilogue
    import os
    if not any(k in os.environ for k in ("MI355_CONV_IMPL", "MI355_F16_DMA", "MI355_F16_C32", "MI355_FUSE_NORM", "MI355_FUSE_HEAD")):
        want = {"A": {"conv3_f16_c32_kernel<false, false, false>", "conv3_f16_c32_kernel<false, false, true>"},
                "A_in": {"conv3_f16_c32_kernel<true, true, false>"}, "B": {"conv3_f16_c32_kernel<true, true, false>"}}[name]
        assert want <= kernels, sorted(kernels)
    net.close()


def test_forward_f16_batch_ragged_and_simple_kernel(amd, gpu, monkeypatch):
    sd, meta = amd.synthetic.make_model("A_in", seed=3, num_pool=3, max_feat=128)
    x = np.random.RandomState(4).standard_normal((3, 4, 32, 64, 96)).astype(np.float32)
    ref = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm="instance")).numpy()
    net = amd.UNet(sd, norm="instance", dtype="f16")
    got = net(torch.from_numpy(x).to(gpu)).cpu().numpy()
    for n in range(3):
        _check_logits_f16(got[n:n + 1], ref[n:n + 1])


def test_f16_fused_input_norm_agrees_with_the_separate_pass(amd, gpu):
    """The Instance/GroupNorm of a stage's first conv is applied by the second conv while it stages its input (no
    norm_apply pass).  Same math as the separate pass except that scale and shift are rounded to fp16: the logits of the
    two builds agree to a small fraction of the fp16 path's own error against the oracle.  The switch is read once per
    process, so the un-fused build runs in a child process."""
    import os
    import subprocess
    import sys
    import tempfile
    code = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
sd, meta = brats_amd.synthetic.make_model("B", seed=7)
net = brats_amd.UNet(sd, norm="group", num_groups=16, dtype="f16")
x = np.random.RandomState(1).standard_normal((1, 4, 64, 64, 64)).astype(np.float32)
net.profile(True)
y = net(torch.from_numpy(x).cuda()).cpu().numpy()
names = sorted(e["name"] for e in net.read_profile())
np.savez(sys.argv[1], y=y, names=np.array(names))
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for flag in ("1", "0"):
            path = os.path.join(td, f"y{flag}.npz")
            res = subprocess.run([sys.executable, "-c", code % root, path], env=dict(os.environ, MI355_FUSE_NORM=flag),
                                 capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
            outs[flag] = np.load(path)
    fused, plain = outs["1"], outs["0"]
    def inaff(n):  # conv3_f16_mfma_pipe_kernel<MF, NF, HEAD, INAFF, STRIDE, WHOLE> / conv3_f16_dma_kernel<STATS, INAFF>
        return (("pipe_kernel<" in n and n.split("<")[1].split(",")[3].strip() == "true") or ("dma_kernel<" in n and n.endswith(", true>")) or
                ("c32_kernel<" in n and n.split("<")[1].split(",")[1].strip() == "true"))   # conv3_f16_c32_kernel<STATS, INAFF, HEAD>
    assert any(inaff(n) for n in fused["names"]), list(fused["names"])         # the INAFF kernels ran ...
    assert any("dma_kernel<" in n and inaff(n) for n in fused["names"]), list(fused["names"])   # ... the in-LDS variant among them
    assert not any(inaff(n) for n in plain["names"])
    spread = float(plain["y"].std())
    err = float(np.abs(fused["y"] - plain["y"]).max())
    print(f"PARITY fused-vs-separate norm (f16, B 64^3): {err / spread:.2e} x spread")
    # gate re-derived in round 4 from four input seeds (tests/diagnostics/gate_seeds.py, profiles/r04_gate_seeds.txt): 7.7e-3, 7.7e-3,
    # 8.4e-3, 8.4e-3 x spread (this seed: 8.4e-3) - what any 2^-11 perturbation of an early activation grows to; each build is
    # within 6.9e-3 .. 8.2e-3 of the oracle on the same inputs.  1.2e-2 = 1.4 x the largest of the four.
    assert err <= 1.2e-2 * spread


def test_f32_fused_input_norm_agrees_with_the_separate_pass(amd, gpu):
    """Round 4: on the fp32 path the Instance/GroupNorm (+ LeakyReLU) of a stage's first conv is applied by the second conv when that
    conv runs on the F(2x2x2,3x3x3) kernel, which normalises its brick in LDS (conv3_f32_wino3_kernel<2, true>): the same fp32
    arithmetic as the separate norm_apply pass (one fma, max(y, slope y)), so the two builds agree to summation-order noise and
    each is within the file's fp32 gate of the oracle.  The switch is read once per process: one child per setting."""
    import os
    import subprocess
    import sys
    import tempfile
    code = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
sd, meta = brats_amd.synthetic.make_model("B", seed=7)
net = brats_amd.UNet(sd, norm="group", num_groups=16)
x = np.random.RandomState(1).standard_normal((2, 4, 64, 64, 64)).astype(np.float32)
net.profile(True)
y = net(torch.from_numpy(x).cuda()).cpu().numpy()
prof = net.read_profile()
np.savez(sys.argv[1], y=y, names=np.array(sorted(e["name"] for e in prof)), norm_launches=sum(e["launches"] for e in prof if e["name"].startswith("norm_apply")))
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for flag in ("1", "0"):
            path = os.path.join(td, f"y{flag}.npz")
            res = subprocess.run([sys.executable, "-c", code % root, path], env=dict(os.environ, MI355_FUSE_NORM=flag),
                                 capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
            outs[flag] = np.load(path)
    fused, plain = outs["1"], outs["0"]
    assert "conv3_f32_wino3_kernel<2, true>" in list(fused["names"]), list(fused["names"])
    assert "conv3_f32_wino3_kernel<2, true>" not in list(plain["names"])
    assert int(fused["norm_launches"]) < int(plain["norm_launches"])     # the deferred blocks' separate passes are gone
    sd, meta = amd.synthetic.make_model("B", seed=7)
    x = np.random.RandomState(1).standard_normal((2, 4, 64, 64, 64)).astype(np.float32)
    ref = unet_ref.unet_forward(sd, x, unet_ref.default_cfg(norm="group", num_groups=16)).numpy()
    _check_logits(fused["y"], ref, "64^3 B f32, norm fused into the consumer")
    _check_logits(plain["y"], ref, "64^3 B f32, separate norm pass")
    spread = float(ref.std())
    err = float(np.abs(fused["y"] - plain["y"]).max())
    print(f"PARITY fused-vs-separate norm (f32, B 64^3): {err / spread:.2e} x spread")
    assert err <= LOGIT_REL_TOL * spread


def test_sliding_window_f16_tta(amd, gpu):
    sd = _small_net(amd)
    net = amd.UNet(sd, norm="batch", dtype="f16")
    patch = (32, 32, 32)
    vol = np.random.RandomState(31).standard_normal((4, 40, 56, 44)).astype(np.float32)
    ref = tiler_ref.predict_3d_tiled(tiler_ref.make_net_fn(sd, unet_ref.default_cfg("batch")), vol, patch, 3)
    got = amd.predictor.predict_folds([net], vol, patch).cpu().numpy()
    assert np.abs(got - ref).max() <= 5e-2
    d = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(ref))
    assert d["mean"] >= 0.999


# --------------------------------------------------------------------------- full BASELINE size
def test_full_size_config2_properties_and_oracle_tiles(amd, gpu):
    """BASELINE.json configs[1] at full size (4x155x240x240 synthetic case, model A, 128^3 tiles, no TTA):
    size-independent properties of the whole path + the CPU oracle on two of the eight tiles."""
    sd, meta = amd.synthetic.make_model("A", seed=7)
    net = amd.UNet(sd, norm="batch")
    raw = amd.synthetic.make_volume(seed=1000)
    data, props = amd.preprocessing.preprocess_case(raw)
    patch = (128, 128, 128)
    kw = dict(patch_size=patch, step_size=0.5, do_mirroring=False, use_gaussian=True, nonlin="sigmoid")
    p1 = amd.predictor.predict_folds([net], data, **kw)
    assert p1.shape == (3,) + tuple(data.shape[1:]) and bool(torch.isfinite(p1).all())
    assert float(p1.min()) >= 0.0 and float(p1.max()) <= 1.0
    # (1) determinism: a second run is bit-identical (no atomics on the BN-folded path)
    assert torch.equal(amd.predictor.predict_folds([net], data, **kw), p1)
    # (2) batching invariance: one tile per forward instead of eight
    p_b1 = amd.predictor.predict_folds([net], data, batch_tiles=1, **kw)
    assert float((p_b1 - p1).abs().max()) <= 5e-5
    # (3) mirror equivariance of the whole sliding window: flipping the volume along x and predicting with the
    #     x-mirror-only TTA schedule visits the same forwards -> probabilities are the flipped ones.  Uniform
    #     tile weights here: nnU-Net's Gaussian is centred on index patch//2 = 64 of 128, i.e. not mirror-symmetric
    kw_tta = dict(kw, do_mirroring=True, mirror_axes=(2,), use_gaussian=False)
    pa = amd.predictor.predict_folds([net], data, **kw_tta)
    pb = amd.predictor.predict_folds([net], torch.flip(data, (3,)).contiguous(), **kw_tta)
    assert float((torch.flip(pb, (3,)) - pa).abs().max()) <= 2e-4
    # (4) labels, pasted into the raw-size volume
    lo = [b[0] for b in props["crop_bbox"]]
    seg = amd.ops.regions_to_labels(p1, (1, 2, 3), lo, props["original_size_of_raw_data"]).cpu().numpy()
    assert seg.shape == (155, 240, 240) and set(np.unique(seg)) <= {0, 1, 2, 3}
    outside = np.ones_like(seg, dtype=bool)
    outside[tuple(slice(b[0], b[1]) for b in props["crop_bbox"])] = False
    assert not seg[outside].any()
    # (5) CPU oracle on the first and the last tile of the step table (2 x ~4 s of CPU forwards)
    cfg = unet_ref.default_cfg("batch")
    host = data.cpu().numpy()
    steps = tiler_ref.compute_steps_for_sliding_window(patch, host.shape[1:], 0.5)
    for z0, y0, x0 in ((steps[0][0], steps[1][0], steps[2][0]), (steps[0][-1], steps[1][-1], steps[2][-1])):
        tile = np.ascontiguousarray(host[None, :, z0:z0 + 128, y0:y0 + 128, x0:x0 + 128])
        ref = unet_ref.unet_forward(sd, tile, cfg).numpy()
        got = net(torch.from_numpy(tile).to(gpu)).cpu().numpy()
        _check_logits(got, ref)
        d = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(1 / (1 + np.exp(-got[0]))),
                                        tiler_ref.regions_to_labels(1 / (1 + np.exp(-ref[0]))))
        assert d["mean"] >= 0.999


def test_full_size_config3_f16_agrees_with_f32(amd, gpu):
    """BASELINE.json configs[2] at full size (8-way mirror TTA, models A + B, label-round ensemble): a CONSISTENCY check of
    the fp16 path against the fp32 path of the same library over all 8 tiles (Dice of the ensembled label maps >= 0.999).
    The oracle's own verdict on this configuration is test_tta_full_tile_matches_oracle / test_forward_128_model_b_* below
    (one full 128^3 tile per model, fp32 and fp16, against the CPU oracle)."""
    raw = amd.synthetic.make_volume(seed=1001)
    data, props = amd.preprocessing.preprocess_case(raw)
    lo = [b[0] for b in props["crop_bbox"]]
    kw = dict(patch_size=(128, 128, 128), step_size=0.5, do_mirroring=True, mirror_axes=(0, 1, 2), use_gaussian=True, nonlin="sigmoid")
    segs = {}
    for dtype in ("f32", "f16"):
        per_model = []
        for name, seed in (("A", 7), ("B", 8)):
            sd, meta = amd.synthetic.make_model(name, seed=seed)
            net = amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"], dtype=dtype)
            probs = amd.predictor.predict_folds([net], data, **kw)
            assert bool(torch.isfinite(probs).all())
            per_model.append(amd.ops.regions_to_labels(probs, (1, 2, 3), lo, props["original_size_of_raw_data"]))
            net.close()
        segs[dtype] = amd.ops.label_ensemble(per_model[0], per_model[1]).cpu().numpy()
    d = tiler_ref.brats_region_dice(segs["f16"], segs["f32"])
    assert d["mean"] >= 0.999, d
    assert set(np.unique(segs["f16"])) <= {0, 1, 2, 3}


# --------------------------------------------------------------------------- the reference's real setting at full size
# run_brats2021_inference_singlethread.py:208-211 (do_tta=True) and :263-264 (both ensemble members): one full 128^3
# tile against the CPU oracle for model B (GroupNorm-16, encoder_scale=2, 3.34 TFLOP per forward) in fp32 and fp16, and
# the 8-way mirror TTA of one tile through the sliding-window entry point for models A and B.
@pytest.fixture(scope="module")
def tile128():
    return np.random.RandomState(2).standard_normal((1, 4, 128, 128, 128)).astype(np.float32)


@pytest.fixture(scope="module")
def oracle_b_128(amd, tile128):
    sd, meta = amd.synthetic.make_model("B", seed=8)
    ref = unet_ref.unet_forward(sd, tile128, unet_ref.default_cfg(norm="group", num_groups=16)).numpy()
    return sd, ref


def test_forward_128_model_b_f32(amd, gpu, tile128, oracle_b_128):
    sd, ref = oracle_b_128
    net = amd.UNet(sd, norm="group", num_groups=16)
    got = net(torch.from_numpy(tile128).to(gpu)).cpu().numpy()
    _check_logits(got, ref, "128^3 B f32")
    d = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(1 / (1 + np.exp(-got[0]))), tiler_ref.regions_to_labels(1 / (1 + np.exp(-ref[0]))))
    assert d["mean"] >= 0.999
    net.close()


def test_forward_128_model_b_f16(amd, gpu, tile128, oracle_b_128):
    """fp16 storage at the size the reference runs: the north_star gate (Dice >= 0.999 against the CPU path)."""
    sd, ref = oracle_b_128
    net = amd.UNet(sd, norm="group", num_groups=16, dtype="f16")
    got = net(torch.from_numpy(tile128).to(gpu)).cpu().numpy()
    rel = _check_logits_f16(got, ref, dice_all=0.999)
    print(f"PARITY 128^3 B f16: max logit err / spread = {rel:.2e}")
    net.close()


@pytest.mark.parametrize("name,seed", [("A", 7), ("B", 8)])
def test_tta_full_tile_matches_oracle(amd, gpu, tile128, name, seed):
    """8 mirrored forwards of one 128^3 volume (= one tile, so no Gaussian: nnU-Net's single-tile case), summed with
    weight 1/8 after flipping back, against tiler_ref.mirror_and_predict on the CPU (8 x 4 s / 8 x 10 s of oracle)."""
    sd, meta = amd.synthetic.make_model(name, seed=seed)
    cfg = unet_ref.default_cfg(norm=meta["norm"], num_groups=meta["num_groups"])
    net_fn = tiler_ref.make_net_fn(sd, cfg)
    ref = tiler_ref.mirror_and_predict(net_fn, torch.from_numpy(tile128), (0, 1, 2), True, "sigmoid", None)[0].numpy()
    for dtype, tol, dice_min in (("f32", 1e-4, 0.9999), ("f16", 2e-2, 0.999)):
        net = amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"], dtype=dtype)
        got = amd.predictor.predict_folds([net], tile128[0], (128, 128, 128), 0.5, True, (0, 1, 2), True, "sigmoid").cpu().numpy()
        err = float(np.abs(got - ref).max())
        d = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(ref))
        print(f"PARITY TTA 128^3 {name} {dtype}: prob err {err:.2e}, Dice {d['mean']:.6f}")
        assert err <= tol and d["mean"] >= dice_min
        net.close()


def test_five_fold_mean_at_full_patch(amd, gpu, tile128):
    """The reference's fold mean at the size it runs (run_brats2021_inference_singlethread.py:161 folds=(0, 1, 2, 3, 4),
    :112-128: one prediction per fold, np.mean over them) WITHOUT the mirrors it also runs: five model-A folds (seeds 7..11)
    through predict_folds on one 128^3 Gaussian-noise volume (= one tile) against the mean of five CPU-oracle forwards.
    fp32 is gated at the north_star's tolerances.  For fp16 this is a DIAGNOSTIC of the least stable label map the suite can
    produce, not the reference's setting (that is test_reference_fold_ensemble_with_tta below, gated at Dice >= 0.999): the
    mean of five INDEPENDENT random-weight folds on a noise volume has its decision surface wherever the folds split 2 : 2,
    and without the eight mirrors nothing averages the fp16 rounding down.  Measured (round 3): all-voxel Dice 0.99898,
    probabilities within 8.0e-3.  Gated for fp16: probabilities within 2e-2 and Dice >= 0.9999 on the voxels whose reference
    mean is at least 0.05 away from the threshold; the all-voxel Dice is printed."""
    sds = [amd.synthetic.make_model("A", seed=7 + k)[0] for k in range(5)]
    cfg = unet_ref.default_cfg(norm="batch")
    x = torch.from_numpy(tile128)
    ref = np.mean([torch.sigmoid(unet_ref.unet_forward(sd, x, cfg))[0].numpy() for sd in sds], axis=0)  # driver :128
    for dtype, tol in (("f32", PROB_TOL), ("f16", 2e-2)):
        nets = [amd.UNet(sd, norm="batch", dtype=dtype) for sd in sds]
        got = amd.predictor.predict_folds(nets, tile128[0], (128, 128, 128), 0.5, False, (0, 1, 2), True, "sigmoid").cpu().numpy()
        err = float(np.abs(got - ref).max())
        lg, lr = tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(ref)
        d = tiler_ref.brats_region_dice(lg, lr)
        sure = (np.abs(ref - 0.5) >= 0.05).all(0)
        d_sure = tiler_ref.brats_region_dice(lg[sure], lr[sure])
        print(f"PARITY 5-fold mean 128^3 A {dtype} (no TTA): prob err {err:.2e}, Dice {d['mean']:.6f} (clear voxels {d_sure['mean']:.6f})")
        assert err <= tol and d_sure["mean"] >= 0.9999
        if dtype == "f32":
            assert d["mean"] >= 0.9999
        else:
            # numeric floor for the all-voxel figure: this seed set reads 0.998977; over 5 weight-seed sets x 2 noise
            # tiles the setting ranges 0.99898 - 0.99995 (profiles/r05_f16_seed_study_noise_tiles.txt: noise tiles are the
            # ill-conditioned case - on brain tiles the same setting never reads below 0.99941).  0.9985 = the minimum - 5e-4.
            assert d["mean"] >= 0.9985
        for n in nets:
            n.close()


@pytest.fixture(scope="module")
def brain_block(amd, gpu):
    """A 64 x 64 x 96 block of bench.py's synthetic brain volume (synthetic.make_volume(1000), cropped and z-scored on the
    device): smooth tissue, part of the ellipsoid's surface and the exact zeros outside it."""
    data, _ = amd.preprocessing.preprocess_case(amd.synthetic.make_volume(seed=1000), gpu)
    return data[:, 40:104, 50:114, 0:96].contiguous().cpu().numpy()


@pytest.mark.parametrize("name,seed0,shape", [("A", 7, (64, 64, 96)), ("B", 8, (64, 64, 64))])
def test_reference_fold_ensemble_with_tta(amd, gpu, brain_block, name, seed0, shape):
    """The fold ensemble AS THE REFERENCE RUNS IT (run_brats2021_inference_singlethread.py:161 folds=(0, 1, 2, 3, 4); :208-211
    do_tta=True -> 8 mirrors; :112-128 one sliding-window prediction per fold, np.mean over the five), fp32 and fp16, against
    the CPU oracle with the north_star's gate on ALL voxels: Dice >= 0.999 (fp32: probabilities within 1e-3 as well).
    Sized for the suite: 64^3 patches (the smallest this topology takes) on a brain-like block - model A: 64 x 64 x 96 ->
    two Gaussian-blended tiles, 80 oracle forwards; model B (GroupNorm-16, 3.5 x the flops): one tile, 40 forwards."""
    data = np.ascontiguousarray(brain_block[:, :shape[0], :shape[1], :shape[2]])
    patch = (64, 64, 64)
    sds, meta = [], None
    for k in range(5):
        sd, meta = amd.synthetic.make_model(name, seed=seed0 + k)
        sds.append(sd)
    cfg = unet_ref.default_cfg(norm=meta["norm"], num_groups=meta["num_groups"])
    per_fold = [tiler_ref.predict_3d_tiled(tiler_ref.make_net_fn(sd, cfg), data, patch, 3, 0.5, True, (0, 1, 2), True, "sigmoid")
                for sd in sds]
    ref = np.mean(per_fold, axis=0)  # driver :128
    lr = tiler_ref.regions_to_labels(ref)
    assert lr.any(), "the block must contain foreground labels for the Dice to mean anything"
    for dtype, tol in (("f32", PROB_TOL), ("f16", 2e-2)):
        nets = [amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"], dtype=dtype) for sd in sds]
        got = amd.predictor.predict_folds(nets, data, patch, 0.5, True, (0, 1, 2), True, "sigmoid").cpu().numpy()
        for n in nets:
            n.close()
        err = float(np.abs(got - ref).max())
        lg = tiler_ref.regions_to_labels(got)
        d = tiler_ref.brats_region_dice(lg, lr)
        print(f"PARITY reference setting (5 folds x 8 mirrors, fold mean) {name} {dtype}: prob err {err:.2e}, "
              f"{int((lg != lr).sum())} of {lr.size} labels differ, Dice WT/TC/ET {d['WT']:.6f} {d['TC']:.6f} {d['ET']:.6f} mean {d['mean']:.6f}")
        assert err <= tol, (dtype, err)
        assert d["mean"] >= 0.999 and min(d["WT"], d["TC"], d["ET"]) >= 0.999, (dtype, d)   # north_star, un-lowered


@pytest.fixture(scope="module")
def bench_tile(amd, gpu):
    """The first 128^3 tile of bench.py's timed synthetic brain volume (synthetic.make_volume(1000), cropped and z-scored on
    the device): smooth low-frequency tissue inside an ellipsoidal mask, exact zeros outside - not Gaussian noise."""
    data, _ = amd.preprocessing.preprocess_case(amd.synthetic.make_volume(seed=1000), gpu)
    steps = [amd.ops.compute_steps(128, max(128, data.shape[1 + a]), 0.5) for a in range(3)]
    t = data[:, steps[0][0]:steps[0][0] + 128, steps[1][0]:steps[1][0] + 128, steps[2][0]:steps[2][0] + 128]
    pad = [128 - t.shape[1 + i] for i in range(3)]
    return torch.nn.functional.pad(t, (0, pad[2], 0, pad[1], 0, pad[0]))[None].contiguous().cpu().numpy()


@pytest.mark.parametrize("name,seed", [("A", 7), ("B", 8)])
def test_bench_tile_f16_margin(amd, gpu, bench_tile, name, seed):
    """VERDICT r2 (weak #2): the fp16 gates were only ever applied to Gaussian-noise tiles; this is the tile the bench's
    parity block uses.  Gates: the north_star's Dice >= 0.999 on all voxels, logits within 7 % of their spread, and
    probabilities within 0.15 - on this tile 0.6 % of the logits lie within 0.05 of the decision threshold (the synthetic
    seg head is scaled for confident logits, but a brain-shaped input leaves a wide transition band), where a logit error
    of 0.8 (6 % of the spread, the worst voxel of 6 M) moves a probability by 0.11.  Measured (round 3, tests/diagnostics/f16_margin.py):
    A: logit max 0.49 / rms 0.013 of spread 24.2, probability 0.089, 575 of 2.1 M labels differ, Dice 0.999865;
    B: logit max 0.81 / rms 0.017 of spread 13.5, probability 0.113, 1875 labels, Dice 0.999498 - and 0.999538 with the
    producer's normalisation as a separate fp32 pass (MI355_FUSE_NORM=0): the fused fp16 scale / shift is not what the
    margin is made of, the 2^-11 rounding of ~50 stored activations is."""
    sd, meta = amd.synthetic.make_model(name, seed=seed)
    ref = unet_ref.unet_forward(sd, torch.from_numpy(bench_tile), unet_ref.default_cfg(norm=meta["norm"], num_groups=meta["num_groups"])).numpy()
    net = amd.UNet(sd, norm=meta["norm"], num_groups=meta["num_groups"], dtype="f16")
    got = net(torch.from_numpy(bench_tile).to(gpu)).cpu().numpy()
    net.close()
    spread = float(ref.std())
    err = np.abs(got.astype(np.float64) - ref)
    pg, pr = 1 / (1 + np.exp(-got.astype(np.float64))), 1 / (1 + np.exp(-ref.astype(np.float64)))
    lg, lr = tiler_ref.regions_to_labels(pg[0].astype(np.float32)), tiler_ref.regions_to_labels(pr[0].astype(np.float32))
    d = tiler_ref.brats_region_dice(lg, lr)
    print(f"PARITY bench tile {name} f16: logit err max {err.max():.3f} rms {np.sqrt((err ** 2).mean()):.4f} (spread {spread:.2f}), "
          f"prob err {np.abs(pg - pr).max():.3f}, {int((lg != lr).sum())} labels differ, Dice {d['mean']:.6f}")
    assert d["mean"] >= 0.999 and min(d["WT"], d["TC"], d["ET"]) >= 0.999, d
    assert err.max() <= 7e-2 * spread and np.sqrt((err ** 2).mean()) <= 3e-3 * spread
    assert np.abs(pg - pr).max() <= 0.15
    sure = (np.abs(ref[0]) >= 1.0).all(0)
    assert tiler_ref.brats_region_dice(lg[sure], lr[sure])["mean"] >= 0.9999
