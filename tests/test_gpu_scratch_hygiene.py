"""-m gpu: no result depends on what device scratch held before the call ("Scratch holds no state").

Every entry point that takes working memory from device_scratch (tests/scratch_util.py: one case each) runs
* after its slots were filled with a poison word (per case and pattern),
* after another size of itself, larger and smaller, with a fresh lane in front (the grow path reallocates in between),
* on a lane taken over from another stream (one stream more than the library has lanes),
and passes the gate of its existing test against that test's CPU reference each time; where that test asserts equality, the poisoned
run also equals the clean one bit for bit.  The two shared zero pages hold zeros after the convolutions that read them and at the
end of the module.  The network runs its forward and its sliding window on a poisoned arena, aggregation buffer and split-K
partials, and a sequence of three arena layouts over the same bytes.

Every case runs on a stream of this module's own through torch.cuda.stream; the poison is written by mi355_scratch_fill on that
stream, in front of the call it is meant for."""
import numpy as np
import pytest
import torch

import scratch_util as sx
import test_gpu_network as tn
from oracle import tiler_ref, unet_ref

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in sx.CASES]
POISON = [(c.name, w) for c in sx.CASES for w in c.patterns]
# cases whose scratch request follows the size of the input: the smaller-then-larger order must reallocate
GROWS = {"crop_mask": "SCR_CROP", "resize_axis_order3": "SCR_RESAMPLE", "label_components_6": "SCR_COMPONENTS", "binary_fill_holes": "SCR_QUALITY",
         "binary_morphology": "SCR_MORPHOLOGY", "cosine_topk": "SCR_TOPK", "conv_splitk_f32": "SCR_SPLITK_F32", "conv_splitk_f16": "SCR_SPLITK_F16"}


@pytest.fixture(scope="module")
def streams(amd, gpu):
    """one stream more than the library has lanes; [0] is the stream the per-case tests run on"""
    return [torch.cuda.Stream(device=gpu) for _ in range(amd.ops.SCRATCH_LANES + 1)]


def run(amd, gpu, name, which, stream):
    with torch.cuda.stream(stream):
        got = sx.BY_NAME[name].call(amd, gpu, sx.inputs_of(name, which))
    stream.synchronize()
    return got


def lane_owned(amd, slots):
    return [s for s in slots if s not in amd.ops.SCRATCH_SHARED]


def test_the_aids_report_and_refuse(amd, gpu, streams):
    ops = amd.ops
    fresh = torch.cuda.Stream(device=gpu)
    sizes = ops.scratch_sizes(fresh)
    assert list(sizes) == list(ops.SCRATCH_SLOTS)
    assert all(sizes[s] == 0 for s in lane_owned(amd, ops.SCRATCH_SLOTS)), "a stream without a lane reports its lane-owned slots as empty"
    assert ops.scratch_fill(None, 0xFFFFFFFF, fresh) == 0 and ops.scratch_sizes(fresh) == sizes, "filling claimed a lane or allocated"
    ops.scratch_release(fresh)
    for slot in ops.SCRATCH_SHARED:
        with pytest.raises(amd._lib.Mi355Error, match="zero page"):
            ops.scratch_fill(slot, 0xFFFFFFFF, streams[0])
    rc = amd._lib.load().mi355_scratch_fill(streams[0].cuda_stream, len(ops.SCRATCH_SLOTS), 0)
    assert rc == -1
    run(amd, gpu, "label_stats", 1, streams[0])
    assert ops.scratch_sizes(streams[0])["SCR_SMALL"] == 1 << 20
    assert ops.scratch_fill("SCR_SMALL", 0x5A5A5A5A, streams[0]) == 1 << 20
    ops.scratch_release(streams[0])
    assert all(v == 0 for s, v in ops.scratch_sizes(streams[0]).items() if s not in ops.SCRATCH_SHARED)


@pytest.mark.parametrize("name,word", POISON, ids=[f"{n}-{w:08x}" for n, w in POISON])
def test_poisoned_scratch(amd, gpu, streams, name, word):
    """clean run, every declared slot allocated, fill, run again: the second result passes the gate, and equals the first bit for
    bit where the op's own test asserts equality - at the larger and at the smaller shape."""
    case, st = sx.BY_NAME[name], streams[0]
    mine = lane_owned(amd, case.slots)
    for which in (0, 1):
        clean = run(amd, gpu, name, which, st)
        sx.check(name, which, clean)
        sizes = amd.ops.scratch_sizes(st)
        assert all(sizes[s] > 0 for s in case.slots), f"{name}: {[s for s in case.slots if not sizes[s]]} not allocated: the fill would be vacuous"
        # (a case whose only slot is a zero page has nothing of its own to poison: everything its lane holds is)
        filled = sum(amd.ops.scratch_fill(s, word, st) for s in mine) if mine else amd.ops.scratch_fill(None, word, st)
        assert not mine or filled >= sum(sizes[s] // 4 * 4 for s in mine) > 0
        again = run(amd, gpu, name, which, st)
        sx.check(name, which, again)
        if case.bit_repeatable:
            assert sx.bits(again) == sx.bits(clean), f"{name} at {case.shapes[which]}: the run on scratch full of {word:#010x} differs from the clean run"


@pytest.mark.parametrize("name", NAMES)
def test_stale_scratch_of_another_size(amd, gpu, streams, name):
    """fresh lane, larger then smaller; fresh lane, smaller then larger (the grow path reallocates between them): the plausible
    tables of another case are what the second call finds"""
    st = streams[0]
    amd.ops.scratch_release(st)
    sx.check(name, 0, run(amd, gpu, name, 0, st))
    big = amd.ops.scratch_sizes(st)
    sx.check(name, 1, run(amd, gpu, name, 1, st))
    assert amd.ops.scratch_sizes(st) == big, "the smaller call reallocated"
    amd.ops.scratch_release(st)
    sx.check(name, 1, run(amd, gpu, name, 1, st))
    small = amd.ops.scratch_sizes(st)
    sx.check(name, 0, run(amd, gpu, name, 0, st))
    after = amd.ops.scratch_sizes(st)
    assert all(after[s] >= small[s] for s in after)
    if name in GROWS:
        assert after[GROWS[name]] > small[GROWS[name]] > 0, f"{name}: {GROWS[name]} did not grow ({small[GROWS[name]]} -> {after[GROWS[name]]})"
    sx.check(name, 1, run(amd, gpu, name, 1, st))


def test_lane_takeover(amd, gpu, streams):
    """One stream more than lanes.  Streams 0..3 run a case each at its larger shape and then hold the four lanes; stream 4 runs
    every exact case at its smaller shape on the lane it takes from stream 0 (the least recently used), finding stream 0's tables;
    stream 0 comes back and takes stream 1's."""
    ops = amd.ops
    assert len(streams) == ops.SCRATCH_LANES + 1
    first = ["binary_fill_holes", "select_ranked", "masked_percentiles_multi", "largest_component"]
    assert len(first) == ops.SCRATCH_LANES and len(set(first)) == len(first)
    for st, name in zip(streams, first):
        sx.check(name, 0, run(amd, gpu, name, 0, st))
    for st, name in zip(streams, first):
        sizes = ops.scratch_sizes(st)
        assert all(sizes[s] > 0 for s in sx.BY_NAME[name].slots), f"stream of {name} lost its lane before the takeover"
    extra = streams[-1]
    assert all(v == 0 for s, v in ops.scratch_sizes(extra).items() if s not in ops.SCRATCH_SHARED)
    exact = [c.name for c in sx.CASES if c.exact]
    for name in exact:
        sx.check(name, 1, run(amd, gpu, name, 1, extra))
    assert all(v == 0 for s, v in ops.scratch_sizes(streams[0]).items() if s not in ops.SCRATCH_SHARED), "stream 0 kept a lane: nothing was taken over"
    assert ops.scratch_sizes(extra)["SCR_QUALITY"] > 0, "the lane came without stream 0's buffers"
    sx.check(first[0], 0, run(amd, gpu, first[0], 0, streams[0]))
    assert all(v == 0 for s, v in ops.scratch_sizes(streams[1]).items() if s not in ops.SCRATCH_SHARED)
    for st, name in zip(streams[2:4], first[2:4]):   # the two lanes nobody took still serve their streams
        sx.check(name, 0, run(amd, gpu, name, 0, st))
    for name in exact:
        sx.check(name, 1, run(amd, gpu, name, 1, extra))


def test_zero_pages_after_the_convolutions(amd, gpu, streams):
    for name in sx.CONV_CASES:
        sx.check(name, 1, run(amd, gpu, name, 1, streams[0]))
    sizes = amd.ops.scratch_sizes(streams[0])
    assert sizes["SCR_ZEROS"] == 256 and sizes["SCR_ZERO_BIAS"] == 4096 * 4, "the convolutions never asked for their zero pages"
    assert amd.ops.scratch_zero_pages() == (0, 0)


# ------------------------------------------------------------------------------------------------------------ network
PATCH = (32, 32, 32)
NETS = [("f32", "batch"), ("f32", "instance"), ("f16", "batch"), ("f16", "instance")]
NET_SLOTS = ("SCR_ARENA", "SCR_SW_AGG", "SCR_SPLITK_F32", "SCR_SPLITK_F16")
VOLUMES = {"odd": (41, 57, 43), "even": (40, 56, 44)}
# the profile entries of the sharing features' gathers, and the nets whose sliding window runs them (the others say so by not
# running them: fp16 and run-time norm statistics turn the sharing off)
GATHERS = ("stage0_gather_kernel", "extract_tiles_kernel merged-slabs", "extract_tiles_kernel skip-half", "stage0_mask_kernel")


@pytest.fixture(scope="module")
def nets(amd, gpu):
    made = {}
    for dtype, norm in NETS:
        sd, _ = amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128, norm=norm)
        made[dtype, norm] = (sd, amd.UNet(sd, norm=norm, dtype=dtype))
    yield made
    for _, net in made.values():
        net.close()


_FORWARD_REFS, _WINDOW_REFS = {}, {}


def forward_input(shape):
    return np.random.RandomState(int(np.prod(shape)) % 9973).standard_normal(shape).astype(np.float32)


def forward_ref(sd, norm, shape):
    if (norm, shape) not in _FORWARD_REFS:
        _FORWARD_REFS[norm, shape] = unet_ref.unet_forward(sd, forward_input(shape), unet_ref.default_cfg(norm=norm)).numpy()
    return _FORWARD_REFS[norm, shape]


def window_input(shape):
    return np.random.RandomState(60 + shape[0]).standard_normal((4,) + shape).astype(np.float32)


def window_ref(sd, norm, shape):
    if (norm, shape) not in _WINDOW_REFS:
        _WINDOW_REFS[norm, shape] = tiler_ref.predict_3d_tiled(tiler_ref.make_net_fn(sd, unet_ref.default_cfg(norm)), window_input(shape), PATCH, 3, 0.5,
                                                               True, (0, 1, 2), True, "sigmoid")
    return _WINDOW_REFS[norm, shape]


def check_forward(dtype, got, ref, what):
    """the gates of test_gpu_network.py: fp32 - probabilities within 1e-3 (and the logit bounds); fp16 - its own, per sample"""
    if dtype == "f32":
        tn._check_logits(got, ref, what)
    else:
        for n in range(got.shape[0]):
            tn._check_logits_f16(got[n:n + 1], ref[n:n + 1])


def check_window(dtype, got, ref, what):
    """test_sliding_window_matches_oracle (fp32: 1e-3) and test_sliding_window_f16_tta (fp16: 5e-2), Dice >= 0.999 for both"""
    err = float(np.abs(got - ref).max())
    dice = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(ref))["mean"]
    print(f"{what}: max probability error {err:.3e}, Dice {dice:.6f}")
    assert got.shape == ref.shape and err <= (tn.PROB_TOL if dtype == "f32" else 5e-2)
    assert dice >= 0.999


def fill_net_slots(amd, word, on):
    return {s: sum(amd.ops.scratch_fill(s, word, st) for st in on) for s in NET_SLOTS}


@pytest.mark.parametrize("dtype,norm", NETS)
def test_forward_on_a_poisoned_arena(amd, gpu, streams, nets, dtype, norm):
    """forward at batch 2 on a 32^3 tile; the arena and both split-K slots filled with zeros, then with 0xFFFFFFFF: both runs are
    the same bits, and pass the gate"""
    sd, net = nets[dtype, norm]
    st, shape = streams[0], (2, 4) + PATCH
    ref = forward_ref(sd, norm, shape)
    out = {}
    with torch.cuda.stream(st):
        x = torch.from_numpy(forward_input(shape)).to(gpu)
        check_forward(dtype, net(x).cpu().numpy(), ref, f"{dtype} {norm} clean")
        assert amd.ops.scratch_sizes(st)["SCR_ARENA"] > 0
        for word in (0, 0xFFFFFFFF):
            filled = fill_net_slots(amd, word, [st])
            assert filled["SCR_ARENA"] > 0
            out[word] = net(x).cpu().numpy()
    print(f"forward {dtype} {norm}: bytes filled {filled}")
    check_forward(dtype, out[0xFFFFFFFF], ref, f"{dtype} {norm} poisoned")
    assert np.array_equal(out[0].view(np.uint32), out[0xFFFFFFFF].view(np.uint32)), "the forward on an arena full of NaN differs from the one on zeros"


@pytest.mark.parametrize("dtype,norm", NETS)
def test_forward_over_three_arena_layouts(amd, gpu, streams, nets, dtype, norm):
    """64 x 32 x 32, then 32^3 at batch 1, then 32^3 at batch 2, nothing cleared in between: the arena is laid out three ways over
    the same bytes"""
    sd, net = nets[dtype, norm]
    st = streams[0]
    amd.ops.scratch_release(st)
    with torch.cuda.stream(st):
        for shape in ((1, 4, 64, 32, 32), (1, 4) + PATCH, (2, 4) + PATCH):
            got = net(torch.from_numpy(forward_input(shape)).to(gpu)).cpu().numpy()
            check_forward(dtype, got, forward_ref(sd, norm, shape), f"{dtype} {norm} {shape}")


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("volume", sorted(VOLUMES))
@pytest.mark.parametrize("dtype,norm", NETS)
def test_sliding_window_on_poisoned_scratch(amd, gpu, streams, nets, dtype, norm, volume, lanes):
    """predict_folds with mirroring and the sharing switches at their defaults; between two calls the arena, the aggregation
    buffer and the split-K partials of every stream the call uses are filled.  One lane: mi355_sw_predict on this module's stream
    (the aggregation lives in SCR_SW_AGG); two lanes: the predictor's own lane streams (the aggregates are the caller's tensors)."""
    sd, net = nets[dtype, norm]
    st, shape = streams[0], VOLUMES[volume]
    ref = window_ref(sd, norm, shape)
    vol = window_input(shape)
    used = [st] if lanes == 1 else list(amd.predictor._lane_streams(gpu, lanes))
    out = {}
    with torch.cuda.stream(st):
        net.profile(True)
        clean = amd.predictor.predict_folds([net], vol, PATCH, 0.5, True, (0, 1, 2), True, "sigmoid", lanes=lanes).cpu().numpy()
        kernels = sorted(e["name"] for e in net.read_profile())
        net.profile(False)
        for s in used:
            sizes = amd.ops.scratch_sizes(s)
            assert sizes["SCR_ARENA"] > 0 and (lanes > 1 or sizes["SCR_SW_AGG"] > 0), sizes
        for word in (0, 0xFFFFFFFF):
            filled = fill_net_slots(amd, word, used)
            assert filled["SCR_ARENA"] > 0 and (lanes > 1 or filled["SCR_SW_AGG"] > 0)
            out[word] = amd.predictor.predict_folds([net], vol, PATCH, 0.5, True, (0, 1, 2), True, "sigmoid", lanes=lanes).cpu().numpy()
    ran = [g for g in GATHERS if g in kernels] + sorted(k for k in kernels if "_view<" in k)
    print(f"sliding window {dtype} {norm} {shape} lanes {lanes}: sharing kernels {ran}, bytes filled {filled}")
    # what this case covered: the fp32 batch-norm net runs on the shared stage 0 (gathered shells, merged slabs), the others on none of it
    if dtype == "f32" and norm == "batch":
        assert {"stage0_gather_kernel", "extract_tiles_kernel merged-slabs"} <= set(ran), kernels
    else:
        assert ran == [], ran
    check_window(dtype, clean, ref, "clean")
    check_window(dtype, out[0xFFFFFFFF], ref, "poisoned")
    assert np.array_equal(out[0].view(np.uint32), out[0xFFFFFFFF].view(np.uint32)), "the window on scratch full of NaN differs from the one on zeros"


def test_zero_pages_at_the_end(amd, gpu):
    """the module's last test: whatever ran above, nothing wrote the two shared pages"""
    assert amd.ops.scratch_zero_pages() == (0, 0)
