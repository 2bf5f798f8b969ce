"""One case per entry point that takes working memory from device_scratch (csrc/runtime.hip): what test_gpu_scratch_hygiene.py runs on
poisoned, stale and taken-over scratch, and what test_scratch_cases_cpu.py keeps closed against the call sites under csrc/.

A case names the call sites it reaches (file, ordinal of the ``device_scratch(`` call within that file), the slots it uses, builds small
inputs, runs the op on the current torch stream and returns everything the op outputs as a tuple of numpy arrays / numbers, and
names the CPU reference and the gate of the op's existing test - imported from the util modules and test modules, never restated.

Fill patterns.  Where no value an op reads from scratch is an address, an index or a loop bound: 0xFFFFFFFF (NaN as fp16 / fp32 /
fp64, -1 as an integer, the identity of a minimum) and 0x5A5A5A5A (a large finite float, a nonzero counter, no identity).  Where a
table of indices or offsets lives in the slot: 0x00000001 and 0x00000003 only - small valid indices, nonzero counters - so that a
stale read would be a wrong number and never a wild address.  The line above each case says which, from a reading of its host
function and kernels; no case reads a scratch value before it writes it.

Shapes.  Volumes are the suite's odd sizes, about 33 x 17 x 29 and 12 x 9 x 20: the reductions' 8192-voxel chunks (RED_CHUNK,
PCT_CHUNK) and select_ranked's 4096-voxel tiles then get one whole unit and a partial one at the larger shape and a single partial
one at the smaller.  A case whose tiling needs more says so in ``need``."""
import functools
from dataclasses import dataclass
from typing import Callable, Dict, Tuple

import numpy as np

import components_util as cu
import mass_effect_util as mx
import morphology_util as mu
import normal_structures_util as nu
import preprocess_util as pp
import quality_util as qu
import sequence_findings_util as su

NAN_WORDS = (0xFFFFFFFF, 0x5A5A5A5A)   # no scratch value is an index
INDEX_WORDS = (0x00000001, 0x00000003)  # index / offset tables in the slot
LARGE, SMALL = (33, 17, 29), (12, 9, 20)

#: hot kernels that read an unwritten scratch value on purpose: (kernel, region, why the product is discarded).  Conv, tconv and
#: stem kernels only; a case listed here runs with 0x5A5A5A5A alone.
ALLOWED_STALE_READS: Tuple[Tuple[str, str, str], ...] = ()


@dataclass(frozen=True)
class Case:
    name: str
    sites: Tuple[Tuple[str, int], ...]   # (file under csrc/, ordinal of the device_scratch( call in it)
    slots: Tuple[str, ...]               # ops.SCRATCH_SLOTS names the entry point uses
    inputs: Callable                     # shape -> dict of numpy inputs
    call: Callable                       # (amd, gpu, inputs) -> tuple of outputs, on the current stream
    reference: Callable                  # inputs -> what the gate compares with
    reference_of: str                    # where that reference comes from: "module.function" (checked to exist)
    exact: bool                          # the op's existing test asserts equality with the reference
    shapes: Tuple[tuple, tuple] = (LARGE, SMALL)
    patterns: Tuple[int, ...] = NAN_WORDS
    gate: Callable = None                # (got, want, inputs) -> asserts; None: equality (exact cases)
    repeatable: bool = None              # two runs are bit equal (the existing test says so); None: = exact
    need: str = ""                       # what the op's own tiling asks of the shapes

    @property
    def bit_repeatable(self):
        return self.exact if self.repeatable is None else self.repeatable


def mod(name):
    """a submodule the package does not import by itself"""
    import importlib
    return importlib.import_module("brats_amd." + name)


def dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def same(got, want, what=""):
    """equal, recursively: tuples / lists element by element, arrays by np.array_equal, numbers by =="""
    if isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), (what, type(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, f"{what}[{i}]")
    elif isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), what
        for k in want:
            same(got[k], want[k], f"{what}[{k!r}]")
    elif isinstance(want, np.ndarray) or isinstance(got, np.ndarray):
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape and np.array_equal(g, w), (what, g.shape, w.shape, int((g != w).sum()) if g.shape == w.shape else -1)
    else:
        assert got == want, (what, got, want)


def bits(x):
    """an output as bytes, for the bit-for-bit comparison of two runs"""
    if isinstance(x, (tuple, list)):
        return tuple(bits(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, bits(x[k])) for k in sorted(x, key=repr))
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, float):
        return np.float64(x).tobytes()
    return x


def rs_of(shape, salt):
    return np.random.RandomState((int(np.prod(shape)) * 31 + salt) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------ elementwise, extras
def _zscore_inputs(shape):
    rs = rs_of(shape, 1)
    return {"vol": (rs.standard_normal((3,) + shape) * 300 + 1000).astype(np.float32),
            "mask": rs.choice(np.array([0, 1, 2, 255], np.uint8), size=shape, p=(0.3, 0.3, 0.2, 0.2))}


def _zscore_gate(got, want, inp):
    ref, bound = want
    err = np.abs(got[0].astype(np.float64) - ref)
    assert np.isfinite(got[0]).all() and (err <= pp.Z_MARGIN * bound).all(), f"{int((err > pp.Z_MARGIN * bound).sum())} elements beyond the bound"
    assert (got[0][:, inp["mask"] == 0] == 0).all()


def _labels(shape, salt, p=(0.7, 0.1, 0.1, 0.1)):
    return rs_of(shape, salt).choice(len(p), size=shape, p=p).astype(np.uint8)


def _confusion_inputs(shape):
    gt = rs_of(shape, 2).choice([0, 1, 2, 3, 4, 7], size=shape, p=[0.6, 0.1, 0.1, 0.1, 0.07, 0.03]).astype(np.uint8)
    pred = gt.copy()
    flip = rs_of(shape, 3).uniform(size=shape) < 0.1
    pred[flip] = _labels(shape, 4)[flip]
    return {"pred": pred, "gt": gt}


_METRIC_KEYS = ("tp", "fp", "fn", "tn", "dice", "iou", "sensitivity", "specificity")


def _confusion_call(amd, gpu, inp):
    res = amd.evaluate.evaluate(dev(inp["pred"], gpu), dev(inp["gt"], gpu))
    return (np.array([[res[lab][k] for k in _METRIC_KEYS] for lab in (1, 2, 3)], dtype=np.float64),)


def _confusion_ref(inp):
    from oracle import extras_ref
    return (np.array([[extras_ref.calculate_metrics(inp["pred"], inp["gt"], lab)[k] for k in _METRIC_KEYS] for lab in (1, 2, 3)], dtype=np.float64),)


def _confusion_gate(got, want, inp):  # test_gpu_extras.test_evaluator_matches_reference_formulas: approx(rel=1e-12, abs=1e-12)
    assert np.all(np.abs(got[0] - want[0]) <= 1e-12 + 1e-12 * np.abs(want[0])), (got[0], want[0])


def _topk_inputs(shape):
    n, d = shape
    rs = rs_of(shape, 5)
    v, q = rs.standard_normal((n, d)), rs.standard_normal(d)
    return {"v": (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32), "q": q / np.linalg.norm(q)}


def _topk_call(amd, gpu, inp):
    got = amd.retrieval.VectorIndex(inp["v"], device=gpu, normalise=False).topk(inp["q"], 5)
    return (np.array([i for i, _ in got]), np.array([s for _, s in got]))


def _topk_ref(inp):  # the reference of test_gpu_extras.test_cosine_topk_large, which is inline there: numpy's argsort of the fp64 scores
    scores = inp["v"].astype(np.float64) @ inp["q"]
    order = np.argsort(scores)[::-1][:5]
    return (order, scores[order])


def _topk_gate(got, want, inp):  # ... and its gate
    assert list(got[0]) == list(want[0])
    assert np.allclose(got[1], want[1], atol=1e-5)


def _crop_inputs(shape):
    rs = rs_of(shape, 6)
    v = rs.standard_normal((2,) + shape).astype(np.float32) * (rs.uniform(size=(2,) + shape) < 0.45)
    v[:, :2], v[:, :, -1], v[:, :, :, :3] = 0, 0, 0   # a background margin: the box is not the volume
    return {"vol": v.astype(np.float32)}


def _crop_call(amd, gpu, inp):
    mask, box = amd.ops.crop_mask(dev(inp["vol"], gpu))
    return (mask.cpu().numpy(), box)


def _label_stats_inputs(shape):
    return {"seg": rs_of(shape, 7).choice([0, 1, 2, 3, 4, 7, 9], size=shape, p=[0.6, 0.1, 0.1, 0.08, 0.06, 0.03, 0.03]).astype(np.uint8)}


# ------------------------------------------------------------------------------------------------------------ resample
def _resize_inputs(shape):
    return {"x": pp.resize_input((2,) + shape, seed=3 + shape[0])}


def _resize_n_out(inp):
    return inp["x"].shape[2] * 3 // 2 + 1


def _resize_gate(got, want, inp):
    ratio = np.abs(got[0].astype(np.float64) - want[0]) / pp.line_scale(inp["x"], 2)
    assert got[0].shape == want[0].shape and np.isfinite(got[0]).all() and (ratio <= pp.G_RESIZE).all(), f"worst {float(ratio.max()):.3e}"


def _clip_inputs(shape):
    rs = rs_of(shape, 8)
    ref = (rs.standard_normal((2,) + shape) * 50 + 20).astype(np.float32)
    x = (rs.standard_normal((2, shape[0], shape[1] + 3, shape[2] + 5)) * 100 + 20).astype(np.float32)  # a third beyond each end
    return {"x": x, "ref": ref}


# ------------------------------------------------------------------------------------------------------------ components
COMPONENT_SHAPES = ((33, 17, 70), SMALL)
COMPONENT_NEED = "bricks of the local pass are 64 long on the last axis: 70 gives a whole brick and a partial one"


def _mask_inputs(shape, p=0.3, salt=9):
    return {"mask": cu.noise(int(np.prod(shape)) % 9973 + salt, shape, p)}


def _label_call(connectivity):
    def call(amd, gpu, inp):
        labels, n = amd.components.label_components(dev(inp["mask"], gpu), connectivity)
        return (labels.cpu().numpy(), n)
    return call


def _label18_call(amd, gpu, inp):
    labels, n = amd.components.label_components_neighbours(dev(inp["mask"], gpu), 18)
    return (labels.cpu().numpy(), n)


def _stats_inputs(shape):
    d = _mask_inputs(shape, 0.25, 11)
    d["seg"] = rs_of(shape, 12).randint(0, 6, shape).astype(np.uint8)
    return d


def _stats_call(amd, gpu, inp):
    labels, n = amd.components.label_components(dev(inp["mask"], gpu), 3)
    return (n, amd.components.component_stats(labels, n, dev(inp["seg"], gpu)))


def _stats_ref(inp):
    lab, n = cu.scipy_labels(inp["mask"], 3)
    return (n, cu.numpy_stats(lab, n, inp["seg"]))


def _largest_inputs(shape):
    return {"seg": _labels(shape, 13, (0.55, 0.2, 0.1, 0.15))}


def _largest_call(amd, gpu, inp):
    out, removed, kept = amd.components.remove_all_but_the_largest_connected_component(dev(inp["seg"], gpu), [1, (2, 3)], 1.0, {1: 3.0, (2, 3): 2.0})
    return (out.cpu().numpy(), removed, kept)


# ------------------------------------------------------------------------------------------------------------ morphology
def _morph_call(amd, gpu, inp):
    m = dev(inp["mask"], gpu)
    return (mod("morphology").binary_erosion(m, 3).cpu().numpy(), mod("morphology").binary_dilation(m, 2).cpu().numpy())


def _gradient_inputs(shape):
    mask = _mask_inputs(shape, 0.6, 15)["mask"]
    return {"d2_in": mu.edt_sq(mask), "d2_out": mu.edt_sq(mask == 0), "surface": ((mask != 0) & (mu.erode(mask) == 0)).astype(np.uint8)}


def _gradient_gate(got, want, inp):  # test_gpu_morphology.test_gradient_statistics_equal_the_numpy_restatement
    assert got[0] == want[0] and got[0] > 0
    assert abs(got[1] - want[1]) <= mu.RTOL * want[1] and abs(got[2] - want[2]) <= mu.RTOL * want[2]


def _moments_inputs(shape):
    rs = rs_of(shape, 16)
    flags = (rs.randint(0, 256, shape) * (rs.random_sample(shape) < 0.3)).astype(np.uint8)
    flags[..., :7] &= 0x0F
    return {"vols": np.rint(rs.uniform(0, 4000, (3,) + shape)).astype(np.float32), "flags": flags}  # integers: sums below 2^53 are exact


# ------------------------------------------------------------------------------------------------------------ percentiles
QS8 = (0, 5, 10, 25, 50, 85, 99, 100)


def _pct_inputs(shape):
    rs = rs_of(shape, 17)
    return {"x": (rs.standard_normal(shape) * 100 + 300).astype(np.float32), "y": rs.uniform(-5, 900, shape).astype(np.float32),
            "flags": rs.randint(0, 256, shape).astype(np.uint8)}


def _pct_selected(x, flags, require, forbid, lo=-np.inf, hi=np.inf):
    keep = ((flags & require) == require) & ((flags & forbid) == 0) & (lo < x.astype(np.float64)) & (x.astype(np.float64) < hi)
    return x[keep]


def _pct_call(amd, gpu, inp):
    count, nans, below, above = mod("percentile").masked_order_stats(dev(inp["x"], gpu), QS8, dev(inp["flags"], gpu), 1, 4, lo=0.0)
    return (count, nans, below, above)


def _pct_ref(inp):
    sel = _pct_selected(inp["x"], inp["flags"], 1, 4, lo=0.0)
    below, above, _ = su.order_stats(sel, QS8)
    return (int(sel.size), 0, below, above)


# four volumes with eight percentiles each (up to 16 live groups per volume in the later passes), then two volumes with one
# percentile each: the second call's passes count into fewer groups of the table the first one left
_MULTI_A = ((("x", QS8, 1, 4), ("y", QS8, 0, 0), ("x", (33.3, 50, 75), 2, 0), ("y", QS8, 8, 1)))
_MULTI_B = ((("y", (50,), 0, 0), ("x", (99,), 1, 0)))


def _multi_call(amd, gpu, inp):
    d = {k: dev(inp[k], gpu) for k in ("x", "y")}
    flags = dev(inp["flags"], gpu)
    out = []
    for batch in (_MULTI_A, _MULTI_B):
        res = mod("percentile").masked_order_stats_multi([(d[v], qs, req, forb) for v, qs, req, forb in batch], flags)
        out.append(tuple(tuple(r) for r in res))
    return tuple(out)


def _multi_ref(inp):
    out = []
    for batch in (_MULTI_A, _MULTI_B):
        res = []
        for v, qs, req, forb in batch:
            sel = _pct_selected(inp[v], inp["flags"], req, forb)
            below, above, _ = su.order_stats(sel, qs)
            res.append((int(sel.size), 0, below, above))
        out.append(tuple(res))
    return tuple(out)


def _i32_inputs(shape):
    rs = rs_of(shape, 18)
    return {"values": rs.randint(0, 1 << 20, shape).astype(np.int32), "flags": rs.randint(0, 256, shape).astype(np.uint8)}


def _i32_call(amd, gpu, inp):
    return tuple(mod("normal_structures").masked_order_stats_i32(dev(inp["values"], gpu), QS8, dev(inp["flags"], gpu), 2, 1))


def _flags_inputs(shape):
    return {"flags": np.array(mx.random_flags(shape, seed=3 + shape[0]))}


# ------------------------------------------------------------------------------------------------------------ quality
def _sobel_inputs(shape):
    return {"x": np.array(qu.integer_volume(shape)), "flags": (rs_of(shape, 19).random_sample(shape) < 0.3).astype(np.uint8) * 16}


def _sobel_gate(got, want, inp):  # test_gpu_quality.test_sobel_statistics_over_everything_and_over_a_subset
    import test_gpu_quality as tq
    n, mean, std = got
    assert n == want[0] and n > 0
    assert abs(mean - want[1]) / want[1] <= n * tq.EPS
    assert abs(std - want[2]) / want[2] <= qu.RTOL_STD


def _shell_inputs(shape):
    rs = rs_of(shape, 20)
    selected = rs.random_sample(shape) < 0.6
    return {"x": np.array(qu.integer_volume(shape, seed=13)), "selected": selected,
            "flags": (selected.astype(np.uint8) * 5) | (rs.random_sample(shape) < 0.5).astype(np.uint8) * 2,
            "centre": [np.float64(int(s)) / 7 for s in (rs.randint(0, 7 * n - 6) for n in shape)]}


def _face_inputs(shape):
    return {"x": np.array(qu.integer_volume(shape)) - 16000.0}


# ------------------------------------------------------------------------------------------------------------ mass effect
def _boxes(shape):
    d0, d1, d2 = shape
    return [(0, d0, 0, d1, 0, d2), (1, d0 // 2, 2, d1 - 1, 3, d2 - 2), (d0 // 2, d0, 0, d1 // 2, d2 // 2, d2), (2, 2, 0, d1, 0, d2), (0, 1, 0, 1, 0, 1)]


def _ranked_inputs(shape):
    f = np.array(mx.density_flags(shape, 0.5))
    return {"flags": f, "ranks": mx.rank_set(int(mx.selected(f, 4, 1).sum()))}


def _ranked_call(amd, gpu, inp):
    index, count = mod("mass_effect").select_ranked(dev(inp["flags"], gpu), inp["ranks"], 4, 1)
    return (index.cpu().numpy(), count)


def _pair_inputs(shape):
    rs = rs_of(shape, 21)
    v = int(np.prod(shape))
    return {"a": rs.choice(v // 2, 300, replace=False).astype(np.int64), "b": (v // 2 + rs.choice(v - v // 2, 700, replace=False)).astype(np.int64),
            "shape": shape}


def _min_inputs(shape):
    d = _flags_inputs(shape)
    d["values"] = rs_of(shape, 22).randint(-(1 << 30), 1 << 30, shape).astype(np.int32)
    return d


# ------------------------------------------------------------------------------------------------------------ convolutions
def _conv_inputs(dtype):
    def inputs(case):
        import test_gpu_ops as tg
        n, d, h, w, cin, cout, stride, act = case
        rs = np.random.RandomState(17)
        t = np.float16 if dtype == "f16" else np.float32
        return {"x": tg._rand(rs, n, d, h, w, cin).astype(t), "w": (tg._rand(rs, cout, cin, 3, 3, 3) / np.sqrt(cin * 27)).astype(t),
                "b": tg._rand(rs, cout), "case": case}
    return inputs


def _conv_call(amd, gpu, inp):
    _, _, _, _, _, _, stride, act = inp["case"]
    y = amd.ops.conv3d_ndhwc(dev(inp["x"], gpu), inp["w"].astype(np.float32), inp["b"], stride=stride, act=act, slope=0.01)
    return (y.cpu().numpy(), amd.ops.last_conv_kernel())


def _conv_ref(inp):
    import test_gpu_ops as tg
    _, _, _, _, _, _, stride, act = inp["case"]
    ref = tg._ref_conv(inp["x"].astype(np.float32), inp["w"].astype(np.float32), inp["b"], stride, act, 0.01)
    ref64 = tg._ref_conv64(inp["x"], inp["w"], inp["b"], stride, act, 0.01) if inp["x"].dtype == np.float16 else None
    return (ref, ref64)


def _conv_gate(expect):
    def gate(got, want, inp):
        import test_gpu_ops as tg
        y, ran = got
        ref, ref64 = want
        assert expect in ran, (inp["case"], ran)
        assert y.shape == ref.shape
        err = np.abs(y.astype(np.float32) - ref).max()
        if ref64 is None:   # test_conv3d_mfma_matches_torch
            assert err <= 2e-5 * max(1.0, np.abs(ref).max()), f"max abs err {err} ({ran})"
        else:               # test_conv3d_f16_matches_torch
            assert err <= 2e-3 * max(1.0, np.abs(ref).max()), f"max abs err {err} ({ran})"
            tg._assert_f16_rounding(inp["case"], ran, y, ref, ref64)
    return gate


SPLITK_SHAPES = ((8, 16, 16, 16, 256, 320, 2, 0), (2, 4, 4, 4, 320, 320, 1, 1))


CASES = (
    # sums and partials are fp64 values, read as values only
    Case("zscore_masked", (("elementwise.hip", 0),), ("SCR_ZSCORE",), _zscore_inputs,
         lambda amd, gpu, i: (amd.ops.zscore_masked_(dev(i["vol"], gpu), dev(i["mask"], gpu)).cpu().numpy(),),
         lambda i: pp.zscore_ref(i["vol"], i["mask"]), "preprocess_util.zscore_ref", exact=False, gate=_zscore_gate, repeatable=True),
    # 64 counters, cleared by the host, read back as counts
    Case("label_confusion", (("extras.hip", 0),), ("SCR_SMALL",), _confusion_inputs, _confusion_call, _confusion_ref,
         "oracle.extras_ref.calculate_metrics", exact=False, gate=_confusion_gate, repeatable=True),
    # `best` packs the index of the winning row, which take_best_kernel uses as a subscript: an index table
    Case("cosine_topk", (("extras.hip", 1),), ("SCR_TOPK",), _topk_inputs, _topk_call, _topk_ref, "test_gpu_extras.test_cosine_topk_large",
         exact=False, shapes=((3001, 48), (517, 48)), patterns=INDEX_WORDS, gate=_topk_gate, repeatable=True,
         need="rows, not voxels: 3001 and 517 rows of 48 floats (the 16-byte path), more rows than one workgroup's 4 waves"),
    # a `changed` flag, six bounds and the flood-fill bytes, all compared or combined, none a subscript
    Case("crop_mask", (("extras.hip", 2),), ("SCR_CROP",), _crop_inputs, _crop_call, lambda i: tuple(pp.crop_expected(i["vol"])),
         "preprocess_util.crop_expected", exact=True),
    # 80 integers, initialised by a host copy, combined with atomics
    Case("label_stats", (("extras.hip", 3),), ("SCR_SMALL",), _label_stats_inputs,
         lambda amd, gpu, i: (amd.evaluate.label_stats(dev(i["seg"], gpu), 8),), lambda i: (mu.label_stats(i["seg"], 8),),
         "morphology_util.label_stats", exact=True),
    # spline coefficients: floats
    Case("resize_axis_order3", (("resample.hip", 0),), ("SCR_RESAMPLE",), _resize_inputs,
         lambda amd, gpu, i: (amd.ops.resize_axis(dev(i["x"], gpu), 2, _resize_n_out(i), 3).cpu().numpy(),),
         lambda i: (pp.resize_zoom(i["x"], 2, _resize_n_out(i), 3),), "preprocess_util.resize_zoom", exact=False, gate=_resize_gate, repeatable=True),
    # min / max words in an order-preserving integer image: compared, never subscripts
    Case("clip_to_range_of", (("resample.hip", 1),), ("SCR_RESAMPLE_MM",), _clip_inputs,
         lambda amd, gpu, i: (amd.ops.clip_to_range_of_(dev(i["x"], gpu), dev(i["ref"], gpu), 2).cpu().numpy(),),
         lambda i: (pp.clip_ref(i["x"], i["ref"], 2),), "preprocess_util.clip_ref", exact=True),
    # the parent table holds voxel indices that the find loops follow, the chunk offsets number the labels: index tables
    Case("label_components_6", (("components.hip", 0),), ("SCR_COMPONENTS",), _mask_inputs, _label_call(1),
         lambda i: cu.scipy_labels(i["mask"], 1), "components_util.scipy_labels", exact=True, shapes=COMPONENT_SHAPES, patterns=INDEX_WORDS,
         need=COMPONENT_NEED),
    Case("label_components_18", (("components.hip", 0),), ("SCR_COMPONENTS",), _mask_inputs, _label18_call,
         lambda i: cu.scipy_labels(i["mask"], 2), "components_util.scipy_labels", exact=True, shapes=COMPONENT_SHAPES, patterns=INDEX_WORDS,
         need=COMPONENT_NEED),
    Case("label_components_26", (("components.hip", 0),), ("SCR_COMPONENTS",), _mask_inputs, _label_call(3),
         lambda i: cu.scipy_labels(i["mask"], 3), "components_util.scipy_labels", exact=True, shapes=COMPONENT_SHAPES, patterns=INDEX_WORDS,
         need=COMPONENT_NEED),
    # the statistics table shares the slot with the parent table of the labelling in front of it: index tables
    Case("component_stats", (("components.hip", 0), ("components.hip", 1)), ("SCR_COMPONENTS",), _stats_inputs, _stats_call, _stats_ref,
         "components_util.numpy_stats", exact=True, shapes=COMPONENT_SHAPES, patterns=INDEX_WORDS, need=COMPONENT_NEED),
    # label, statistics and the keep table of the filter (subscripted by label): index tables
    Case("largest_component", (("components.hip", 0), ("components.hip", 1), ("components.hip", 2)), ("SCR_COMPONENTS",), _largest_inputs,
         _largest_call, lambda i: cu.largest_component_ref(i["seg"], [1, (2, 3)], 1.0, {1: 3.0, (2, 3): 2.0}), "components_util.largest_component_ref",
         exact=True, shapes=COMPONENT_SHAPES, patterns=INDEX_WORDS, need=COMPONENT_NEED),
    # the second mask of the ping-pong: bytes tested against zero
    Case("binary_morphology", (("morphology.hip", 0),), ("SCR_MORPHOLOGY",), lambda s: _mask_inputs(s, 0.8, 14), _morph_call,
         lambda i: (mu.erode(i["mask"], 3), mu.dilate(i["mask"], 2)), "morphology_util.erode", exact=True),
    # one counter of background voxels, cleared by the host
    Case("edt_squared", (("morphology.hip", 1),), ("SCR_MORPHOLOGY",), lambda s: _mask_inputs(s, 0.7, 14),
         lambda amd, gpu, i: (mod("morphology").distance_transform_edt_sq(dev(i["mask"], gpu)).cpu().numpy(),), lambda i: (mu.edt_sq(i["mask"]),),
         "morphology_util.edt_sq", exact=True),
    # fp64 partial sums per chunk
    Case("surface_gradient_stats", (("morphology.hip", 2),), ("SCR_MORPHOLOGY",), _gradient_inputs,
         lambda amd, gpu, i: mod("morphology").surface_gradient_stats(dev(i["d2_in"], gpu), dev(i["d2_out"], gpu), dev(i["surface"], gpu)),
         lambda i: mu.gradient_stats(i["d2_in"], i["d2_out"], i["surface"]), "morphology_util.gradient_stats", exact=False, gate=_gradient_gate,
         repeatable=True),
    # ten integer sums, cleared by the host
    Case("second_moments", (("morphology.hip", 3),), ("SCR_MORPHOLOGY",), lambda s: _mask_inputs(s, 0.4, 14),
         lambda amd, gpu, i: (mod("morphology").second_moments(dev(i["mask"], gpu)),), lambda i: (mu.second_moments(i["mask"]),),
         "morphology_util.second_moments", exact=True),
    # fp64 partial sums and per-chunk counts that are only added up
    Case("masked_moments", (("morphology.hip", 4),), ("SCR_MORPHOLOGY",), _moments_inputs,
         lambda amd, gpu, i: (mod("morphology").masked_moments(dev(i["vols"], gpu), dev(i["flags"], gpu)),), lambda i: (mu.masked_moments(i["vols"], i["flags"]),),
         "morphology_util.masked_moments", exact=True),
    # the radix table: counters the HOST reads and walks with bounded digits; no kernel subscripts with them
    Case("masked_percentiles", (("radix_select.h", 0),), ("SCR_MORPHOLOGY",), _pct_inputs, _pct_call, _pct_ref, "sequence_findings_util.order_stats",
         exact=True),
    Case("masked_percentiles_multi", (("percentile.hip", 0),), ("SCR_MORPHOLOGY",), _pct_inputs, _multi_call, _multi_ref,
         "sequence_findings_util.order_stats", exact=True),
    Case("masked_order_stats_i32", (("radix_select.h", 0),), ("SCR_MORPHOLOGY",), _i32_inputs, _i32_call,
         lambda i: nu.order_stats(i["values"][nu.selected(i["flags"], 2, 1)], QS8), "normal_structures_util.order_stats", exact=True),
    # one word, a maximum, cleared by the host
    Case("column_count_max", (("normal_structures.hip", 0),), ("SCR_MORPHOLOGY",), _flags_inputs,
         lambda amd, gpu, i: (mod("normal_structures").column_count_max(dev(i["flags"], gpu), 3, 5, 2),),
         lambda i: (nu.column_count_max(i["flags"], 3, 5, 2),), "normal_structures_util.column_count_max", exact=True),
    # the label map of the complement subscripts the mark table (guarded by 1 <= l <= n), and the labelling inside uses
    # SCR_COMPONENTS: index tables in both slots
    Case("binary_fill_holes", (("quality.hip", 0), ("components.hip", 0)), ("SCR_QUALITY", "SCR_COMPONENTS"), lambda s: _mask_inputs(s, 0.7, 23),
         lambda amd, gpu, i: (lambda r: (r[0].cpu().numpy(), r[1]))(mod("quality").binary_fill_holes(dev(i["mask"], gpu))),
         lambda i: qu.fill_holes(i["mask"]), "quality_util.fill_holes", exact=True, shapes=COMPONENT_SHAPES, patterns=INDEX_WORDS, need=COMPONENT_NEED),
    # fp64 partial sums per chunk
    Case("sobel_magnitude_stats", (("quality.hip", 1),), ("SCR_QUALITY",), _sobel_inputs,
         lambda amd, gpu, i: mod("quality").sobel_magnitude_stats(dev(i["x"], gpu), dev(i["flags"], gpu), 16),
         lambda i: qu.stats_of(qu.scipy_sobel_magnitude(i["x"])[i["flags"] != 0]), "quality_util.scipy_sobel_magnitude", exact=False, gate=_sobel_gate,
         repeatable=True),
    # a maximum as a bit pattern, a count, fp64 partial sums
    Case("radial_shell_moments", (("quality.hip", 2),), ("SCR_QUALITY",), _shell_inputs,
         lambda amd, gpu, i: mod("quality").radial_shell_moments(dev(i["x"], gpu), dev(i["flags"], gpu), 5, i["centre"]),
         lambda i: qu.radial_shell(i["x"], i["selected"], i["centre"]), "quality_util.radial_shell", exact=True),
    # six counters, cleared by the host
    Case("face_slab_counts", (("quality.hip", 3),), ("SCR_QUALITY",), _face_inputs,
         lambda amd, gpu, i: (mod("quality").face_slab_counts(dev(i["x"], gpu), 3),), lambda i: (qu.face_slab_counts(i["x"], 3),),
         "quality_util.face_slab_counts", exact=True),
    # counters, cleared by the host; the slot also serves the offset tables of select_ranked: index patterns for the whole slot
    Case("axis_counts", (("mass_effect.hip", 0),), ("SCR_MASS_EFFECT",), _flags_inputs,
         lambda amd, gpu, i: tuple(mod("mass_effect").axis_counts(dev(i["flags"], gpu), 5, 2)), lambda i: mx.axis_counts(i["flags"], 5, 2),
         "mass_effect_util.axis_counts", exact=True, patterns=INDEX_WORDS),
    Case("box_counts", (("mass_effect.hip", 1),), ("SCR_MASS_EFFECT",), _flags_inputs,
         lambda amd, gpu, i: (mod("mass_effect").box_counts(dev(i["flags"], gpu), _boxes(i["flags"].shape), 1, 4),),
         lambda i: (mx.box_counts(i["flags"], _boxes(i["flags"].shape), 1, 4),), "mass_effect_util.box_counts", exact=True, patterns=INDEX_WORDS),
    # block counts, offsets and segment bases that pick_kernel searches and subtracts from a rank: offset tables
    Case("select_ranked", (("mass_effect.hip", 2),), ("SCR_MASS_EFFECT",), _ranked_inputs, _ranked_call,
         lambda i: (mx.select_ranked(i["flags"], i["ranks"], 4, 1), int(mx.selected(i["flags"], 4, 1).sum())), "mass_effect_util.select_ranked",
         exact=True, patterns=INDEX_WORDS),
    # a minimum and an error flag, set by the host
    Case("min_pair_dist2", (("mass_effect.hip", 3),), ("SCR_MASS_EFFECT",), _pair_inputs,
         lambda amd, gpu, i: (mod("mass_effect").min_pair_dist2(dev(i["a"], gpu), dev(i["b"], gpu), i["shape"]),),
         lambda i: (mx.min_pair_dist2(i["a"], i["b"], i["shape"]),), "mass_effect_util.min_pair_dist2", exact=True, patterns=INDEX_WORDS),
    # a count and a minimum, set by the host
    Case("masked_min", (("mass_effect.hip", 4),), ("SCR_MASS_EFFECT",), _min_inputs,
         lambda amd, gpu, i: mod("mass_effect").masked_min(dev(i["values"], gpu), dev(i["flags"], gpu), 5, 2),
         lambda i: mx.masked_min(i["values"], i["flags"], 5, 2), "mass_effect_util.masked_min", exact=True, patterns=INDEX_WORDS),
    # fp32 partial sums per K slice, every element of every slice written by the conv kernel; the zero bias page is read only
    Case("conv_splitk_f32", (("conv3d.hip", 1), ("conv3d.hip", 2)), ("SCR_SPLITK_F32", "SCR_ZERO_BIAS"), _conv_inputs("f32"), _conv_call, _conv_ref,
         "test_gpu_ops._ref_conv", exact=False, shapes=SPLITK_SHAPES, gate=_conv_gate(" split-K"), need="the two split-K cases of test_gpu_ops.py"),
    Case("conv_splitk_f16", (("conv3d_f16.hip", 1),), ("SCR_SPLITK_F16",), _conv_inputs("f16"), _conv_call, _conv_ref, "test_gpu_ops._ref_conv64",
         exact=False, shapes=SPLITK_SHAPES, gate=_conv_gate(" split-K"), need="the two split-K cases of test_gpu_ops.py"),
    # the zero page: 256 bytes every out-of-volume DMA piece reads; nothing may write it
    Case("conv_wino3_f32", (("conv3d_wino3.hip", 0),), ("SCR_ZEROS",), _conv_inputs("f32"), _conv_call, _conv_ref, "test_gpu_ops._ref_conv", exact=False,
         shapes=((4, 8, 8, 24, 128, 160, 1, 0), (8, 4, 16, 16, 128, 128, 1, 1)), gate=_conv_gate("conv3_f32_wino3_kernel"),
         need="two F(2x2x2,3x3x3) cases of test_gpu_ops.py: the planner chooses the kernel by tile count"),
    Case("conv_s2dma_f32", (("conv3d.hip", 0),), ("SCR_ZEROS",), _conv_inputs("f32"), _conv_call, _conv_ref, "test_gpu_ops._ref_conv", exact=False,
         shapes=((2, 64, 64, 128, 32, 64, 2, 1), (3, 50, 62, 90, 16, 128, 2, 0)), gate=_conv_gate("conv3_f32_s2dma_kernel"),
         need="the LDS-DMA stride-2 kernel runs from 1024 tiles: its two smallest cases of test_gpu_ops.py"),
    Case("conv_dma_f16", (("conv3d_f16.hip", 0),), ("SCR_ZEROS",), _conv_inputs("f16"), _conv_call, _conv_ref, "test_gpu_ops._ref_conv64", exact=False,
         shapes=((8, 16, 16, 16, 256, 256, 1, 1), (4, 24, 40, 72, 16, 64, 1, 1)), gate=_conv_gate("conv3_f16_dma_kernel"),
         need="the LDS-DMA kernel runs from 256 (tile, cout block) units: two of its cases of test_gpu_ops.py"),
    Case("conv_s2dma_f16", (("conv3d_f16_s2.hip", 0),), ("SCR_ZEROS",), _conv_inputs("f16"), _conv_call, _conv_ref, "test_gpu_ops._ref_conv64",
         exact=False, shapes=((2, 32, 32, 64, 64, 256, 2, 0), (6, 24, 40, 48, 16, 128, 2, 1)), gate=_conv_gate("conv3_f16_s2dma_kernel"),
         need="whole 4 x 4 x 8 output tiles and Cout % 128 == 0: two of the kernel's cases of test_gpu_ops.py"),
)

BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
CONV_CASES = tuple(c.name for c in CASES if c.name.startswith("conv_"))

#: the network's scratch users: run by the network tests of test_gpu_scratch_hygiene.py, not through Case.call
NETWORK_SITES = {
    "unet_forward": {"sites": (("unet.hip", 0),), "slots": ("SCR_ARENA", "SCR_SPLITK_F32", "SCR_SPLITK_F16"), "reference_of": "oracle.unet_ref.unet_forward"},
    "sw_predict": {"sites": (("unet.hip", 0), ("sliding_window.hip", 0)), "slots": ("SCR_ARENA", "SCR_SW_AGG", "SCR_SPLITK_F32", "SCR_SPLITK_F16"),
                   "reference_of": "oracle.tiler_ref.predict_3d_tiled"},
}


@functools.lru_cache(maxsize=None)
def inputs_of(name, which):
    """the inputs of a case at its larger (0) or smaller (1) shape, built once"""
    c = BY_NAME[name]
    return c.inputs(c.shapes[which])


@functools.lru_cache(maxsize=None)
def reference_of(name, which):
    """the reference of a case at that shape, computed once and shared by every test that needs it"""
    return BY_NAME[name].reference(inputs_of(name, which))


def check(name, which, got):
    """the gate of the op's existing test on one result"""
    c = BY_NAME[name]
    want = reference_of(name, which)
    if c.gate is not None:
        c.gate(got, want, inputs_of(name, which))
    else:
        same(got, want, f"{name} at {c.shapes[which]}")


def resolve(dotted):
    """the object a ``reference_of`` string names"""
    import importlib
    parts = dotted.split(".")
    for cut in range(len(parts) - 1, 0, -1):
        try:
            obj = importlib.import_module(".".join(parts[:cut]))
        except ImportError:
            continue
        for p in parts[cut:]:
            obj = getattr(obj, p)
        return obj
    raise ImportError(dotted)


def call_sites(csrc):
    """{file: number of device_scratch( call sites} under csrc/: every occurrence that is not a comment line, the declaration or
    the definition"""
    import os
    import re
    out = {}
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".h")):
            continue
        n = 0
        with open(os.path.join(csrc, fn), encoding="utf-8") as f:
            for line in f:
                s = line.strip()
                if s.startswith("//") or re.match(r"int\s+device_scratch\(", s):
                    continue
                n += len(re.findall(r"\bdevice_scratch\(", s))
        if n:
            out[fn] = n
    return out
