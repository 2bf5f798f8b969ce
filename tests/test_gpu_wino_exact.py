"""-m gpu: the fp32 Winograd conv kernels - conv3_f32_wino3_kernel (F(2x2x2, 3x3x3), five instantiations) and
conv3_f32_wino2_kernel (F(2x2, 3x3) over z and y, three) - on exact operands, at their edges and between guard bands.

Every other test that reaches these kernels compares random normal data with 2e-5 of the range: a product that keeps 16
significant bits of an operand passes that, and so does a stale piece of a brick that is small against the range.  Here:

* Every run of wino_exact_util.RUNS (a case of GPU_CASES with one of its operand classes) goes through the C entry - the
  forced single-op entry mi355_conv3d_wino3_ndhwc, or mi355_conv3d_fused_ndhwc through the planner - with integer operands whose
  all-absolute-values bound the emulation has asserted below 2^24 (wino_exact_util.checked_case: nothing is launched on
  operands it has not passed).  Nothing rounds, in whatever order the kernel adds, so
    - the kernel that ran is the case's (mi355_last_conv_kernel),
    - the output - or the logits of a fused head - must EQUAL the integer reference (np.array_equal, no tolerance),
    - the output lies in the middle of a buffer of sentinels, a sample's worth of 4096.0 on either side, and both bands must be
      untouched: both kernels store straight into the caller's tensor, wino2 on ragged volumes,
    - with statistics, sum y must equal the reference's (a tile's partial sum stays below 2^24 halves of the unit - asserted -
      and the quantised partials add exactly in fp64); sum y^2 stays with the 1e-4 gates of test_gpu_ops.py.
  The shapes are the smallest at which each path exists (tests/test_wino_exact_cpu.py checks the grids): one tile, a tile count
  that is no multiple of 8, a second tile per workgroup, tile ranges that cross a sample, concat chunks, ragged edges.
* Bit-for-bit invariants on random float data (the generator of test_gpu_s2_split.py), torch.equal:
    - a sample replicated N times gives N equal outputs (and equal statistics) - equal to the N = 1 run where the forced entry
      makes that run take the same kernel.  A stale piece of the other brick buffer, a statistics or addend pointer that lags
      a sample, a tile decoded against the wrong sample show here;
    - conv([x0 | x1]) from one tensor equals the two-tensor concat call, on both kernels: only the source of a chunk changes.
      The fp64 gate of 2e-5 is asserted on it once.

These classes pin the present exact-fmaf product form.  A later change of product form that legitimately cannot meet a class
must restate that class in the same change, the way tests/test_gpu_s2_split.py does for the stride-2 kernel; it must not
delete it."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wino_exact_util as W
from test_gpu_s2_split import _random_case

pytestmark = pytest.mark.gpu

SENTINEL = 4096.0


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch(amd, dev, c, ops, out, sums):
    """one call of the case's C entry, storing into `out`; returns the kernel that ran"""
    n, d, h, w = c.shape
    x = _dev(ops.x, dev)
    x0 = x[..., :c.c0].contiguous()
    x1 = x[..., c.c0:].contiguous() if c.c1 else None
    wf, bf = np.ascontiguousarray(ops.wt, dtype=np.float32), np.ascontiguousarray(ops.bias, dtype=np.float32)
    lib, stream = amd._lib.load(), torch.cuda.current_stream(dev).cuda_stream
    if c.entry == "wino3":
        addend = _dev(ops.addend, dev)
        amd._lib.check(lib.mi355_conv3d_wino3_ndhwc(x0.data_ptr(), _ptr(x1), n, d, h, w, c.c0, c.c1, amd._lib.fptr(wf), amd._lib.fptr(bf), c.cout,
                                                    1, W.SLOPE, _ptr(addend), out.data_ptr(), stream), "mi355_conv3d_wino3_ndhwc")
    else:
        scale, shift, hw, hb = _dev(ops.scale, dev), _dev(ops.shift, dev), _dev(ops.head_w, dev), _dev(ops.head_b, dev)
        amd._lib.check(lib.mi355_conv3d_fused_ndhwc(
            x0.data_ptr(), _ptr(x1), 0, n, d, h, w, c.c0, c.c1, amd._lib.fptr(wf), amd._lib.fptr(bf), c.cout, 1, 1, W.SLOPE, 0,
            _ptr(scale), _ptr(shift), 1 if c.norm else 0, _ptr(hw), _ptr(hb), c.head, out.data_ptr() if c.head else None,
            None if c.head else out.data_ptr(), _ptr(sums), stream), "mi355_conv3d_fused_ndhwc")
    return amd.ops.last_conv_kernel()


@pytest.mark.parametrize("case,cls", W.RUNS, ids=[f"{c.name}-{cls}" for c, cls in W.RUNS])
def test_integer_operands_are_exact(amd, gpu, case, cls):
    t0 = time.time()
    c = case
    ops, exp = W.checked_case(c, cls)  # the reference, the emulation equal to it, the bound < 2^24 (and the bits condition) asserted
    want = exp.logits2 if c.head else exp.y_scaled
    scale = 2 * exp.unit           # `want` is in units of 1 / scale
    n, numel = c.shape[0], want.size
    guard = -(-max(4096, numel // n) // 256) * 256  # a sample's worth, a multiple of 256 elements: the output keeps its alignment
    buf = torch.full((guard + numel + guard,), SENTINEL, dtype=torch.float32, device=gpu)
    out = buf[guard:guard + numel]
    sums = torch.full((n, c.cout, 2), float("nan"), dtype=torch.float64, device=gpu) if c.stats else None
    ran = _launch(amd, gpu, c, ops, out, sums)
    assert ran == c.kernel, (c.name, ran)
    got = buf.cpu().numpy().astype(np.float64)
    got_scaled = scale * got[guard:guard + numel].reshape(want.shape)
    equal = int((got_scaled == want).sum())
    if equal != numel:
        where = W.describe_tap_failure(ops, want, got_scaled) if cls == "taps" and not c.head else ""
        bad = np.argwhere(got_scaled != want)
        raise AssertionError(f"{c.name} {cls} [{ran}]: {len(bad)} of {numel} outputs differ from the integer conv, first at {tuple(bad[0])}: "
                             f"{got_scaled[tuple(bad[0])] / scale} instead of {want[tuple(bad[0])] / scale}. {where}")
    assert np.array_equal(got_scaled, want)
    front, back = got[:guard], got[guard + numel:]
    assert np.array_equal(front, np.full(guard, SENTINEL)) and np.array_equal(back, np.full(guard, SENTINEL)), (
        f"{c.name} {cls} [{ran}]: stores outside the output: {int((front != SENTINEL).sum())} elements in front, "
        f"{int((back != SENTINEL).sum())} behind (first behind at +{int(np.argmax(back != SENTINEL))})")
    note = ""
    if sums is not None:
        got_sums = sums.cpu().numpy()
        assert np.isfinite(got_sums).all(), (c.name, ran)
        assert 512 * int(np.abs(want).max()) < W.LIMIT  # a tile's partial sum of y, in units of 1 / scale, is an integer that fp32 holds
        want_sum = want.sum(axis=(1, 2, 3))
        assert np.array_equal(scale * got_sums[..., 0], want_sum), (
            f"{c.name} {cls} [{ran}]: sum y differs from the integer conv's, worst by {np.abs(scale * got_sums[..., 0] - want_sum).max() / scale}")
        note = ", sum y exact"
    bits = (f" | bound {100.0 * exp.emu.bound / W.LIMIT:.1f} % of 2^24, widest V / U / product {exp.emu.v_bits} / {exp.emu.u_bits} / "
            f"{exp.emu.product_bits} bits" if cls in W.BITS_CLASSES else "")
    print(f"WINO EXACT {c.name} {cls} | {ran} | {equal} of {numel} {'logits' if c.head else 'outputs'} equal the integer conv | max |y| "
          f"{np.abs(want).max() / scale:g} | 2 x {guard} sentinels untouched{note}{bits} | {time.time() - t0:.1f} s", flush=True)


def _ref64(x, wt):
    y = F.conv3d(torch.from_numpy(x).double().permute(0, 4, 1, 2, 3), torch.from_numpy(wt).double(), None, padding=1)
    return y.permute(0, 2, 3, 4, 1).contiguous()


def _case(name):
    return next(c for c in W.GPU_CASES if c.name == name)


@pytest.mark.parametrize("with_addend", (False, True), ids=("plain", "addend"))
def test_wino3_replicated_sample_equals_the_single_run(amd, gpu, with_addend):
    """3 x 8 x 32 x 32 built from one 8 x 32 x 32 sample, forced entry: 96 tiles on 64 workgroups, a second tile per workgroup in
    every XCD range, ranges that cross a sample"""
    c = _case("w3_second_tile")
    n, vol, cin, cout = c.shape[0], c.shape[1:], c.c0, c.cout
    rs = np.random.RandomState(41 + with_addend)
    x, wt = _random_case(rs, 1, vol, cin, cout)
    bias = rs.standard_normal(cout).astype(np.float32)
    add = torch.from_numpy(rs.standard_normal((1,) + vol + (cout,)).astype(np.float32)).to(gpu) if with_addend else None
    xg = torch.from_numpy(x).to(gpu)
    kernel = W.W3 % ("3, false" if with_addend else "0, false")
    one = amd.ops.conv3d_wino3_ndhwc(xg, wt, bias, addend=add, act=1)
    assert amd.ops.last_conv_kernel() == kernel
    many = amd.ops.conv3d_wino3_ndhwc(xg.repeat(n, 1, 1, 1, 1), wt, bias, addend=None if add is None else add.repeat(n, 1, 1, 1, 1), act=1)
    assert amd.ops.last_conv_kernel() == kernel
    assert torch.isfinite(one).all() and float(one.abs().max()) > 0
    for i in range(n):
        assert torch.equal(many[i], one[0]), (i, int((many[i] != one[0]).sum()))


@pytest.mark.parametrize("name", ("w3_stats_second_tile", "w3_norm_second_tile", "w2_second_tile", "w2_stats"))
def test_replicated_samples_agree_bit_for_bit(amd, gpu, name):
    """Through the planner (a single sample of these shapes goes to another kernel, so the copies are compared with copy 0):
    12 x 4 x 16 x 16, 128 -> 256 with statistics, without and with the fused producer norm - two tiles per workgroup with a
    sample change; 16 x 6 x 7 x 40, 16 -> 128 on conv3_f32_wino2_kernel<0> and, with statistics, <2>"""
    c = _case(name)
    n, vol, cin, cout = c.shape[0], c.shape[1:], c.c0, c.cout
    rs = np.random.RandomState(43 + len(name))
    x, wt = _random_case(rs, 1, vol, cin, cout)
    bias = rs.standard_normal(cout).astype(np.float32)
    xg = torch.from_numpy(x).to(gpu).repeat(n, 1, 1, 1, 1)
    scale = shift = None
    if c.norm:
        scale = torch.from_numpy(rs.uniform(0.5, 2.0, (1, cin)).astype(np.float32)).to(gpu).repeat(n, 1)
        shift = torch.from_numpy(rs.standard_normal((1, cin)).astype(np.float32)).to(gpu).repeat(n, 1)
    y, sums = amd.ops.conv3d_fused_ndhwc(xg, wt, bias, in_scale=scale, in_shift=shift, in_act=1 if c.norm else 0, stats=c.stats, act=1)
    assert amd.ops.last_conv_kernel() == c.kernel
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0
    for i in range(1, n):
        assert torch.equal(y[i], y[0]), (name, i, int((y[i] != y[0]).sum()))
    if c.stats:
        assert torch.isfinite(sums).all()
        for i in range(1, n):
            assert torch.equal(sums[i], sums[0]), (name, i)


@pytest.mark.parametrize("name", ("w3_concat", "w2_concat"))
def test_a_concat_of_two_tensors_equals_the_whole(amd, gpu, name):
    """the chunk order does not change, only the tensor a chunk comes from: the same sums in the same order"""
    c = _case(name)
    n, vol, cin, cout = c.shape[0], c.shape[1:], c.c0 + c.c1, c.cout
    x, wt = _random_case(np.random.RandomState(47 + cin), n, vol, cin, cout)
    ref = _ref64(x, wt)
    xg = torch.from_numpy(x).to(gpu)
    x0, x1 = xg[..., :c.c0].contiguous(), xg[..., c.c0:].contiguous()
    if c.entry == "wino3":
        run = lambda a, b: amd.ops.conv3d_wino3_ndhwc(a, wt, None, x1=b, act=0)  # noqa: E731
    else:
        run = lambda a, b: amd.ops.conv3d_fused_ndhwc(a, wt, None, x1=b, act=0)[0]  # noqa: E731
    whole = run(xg, None)
    assert amd.ops.last_conv_kernel() == c.kernel
    halves = run(x0, x1)
    assert amd.ops.last_conv_kernel() == c.kernel
    ratio = float((halves.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"WINO EXACT {name} {c.kernel}: concat {c.c0} + {c.c1} equals the whole; max error / max|y| = {ratio:.2e} (gate 2e-5)")
    assert torch.isfinite(halves).all() and ratio <= 2e-5 and torch.equal(halves, whole)
