"""-m gpu: the fp32 stride-2 LDS-DMA kernels as split-bf16 products (conv3d_s2dma_body.h), on single ops.

Every fp32 operand is cut into three bf16 pieces (hi, mid, lo) and six of the nine piece products are summed on the bf16 matrix
pipe.  Everything here goes through ops.conv3d_s2dma_view_ndhwc(force=True), act = none, with and without the least-padding hint
(on S1 both give 2 x 2 x 32 tiles - its padded sizes tie -, on S2 the hint swaps the tile shape); the view twin runs in the last test:

  S1  1 x 6 x 8 x 48, 8 -> 64: outputs 3 x 4 x 24 on 2 x 2 x 32 tiles, ragged in x; one channel chunk, one cout block;
  S2  2 x 9 x 20 x 40, 16 -> 128: outputs 5 x 10 x 20 on 2 x 4 x 16 tiles (2 x 2 x 32 with the hint), ragged on every axis; two
      chunks, two cout blocks; also with its channels as a concat of 8 + 8.

* exactness by piece class: integer operands whose sums stay below 2^24 (no order of addition rounds), so the output must EQUAL the
  integer reference.  Each class puts its information into one kind of piece: a dropped or misplaced piece moves an output by >= 1;
* the two tile shapes, and view against plain, agree bit for bit;
* random data within the suite's 2e-5 of max|y| of an fp64 reference (the measured ratio is printed: run with -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_stage0_views import S2, S2_VIEW, view_case

pytestmark = pytest.mark.gpu

SHAPES = {"S1": (1, (6, 8, 48), 8, 64), "S2": (2, (9, 20, 40), 16, 128)}   # name: (N, input D x H x W, cin, cout)


def _ref64(x, wt):
    y = F.conv3d(torch.from_numpy(x).double().permute(0, 4, 1, 2, 3), torch.from_numpy(wt).double(), None, stride=2, padding=1)
    return y.permute(0, 2, 3, 4, 1).contiguous()


def _thin(rs, wt, keep):
    """at most `keep` non-zero weights per output channel"""
    flat = wt.reshape(wt.shape[0], -1)
    out = np.zeros_like(flat)
    for co in range(flat.shape[0]):
        idx = rs.choice(flat.shape[1], size=keep, replace=False)
        out[co, idx] = flat[co, idx]
    return out.reshape(wt.shape)


def _ints(rs, shape, bound):
    return rs.randint(-bound, bound + 1, size=shape).astype(np.float32)


def _signs_nonzero(rs, shape):
    return rs.choice(np.array([-1.0, 1.0], np.float32), size=shape)


def _operands(rs, cls, n, P, cin, cout):
    xs, ws = (n,) + P + (cin,), (cout, cin, 3, 3, 3)
    if cls == "x_mid":      # (i) the mid pieces of x: 12-bit inputs, weights in {-1, 0, 1}; |sum| <= 27 * 16 * 4095 < 2^21
        return _ints(rs, xs, 4095), _ints(rs, ws, 1)
    if cls == "w_mid":      # (ii) the mid pieces of w; |sum| <= 27 * 16 * 4 * 4095 < 2^23
        return _ints(rs, xs, 4), _ints(rs, ws, 4095)
    if cls == "x_lo":       # (iii) the lo pieces of x: 20-bit inputs, 8 unit weights per output channel; |sum| < 8 * 2^20
        return _ints(rs, xs, (1 << 20) - 1), _thin(rs, _signs_nonzero(rs, ws), 8)
    if cls == "w_lo":       # (iv) mirrored: 20-bit weights, 8 per output channel, inputs in {-1, 0, 1}
        return _ints(rs, xs, 1), _thin(rs, _ints(rs, ws, (1 << 20) - 1), 8)
    if cls == "mid_mid":    # (v) the mid x mid product: both 12-bit, one weight per output channel; 4095^2 < 2^24
        return _ints(rs, xs, 4095), _thin(rs, _ints(rs, ws, 4095), 1)
    raise KeyError(cls)


@pytest.mark.parametrize("cls", ["x_mid", "w_mid", "x_lo", "w_lo", "mid_mid"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_integer_operands_are_exact_by_piece_class(amd, gpu, shape, cls):
    n, P, cin, cout = SHAPES[shape]
    rs = np.random.RandomState(sum(map(ord, shape + cls)))
    x, wt = _operands(rs, cls, n, P, cin, cout)
    ref = _ref64(x, wt)
    assert float(ref.abs().max()) < 2 ** 24 and float(ref.abs().max()) > 0
    assert float(_ref64(np.abs(x), np.abs(wt)).max()) < 2 ** 24   # no partial sum in any order rounds
    want = ref.to(torch.int64)
    for hint in (False, True):
        y = amd.ops.conv3d_s2dma_view_ndhwc(torch.from_numpy(x).to(gpu), wt, None, act=0, s2_least_padding=hint).cpu()
        assert amd.ops.last_conv_kernel() in (S2 % 4, S2 % 5)
        assert torch.isfinite(y).all() and torch.equal(y, y.round())
        bad = int((y.to(torch.int64) != want).sum())
        assert bad == 0, (shape, cls, hint, bad, float((y.double() - ref).abs().max()))


def _random_case(rs, n, P, cin, cout):
    x = rs.standard_normal((n,) + P + (cin,)).astype(np.float32)
    x = (3.0 * np.where(x > 0, x, 0.01 * x)).astype(np.float32)
    wt = (rs.standard_normal((cout, cin, 3, 3, 3)) * np.sqrt(2.0 / (cin * 27))).astype(np.float32)
    return x, wt


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_random_data_within_the_fp32_gate(amd, gpu, shape):
    n, P, cin, cout = SHAPES[shape]
    x, wt = _random_case(np.random.RandomState(11 + cin), n, P, cin, cout)
    ref = _ref64(x, wt)
    top = float(ref.abs().max())
    for hint in (False, True):
        y = amd.ops.conv3d_s2dma_view_ndhwc(torch.from_numpy(x).to(gpu), wt, None, act=0, s2_least_padding=hint)
        ratio = float((y.double().cpu() - ref).abs().max()) / top
        print(f"s2 split {shape} {amd.ops.last_conv_kernel()}: max error / max|y| = {ratio:.2e} (gate 2e-5)")
        assert torch.isfinite(y).all() and ratio <= 2e-5, (shape, hint, ratio)


def test_both_tile_shapes_sum_in_one_order(amd, gpu):
    """S2: 2 x 4 x 16 tiles without the hint, 2 x 2 x 32 with it (Wo = 20: 32 columns either way, 12 rows against 10)."""
    n, P, cin, cout = SHAPES["S2"]
    x, wt = _random_case(np.random.RandomState(23), n, P, cin, cout)
    xg = torch.from_numpy(x).to(gpu)
    outs = []
    for hint, txl in ((False, 4), (True, 5)):
        outs.append(amd.ops.conv3d_s2dma_view_ndhwc(xg, wt, None, act=0, s2_least_padding=hint))
        assert amd.ops.last_conv_kernel() == S2 % txl
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def test_a_concat_of_two_halves_equals_the_whole(amd, gpu):
    """S2 with its 16 channels as 8 + 8 from two tensors: chunk 1 comes from the second one; the same sums in the same order."""
    n, P, cin, cout = SHAPES["S2"]
    x, wt = _random_case(np.random.RandomState(29), n, P, cin, cout)
    ref = _ref64(x, wt)
    xg = torch.from_numpy(x).to(gpu)
    x0, x1 = xg[..., :8].contiguous(), xg[..., 8:].contiguous()
    for hint in (False, True):
        whole = amd.ops.conv3d_s2dma_view_ndhwc(xg, wt, None, act=0, s2_least_padding=hint)
        halves = amd.ops.conv3d_s2dma_view_ndhwc(x0, wt, None, act=0, s2_least_padding=hint, x1=x1)
        assert amd.ops.last_conv_kernel() == S2 % (5 if hint else 4)
        ratio = float((halves.double().cpu() - ref).abs().max() / ref.abs().max())
        print(f"s2 split concat 8 + 8, hint {hint}: max error / max|y| = {ratio:.2e} (gate 2e-5)")
        assert torch.isfinite(halves).all() and ratio <= 2e-5 and torch.equal(halves, whole)


def test_view_and_plain_agree_bit_for_bit(amd, gpu):
    """S2's tile inside a 12 x 28 x 48 volume, shells 2 deep with a face on every axis (sample 1: the opposite faces)."""
    n, P, cin, cout = SHAPES["S2"]
    rs = np.random.RandomState(31)
    _, wt = _random_case(rs, n, P, cin, cout)
    vol = (3.0 * rs.standard_normal((1, 12, 28, 48, cin))).astype(np.float32)
    dense, assembled, samples = view_case(rs, vol, P, 2, ((1, 0, 0, 1, 1, 0), (0, 1, 1, 0, 0, 1)))
    src = torch.from_numpy(vol).to(gpu)
    for hint, txl in ((False, 4), (True, 5)):
        want = amd.ops.conv3d_s2dma_view_ndhwc(torch.from_numpy(assembled).to(gpu), wt, None, act=0, s2_least_padding=hint)
        assert amd.ops.last_conv_kernel() == S2 % txl
        got = amd.ops.conv3d_s2dma_view_ndhwc(torch.from_numpy(dense).to(gpu), wt, None, view=(src, samples, 2), act=0, s2_least_padding=hint)
        assert amd.ops.last_conv_kernel() == S2_VIEW % txl
        assert torch.isfinite(want).all() and torch.equal(got, want), txl
