"""-m gpu: the least-padding hint of the stride-2 LDS-DMA planner (ConvCall::s2_least_padding, MI355_S2_LEAST_PADDING) on single ops.

The hint swaps conv3_f32_s2dma_kernel<5> (2 x 2 x 32 output tiles) for <4> (2 x 4 x 16) where that pads fewer lanes.  Both
instantiations sum an output voxel in the same order (channel chunk, dz, tap), so the two outputs are EQUAL BIT FOR BIT; both lie
within the suite's fp32 conv gate of the fp64 reference (2e-5 of max(1, |ref|), tests/test_gpu_ops.py).  Through the plain kernel
and through its view twin (tests/test_gpu_stage0_views.py), 32 -> 64:
  * N = 2, 8 x 16 x 80: Wo = 40, three 16-wide tiles against two 32-wide, the last tile of either half empty;
  * N = 1, 6 x 24 x 144: Wo = 72, the region launch of the bench geometry in small - five tiles against three, Do = 3 (an odd depth:
    the last z tile is half empty), Ho = 12 a whole number of both tiles' rows;
  * the view with a face bit set on every axis (and, on the second sample, the opposite faces): shell pieces and in-place pieces in
    one brick of either shape."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_stage0_views import S2, S2_VIEW, view_case

pytestmark = pytest.mark.gpu

CASES = {"wo40": (2, (8, 16, 80), (12, 24, 88)), "wo72": (1, (6, 24, 144), (10, 32, 152))}   # name: (N, P, volume of the view's source)
FACES = ((1, 0, 0, 1, 1, 0), (0, 1, 1, 0, 0, 1))   # a face on every axis; sample 1: the opposite ones


@pytest.fixture(scope="module")
def operands():
    rs = np.random.RandomState(77)
    wt = (rs.standard_normal((64, 32, 3, 3, 3)) / np.sqrt(32 * 27)).astype(np.float32)
    b = (0.1 * rs.standard_normal(64)).astype(np.float32)
    return wt, b


def _ref(x, wt, b):
    y = F.conv3d(torch.from_numpy(x).double().permute(0, 4, 1, 2, 3), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), stride=2, padding=1)
    return F.leaky_relu(y, 0.01).permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_hint_flips_the_kernel_and_no_bit(amd, gpu, operands, name):
    n, P, Ve = CASES[name]
    wt, b = operands
    rs = np.random.RandomState(len(name) + P[2])
    vol = rs.standard_normal((1,) + Ve + (32,)).astype(np.float32)
    dense, assembled, samples = view_case(rs, vol, P, 2, FACES)   # (two samples at ORIGINS (3, 5, 7) and (0, 8, 0): both fit Ve)
    dense, assembled, samples = dense[:n], assembled[:n], samples[:n]
    src = torch.from_numpy(vol).to(gpu)
    ref = _ref(assembled, wt, b)
    gate = 2e-5 * max(1.0, float(ref.abs().max()))
    outs = {}
    for hint, txl in ((False, 5), (True, 4)):
        outs["plain", hint] = amd.ops.conv3d_s2dma_view_ndhwc(torch.from_numpy(assembled).to(gpu), wt, b, act=1, s2_least_padding=hint)
        assert amd.ops.last_conv_kernel() == S2 % txl
        outs["view", hint] = amd.ops.conv3d_s2dma_view_ndhwc(torch.from_numpy(dense).to(gpu), wt, b, view=(src, samples, 2), act=1, s2_least_padding=hint)
        assert amd.ops.last_conv_kernel() == S2_VIEW % txl
    for key, y in outs.items():
        err = float((y.double().cpu() - ref).abs().max())
        print(f"s2 least padding {name} {key}: max error {err:.2e}, gate {gate:.2e}")
        assert torch.isfinite(y).all() and err <= gate, key
    assert torch.equal(outs["plain", True], outs["plain", False])
    assert torch.equal(outs["view", True], outs["view", False])
    assert torch.equal(outs["view", True], outs["plain", True])


def test_the_planned_call_takes_the_hint_too(amd, gpu, operands):
    """Not forced: a call large enough for the planner's own rule (tiles x cout blocks >= 768 in either shape) - N = 8, 32 x 32 x 80."""
    wt, b = operands
    x = torch.from_numpy(np.random.RandomState(5).standard_normal((8, 32, 32, 80, 32)).astype(np.float32)).to(gpu)
    want = amd.ops.conv3d_s2dma_view_ndhwc(x, wt, b, act=1, force=False)
    assert amd.ops.last_conv_kernel() == S2 % 5
    got = amd.ops.conv3d_s2dma_view_ndhwc(x, wt, b, act=1, force=False, s2_least_padding=True)
    assert amd.ops.last_conv_kernel() == S2 % 4
    assert torch.isfinite(want).all() and torch.equal(got, want)
