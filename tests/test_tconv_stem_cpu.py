"""The cases of tconv_stem_util.py are what they claim to be, and the references of tests/test_gpu_tconv_stem.py are right
(no device).

* int_tconv equals torch's float64 conv_transpose3d on the operands of every version-2 case and on a crop of a version-3 case;
  int_conv on the stem cases equals torch's float64 conv3d.
* Closure: each of the six tconv kernel names has a case with a ragged last tile, one with whole tiles and one whose tiles
  straddle a sample boundary; the version-2 names have a whole chunk followed by a partial one and the minimum Cin; every stem
  dtype is ragged in z, in y, in x and in none, with and without statistics.  What a case declares (kernel, tail, straddles,
  ragged_axes) is recomputed from its shape.
* expected_tconv_kernel against the thresholds of tconv.hip written out once more.
* dot_bound, the per-element fp32 gate, holds for numpy float32 dot products in three summation orders and rejects a result
  that is off by 2^-12 relative."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_rows_util as R
import tconv_stem_util as U


def _torch_tconv64(x, wt):
    ref = F.conv_transpose3d(torch.from_numpy(x.astype(np.float64)).permute(0, 4, 1, 2, 3), torch.from_numpy(wt.astype(np.float64)), None, stride=2)
    return ref.permute(0, 2, 3, 4, 1).contiguous().numpy()


def _torch_conv64(x, wt, b):
    ref = F.conv3d(torch.from_numpy(x.astype(np.float64)).permute(0, 4, 1, 2, 3), torch.from_numpy(wt.astype(np.float64)),
                   torch.from_numpy(b.astype(np.float64)), padding=1)
    return ref.permute(0, 2, 3, 4, 1).contiguous().numpy()


V2_CASES = [c for c in U.TCONV_CASES if U.is_v2(c)]
V3_CASES = [c for c in U.TCONV_CASES if not U.is_v2(c)]


@pytest.mark.parametrize("case", V2_CASES, ids=[c.name for c in V2_CASES])
def test_int_tconv_is_conv_transpose3d(case):
    x, wt = U.int_tconv_operands(case)
    assert -4 <= x.min() < 0 < x.max() <= 4 and set(np.unique(wt)) == {-1, 0, 1}
    assert (wt != 0).any(axis=(1, 2, 3, 4)).all()  # no input channel is dropped from the check
    got = U.int_tconv(x, wt)
    n, d, h, w = case.shape
    assert got.dtype == np.int64 and got.shape == (n, 2 * d, 2 * h, 2 * w, case.cout)
    assert np.array_equal(got, _torch_tconv64(x, wt)), case.name
    assert np.abs(got).max() <= 4 * case.cin < R.INT_BOUND
    assert np.array_equal(U.int_tconv(x, wt, np.int16), got)  # (the narrow form the version-3 cases use)


def test_int_tconv_is_conv_transpose3d_on_a_v3_crop():
    """the operands of a persistent-kernel case, cropped to 3 x 5 x 65 voxels: the narrow reference type, a long x row"""
    case = next(c for c in V3_CASES if c.dtype == "f16" and c.cin == 128)
    x, wt = U.int_tconv_operands(case)
    x = np.ascontiguousarray(x[:, 7:10, 11:16])
    got = U.int_tconv(x, wt, np.int16)
    assert got.dtype == np.int16 and np.array_equal(got, _torch_tconv64(x, wt))


def test_int_tconv_sees_a_shifted_parity():
    """the scatter itself: every one of the eight parity planes of the output is its own GEMM, and moving one of them by a voxel
    changes the result"""
    case = next(c for c in V2_CASES if c.shape == U.T_STRADDLE)
    x, wt = U.int_tconv_operands(case)
    got = U.int_tconv(x, wt)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                plane = np.einsum("ndhwi,io->ndhwo", x.astype(np.int64), wt[:, :, a, b, c].astype(np.int64))
                assert np.array_equal(got[:, a::2, b::2, c::2], plane), (a, b, c)
                assert not np.array_equal(got[:, a::2, b::2, c::2], np.roll(plane, 1, axis=3))


@pytest.mark.parametrize("case", U.STEM_CASES, ids=[c.name for c in U.STEM_CASES])
def test_int_conv_on_stem_cases_is_conv3d(case):
    c = U.stem_as_conv_case(case)
    assert (c.cin, c.stride, c.env, c.slope, c.kernel) == (4, 1, {}, 0.01, U.STEM_KERNEL[case.dtype])
    x, wt, b = R.int_operands(c)
    assert 27 * 4 * 4 + 8 < R.INT_BOUND
    acc = R.int_conv(x, wt, b, 1)
    assert acc.shape == case.shape + (case.cout,) and np.array_equal(acc, _torch_conv64(x, wt, b))
    assert np.abs(acc).max() < R.INT_BOUND


def test_tconv_cases_declare_what_their_shapes_are():
    for c in U.TCONV_CASES:
        n, d, h, w = c.shape
        m = n * d * h * w
        assert c.tail == m % 128, c
        # tile by tile: the samples of the first and the last voxel of every 128-voxel tile
        first = np.arange(0, m, 128) // (d * h * w)
        last = np.minimum(np.arange(0, m, 128) + 127, m - 1) // (d * h * w)
        assert c.straddles == bool((first != last).any()) == (n > 1 and bool((first != last).any())), c
        assert c.kernel == U.expected_tconv_kernel(c.dtype, c.cin, m) and c.kernel in U.TCONV_KERNELS, c
        assert c.cin % U.TCONV_MIN_CIN[c.dtype] == 0 and c.cout in (32, 64, 96) and c.cout % 32 == 0, c
        assert 4 * c.cin < R.INT_BOUND, c
    v3 = {c.shape for c in V3_CASES}
    assert v3 == {U.T_V3_RAGGED, U.T_V3_STRADDLE}
    assert U.tconv_tiles(U.tconv_voxels(U.T_V3_RAGGED)) == 1024 and U.tconv_voxels(U.T_V3_RAGGED) % 128 == 31
    assert U.tconv_voxels(U.T_V3_STRADDLE) == 1037 * 128 and (17 * 61 * 64) // 128 == 518 and (17 * 61 * 64) % 128 == 64


def test_every_tconv_kernel_has_ragged_whole_and_straddling_cases():
    by_kernel = collections.defaultdict(list)
    for c in U.TCONV_CASES:
        by_kernel[c.kernel].append(c)
    assert set(by_kernel) == set(U.TCONV_KERNELS) and len(U.TCONV_KERNELS) == 6
    for kernel, mine in by_kernel.items():
        assert any(c.tail != 0 for c in mine), f"{kernel}: no case with a ragged last tile"
        assert any(c.tail == 0 for c in mine), f"{kernel}: no whole-tile case"
        assert any(c.straddles for c in mine), f"{kernel}: no case whose tiles straddle a sample boundary"
    for dtype, kernel in (("f32", U.F32_V2), ("f16", U.F16_V2)):
        mine = by_kernel[kernel]
        assert all(c.dtype == dtype for c in mine) and 10 <= len(mine) <= 14
        assert any(U.full_then_partial_chunk(c.cin) for c in mine), kernel
        assert any(c.cin == U.TCONV_MIN_CIN[dtype] for c in mine), kernel
        # the stale quads of a whole chunk behind a partial one, on the shape whose tiles straddle and end ragged
        assert any(U.full_then_partial_chunk(c.cin) and 64 < c.cin < 128 and c.shape == U.T_STRADDLE for c in mine), kernel
        want_cin = {"f32": {8, 24, 64, 72, 136, 320}, "f16": {16, 48, 64, 80, 144, 320}}[dtype]
        assert {c.cin for c in mine} == want_cin and {c.cout for c in mine} == {32, 96}
        assert {c.shape for c in mine} == {U.T_M3, U.T_TILE, U.T_STRADDLE, U.T_W1}
        assert any(U.tconv_voxels(c.shape) < 32 for c in mine) and any(U.tconv_voxels(c.shape) == 128 for c in mine)
    # the persistent kernels: two cout blocks (half as many workgroups per block) in fp32 and on <2> or <4>
    assert {(c.shape, c.cout) for c in by_kernel[U.F32_V3]} == {(U.T_V3_RAGGED, 32), (U.T_V3_RAGGED, 64), (U.T_V3_STRADDLE, 64)}
    assert any(c.cout == 64 for c in by_kernel[U.F16_V3[32]] + by_kernel[U.F16_V3[64]])


def test_every_stem_dtype_is_ragged_on_each_axis_and_on_none_with_and_without_statistics():
    for c in U.STEM_CASES:
        assert c.ragged_axes == U.stem_ragged_axes(c.shape) == "".join(a for a, v, t in zip("zyx", c.shape[1:], (4, 4, 32)) if v % t), c
        assert c.cout % 32 == 0 and c.act in (0, 1), c
    for dtype in ("f32", "f16"):
        mine = [c for c in U.STEM_CASES if c.dtype == dtype]
        assert [(c.shape, c.cout, c.act, c.stats) for c in mine] == [
            ((1, 1, 1, 1), 32, 1, False), ((1, 5, 6, 7), 32, 1, False), ((1, 3, 2, 33), 96, 1, False), ((2, 9, 7, 35), 64, 0, True),
            ((1, 4, 4, 32), 32, 1, False), ((1, 8, 8, 64), 64, 1, True)]
        for stats in (False, True):
            for axis in "zyx":
                assert any(axis in c.ragged_axes for c in mine if c.stats == stats), (dtype, stats, axis)
            assert any(not c.ragged_axes for c in mine if c.stats == stats), (dtype, stats)
        assert any(c.shape[1] < 4 and c.shape[2] < 4 and c.shape[3] % 32 == 1 and c.cout == 96 for c in mine), dtype


def test_expected_tconv_kernel_thresholds():
    """the rule of tconv2_mfma_f32 / tconv2_mfma_f16, written out: 1024 tiles of 128 voxels, Cin 64 (fp32), Cin 32 / 64 / 128 (fp16)"""
    e = U.expected_tconv_kernel
    lo, hi = 1023 * 128, 1023 * 128 + 1   # 1023 tiles, 1024 tiles
    assert e("f32", 64, lo) == "tconv2_f32_mfma_v2_kernel" and e("f32", 64, hi) == "tconv2_f32_mfma_v3_kernel<8>"
    assert e("f32", 64, 1024 * 128) == "tconv2_f32_mfma_v3_kernel<8>" and e("f32", 64, 1 << 24) == "tconv2_f32_mfma_v3_kernel<8>"
    for cin in (8, 32, 72, 128, 320):
        assert e("f32", cin, hi) == "tconv2_f32_mfma_v2_kernel" == e("f32", cin, 1 << 24), cin
    for cin, g in ((32, 2), (64, 4), (128, 8)):
        assert e("f16", cin, lo) == "tconv2_f16_mfma_v2_kernel" and e("f16", cin, hi) == f"tconv2_f16_mfma_v3_kernel<{g}>"
    for cin in (16, 48, 80, 96, 144, 256, 320):
        assert e("f16", cin, hi) == "tconv2_f16_mfma_v2_kernel" == e("f16", cin, 1 << 24), cin
    assert e("f32", 64, 1) == "tconv2_f32_mfma_v2_kernel" and e("f16", 64, 1) == "tconv2_f16_mfma_v2_kernel"


# ------------------------------------------------------------------ dot_bound
# Operands with a mean: on zero-mean Gaussians a K-term sum cancels to ~ K^-1/2 of sum |x_i w_i|, and a relative perturbation of
# the RESULT by 2^-12 is then smaller than (K + 4) 2^-24 sum |x_i w_i| wherever |sum| / sum| | < (K + 4) 2^-12 - about 8 % of the
# outputs at K = 108, whatever the gate.  x ~ N(1, 1), w ~ N(1, 1) K^-1/2 keeps |sum| / sum| | near 0.6: what is measured is
# the gate, not the cancellation of the operands.
def _gauss(rs, shape, mean):
    return (rs.standard_normal(shape) + mean).astype(np.float32)


def _assert_gate_holds_and_has_teeth(label, a, b, bias, k):
    """a [M, K], b [K, N] float32, bias [N] float32 or None"""
    assert a.shape[1] == b.shape[0] and k >= a.shape[1]
    ref64 = a.astype(np.float64) @ b.astype(np.float64)
    abs_sum = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    if bias is not None:
        ref64 = ref64 + bias.astype(np.float64)
        abs_sum = abs_sum + np.abs(bias).astype(np.float64)
    bound = U.dot_bound(abs_sum, k)
    for order in ("forward", "reversed", "pairwise"):
        got = U.dots_f32(a, b, order)
        if bias is not None:
            got = got + bias
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - ref64)
        print(f"DOT BOUND {label} {order}: worst error / bound {np.max(err / bound):.3f} over {err.size} outputs")
        assert (err <= bound).all(), (label, order, float(np.max(err / bound)))
    outside = np.abs(ref64 * (1.0 + 2.0 ** -12) - ref64) > bound
    print(f"DOT BOUND {label}: a result off by 2^-12 relative is outside the bound on {outside.mean():.4f} of the outputs")
    assert outside.mean() >= 0.99, (label, float(outside.mean()))


def test_dot_bound_holds_for_fp32_sums_and_has_teeth_tconv():
    case = next(c for c in V2_CASES if c.dtype == "f32" and c.shape == U.T_STRADDLE and c.cin == 72)
    rs = np.random.RandomState(31)
    x = _gauss(rs, case.shape + (case.cin,), 1.0)
    wt = (_gauss(rs, (case.cin, case.cout, 2, 2, 2), 1.0) / np.sqrt(case.cin)).astype(np.float32)
    _assert_gate_holds_and_has_teeth(case.name, x.reshape(-1, case.cin), U.tconv_matrix(wt), None, case.cin)
    # (the GEMM form is the op: scattered, it is torch's transposed conv)
    got = U.scatter_parities(x.reshape(-1, case.cin).astype(np.float64) @ U.tconv_matrix(wt).astype(np.float64), case.shape, case.cout)
    assert np.allclose(got, _torch_tconv64(x, wt), rtol=1e-12, atol=1e-12)


def test_dot_bound_holds_for_fp32_sums_and_has_teeth_stem():
    case = next(c for c in U.STEM_CASES if c.dtype == "f32" and c.shape == (1, 5, 6, 7))
    rs = np.random.RandomState(32)
    x = _gauss(rs, case.shape + (4,), 1.0)
    wt = (_gauss(rs, (case.cout, 4, 3, 3, 3), 1.0) / np.sqrt(108)).astype(np.float32)
    b = _gauss(rs, (case.cout,), 0.0)
    cols, wmat = U.conv_cols(x), U.conv_matrix(wt)
    assert cols.shape[1] == 108
    _assert_gate_holds_and_has_teeth(case.name, cols, wmat, b, 108)
    got = (cols.astype(np.float64) @ wmat.astype(np.float64) + b).reshape(case.shape + (case.cout,))
    assert np.allclose(got, _torch_conv64(x, wt, b), rtol=1e-12, atol=1e-12)


def test_dot_bound_is_the_formula():
    assert U.dot_bound(1.0, 108) == 112 * 2.0 ** -24 + 1e-30 and U.dot_bound(0.0, 8) == 1e-30
    assert np.array_equal(U.dot_bound(np.array([2.0, 4.0]), 64), np.array([68 * 2.0 ** -23, 68 * 2.0 ** -22]) + 1e-30)
