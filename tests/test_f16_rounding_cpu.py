"""The power of the fp16 rounding gate (f16_rounding_util.py), where no GPU is needed: on the operands of the GPU tests
(test_gpu_ops.py: same seeds, same draw order) torch's own fp32 conv passes the gate it calibrates, and each defect an fp16
kernel's epilogue can have - output truncated, conv rounded before bias and LeakyReLU, LeakyReLU in fp16, half the channels
accumulated to an fp16 partial - misses the mismatch cap by at least 3x.  The old gate (2e-3 of the output range) passes
every one of them; their error relative to it is printed next to the mismatch rate."""
import numpy as np
import pytest

import f16_rounding_util as ru

# (n, d, h, w, cin, cout, stride, act): shapes of F16_CONV_CASES - register-staged kernel shape, the stem (Cin = 4), stride 2
# with odd output dims, the bottleneck (K = 27 * 320) - with the network's activation, and the first one as the table has it
CONV_CASES = [
    (1, 8, 8, 32, 32, 32, 1, 1),
    (1, 8, 8, 32, 32, 32, 1, 0),
    (2, 8, 12, 40, 4, 32, 1, 1),
    (2, 10, 6, 14, 64, 32, 2, 1),
    (2, 4, 4, 4, 320, 320, 1, 1),
]
TCONV_CASES = [(2, 3, 5, 6, 64, 32)]
SLOPE = 0.01


def _conv_operands(case):
    """test_conv3d_f16_matches_torch's operands"""
    n, d, h, w, cin, cout, stride, act = case
    rs = np.random.RandomState(17)
    x = rs.standard_normal((n, d, h, w, cin)).astype(np.float32).astype(np.float16)
    wt = (rs.standard_normal((cout, cin, 3, 3, 3)).astype(np.float32) / np.sqrt(cin * 27)).astype(np.float16)
    b = rs.standard_normal((cout,)).astype(np.float32)
    return ru.Operands("conv", x.transpose(0, 4, 1, 2, 3), wt, stride), b, act


def _tconv_operands(case):
    """test_tconv_f16_matches_torch's operands (no bias, no activation)"""
    n, d, h, w, cin, cout = case
    rs = np.random.RandomState(5)
    x = rs.standard_normal((n, d, h, w, cin)).astype(np.float32).astype(np.float16)
    wt = (rs.standard_normal((cin, cout, 2, 2, 2)).astype(np.float32) / np.sqrt(cin)).astype(np.float16)
    return ru.Operands("tconv", x.transpose(0, 4, 1, 2, 3), wt), None, 0


_REFS = {}


def _refs(case):
    """(operands, bias, act, ref32, ref64) of a case, computed once and shared"""
    if case not in _REFS:
        ops, b, act = _conv_operands(case) if len(case) == 8 else _tconv_operands(case)
        ref32, ref64 = ru.reference(ops, b, act, SLOPE, "float32"), ru.reference(ops, b, act, SLOPE, "float64")
        ref32.setflags(write=False); ref64.setflags(write=False)
        _REFS[case] = (ops, b, act, ref32, ref64)
    return _REFS[case]


def _old_gate_ratio(got16, ref32):
    return float(np.abs(got16.astype(np.float32) - ref32).max() / (2e-3 * max(1.0, np.abs(ref32).max())))


@pytest.mark.parametrize("case", CONV_CASES + TCONV_CASES, ids=str)
def test_fp32_reference_passes_its_own_gate(case):
    _, _, _, ref32, ref64 = _refs(case)
    got = ref32.astype(np.float16)
    mismatch, cap, worst, worst_cap = ru.check(f"{case} [torch CPU float32]", got, ref32, ref64)
    assert mismatch <= 0.005, "inputs on which a correct fp32 implementation mismatches more than the floor of the cap"
    assert mismatch <= cap and worst <= worst_cap
    assert cap <= 0.02, cap  # (4 x a natural rate of at most 0.5 %)


@pytest.mark.parametrize("case", CONV_CASES + TCONV_CASES, ids=str)
def test_every_mutant_misses_the_gate(case):
    ops, b, act, ref32, ref64 = _refs(case)
    cap, _ = ru.gate(ref32, ref64)
    names = ru.mutants_that_apply(b, act)
    assert names[:2] == ["truncate", "f16_partial"]
    if len(case) == 8:
        assert "round_before_bias_act" in names and ("act_in_f16" in names) == bool(act)
    weak = {}
    for name in names:
        got = ru.MUTANTS[name](ops, b, act, SLOPE)
        assert got.dtype == np.float16 and got.shape == ref64.shape
        mismatch, worst, bias = ru.rounding_report(got, ref64)
        print(f"MUTANT {case} {name}: mismatch={mismatch:.3f} = {mismatch / cap:.1f} x cap, worst={worst:.2f} bias={bias:+.3f}, "
              f"error / old gate = {_old_gate_ratio(got, ref32):.2f}")
        if not mismatch >= ru.MUTANT_FACTOR * cap:
            weak[name] = mismatch
    assert not weak, f"mutants within {ru.MUTANT_FACTOR} x the cap {cap:.4f}: {weak}"


def test_mutants_that_do_not_apply_are_the_correct_kernel():
    """without bias and activation a second rounding changes nothing; without activation act_in_f16 is one rounding"""
    ops, b, act, ref32, _ = _refs(TCONV_CASES[0])
    want = ref32.astype(np.float16)
    assert np.array_equal(ru.round_before_bias_act(ops, b, act, SLOPE).view(np.uint16), want.view(np.uint16))
    assert np.array_equal(ru.act_in_f16(ops, b, act, SLOPE).view(np.uint16), want.view(np.uint16))


def test_truncate_mutant_rounds_toward_zero():
    ops, b, act, ref32, _ = _refs(CONV_CASES[0])
    got = ru.truncate(ops, b, act, SLOPE).astype(np.float32)
    assert (np.abs(got) <= np.abs(ref32)).all()
    assert (np.abs(ref32) - np.abs(got) < ru.ulp16(ref32)).all()
    _, _, bias = ru.rounding_report(got.astype(np.float16), ref32.astype(np.float64))
    assert -0.55 <= bias <= -0.45, bias


def test_ulp16_binade_edges_subnormal_zero():
    v = np.array([1.0, 2.0 - 2.0 ** -10, 2.0, 0.999, 1000.0, 1024.0, 65504.0, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12),
                  2.0 ** -20, 2.0 ** -24, 0.0])
    want = np.array([2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 0.5, 1.0, 32.0, 2.0 ** -24, 2.0 ** -24,
                     2.0 ** -24, 2.0 ** -24, 2.0 ** -24])
    assert np.array_equal(ru.ulp16(v), want)
    assert np.array_equal(ru.ulp16(-v), want)
    # agrees with numpy's spacing of the fp16 numbers themselves
    h = np.array([1.0, 1.5, 3.0, 0.1, 6.1e-5, 6e-8, 300.0], np.float16)
    assert np.array_equal(ru.ulp16(h.astype(np.float64)), np.spacing(h).astype(np.float64))
    # the binade is the REFERENCE's: just below a power of two the spacing is the smaller one
    assert ru.ulp16(1.0 - 1e-9) == 2.0 ** -11


def test_rounding_report_counts_known_differences():
    ref = np.linspace(0.51, 3.9, 1000)
    ref[10], ref[11] = 0.0, -0.0
    got = ref.astype(np.float16)
    got[11], got[10] = 0.0, -0.0            # signed zeros swapped: equal
    up, down = [100, 200, 300], [400, 500]  # five one-ulp differences
    got[up] = np.nextafter(got[up], np.float16(np.inf))
    got[down] = np.nextafter(got[down], np.float16(-np.inf))
    mismatch, worst, bias = ru.rounding_report(got, ref)
    assert mismatch == 5 / 1000
    assert 0.5 <= worst <= 1.5  # one ulp away from RNE16(ref), which is itself within half an ulp of ref
    exact = ref.astype(np.float16)
    assert ru.rounding_report(exact, ref)[0] == 0.0 and ru.rounding_report(exact, ref)[1] <= 0.5
    assert abs(bias) < 0.05
    # two ulps off at one element: worst sees it although the rate does not
    got = exact.copy()
    got[700] = np.nextafter(np.nextafter(got[700], np.float16(np.inf)), np.float16(np.inf))
    mismatch, worst, _ = ru.rounding_report(got, ref)
    assert mismatch == 1 / 1000 and worst > 1.0
    # near zero the error scale is 2^-16, not the subnormal spacing
    tiny_ref = np.array([1e-7, -3e-6, 0.0])
    tiny_got = np.array([1e-5, -3e-6, 0.0], np.float16)
    mismatch, worst, _ = ru.rounding_report(tiny_got, tiny_ref)
    assert mismatch == pytest.approx(1 / 3) and worst == pytest.approx(abs(float(tiny_got[0]) - 1e-7) / 2.0 ** -16)
    # a NaN from the kernel fails both
    bad = exact.copy()
    bad[5] = np.nan
    mismatch, worst, _ = ru.rounding_report(bad, ref)
    assert mismatch == 1 / 1000 and not worst <= 1.0


def test_natural_rate_and_gate():
    ref64 = np.linspace(0.51, 3.9, 1000)
    ref32 = ref64.astype(np.float32)
    assert ru.natural_rate(ref32, ref64) == 0.0
    assert ru.gate(ref32, ref64) == (0.005, 1.0)
    off = ref32.copy()
    off[:20] *= 1.002  # 2 % of the elements on another fp16 number
    assert ru.natural_rate(off, ref64) == pytest.approx(0.02)
    assert ru.gate(off, ref64) == (pytest.approx(0.08), 1.0)
