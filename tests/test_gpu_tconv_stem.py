"""-m gpu: every case of tconv_stem_util.py on the GPU - the first-layer kernels of conv_stem.hip and the transposed-conv kernels
of tconv.hip, nine instantiations that sit in no conv row table (tests/test_tconv_stem_cpu.py keeps the set of cases closed and
checks the references used here).  They are held to the three checks of test_gpu_conv_rows.py:

a. the gates of test_gpu_ops.py, by calling that module's test functions with the case's shape (2e-5 / 2e-3 of the range, the
   RNE16 gate in fp16, the two 1e-4 gates of the statistics), and the kernel that ran is asserted (mi355_last_conv_kernel);
   in fp32, on Gaussian operands, also element by element: |y - ref64| <= dot_bound(sum |x_i w_i|, K), the worst-case bound of
   a K-term fp32 dot product in any order (tconv_stem_util.dot_bound; version-2 tconv cases and stem cases);
b. exact integers: operands so small that no partial sum is rounded in fp32 or fp16, so the output must EQUAL the integer
   reference (np.array_equal; the message names the first differing (n, z, y, x, cout)); a store from a lane past a ragged
   edge, a wrong parity offset or a stale LDS quad changes some output by at least 1/2;
c. nothing outside the output may be written: the output pointer sits in the middle of a buffer of sentinels, a sample's worth
   on either side.  The fp32 kernels store straight into it.  The fp16 kernels store into a channel-blocked buffer the entry
   point owns; it has guard bands of its own there and fails the call if one changed (single_op.hip guards_intact), and the
   sentinels here watch the layout converter.

Stem cases run through test_gpu_conv_rows.run_case (a stem case is a conv case with Cin = 4); tconv cases call
mi355_tconv3d_ndhwc / mi355_tconv3d_ndhwc_f16 directly.  MI355_TCONV_V3 is read once per process, so the switched-off form of
the two smallest persistent-kernel cases runs in one child."""
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest
import torch

import conv_rows_util as R
import tconv_stem_util as U
import test_gpu_conv_rows as rows
import test_gpu_ops as ops_tests

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = rows.SENTINEL  # 4096: exact in fp16 and fp32, and no output of an integer run reaches it (|y| < 2048)


def _per_element(label, ran, y, ref64, abs_sum, k):
    """the fp32 gate of (a): returns the worst error as a share of the bound"""
    assert y.dtype == np.float32 and y.shape == ref64.shape == abs_sum.shape, (label, y.dtype, y.shape, ref64.shape)
    err, bound = np.abs(y.astype(np.float64) - ref64), U.dot_bound(abs_sum, k)
    worst = float(np.max(err / bound))
    print(f"PER ELEMENT {label} [{ran}]: worst |y - ref64| is {worst:.3f} of dot_bound (K = {k}) over {err.size} outputs", flush=True)
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, (f"{label} [{ran}]: {len(bad)} of {err.size} outputs miss the fp32 dot-product bound, first at (n, z, y, x, cout) = "
                           f"{tuple(bad[0])}: {y[tuple(bad[0])]!r} against {ref64[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]:.3e}")
    return worst


# ------------------------------------------------------------------ stem
def _stem_per_element(amd, dev, c):
    """Gaussian operands scaled as test_conv3d_mfma_matches_torch scales them, judged element by element against the fp64 conv"""
    rs = np.random.RandomState(zlib.crc32(("gauss " + c.name).encode()) % (2 ** 31))
    x = ops_tests._rand(rs, *c.shape, 4)
    wt = (ops_tests._rand(rs, c.cout, 4, 3, 3, 3) / np.sqrt(108)).astype(np.float32)
    b = ops_tests._rand(rs, c.cout)
    y = amd.ops.conv3d_ndhwc(torch.from_numpy(x).to(dev), wt, b, stride=1, act=c.act, slope=0.01).cpu().numpy()
    ran = amd.ops.last_conv_kernel()
    assert ran == U.STEM_KERNEL["f32"], (c.name, ran)
    ref64 = ops_tests._ref_conv64(x, wt, b, 1, c.act, 0.01)
    abs_sum = ops_tests._ref_conv64(np.abs(x), np.abs(wt), np.abs(b), 1, 0, 0.01)  # conv(|x|, |w|) + |b|
    return _per_element(c.name, ran, y, ref64, abs_sum, 108)


@pytest.mark.parametrize("case", U.STEM_CASES, ids=[c.name for c in U.STEM_CASES])
def test_stem_case(amd, gpu, case):
    rows.run_case(amd, gpu, U.stem_as_conv_case(case), check_kernel=True,
                  tag=f"STEM CASE (ragged in {case.ragged_axes or 'no axis'})")
    if case.dtype == "f32":
        _stem_per_element(amd, gpu, case)


# ------------------------------------------------------------------ tconv
def _tconv_gates_of_test_gpu_ops(amd, dev, c):
    """(a): the assertions of test_gpu_ops.py on this case's shape; returns the kernel that ran"""
    case = c.shape + (c.cin, c.cout)
    if c.dtype == "f16":
        ops_tests.test_tconv_f16_matches_torch(amd, dev, case)
    else:
        ops_tests.test_tconv_matches_torch(amd, dev, case)
    return amd.ops.last_conv_kernel()


def _tconv_per_element(amd, dev, c):
    """Gaussian operands as test_tconv_matches_torch draws them, judged element by element against the fp64 tconv"""
    rs = np.random.RandomState(5)
    x = ops_tests._rand(rs, *c.shape, c.cin)
    wt = (ops_tests._rand(rs, c.cin, c.cout, 2, 2, 2) / np.sqrt(c.cin)).astype(np.float32)
    y = amd.ops.tconv3d_ndhwc(torch.from_numpy(x).to(dev), wt).cpu().numpy()
    ran = amd.ops.last_conv_kernel()
    return _per_element(c.name, ran, y, ops_tests._ref_tconv64(x, wt), ops_tests._ref_tconv64(np.abs(x), np.abs(wt)), c.cin)


def tconv_integer_run(amd, dev, c):
    """(b) and (c); returns (kernel that ran, number of outputs, max |output|, what guarded the stores)"""
    x, wt = U.int_tconv_operands(c)
    want = U.int_tconv(x, wt, np.int16)  # (narrow: the Cout = 64 outputs of the persistent-kernel cases have 6.7e7 elements)
    f16 = c.dtype == "f16"
    dt = torch.float16 if f16 else torch.float32
    n, d, h, w = c.shape
    numel = want.size
    assert want.shape == (n, 2 * d, 2 * h, 2 * w, c.cout)
    guard = -(-max(4096, numel // n) // 256) * 256  # a sample's worth, a multiple of 256 elements: the output keeps its alignment
    buf = torch.full((guard + numel + guard,), SENTINEL, dtype=dt, device=dev)
    out = buf[guard:guard + numel]
    xg = torch.from_numpy(x).to(dev).to(dt).contiguous()
    wf = np.ascontiguousarray(wt, dtype=np.float32)
    lib = amd._lib.load()
    entry, what = (lib.mi355_tconv3d_ndhwc_f16, "mi355_tconv3d_ndhwc_f16") if f16 else (lib.mi355_tconv3d_ndhwc, "mi355_tconv3d_ndhwc")
    amd._lib.check(entry(xg.data_ptr(), n, d, h, w, c.cin, amd._lib.fptr(wf), c.cout, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), what)
    ran = amd.ops.last_conv_kernel()
    got = out.cpu().numpy().reshape(want.shape)
    differs = got != want  # (a NaN differs)
    if differs.any():
        first = np.unravel_index(int(np.argmax(differs)), want.shape)
        raise AssertionError(f"{c.name} [{ran}]: {int(differs.sum())} of {numel} outputs differ from the integer tconv, first at (n, z, y, x, cout) = "
                             f"{tuple(int(i) for i in first)}: {got[first]!r} instead of {want[first]}")
    assert np.array_equal(got, want)
    front, back = buf[:guard] != SENTINEL, buf[guard + numel:] != SENTINEL
    n_front, n_back = int(front.sum()), int(back.sum())
    assert n_front == 0 and n_back == 0, (f"{c.name} [{ran}]: stores outside the output: {n_front} elements in front, {n_back} behind "
                                          f"(first behind at +{int(torch.argmax(back.to(torch.uint8)))})")
    guarded = f"2 x {guard} sentinels untouched"
    if f16:
        guarded += " (layout converter), the entry point's guard bands around the kernel's own buffer intact"
    return ran, numel, int(np.abs(want).max()), guarded


def _describe(c):
    return (f"M = {U.tconv_voxels(c.shape)}, {U.tconv_tiles(U.tconv_voxels(c.shape))} tiles, {'tail ' + str(c.tail) if c.tail else 'whole tiles'}"
            f"{', straddles samples' if c.straddles else ''}, Cin {c.cin} -> Cout {c.cout}")


@pytest.mark.parametrize("case", U.TCONV_CASES, ids=[c.name for c in U.TCONV_CASES])
def test_tconv_case(amd, gpu, case):
    # (MI355_TCONV_V3 in the caller's environment sends the persistent-kernel cases elsewhere: the checks hold, the name does not)
    check_kernel = "MI355_TCONV_V3" not in os.environ
    t0 = time.time()
    ran_a = _tconv_gates_of_test_gpu_ops(amd, gpu, case)
    if check_kernel:
        assert ran_a == case.kernel, (case.name, ran_a)
    per_element = ""
    if case.dtype == "f32" and U.is_v2(case):
        per_element = f" | worst element at {_tconv_per_element(amd, gpu, case):.3f} of dot_bound"
    ran_b, numel, top, guarded = tconv_integer_run(amd, gpu, case)
    if check_kernel:
        assert ran_b == case.kernel, (case.name, ran_b)
    # the dry run names what ran (whatever the switch: both read it in this process)
    assert amd.ops.tconv_plan(case.dtype, case.shape, case.cin, case.cout)["kernel"] == ran_b == ran_a, (case.name, ran_a, ran_b)
    print(f"TCONV CASE {case.name} gates of test_gpu_ops on {ran_a}{per_element} | integers: {numel} outputs of {ran_b} equal the integer tconv "
          f"(max |y| {top}), {guarded} | {_describe(case)} | {time.time() - t0:.1f} s", flush=True)


# ------------------------------------------------------------------ MI355_TCONV_V3=0
def _switch_off_cases():
    """the smallest persistent-kernel case of each dtype (input plus output elements)"""
    v3 = [c for c in U.TCONV_CASES if not U.is_v2(c)]
    return [min((c for c in v3 if c.dtype == dt), key=lambda c: U.tconv_voxels(c.shape) * (c.cin + 8 * c.cout)) for dt in ("f32", "f16")]


_CHILD = r"""
import os, sys, time
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch
import brats_amd as amd
import tconv_stem_util as U
import test_gpu_tconv_stem as T
assert os.environ["MI355_TCONV_V3"] == "0"
assert torch.cuda.is_available() and amd._lib.load().mi355_device_count() > 0
for c in T._switch_off_cases():
    t0 = time.time()
    ran, numel, top, guarded = T.tconv_integer_run(amd, torch.device("cuda:0"), c)
    assert ran == {"f32": U.F32_V2, "f16": U.F16_V2}[c.dtype] != c.kernel, (c.name, ran)
    print(f"TCONV CASE {c.name} [MI355_TCONV_V3=0] integers: {numel} outputs of {ran} equal the integer tconv (max |y| {top}), {guarded} | "
          f"{time.time() - t0:.1f} s", flush=True)
print("ALL OK")
"""


def test_tconv_v3_switch_off(amd, gpu):
    cases = _switch_off_cases()
    assert [c.dtype for c in cases] == ["f32", "f16"] and not any(U.is_v2(c) for c in cases)
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=R.child_env({"MI355_TCONV_V3": "0"}), capture_output=True, text=True, timeout=120)
    lines = [line for line in res.stdout.splitlines() if line.startswith("TCONV CASE ")]
    print("".join(line + "\n" for line in lines), end="")
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    assert [line.split()[2] for line in lines] == [c.name for c in cases]
