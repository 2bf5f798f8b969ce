"""-m gpu: every entry of conv_rows_util.CASES on the GPU - the 3x3x3 conv kernel instantiations that the planner selects and
that no case of test_gpu_ops.py / test_gpu_conv_fused.py reaches (tests/test_conv_rows_cpu.py keeps that set closed).

Each entry runs twice, and the kernel that ran is asserted both times (mi355_last_conv_kernel):

a. through amd.ops.conv3d_ndhwc / conv3d_sums_ndhwc, judged by the gates of test_gpu_ops.py themselves - the test functions
   of that module are called with the entry's shape, not copied: test_conv3d_mfma_matches_torch (fp32: 2e-5 of the range),
   test_conv3d_f16_matches_torch (fp16: 2e-3 of the range and the RNE16 gate against the fp64 conv on the fp16-rounded operands),
   test_conv3d_norm_sums_match_reference (entries with statistics: the same output gates and the two 1e-4 gates).  These
   kernels are direct, non-Winograd siblings of instantiations those gates already judge.
b. on exact integers (conv_rows_util.int_operands: x in [-4, 4], weights in {-1, 0, 1}, integer bias, LeakyReLU at 0.5; no
   partial sum reaches 2048, so nothing is rounded in fp32 or fp16 whatever the summation order or split-K slicing), through
   mi355_conv3d_fused_ndhwc into the middle of a buffer of sentinels: the output must EQUAL the int64 reference
   (np.array_equal, no tolerance), and
c. nothing outside the N x Do x Ho x Wo x Cout outputs may be written: a store past the volume that the gates of (a) cannot
   see, because ops allocates exactly the output.  (A store past a ragged edge INSIDE the tensor lands on another voxel's
   output and shows in (b).)  Every entry, whole-tile ones included, but by two different means:
   - fp32: the kernel under test stores straight into the caller's tensor, so the sentinels in front of and behind it - a whole
     sample's worth on either side - are read back here and must be untouched.
   - fp16: the kernels store into a channel-blocked buffer that the single-op entry point owns; only its layout converter
     writes the caller's tensor.  The entry point therefore puts its own guard bands (a sample's worth, at most 4 MiB) around
     that buffer, reads them back after the launch and fails the call if a byte changed (single_op.hip guards_intact): for an fp16
     entry the check is that the call returns without that error.  The sentinels here then only watch the converter.
   - split-K, both dtypes: the conv kernel stores partial sums into library scratch, which nothing guards; what is checked
     as above is the finishing pass.
   With statistics, sum y of the integer run is exact too (a partial sum over a tile's <= 512 voxels of half-integers below
   2048 fits fp32, the quantised partials add exactly in fp64): it must equal the reference's, which counts no voxel past a
   ragged edge.  Sum y^2 does not fit fp32 exactly and is left to the 1e-4 gates of (a).

Entries of the default switches run in this process; the switches are read once per process, so the entries of each other
switch setting run in one child, which prints a line per entry and stops at the first failing one."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import conv_rows_util as U
import test_gpu_ops as ops_tests

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 4096.0  # exact in fp16 and fp32, and no output of the integer run reaches it (|y| < 2048)


def _gates_of_test_gpu_ops(amd, dev, c):
    """(a): the assertions of test_gpu_ops.py on this entry's shape; returns the kernel that ran"""
    case = c.shape + (c.cin, c.cout, c.stride, c.act)
    if c.stats:
        ops_tests.test_conv3d_norm_sums_match_reference(amd, dev, case + (c.dtype,))
    elif c.dtype == "f16":
        ops_tests.test_conv3d_f16_matches_torch(amd, dev, case)
    else:
        ops_tests.test_conv3d_mfma_matches_torch(amd, dev, case)
    return amd.ops.last_conv_kernel()


def _integer_run(amd, dev, c):
    """(b) and (c); returns (kernel that ran, number of outputs, max |output|, what guarded the kernel's stores)"""
    x, wt, b = U.int_operands(c)
    acc = U.int_conv(x, wt, b, c.stride)
    assert np.abs(acc).max() < U.INT_BOUND  # (int_operands asserts the bound on every partial sum)
    want2 = U.int_expected_doubled(acc)
    dt = torch.float16 if c.dtype == "f16" else torch.float32
    n, d, h, w = c.shape
    numel = acc.size
    guard = -(-max(4096, numel // n) // 256) * 256  # a sample's worth, a multiple of 256 elements: the output keeps its alignment
    buf = torch.full((guard + numel + guard,), SENTINEL, dtype=dt, device=dev)
    out = buf[guard:guard + numel]
    sums = torch.full((n, c.cout, 2), float("nan"), dtype=torch.float64, device=dev) if c.stats else None
    xg = torch.from_numpy(x).to(dt).to(dev).contiguous()
    wf, bf = np.ascontiguousarray(wt, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    lib = amd._lib.load()
    amd._lib.check(lib.mi355_conv3d_fused_ndhwc(
        xg.data_ptr(), None, 1 if c.dtype == "f16" else 0, n, d, h, w, c.cin, 0, amd._lib.fptr(wf), amd._lib.fptr(bf), c.cout, c.stride,
        1, U.INT_SLOPE, 0, None, None, 0, None, None, 0, None, out.data_ptr(), None if sums is None else sums.data_ptr(),
        torch.cuda.current_stream(dev).cuda_stream), "mi355_conv3d_fused_ndhwc")
    ran = amd.ops.last_conv_kernel()
    got = buf.cpu().numpy().astype(np.float64)
    y2 = 2.0 * got[guard:guard + numel].reshape(acc.shape)
    bad = np.argwhere(y2 != want2)
    assert bad.size == 0, (f"{c.name} [{ran}]: {len(bad)} of {numel} outputs differ from the integer conv, first at (n, z, y, x, cout) = "
                           f"{tuple(bad[0])}: {y2[tuple(bad[0])] / 2} instead of {want2[tuple(bad[0])] / 2}")
    assert np.array_equal(y2, want2)
    front, back = got[:guard], got[guard + numel:]
    assert np.array_equal(front, np.full(guard, SENTINEL)) and np.array_equal(back, np.full(guard, SENTINEL)), (
        f"{c.name} [{ran}]: stores outside the output: {int((front != SENTINEL).sum())} elements in front, {int((back != SENTINEL).sum())} behind "
        f"(first behind at +{int(np.argmax(back != SENTINEL))})")
    guarded = (f"2 x {guard} sentinels untouched" if c.dtype == "f32" else
               "the entry point's guard bands around the kernel's own buffer intact")
    if ran.endswith(" split-K"):
        guarded += " (finishing pass; the partial sums go to unguarded scratch)"
    if sums is not None:
        got_sums = sums.cpu().numpy()
        assert np.isfinite(got_sums).all(), (c.name, ran)
        assert 512 * int(np.abs(want2).max()) < 2 ** 24  # a tile's partial sum of 2 y is an integer that fp32 holds
        want_sum2 = want2.sum(axis=(1, 2, 3))
        assert np.array_equal(2.0 * got_sums[..., 0], want_sum2), (
            f"{c.name} [{ran}]: sum y differs from the integer conv's, worst by {np.abs(2.0 * got_sums[..., 0] - want_sum2).max() / 2}")
        guarded += ", sum y exact"
    return ran, numel, float(np.abs(y2).max() / 2), guarded


def run_case(amd, dev, c, check_kernel, tag="CONV ROW"):
    """one entry: (a), then (b) and (c); prints the entry's line (`tag`: what the line starts with; test_gpu_tconv_stem.py runs
    the stem cases through here)"""
    t0 = time.time()
    ran_a = _gates_of_test_gpu_ops(amd, dev, c)
    if check_kernel:
        assert ran_a == c.kernel, (c.name, ran_a)
    ran_b, numel, top, guarded = _integer_run(amd, dev, c)
    if check_kernel:
        assert ran_b == c.kernel, (c.name, ran_b)
    print(f"{tag} {c.name} [{U.env_key(c.env)}] gates of test_gpu_ops on {ran_a} | integers: {numel} outputs of {ran_b} equal the int64 conv "
          f"(max |y| {top:g}), {guarded} | {'ragged' if c.ragged else 'whole tiles'}"
          f"{', statistics' if c.stats else ''} | {time.time() - t0:.1f} s", flush=True)


DEFAULT_CASES = [c for c in U.CASES if not c.env]


@pytest.mark.parametrize("case", DEFAULT_CASES, ids=[c.name for c in DEFAULT_CASES])
def test_conv_row_default_switches(amd, gpu, case):
    # (a dispatch switch in the caller's environment sends the call elsewhere: the parity checks still hold, the name does not)
    run_case(amd, gpu, case, check_kernel=not any(k in os.environ for k in U.SWITCHES))


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch
import brats_amd as amd
import conv_rows_util as U
import test_gpu_conv_rows as T
assert torch.cuda.is_available() and amd._lib.load().mi355_device_count() > 0
if torch.get_num_threads() > 16:
    torch.set_num_threads(16)  # (the CPU references, as tests/conftest.py caps them)
for c in U.CASES:
    if U.env_key(c.env) == sys.argv[2]:
        T.run_case(amd, torch.device("cuda:0"), c, True)
print("ALL OK")
"""

SWITCH_ENVS = {U.env_key(c.env): c.env for c in U.CASES if c.env}


@pytest.mark.parametrize("key", sorted(SWITCH_ENVS))
def test_conv_rows_under_switches(amd, gpu, key):
    cases = [c for c in U.CASES if U.env_key(c.env) == key]
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT, key], env=U.child_env(SWITCH_ENVS[key]), capture_output=True, text=True,
                         timeout=60 + 10 * len(cases))
    lines = [line for line in res.stdout.splitlines() if line.startswith("CONV ROW ")]
    print("".join(line + "\n" for line in lines), end="")
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    assert [line.split()[2] for line in lines] == [c.name for c in cases]
