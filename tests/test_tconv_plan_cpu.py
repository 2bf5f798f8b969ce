"""Which kernel a transposed conv is sent to, checked on the CPU through the dry-run entry point mi355_tconv3d_plan (plan_tconv of
tconv.hip: the planner a real call and the network run, without a device).

* ops.tconv_plan equals tconv_stem_util.expected_tconv_kernel over a sweep of both dtypes, the channel counts on both sides of every
  rule and voxel counts on both sides of the 1024-tile threshold, and for every case of TCONV_CASES.
* The grid: one workgroup per 128-voxel tile (version 2); 512 / (Cout / 32) workgroups per cout block, at least 8, at most the
  tiles (version 3).  The LDS figure is the kernels' static LDS as their listings give it.
* Refusals carry the launcher's messages.
* With MI355_TCONV_V3=0 (read once per process: a child) only version-2 kernels are named.
* The rows of tconv_rows, read from the source, are exactly TCONV_KERNELS, and every planned name is one of them."""
import json
import os
import re
import subprocess
import sys

import conv_rows_util as R
import tconv_stem_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CINS = (8, 16, 32, 64, 72, 128, 320)
COUTS = (32, 64, 96, 2048)
# 1023 tiles, 1024 tiles (one voxel in the last), 1024 tiles (one voxel short of whole)
VOXELS = (1023 * 128, 1023 * 128 + 1, 1024 * 128 - 127)
# the kernels' static LDS: the input image (16-B pieces x 129 slots of 16 B) and four 4-KB transpose buffers
LDS = {U.F32_V2: 49408, U.F32_V3: 49408, U.F16_V2: 32896, U.F16_V3[32]: 24640, U.F16_V3[64]: 32896, U.F16_V3[128]: 49408}


def _defaults():
    return "MI355_TCONV_V3" not in os.environ


def _shapes(m):
    """shapes (N, D, H, W) of m voxels: flat, and split over two or three axes where m allows"""
    out = [(1, 1, 1, m)]
    for n, d in ((1, 3), (3, 11), (2, 1), (1, 31)):
        if m % (n * d) == 0:
            out.append((n, d, 1, m // (n * d)))
    return out


def _sweep():
    for dtype in ("f32", "f16"):
        for cin in CINS:
            if cin % U.TCONV_MIN_CIN[dtype]:
                continue
            for cout in COUTS:
                for m in VOXELS:
                    for shape in _shapes(m):
                        yield dtype, shape, cin, cout


def _expected_grid(kernel, m, cout):
    tiles, nblk = U.tconv_tiles(m), cout // 32
    if kernel in U.V2_KERNELS:
        return (tiles, nblk, 1)
    return (min(max(512 // nblk, 8), tiles), nblk, 1)


def test_sweep_covers_both_sides_of_every_rule():
    calls = list(_sweep())
    assert [U.tconv_tiles(m) for m in VOXELS] == [1023, 1024, 1024] and VOXELS[2] % 128 == 1 and VOXELS[1] % 128 == 1
    assert {c[2] for c in calls if c[0] == "f32"} == set(CINS) and {c[2] for c in calls if c[0] == "f16"} == {16, 32, 64, 128, 320}
    assert all(U.tconv_voxels(s) in VOXELS for _, s, _, _ in calls) and len({s for _, s, _, _ in calls}) >= 6
    want = {U.expected_tconv_kernel(dt, cin, U.tconv_voxels(s)) for dt, s, cin, _ in calls}
    assert want == set(U.TCONV_KERNELS)
    # the grid rule's three regimes: 512 / nblk (Cout 32, 64), rounded down (96: 170), the floor of 8 (2048: 512 / 64 = 8)
    assert [512 // (c // 32) for c in COUTS] == [512, 256, 170, 8]


def test_plan_is_the_written_out_rule(amd):
    n = 0
    for dtype, shape, cin, cout in _sweep():
        m = U.tconv_voxels(shape)
        p = amd.ops.tconv_plan(dtype, shape, cin, cout)
        assert p["rc"] == 0 and p["kernel"] in U.TCONV_KERNELS, (dtype, shape, cin, cout, p)
        if not _defaults():  # (the switch is set by the caller: the names are those of the other setting)
            continue
        want = U.expected_tconv_kernel(dtype, cin, m)
        assert p["kernel"] == want, (dtype, shape, cin, cout, p)
        assert p["grid"] == _expected_grid(want, m, cout), (dtype, shape, cin, cout, p)
        assert p["lds_bytes"] == LDS[want], (dtype, shape, cin, cout, p)
        n += 1
    assert n == (len(list(_sweep())) if _defaults() else 0) and len(list(_sweep())) >= 300


def test_grid_floor_and_cap(amd):
    """the persistent grid at its two ends: the floor of 8 workgroups per cout block, and no more workgroups than tiles"""
    if not _defaults():
        return
    shape = (1, 1, 1, 1024 * 128)
    assert amd.ops.tconv_plan("f32", shape, 64, 2048)["grid"] == (8, 64, 1)
    assert amd.ops.tconv_plan("f32", shape, 64, 4096)["grid"] == (8, 128, 1)      # 512 / 128 = 4 < 8
    assert amd.ops.tconv_plan("f16", shape, 128, 32)["grid"] == (512, 1, 1)
    assert amd.ops.tconv_plan("f16", shape, 128, 96)["grid"] == (170, 3, 1)
    # (the cap at the tile count cannot bind while version 3 starts at 1024 tiles: 512 / nblk <= 512.  Version 2 is the capped
    # form, one workgroup per tile)
    assert amd.ops.tconv_plan("f32", (1, 1, 1, 1023 * 128), 64, 32)["grid"] == (1023, 1, 1)
    big = (2, 64, 128, 128)
    assert amd.ops.tconv_plan("f32", big, 64, 32)["grid"] == (512, 1, 1) and amd.ops.tconv_plan("f32", big, 72, 32)["grid"] == (16384, 1, 1)


def test_plan_names_the_kernel_of_every_gpu_case(amd):
    for c in U.TCONV_CASES:
        p = amd.ops.tconv_plan(c.dtype, c.shape, c.cin, c.cout)
        assert p["rc"] == 0, (c.name, p)
        if _defaults():
            assert p["kernel"] == c.kernel, (c.name, p)
            assert p["grid"] == _expected_grid(c.kernel, U.tconv_voxels(c.shape), c.cout) and p["lds_bytes"] == LDS[c.kernel], (c.name, p)


def test_refusals_carry_the_launchers_messages(amd):
    plan = amd.ops.tconv_plan
    for shape in ((1, 1024, 1024, 1024), (4, 1024, 1024, 256), (2, 1024, 1024, 1024)):
        p = plan("f32", shape, 64, 32)
        assert p["rc"] < 0 and p["error"].endswith(f"tconv: {U.tconv_voxels(shape)} voxels out of range"), p
        assert p["kernel"] == "" and p["grid"] == (0, 0, 0)
    assert plan("f16", (1, 1024, 1024, 1023), 64, 32)["rc"] == 0  # 2^30 - 2^20 voxels
    for dtype, cin, cout, msg in (("f32", 12, 32, "tconv 12->32: need cin % 8 == 0 and cout % 32 == 0"),
                                  ("f32", 64, 48, "tconv 64->48: need cin % 8 == 0 and cout % 32 == 0"),
                                  ("f16", 8, 32, "fp16 tconv 8->32: need cin % 16 == 0 and cout % 32 == 0"),
                                  ("f16", 72, 32, "fp16 tconv 72->32: need cin % 16 == 0 and cout % 32 == 0"),
                                  ("f16", 64, 16, "fp16 tconv 64->16: need cin % 16 == 0 and cout % 32 == 0")):
        p = plan(dtype, (1, 4, 4, 8), cin, cout)
        assert p["rc"] < 0 and p["error"].endswith(msg), (dtype, cin, cout, p)
    assert not plan("f32", (1, 4, 4, 8), 12, 32)["error"].endswith("fp16 tconv 12->32: need cin % 8 == 0 and cout % 32 == 0")
    assert plan("f32", (1, 0, 4, 8), 64, 32)["rc"] < 0 and plan("f32", (1, 4, 4, 8), 0, 32)["rc"] < 0 and plan("f32", (1, 4, 4, 8), 64, 0)["rc"] < 0


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import brats_amd as amd
import test_tconv_plan_cpu as T
print("RESULT " + json.dumps([[list(c[1]), c[0], c[2], c[3], amd.ops.tconv_plan(*c)] for c in T._sweep()]))
"""


def test_switch_off_names_only_version_2(amd):
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(R.child_env({}), MI355_TCONV_V3="0"), capture_output=True, text=True,
                         timeout=120)
    lines = [line for line in res.stdout.splitlines() if line.startswith("RESULT ")]
    assert res.returncode == 0 and lines, res.stdout[-1000:] + res.stderr[-2000:]
    rows = json.loads(lines[-1][7:])
    assert len(rows) == len(list(_sweep()))
    for shape, dtype, cin, cout, p in rows:
        want = {"f32": U.F32_V2, "f16": U.F16_V2}[dtype]
        assert (p["rc"], p["kernel"]) == (0, want), (shape, dtype, cin, cout, p)
        assert tuple(p["grid"]) == _expected_grid(want, U.tconv_voxels(shape), cout) and p["lds_bytes"] == LDS[want]
    # (the sweep does reach version 3 where the switch is on)
    assert any(U.expected_tconv_kernel(dtype, cin, U.tconv_voxels(shape)) not in U.V2_KERNELS for shape, dtype, cin, _, _ in rows)


def test_rows_of_the_table_are_the_declared_kernels(amd):
    """tconv_rows as tconv.hip lists it (the table is in no listing entry point: mi355_conv_kernel_names is the 3x3x3 tables')"""
    src = os.path.join(os.path.dirname(os.path.abspath(amd.ops.__file__)), "csrc", "tconv.hip")
    with open(src) as fh:
        text = fh.read()
    table = re.search(r"static KernelRow tconv_rows\[\] = \{(.*?)\n\};", text, re.S)
    assert table, "tconv_rows not found in tconv.hip"
    rows = re.findall(r"MI355_KERNEL_ROW\(([^()]+)\)", table.group(1))
    assert tuple(rows) == U.TCONV_KERNELS and len(set(rows)) == 6
    assert "hipLaunchKernelGGL" not in text  # every launch of the file goes through a row
    planned = {amd.ops.tconv_plan(*c)["kernel"] for c in _sweep()}
    assert planned <= set(rows) and (not _defaults() or planned == set(rows))
