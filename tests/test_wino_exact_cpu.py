"""The exact-integer checks of the fp32 Winograd conv kernels, as far as they go without a device (wino_exact_util.py has the
argument and the operand classes; tests/test_gpu_wino_exact.py runs the table on the GPU).

* The integer emulation of both transform domains equals conv_rows_util.int_conv for every operand class, on a 4 x 8 x 8 volume
  with 16 and 48 input channels (320 for `dense`), and so does the same pipeline in fp32 arithmetic with the input channels
  accumulated in a shuffled order and the output transform applied axis by axis: the exactness the GPU module relies on.
* The all-absolute-values bound (< 2^24, asserted inside the emulation) and the conditions of the bits classes (more than 16
  significant bits in V, U or the product) hold for every run of the table.
* Every planner-routed case plans to its kernel and grid (mi355_conv3d_plan, under the default switches, in a child process);
  the grid of a forced-entry case is recomputed from the rule of conv_plan.h; and from the grid, what each case says it reaches:
  a workgroup with a second tile, a tile range that crosses a sample, a tile count that is no multiple of 8, fewer than 8 tiles.
* The classes see what they are for: a dropped tap, a channel pair swapped within a quad, V cut to 16 significant bits and a
  norm shift given to an out-of-volume piece, applied to the fp32 emulation, each make the comparison of the class written for
  it fail."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_rows_util as U
import wino_exact_util as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOL = (1, 4, 8, 8)


def _small(cls, form, cin):
    cout = 32 if cin == 320 else 64
    return W.operands(cls, form, VOL, cin, cout, "small", head=3 if cls == "head" else 0, addend=cls == "dense" and cin == 16)


SMALL = [(form, cls, cin) for form in (3, 2) for cls in W.CLASSES for cin in ((16, 48, 320) if cls == "dense" else (16, 48))]


@pytest.mark.parametrize("form,cls,cin", SMALL, ids=[f"F{f}-{c}-{n}" for f, c, n in SMALL])
def test_emulation_equals_the_integer_conv(form, cls, cin):
    ops = _small(cls, form, cin)
    exp = W.expected(ops, product_bits=cls in W.BITS_CLASSES)  # (asserts: emulation == int_conv, bound < 2^24)
    assert 0 < exp.emu.bound < W.LIMIT and np.abs(exp.pre).max() > 0
    if cls in W.BITS_CLASSES:
        W.assert_bits(cls, exp.emu)
    if cls == "norm":
        assert exp.unit == 2 and (ops.shift != 0).all() and (exp.pre % 2 != 0).any()  # half-integers do occur
    for seed in (1, 2):
        f32 = W.emulate_f32(ops, np.random.RandomState(seed))
        assert np.array_equal(f32 * exp.unit, exp.pre), (form, cls, cin, seed)
    print(f"WINO EXACT F{form} {cls} cin {cin}: bound {exp.emu.bound} = {100.0 * exp.emu.bound / W.LIMIT:.2f} % of 2^24, widest V / U / product "
          f"{exp.emu.v_bits} / {exp.emu.u_bits} / {exp.emu.product_bits} significant bits, fp32 emulation equal")


def test_the_table_covers_what_it_is_for():
    assert {c.kernel for c in W.GPU_CASES} == set(W.INSTANTIATIONS)
    for c in W.GPU_CASES:
        assert c.entry in ("wino3", "fused") and c.form == (3 if "wino3" in c.kernel else 2) and set(c.classes) <= set(W.CLASSES), c
        assert c.c0 % 16 == 0 and c.c1 % 16 == 0 and c.cout % 32 == 0, c
        fits = {"dense", "taps"} if c.cout >= max(27, c.c0 + c.c1) else {"dense"}
        # `norm` and `head` run on their own rows; every other row runs dense and taps wherever they fit
        assert set(c.classes) == ({"norm"} if c.norm else {"head"} if c.head else fits | (set(c.classes) & set(W.BITS_CLASSES))), c
        if c.entry == "wino3":  # the forced entry takes an addend and nothing else; the planner never routes an addend
            assert c.kernel == W.W3 % ("3, false" if c.addend else "0, false") and not (c.stats or c.norm or c.head), c
        else:
            assert not c.addend, c
    for form in (3, 2):  # the bits classes: one shape per form
        assert len([c for c in W.GPU_CASES if c.form == form and set(W.BITS_CLASSES) <= set(c.classes)]) == 1
    assert any(c.c0 + c.c1 == 48 and c.c1 and "taps" in c.classes for c in W.GPU_CASES)      # three chunks, the last from x1
    assert any(c.form == 2 and c.c1 for c in W.GPU_CASES)


@pytest.mark.parametrize("case,cls", W.RUNS, ids=[f"{c.name}-{cls}" for c, cls in W.RUNS])
def test_bound_and_bits_of_every_run(case, cls):
    ops, exp = W.checked_case(case, cls)  # (asserts the bound, the bits condition and emulation == reference)
    assert exp.emu.bound < W.LIMIT
    if case.stats:  # a tile's partial sum of y, in halves of the unit, is an integer that fp32 holds (test_gpu_conv_rows.py)
        assert 512 * int(np.abs(exp.y_scaled).max()) < W.LIMIT
    if cls == "taps":
        nz = ops.wt.reshape(case.cout, -1, 27) != 0
        assert (nz.sum(axis=(1, 2)) == 1).all() and nz.any(axis=(0, 2)).all() and nz.any(axis=(0, 1)).all()
    print(f"WINO EXACT {case.name} {cls}: bound {100.0 * exp.emu.bound / W.LIMIT:.2f} % of 2^24, widest V / U / product "
          f"{exp.emu.v_bits} / {exp.emu.u_bits} / {exp.emu.product_bits or '-'} significant bits, max |y| {np.abs(exp.y_scaled).max() / (2 * exp.unit):g}")


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import brats_amd as amd
import wino_exact_util as W
out = {c.name: amd.ops.conv3d_plan("f32", c.shape, c.c0, c.cout, c1=c.c1, stats=c.stats, in_norm=c.norm, head_ncls=c.head)
       for c in W.GPU_CASES if c.entry == "fused"}
print("RESULT " + json.dumps({"plans": out, "rows": amd.ops.conv_kernel_names()}))
"""


@pytest.fixture(scope="module")
def planned(amd):
    """what the planner says about the planner-routed cases, under the default switches (they are read once per process)"""
    res = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=U.child_env({}), capture_output=True, text=True, timeout=300)
    lines = [line for line in res.stdout.splitlines() if line.startswith("RESULT ")]
    assert res.returncode == 0 and lines, (res.stdout[-1000:], res.stderr[-2000:])
    return json.loads(lines[-1][7:])


def _reached(c, gx):
    """what a launch of `gx` workgroups per cout block contains, from the kernels' tile-range rule"""
    tiles = W.case_tiles(c)
    per_n = tiles // c.shape[0]
    walks = W.workgroup_tiles(gx, tiles)
    assert sorted(t for wg in walks for t in wg) == list(range(tiles))  # every tile once
    got = set()
    if tiles < 8 and any(not wg for wg in walks):
        got.add("few")
    if tiles % 8:
        got.add("r8")
    if any(len(wg) > 1 for wg in walks):
        got.add("second")
    if any(a // per_n != b // per_n for wg in walks for a, b in zip(wg, wg[1:])):
        got.add("sample")
    if any(v % t for v, t in zip(c.shape[1:], W.TILE[c.form])):
        got.add("ragged")
    return got


def test_every_case_has_the_kernel_and_grid_it_counts_on(planned):
    rows = {name for _, name in planned["rows"]}
    assert set(W.INSTANTIATIONS) <= rows
    for c in W.GPU_CASES:
        tiles, gy = W.case_tiles(c), c.cout // 32
        if c.entry == "fused":
            p = planned["plans"][c.name]
            assert (p["rc"], p["kernel"], tuple(p["grid"]), tuple(p["tile"]), p["splitk"]) == (0, c.kernel, c.grid + (1,), W.TILE[c.form], 1), (c.name, p)
            assert p["fuses_in_norm"] or not c.norm, c.name
        else:  # the forced entry: plan_wino3(force) = whole tiles, one persistent workgroup per CU shared by the cout blocks
            assert not any(v % t for v, t in zip(c.shape[1:], W.TILE[3])), c.name
        assert c.grid == (W.persistent_grid_x(256, gy, tiles), gy), (c.name, tiles)
        assert _reached(c, c.grid[0]) == set(c.reaches), (c.name, _reached(c, c.grid[0]))
    for what in ("few", "r8", "second", "sample"):
        assert any(what in c.reaches for c in W.GPU_CASES if c.form == 3), what
    for what in ("second", "sample", "ragged"):
        assert any(what in c.reaches for c in W.GPU_CASES if c.form == 2), what
    assert all("ragged" in c.reaches for c in W.GPU_CASES if c.form == 2)


#: defect -> the class written for it (its comparison MUST fail) - and `dense` need not see any of them
DEFECTS = {"drop_tap": "taps", "swap_pair": "taps", "trunc_v16": "wide_x", "shift_outside": "norm"}


@pytest.mark.parametrize("form", (3, 2))
def test_the_classes_see_the_defects_they_are_for(form):
    rs = np.random.RandomState(7)
    failing = {d: [] for d in DEFECTS}
    for cls in W.CLASSES:
        ops = _small(cls, form, 16)
        exp = W.expected(ops)
        assert np.array_equal(W.emulate_f32(ops, rs) * exp.unit, exp.pre)  # (no defect: equal)
        for defect in DEFECTS:
            if defect == "shift_outside" and cls != "norm":
                continue
            got = W.emulate_f32(ops, rs, defect=defect) * exp.unit
            if not np.array_equal(got, exp.pre):
                # ... and by at least 1/2 of an output after the activation: nothing that a rounding could hide
                y = np.where(got >= 0, 2 * got, got)
                assert np.abs(y - exp.y_scaled).max() >= exp.unit, (cls, defect)
                failing[defect].append(cls)
    for defect, cls in DEFECTS.items():
        assert cls in failing[defect], (form, defect, failing[defect])
    # 16 significant bits of V are enough for every class but the one that asks for more
    assert set(failing["trunc_v16"]) <= set(W.BITS_CLASSES), failing["trunc_v16"]
    print(f"WINO EXACT F{form}: defects seen by {failing}")


def test_a_tap_failure_names_its_tap_and_place():
    ops = _small("taps", 3, 16)
    exp = W.expected(ops)
    got = exp.y_scaled.copy()
    got[0, 3, 5, 6, 29] += 1
    msg = W.describe_tap_failure(ops, exp.y_scaled, got)
    assert "cout 29 reads tap (dz, dy, dx) = (0, 0, 2) of input channel 13 (chunk 0, quad 3, pair 0)" in msg, msg
    assert "tile (z, y, x) = (0, 0, 0) of sample 0, 2x2x2 block (1, 2, 3) of it, output (1, 1, 0) of the block" in msg, msg
    assert W.describe_tap_failure(ops, exp.y_scaled, exp.y_scaled) == ""
