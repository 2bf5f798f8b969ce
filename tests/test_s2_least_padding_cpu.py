"""The least-padding hint of the stride-2 LDS-DMA planner (ConvCall::s2_least_padding, MI355_S2_LEAST_PADDING), on the CPU through
the dry runs mi355_conv3d_plan_hinted / mi355_conv3d_plan: no device.

conv3_f32_s2dma_kernel runs on 2 x 2 x 32 output tiles (<5>) or 2 x 4 x 16 ones (<4>); without the hint the planner asks Wo >= 24.
With it - only enc[1][0] of the shared level 1 carries it - the shape whose padded columns times padded rows are fewer wins, ties to
<5>.  The region launch of the bench geometry (Wo = 72: 96 columns of 32, 80 of 16) is the case it was made for.

* with the hint: <4> at 2 x 128 x 176 x 144 and at Wo = 16, <5> at Wo = 64 and 96 (ties) and where the 4-row tile pads more rows
  than the 16-wide tile saves columns; the plan is a whole one (tile, grid, LDS bytes of that instantiation);
* without it, every stride-2 row of tests/golden/conv_plan_rows.txt plans as written there, through both entries, and the hint
  moves no row that is not a launch of this kernel."""
import ctypes as C
import os

import test_conv_plan as plan_rows

S2 = "conv3_f32_s2dma_kernel<%d>"
LDS = {5: 143072, 4: 134272}   # S2Geom<5>::LDS_BYTES, S2Geom<4>::LDS_BYTES (as the golden rows of both record them)


def _plan(amd, shape, hint, cin=32, cout=64):
    return amd.ops.conv3d_plan("f32", shape, cin, cout, stride=2, s2_least_padding=hint)


def _padded(wo, ho, txl):
    tx, ty = 1 << txl, 64 >> txl
    return -(-wo // tx) * tx * (-(-ho // ty) * ty)


def test_the_hint_picks_the_tile_that_pads_less(amd):
    if "MI355_S2_DMA" in os.environ:
        return
    # (shape, kernel with the hint, kernel without)
    cases = [((2, 128, 176, 144), 4, 5),    # the region launch of the bench geometry: Wo = 72
             ((8, 64, 64, 32), 4, 4),       # Wo = 16
             ((8, 64, 64, 128), 5, 5),      # Wo = 64: a tie
             ((8, 64, 64, 192), 5, 5),      # Wo = 96: a tie
             ((8, 64, 64, 80), 4, 5),       # Wo = 40: three 16-wide tiles against two 32-wide
             ((8, 64, 12, 80), 5, 5),       # Wo = 40, Ho = 6: 48 x 8 rows of four against 64 x 6 rows of two - a tie, to <5>
             ((8, 64, 20, 272), 5, 5)]      # Wo = 136, Ho = 10: 144 x 12 > 160 x 10
    for shape, with_hint, without in cases:
        ho, wo = (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1
        assert (4 if _padded(wo, ho, 4) < _padded(wo, ho, 5) else 5) == with_hint, shape   # (the rule, stated once more)
        for hint, txl in ((True, with_hint), (False, without)):
            p = _plan(amd, shape, hint)
            assert p["rc"] == 0 and p["kernel"] == S2 % txl, (shape, hint, p)
            assert p["tile"] == (2, 64 >> txl, 1 << txl) and p["lds_bytes"] == LDS[txl] and p["grid"][0] % 8 == 0 and p["grid"][1:] == (1, 1), p


def test_without_the_hint_every_recorded_stride2_row_stands(amd):
    lib = amd._lib.load()
    p = amd._lib.ConvPlan()
    rows = [r for r in plan_rows.ROWS if r[2]["stride"] == 2]
    assert len(rows) >= 40 and any(r[3][1] == S2 % 5 for r in rows) and any(r[3][1] == S2 % 4 for r in rows)
    if not plan_rows._defaults() or "MI355_S2_DMA" in os.environ:
        return
    moved = 0
    for label, key, call, want in rows:
        args = (int(call["dtype"] == "f16"), *call["shape"], call["c0"], call["c1"], call["cout"], 2, int(call["impl"] == "direct"), int(call["stats"]),
                int(call["in_norm"]), call["head_ncls"])
        got = {}
        for name, call_it in (("plain", lambda: lib.mi355_conv3d_plan(*args, C.byref(p))), ("hint 0", lambda: lib.mi355_conv3d_plan_hinted(*args, 0, C.byref(p))),
                              ("hint 1", lambda: lib.mi355_conv3d_plan_hinted(*args, 1, C.byref(p)))):
            rc = call_it()   # (p is shared: read it before the next call)
            got[name] =[str(rc)] if rc < 0 else [str(rc), p.kernel.decode(), ",".join(str(v) for v in p.grid), str(p.lds_bytes), str(p.splitk)]
            if name != "hint 1":
                assert got[name] == (want[:1] if rc < 0 else want), (label, key, name, got[name])
        if got["hint 1"] != got["plain"]:   # the hint reaches plan_s2dma alone: it can only swap the two instantiations
            assert {got["plain"][1], got["hint 1"][1]} == {S2 % 4, S2 % 5}, (label, key, got)
            moved += 1
    print(f"stride-2 rows: {len(rows)}, moved by the hint: {moved}")
