"""Which kernel a 3x3x3 conv call is sent to, checked on the CPU through the dry-run entry point mi355_conv3d_plan (the pack
layout and the planners plan_conv_f32 / plan_conv_f16 of a real call, without a device).

* tests/golden/conv_plan_rows.txt holds the decisions of the dispatch functions as they were before selection and launching
  were separated (commit 467bf0f), recorded from that commit: every conv of the networks bench.py runs (models A and B, both
  dtypes, at the sample counts sw_accumulate uses for 8-tile cases) and every case of tests/test_gpu_ops.py and
  tests/test_gpu_conv_fused.py, its REFUSALS included.  The planner must reproduce each row: kernel name, grid, dynamic LDS
  bytes, split-K slices, or the refusal with its message.
* Conditions the selection must meet on every call of a sweep over dtypes, strides, channel counts, batch sizes, volumes, concat
  splits and fused operands (test_plan_properties).  They are conditions read off the kernels' requirements, not measurements.
"""
import importlib.util
import itertools
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("MI355_CONV_IMPL", "MI355_WINOGRAD", "MI355_WINO3", "MI355_S2_DMA", "MI355_SPLITK", "MI355_FUSE_NORM", "MI355_F16_DMA",
            "MI355_F16_C32", "MI355_F16_S2")
LDS_MAX = 160 * 1024


def _rows():
    out = []
    with open(os.path.join(HERE, "golden", "conv_plan_rows.txt")) as fh:
        for line in fh:
            if line.startswith("#") or not line.strip():
                continue
            f = [s.strip() for s in line.rstrip("\n").split(" | ")]
            m = re.fullmatch(r"(f32|f16) (\d+) (\d+)x(\d+)x(\d+) (\d+)\+(\d+) (\d+) s(\d) i(\d) st(\d) nm(\d) hd(\d)", f[1])
            assert m, line
            g = m.groups()
            call = dict(dtype=g[0], shape=tuple(int(v) for v in g[1:5]), c0=int(g[5]), c1=int(g[6]), cout=int(g[7]), stride=int(g[8]),
                        impl="direct" if g[9] == "1" else "mfma", stats=g[10] == "1", in_norm=g[11] == "1", head_ncls=int(g[12]))
            out.append((f[0], f[1], call, f[2:]))
    return out


ROWS = _rows()


def _defaults():
    """the recorded rows are those of the default switches"""
    return not any(k in os.environ for k in SWITCHES)


@pytest.mark.parametrize("row", ROWS, ids=[f"{r[0]} [{r[1]}]".replace(" ", "_") for r in ROWS])
def test_plan_reproduces_the_recorded_dispatch(amd, row):
    label, key, call, want = row
    p = amd.ops.conv3d_plan(**call)
    if not _defaults():  # (an A/B switch is set, as in the GPU tests' kernel expectations: the rows are those of the defaults)
        return
    if int(want[0]) < 0:
        assert (p["rc"], p["error"]) == (int(want[0]), want[1]), (label, key, p)
        return
    got = [str(p["rc"]), p["kernel"], ",".join(str(v) for v in p["grid"]), str(p["lds_bytes"]), str(p["splitk"])]
    assert got == want, (label, key, p)


def _load(name):
    spec = importlib.util.spec_from_file_location("_plan_" + name, os.path.join(HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_rows_cover_the_gpu_cases_and_agree_with_their_expected_kernels():
    """every single-op case of the two GPU test modules has a row; where the GPU test names the kernel it expects, the row names
    the same one; every REFUSALS entry is a recorded refusal with a message"""
    by_key = {r[1]: r[3] for r in ROWS}

    def key(dtype, shape, c0, c1, cout, stride=1, impl="mfma", stats=False, norm=False, head=0):
        n, d, h, w = shape
        return f"{dtype} {n} {d}x{h}x{w} {c0}+{c1} {cout} s{stride} i{int(impl == 'direct')} st{int(bool(stats))} nm{int(bool(norm))} hd{head}"

    ops, fused = _load("test_gpu_ops"), _load("test_gpu_conv_fused")
    checked = 0
    for cases, dtype, stats, expect in ((ops.CONV_CASES, "f32", False, ops.F32_EXPECT_KERNEL), (ops.F16_CONV_CASES, "f16", False, ops.F16_EXPECT_KERNEL),
                                        (ops.SUMS_CASES, None, True, ops.SUMS_EXPECT_KERNEL)):
        for case in cases:
            n, d, h, w, cin, cout, stride = case[:7]
            got = by_key[key(dtype or case[8], (n, d, h, w), cin, 0, cout, stride, stats=stats)]
            assert got[0] == "0", (case, got)
            if case in expect:
                assert got[1] == expect[case], (case, got)
                checked += 1
    for c in fused.CASES:
        got = by_key[key(c.dtype, c.shape, c.c0, c.c1, c.cout, 1, c.impl, c.stats, c.norm is not None, c.head)]
        if c.kernel:
            assert got[:2] == ["0", c.kernel], (c.name, got)
            checked += 1
    for (name, dtype, shape, c0, c1, cout, stride, norm, head, stats, impl) in fused.REFUSALS:
        got = by_key[key(dtype, shape, c0, c1, cout, stride, impl, stats, norm is not None, head)]
        assert int(got[0]) < 0 and got[1], (name, got)
    assert checked >= 70


# ------------------------------------------------------------------ properties over a sweep
VOLS = [(4,) * 3, (8,) * 3, (16,) * 3, (32,) * 3, (64,) * 3, (128,) * 3, (12, 20, 28), (5, 7, 9), (160, 192, 128), (20, 24, 16),
        (8, 16, 32), (16, 16, 32), (32, 64, 64), (15, 16, 32), (24, 24, 24), (6, 5, 7), (40, 56, 44), (64, 64, 32), (2, 2, 2), (96, 96, 96)]
# (stats, in_norm, head classes): each alone, and the combinations the network uses or must refuse
FLAGS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 4), (0, 0, 5), (1, 0, 3), (0, 1, 3), (1, 1, 3)]


def _sweep():
    for dtype in ("f32", "f16"):
        cins = ([8] if dtype == "f32" else []) + [16, 32, 64, 128, 256, 320, 640]
        for stride, cin, cout, n, vol in itertools.product((1, 2), cins, (32, 64, 128, 256, 320), (1, 2, 8, 16, 32), VOLS):
            splits = [(cin, 0), (cin // 2, cin // 2)]
            splits += {64: [(24, 40), (8, 56), (16, 48), (32, 32), (48, 16), (40, 24)], 128: [(64, 64), (32, 96), (72, 56)],
                       32: [(8, 24), (24, 8)]}.get(cin, [])
            for c0, c1 in dict.fromkeys(splits):
                for stats, norm, head in FLAGS:
                    yield dtype, (n,) + vol, c0, c1, cout, stride, stats, norm, head


#: instantiations that read their input in 16-channel chunks and pick in0 or in1 once per chunk
CHUNK16 = re.compile(r"conv3_f32_wino[23]_kernel|conv3_f32_mfma_kernel<1, 16,|conv3_f16_")
#: instantiations that apply a producer's normalisation while staging
INAFF = re.compile(r"conv3_f32_wino3_kernel<2, true>|conv3_f16_mfma_pipe_kernel<\d, \d, false, true, 1, true>|"
                   r"conv3_f16_dma_kernel<(true|false), true>|conv3_f16_c32_kernel<(true|false), true, false>")
#: persistent kernels: blockIdx.x & 7 labels the XCD group
PERSISTENT = re.compile(r"_wino[23]_kernel|_s2dma_kernel|_pipe_kernel|conv3_f16_dma_kernel|conv3_f16_c32_kernel")
#: why a call that carries an input normalisation may be refused (the dispatchers' own messages)
NORM_REFUSALS = re.compile(r"a pending input normalisation reached a kernel that cannot apply it|input normalisation can only be fused into the "
                           r"stride-1 kernels|fused head needs Cout|concat split .* not a multiple of|fused input normalisation needs a volume "
                           r"of whole tiles")
#: calls whose recorded behaviour breaks a property below: (property, dtype, shape, c0, c1, cout, stride, stats, norm, head) -> reason
KNOWN_EXCEPTIONS = {}


def test_plan_properties(amd):
    import ctypes as C
    lib = amd._lib.load()
    p = amd._lib.ConvPlan()
    n_calls = n_accepted = 0
    bad = []

    def plan(dtype, shape, c0, c1, cout, stride, stats, norm, head):
        rc = lib.mi355_conv3d_plan(int(dtype == "f16"), *shape, c0, c1, cout, stride, 0, stats, norm, head, C.byref(p))
        return rc, p.kernel.decode()

    for call in _sweep():
        dtype, shape, c0, c1, cout, stride, stats, norm, head = call
        rc, kernel = plan(*call)
        n_calls += 1

        def broke(prop):
            if (prop,) + call not in KNOWN_EXCEPTIONS:
                bad.append((prop, call, rc, kernel, tuple(p.grid), p.lds_bytes, p.splitk))

        if rc < 0:
            if not (lib.mi355_last_error() or b"").strip():
                broke("refusal without a message")
            if norm and not NORM_REFUSALS.search(lib.mi355_last_error().decode()):
                broke("input norm refused for another reason")
            continue
        n_accepted += 1
        fuses = bool(p.fuses_in_norm)
        grid, lds, splitk = tuple(p.grid), p.lds_bytes, p.splitk
        if head and (grid[1] != 1 or splitk != 1):
            broke("fused head: one cout block per voxel tile, no split-K")
        if CHUNK16.search(kernel) and (c0 % 16 or c1 % 16):
            broke("16-channel-chunk kernel on a split that is not a multiple of 16")
        if norm and not INAFF.fullmatch(kernel):
            broke("input norm accepted by an instantiation that does not apply it")
        if splitk != 1 and (stats or head or not 2 <= splitk <= 8 or not kernel.endswith(" split-K") or grid[2] != splitk):
            broke("split-K only without statistics and head, 2..8 slices")
        if splitk == 1 and (kernel.endswith(" split-K") or grid[2] != 1):
            broke("split-K name or grid.z without slices")
        if not 0 < lds <= LDS_MAX:
            broke("LDS bytes")
        if PERSISTENT.search(kernel) and grid[0] % 8:
            broke("persistent grid.x % 8")
        if fuses and not norm:  # what can_defer_norm relies on: the same call with the norm set is accepted
            rc2, kernel2 = plan(dtype, shape, c0, c1, cout, stride, stats, 1, head)
            if rc2 < 0 or not INAFF.fullmatch(kernel2):
                broke("fuses_input_norm says yes but the call with the norm is refused")
    print(f"PLAN PROPERTIES: {n_calls} calls, {n_accepted} accepted, {len(bad)} violations")
    assert n_calls > 500000 and n_accepted > 100000
    assert not bad, bad[:10]
