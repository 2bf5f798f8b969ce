"""Every 3x3x3 conv kernel instantiation the planner can select is the declared kernel of some GPU case, checked on the CPU
through the dry-run entry points mi355_conv3d_plan and mi355_conv_kernel_names (no device).

* Each entry of conv_rows_util.CASES plans to the kernel it is written for, under its own switch environment, and its `ragged`
  flag is what the plan's tile says.
* Closure: a fixed sweep of the planner (conv_rows_util.sweep: both dtypes, both strides, the channel counts of the networks,
  statistics, batch sizes 1..16; producer norm and head at stride 1 and two batch sizes; thin, ragged and whole-tile volumes) under the default switches and
  under every switch setting of conv_rows_util.SWEEP_ENVS.  Every kernel name it yields, split-K forms apart, must be declared by
  a GPU case: an expectation of test_gpu_ops.py or test_gpu_conv_fused.py, a name of tests/golden/conv_plan_rows.txt (the kernels
  of the bench networks and of those modules' cases) or an entry of the table.
* No silent dead rows: every row of the four tables is selected somewhere in the sweep or listed, with its reason, in
  conv_rows_util.UNPLANNED - and nothing listed there is selected.

The switches are read once per process: one child per switch setting plans that setting's sweep and table entries."""
import collections
import importlib.util
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import conv_rows_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import brats_amd as amd
import conv_rows_util as U
names, n_calls = {}, 0
for call in U.sweep():
    dtype, shape, cin, cout, stride, stats, norm, head = call
    p = amd.ops.conv3d_plan(dtype, shape, cin, cout, stride=stride, stats=stats, in_norm=norm, head_ncls=head)
    n_calls += 1
    if p["rc"] >= 0:
        names.setdefault(p["kernel"], [0, call])[0] += 1
cases = {}
for c in U.CASES:
    if U.env_key(c.env) == sys.argv[2]:
        cases[c.name] = amd.ops.conv3d_plan(c.dtype, c.shape, c.cin, c.cout, stride=c.stride, stats=c.stats)
print("RESULT " + json.dumps({"calls": n_calls, "names": names, "cases": cases, "rows": amd.ops.conv_kernel_names()}))
"""


@pytest.fixture(scope="module")
def plans(amd):
    """{switch setting: what its child planned}; `amd` first, so that the library is built once, not by every child"""
    envs = {U.env_key(e): e for e in U.SWEEP_ENVS + [c.env for c in U.CASES]}

    def run(key):
        res = subprocess.run([sys.executable, "-c", _CHILD, ROOT, key], env=U.child_env(envs[key]), capture_output=True, text=True, timeout=300)
        lines = [line for line in res.stdout.splitlines() if line.startswith("RESULT ")]
        assert res.returncode == 0 and lines, (key, res.stdout[-1000:], res.stderr[-2000:])
        return json.loads(lines[-1][7:])

    with ThreadPoolExecutor(max_workers=8) as pool:  # (the children are single-threaded planners)
        return dict(zip(envs, pool.map(run, envs)))


def _load(name):
    spec = importlib.util.spec_from_file_location("_rows_" + name, os.path.join(HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _declared_elsewhere():
    """the kernels the older GPU cases declare: expectations of the two single-op modules and the names of the recorded rows"""
    ops, fused = _load("test_gpu_ops"), _load("test_gpu_conv_fused")
    out = set(ops.F32_EXPECT_KERNEL.values()) | set(ops.F16_EXPECT_KERNEL.values()) | set(ops.SUMS_EXPECT_KERNEL.values())
    out |= set(fused.EXPECT_KERNEL.values())
    with open(os.path.join(HERE, "golden", "conv_plan_rows.txt")) as fh:
        for line in fh:
            f = [s.strip() for s in line.rstrip("\n").split(" | ")]
            if not line.startswith("#") and line.strip() and int(f[2]) >= 0:
                out.add(f[3])
    return out


#: the table, row by row: how many entries each kernel name has.  The nine instantiations that no test ran before the table
#: existed, in every form the planner selects them in, and four more the sweep found (<1, 2, 2> and the two 8-channel kernels
#: in their plain form, the stride-2 fp16 split-K with one fragment).  Counts, not just names: deleting ANY entry must fail, and
#: the per-name assertions below cannot tell a trio from a pair.
ENTRIES = {
    "conv3_f32_mfma_kernel<1, 16, 4, 1>": 4, "conv3_f32_mfma_kernel<1, 16, 4, 2>": 3,
    "conv3_f16_mfma_pipe_kernel<2, 1, false, false, 1, false>": 2, "conv3_f16_mfma_pipe_kernel<4, 1, false, false, 1, false>": 2,
    "conv3_f16_mfma_pipe_kernel<4, 1, false, false, 1, true>": 2,
    "conv3_f16_mfma_kernel<1, 2, 1> split-K": 3, "conv3_f16_mfma_kernel<1, 2, 1>": 3,
    "conv3_f32_mfma_kernel<1, 16, 2, 1>": 3, "conv3_f32_mfma_kernel<1, 16, 2, 2>": 3, "conv3_f32_mfma_kernel<1, 8, 4, 1>": 2,
    "conv3_f16_mfma_kernel<1, 2, 2>": 3, "conv3_f32_mfma_kernel<1, 8, 2, 1>": 3, "conv3_f32_mfma_kernel<1, 8, 2, 2>": 3,
    "conv3_f16_mfma_kernel<2, 1, 1> split-K": 2,
}


def test_table_has_every_form_of_every_row():
    """per kernel name: the recorded number of entries; statistics on and off where the kernel takes them (a run-time argument
    of the mfma and pipe kernels; split-K never carries them); a ragged and a whole-tile volume unless the name fixes the side"""
    assert dict(collections.Counter(c.kernel for c in U.CASES)) == ENTRIES
    for kernel in ENTRIES:
        mine = [c for c in U.CASES if c.kernel == kernel]
        if not kernel.endswith(" split-K"):
            assert {c.stats for c in mine} == {False, True}, kernel
        else:
            assert not any(c.stats for c in mine), kernel
        sides = {c.ragged for c in mine}
        assert sides == ({U.ONE_SIDED[kernel]} if kernel in U.ONE_SIDED else {False, True}), (kernel, sides)
    for c in U.CASES:
        assert set(c.env) <= set(U.SWITCHES) and c.dtype in ("f32", "f16") and c.stride in (1, 2) and c.act in (0, 1), c
        # the gates of test_gpu_ops.py run at the network's slope; the exact-integer run has its own (0.5)
        assert c.slope == 0.01, c
        # exact-integer run: 16 channels' worth of non-zero weights at most (conv_rows_util.int_weight_period)
        assert c.cin <= 16 or c.cin % 16 == 0, c


def test_each_entry_plans_to_its_kernel(plans):
    for c in U.CASES:
        p = plans[U.env_key(c.env)]["cases"][c.name]
        assert (p["rc"], p["kernel"]) == (0, c.kernel), (c.name, p)
        assert (p["splitk"] > 1) == c.kernel.endswith(" split-K"), (c.name, p)
        out = [(v - 1) // c.stride + 1 for v in c.shape[1:]]
        assert c.ragged == any(o % t for o, t in zip(out, p["tile"])), (c.name, out, p["tile"])


def test_every_selected_kernel_is_declared_by_a_gpu_case(plans):
    declared = _declared_elsewhere() | {c.kernel for c in U.CASES}
    names = set()
    for e in U.SWEEP_ENVS:
        got = plans[U.env_key(e)]
        assert got["calls"] == U.SWEEP_CALLS
        assert len(got["names"]) >= 15, (e, sorted(got["names"]))  # (the sweep did plan)
        missing = {k: v for k, v in got["names"].items() if k not in declared}
        assert not missing, f"under {U.env_key(e)} the planner selects kernels that no GPU case declares (add entries to conv_rows_util.CASES): {missing}"
        names |= set(got["names"])
    print(f"CONV ROWS: {len(names)} kernel names over {len(U.SWEEP_ENVS)} switch settings, all declared")


def test_no_row_is_silently_dead(plans):
    rows = plans["defaults"]["rows"]
    assert all(plans[U.env_key(e)]["rows"] == rows for e in U.SWEEP_ENVS)
    names = [n for _, n in rows]
    assert {t for t, _ in rows} == {"f32_rows", "wino3_rows", "f16_rows", "s2h_rows"} and len(names) >= 55
    assert len(set(names)) == len(names), [n for n, k in collections.Counter(names).items() if k > 1]  # (find_row takes the first)
    selected = {k.replace(" split-K", "") for e in U.SWEEP_ENVS for k in plans[U.env_key(e)]["names"]}
    assert selected <= set(names), selected - set(names)  # (every planned name is a row: none of the sweep's calls is a first layer)
    dead = [n for n in names if n not in selected and n not in U.UNPLANNED]
    assert not dead, f"rows that no plan of the sweep selects: give each a GPU case or list it in conv_rows_util.UNPLANNED with its reason: {dead}"
    stale = [n for n in U.UNPLANNED if n in selected or n not in names]
    assert not stale, f"listed as unplanned, but selected by the sweep or not a row: {stale}"
    assert all(len(reason) > 20 for reason in U.UNPLANNED.values())


def test_integer_reference_and_operands():
    """the int64 conv of the exact-integer run against torch's float64 conv3d (exact on these integers), both strides, and the
    bound that makes the run exact: 16 channels' worth of non-zero weights per output, every (channel, tap) still used"""
    import numpy as np
    import torch
    import torch.nn.functional as F
    for c in [c for c in U.CASES if c.shape[0] * c.shape[1] * c.shape[2] * c.shape[3] <= 4000]:
        x, wt, b = U.int_operands(c)
        assert x.min() == -4 and x.max() == 4 and set(np.unique(wt)) <= {-1, 0, 1} and np.abs(b).max() <= 8
        nnz = (wt != 0).sum(axis=(1, 2, 3, 4))
        assert nnz.max() <= 27 * 16 and (c.cin <= 16 or nnz.min() == 27 * 16), (c.name, nnz.min(), nnz.max())
        assert (wt != 0).any(axis=0).all(), c.name  # no input channel or tap is dropped from the check
        acc = U.int_conv(x, wt, b, c.stride)
        ref = F.conv3d(torch.from_numpy(x).double().permute(0, 4, 1, 2, 3), torch.from_numpy(wt).double(), torch.from_numpy(b).double(),
                       stride=c.stride, padding=1).permute(0, 2, 3, 4, 1).numpy()
        assert acc.shape == ref.shape and np.array_equal(acc, ref), c.name
        assert np.abs(acc).max() < U.INT_BOUND
        assert np.array_equal(U.int_expected_doubled(acc), 2 * np.where(ref >= 0, ref, U.INT_SLOPE * ref))


def test_integer_run_sees_the_defects_it_is_for():
    """the operands and the reference, not the GPU path: on the operands of the small entries a one-voxel shift along each axis, a swapped pair of input or output channels, a
    dropped 16-channel slice (what a lost split-K slice is), a tile edge one voxel short and LeakyReLU at another slope each
    change some output of the exact-integer run by at least 0.5 - which np.array_equal cannot miss"""
    import numpy as np
    for c in [c for c in U.CASES if c.shape[0] * c.shape[1] * c.shape[2] * c.shape[3] <= 4000]:
        x, wt, b = U.int_operands(c)
        want2 = U.int_expected_doubled(U.int_conv(x, wt, b, c.stride))
        swapped_in, swapped_out = wt.copy(), wt.copy()
        swapped_in[:, [0, 1]] = wt[:, [1, 0]]
        swapped_out[[0, 1]] = wt[[1, 0]]
        dropped = wt.copy()
        dropped[:, -16:] = 0
        short = x.copy()
        short[:, :, :, -1] = 0  # the last x column read as padding
        mutants = {f"shift axis {a}": (np.roll(x, 1, axis=a), wt) for a in (1, 2, 3)}
        mutants.update({"input channels 0, 1 swapped": (x, swapped_in), "output channels 0, 1 swapped": (x, swapped_out),
                        "last x column dropped": (short, wt)})
        if c.cin > 16:
            mutants["last 16 channels dropped"] = (x, dropped)
        for name, (mx, mw) in mutants.items():
            got2 = U.int_expected_doubled(U.int_conv(mx, mw, b, c.stride))
            assert np.abs(got2 - want2).max() >= 1, (c.name, name)  # (doubled outputs: 1 = 0.5 of an output)
        acc = U.int_conv(x, wt, b, c.stride)
        assert (acc < 0).any() and (acc[acc < 0] % 2 != 0).any(), c.name  # a slope other than 0.5, or none, shows on these
