"""Mass effect (the reference's step 2) on the MI355X: the five kernels of csrc/mass_effect.hip against numpy, the dicts against
what the reference's step 2 returned under the stored seed (tests/golden/mass_effect.json; a float that contains a std within
1e-9 relative, everything else exactly).  The child processes this file starts run under a time limit of their own; nothing is
retried."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import mass_effect_util as mx

pytestmark = pytest.mark.gpu
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def me(amd):
    return mx.module()


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)  # (a copy: the cached arrays are read-only)


# ---- axis counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mx.AXIS_SHAPES)
def test_axis_counts_equal_numpy(me, gpu, shape):
    for flags in (mx.random_flags(shape), np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)):
        fd = _dev(flags, gpu)
        for require, forbid in mx.SELECTIONS:
            got, want = me.axis_counts(fd, require, forbid), mx.axis_counts(flags, require, forbid)
            for a in range(3):
                assert got[a].dtype == np.int64 and np.array_equal(got[a], want[a]), (shape, require, forbid, a)
    assert int(me.axis_counts(_dev(np.full(shape, 255, np.uint8), gpu))[0].sum()) == int(np.prod(shape))      # all set
    assert int(me.axis_counts(_dev(np.zeros(shape, np.uint8), gpu), 1)[2].sum()) == 0                         # none set


def test_axis_counts_of_an_unaligned_view_and_refusals(me, amd, gpu):
    flags = mx.random_flags((5, 70, 9))
    buf = torch.zeros(flags.size + 3, dtype=torch.uint8, device=gpu)
    view = buf[3:].view(flags.shape)  # three bytes past a 16-byte boundary: the byte-load path
    view.copy_(_dev(flags, gpu))
    assert view.data_ptr() % 16 == 3
    for a, (g, w) in enumerate(zip(me.axis_counts(view, 5, 2), mx.axis_counts(flags, 5, 2))):
        assert np.array_equal(g, w), a
    with pytest.raises(amd._lib.Mi355Error, match="longer than 4096"):
        me.axis_counts(torch.zeros((1, mx.AXIS_MAX + 1, 2), dtype=torch.uint8, device=gpu))
    assert me.axis_counts(torch.ones((1, mx.AXIS_MAX, 2), dtype=torch.uint8, device=gpu), 1)[1].tolist() == [2] * mx.AXIS_MAX
    for require, forbid in ((256, 0), (-1, 0), (3, 1), (0, 256)):
        with pytest.raises(amd._lib.Mi355Error, match="require"):
            me.axis_counts(_dev(flags, gpu), require, forbid)


# ---- box counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mx.box_cases()))
def test_box_counts_equal_numpy(me, gpu, name):
    flags, boxes = mx.random_flags(mx.BOX_SHAPE), mx.box_cases()[name]
    fd = _dev(flags, gpu)
    for require, forbid in ((1, 2), (0, 0)):
        got = me.box_counts(fd, boxes, require, forbid)
        assert got.dtype == np.int64 and np.array_equal(got, mx.box_counts(flags, boxes, require, forbid)), (name, got)
    if name == "empty":
        assert not me.box_counts(fd, boxes).any()
    if name == "whole volume":
        assert me.box_counts(fd, boxes)[0] == flags.size
    if name == "single voxel":
        assert me.box_counts(fd, boxes).tolist() == [1, 1, 1]


def test_box_counts_refuse_boxes_outside_the_volume_and_too_many(me, amd, gpu):
    fd = _dev(mx.random_flags(mx.BOX_SHAPE), gpu)
    for boxes in mx.BAD_BOXES:
        with pytest.raises(amd._lib.Mi355Error, match="spans"):
            me.box_counts(fd, boxes)
    with pytest.raises(amd._lib.Mi355Error, match="boxes"):
        me.box_counts(fd, [(0, 1, 0, 1, 0, 1)] * 17)


# ---- ranked picks -----------------------------------------------------------------------------------------------------
def _check_ranked(me, gpu, flags, require, forbid):
    sel = mx.selected(flags, require, forbid)
    m = int(sel.sum())
    fd = _dev(flags, gpu)
    if m == 0:
        return fd, m
    ranks = mx.rank_set(m)
    index, count = me.select_ranked(fd, ranks, require, forbid)
    assert count == m and index.dtype == torch.int64
    assert np.array_equal(index.cpu().numpy(), mx.select_ranked(flags, ranks, require, forbid)), (flags.shape, m)
    return fd, m


@pytest.mark.parametrize("n", mx.RANK_SIZES)
def test_select_ranked_on_short_lists(me, gpu, n):
    for density in mx.RANK_DENSITIES:
        _check_ranked(me, gpu, mx.density_flags((n,), density, seed=n), 4, 1)
    _check_ranked(me, gpu, mx.random_flags((n,)), 0, 0)


@pytest.mark.parametrize("shape", mx.RANK_SHAPES)
@pytest.mark.parametrize("density", mx.RANK_DENSITIES)
def test_select_ranked_equals_flatnonzero(me, amd, gpu, shape, density):
    flags = mx.density_flags(shape, density)
    fd, m = _check_ranked(me, gpu, flags, 4, 1)
    assert m > 0
    before = torch.full((2,), -7, dtype=torch.int64, device=gpu)
    import ctypes
    ranks, count = (ctypes.c_int64 * 2)(0, m), ctypes.c_int64(-1)  # rank m: one past the last
    rc = amd._lib.load().mi355_select_ranked(fd.data_ptr(), 4, 1, fd.numel(), ranks, 2, before.data_ptr(), ctypes.byref(count), None)
    assert rc < 0 and b"rank" in amd._lib.load().mi355_last_error()
    assert count.value == m and before.tolist() == [-7, -7]  # the count is delivered, nothing is written


def test_select_ranked_refuses_every_rank_of_an_empty_selection(me, amd, gpu):
    fd = _dev(mx.density_flags((17, 33, 65), 0.5), gpu)
    with pytest.raises(amd._lib.Mi355Error, match="of 0 selected"):
        me.select_ranked(fd, [0], 1, 0)  # bit 0 is never set
    with pytest.raises(amd._lib.Mi355Error, match="ranks"):
        me.select_ranked(fd, np.zeros(65537, np.int64), 4, 1)
    with pytest.raises(amd._lib.Mi355Error, match="rank -1"):
        me.select_ranked(fd, [3, -1], 4, 1)


# ---- pair distance ----------------------------------------------------------------------------------------------------
def test_min_pair_dist2(me, amd, gpu):
    shape = (240, 240, 155)
    V = int(np.prod(shape))
    corner = lambda idx: int(np.ravel_multi_index(idx, shape))
    one = lambda v: torch.tensor([v], dtype=torch.int64, device=gpu)
    assert me.min_pair_dist2(one(corner((3, 4, 5))), one(corner((5, 1, 11))), shape) == 4 + 9 + 36                 # 1 x 1
    assert me.min_pair_dist2(one(0), one(V - 1), shape) == 239 ** 2 + 239 ** 2 + 154 ** 2                           # opposite corners
    rs = np.random.RandomState(13)
    g = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    near, far = np.flatnonzero((g[0] < 100) & (g[1] < 240) & (g[2] < 155)), np.flatnonzero((g[0] >= 120) & (g[1] < 240) & (g[2] < 155))
    a, b = rs.choice(near, 1000, replace=False), rs.choice(far, 1000, replace=False)
    want = mx.min_pair_dist2(a, b, shape)
    assert me.min_pair_dist2(_dev(a, gpu), _dev(b, gpu), shape) == want and want >= 21 ** 2                         # 1000 x 1000
    assert me.min_pair_dist2(_dev(b, gpu), _dev(a, gpu), shape) == want
    b2 = b.copy()
    b2[617] = a[401]
    assert me.min_pair_dist2(_dev(a, gpu), _dev(b2, gpu), shape) == 0                                               # a shared voxel
    many = rs.choice(far, 5000, replace=False)  # more than one chunk of list b, a last partial tile of both lists
    assert me.min_pair_dist2(_dev(a[:777], gpu), _dev(many, gpu), shape) == mx.min_pair_dist2(a[:777], many, shape)
    long_axis = (40000, 2, 3)  # an axis above 32768: the 64-bit arithmetic
    assert me.min_pair_dist2(one(0), one(int(np.ravel_multi_index((39999, 1, 2), long_axis))), long_axis) == 39999 ** 2 + 1 + 4
    for bad in (V, -1):
        with pytest.raises(amd._lib.Mi355Error, match="outside"):
            me.min_pair_dist2(one(5), one(bad), shape)
    with pytest.raises(amd._lib.Mi355Error, match="points"):
        me.min_pair_dist2(one(5), torch.zeros(65537, dtype=torch.int64, device=gpu), shape)


# ---- masked minimum ---------------------------------------------------------------------------------------------------
def test_masked_min(me, amd, gpu):
    shape = (17, 33, 65)
    rs = np.random.RandomState(17)
    values = rs.randint(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    flags = mx.random_flags(shape)
    vd, fd = _dev(values, gpu), _dev(flags, gpu)
    for require, forbid in mx.SELECTIONS:
        assert me.masked_min(vd, fd, require, forbid) == mx.masked_min(values, flags, require, forbid)
    assert me.masked_min(vd, fd)[0] < 0                                                                              # negatives
    top = np.full(shape, INT32_MAX, np.int32)
    assert me.masked_min(_dev(top, gpu), fd, 1, 0) == (INT32_MAX, int(mx.selected(flags, 1).sum()))                  # INT32_MAX is a value
    top[3, 4, 5] = -2 ** 31
    one = np.zeros(shape, np.uint8)
    one[3, 4, 5] = 8
    assert me.masked_min(_dev(top, gpu), _dev(one, gpu), 8) == (-2 ** 31, 1)
    assert me.masked_min(vd, torch.zeros(shape, dtype=torch.uint8, device=gpu), 1) == (None, 0)                      # an empty selection
    import ctypes
    lowest, count = ctypes.c_int32(-12345), ctypes.c_int64(-1)
    empty = torch.zeros(shape, dtype=torch.uint8, device=gpu)
    assert amd._lib.load().mi355_masked_min_i32(vd.data_ptr(), empty.data_ptr(), 1, 0, vd.numel(), ctypes.byref(lowest), ctypes.byref(count), None) == 0
    assert (lowest.value, count.value) == (-12345, 0)  # left untouched


# ---- end to end -------------------------------------------------------------------------------------------------------
def _run_case(me, gpu, case, distance="sampled", dev=None):
    if dev is None:
        seg, t1 = mx.fixture_data(case)
        dev = (_dev(seg, gpu), _dev(t1, gpu))
    np.random.seed(case["rng_seed"])
    return me.mass_effect(*dev, case["voxel_dims"], distance=distance)


def test_mass_effect_equals_the_reference_under_the_stored_seed(me, gpu):
    cmp = mx.Comparer()
    for case in mx.load_fixture()["cases"]:
        seg, t1 = mx.fixture_data(case)
        dev = (_dev(seg, gpu), _dev(t1, gpu))
        if case["args"]["shape"] == [240, 240, 155]:
            _run_case(me, gpu, case, dev=dev)  # warm: scratch buffers at their final size
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = _run_case(me, gpu, case, dev=dev)
            print(f"mass_effect, 240 x 240 x 155, sampled, warm: {(time.perf_counter() - t0) * 1e3:.1f} ms wall")
        else:
            got = _run_case(me, gpu, case, dev=dev)
        assert tuple(got) == mx.SECTIONS
        cmp.same(got, case["expected"], case["name"])
        assert type(got["midline_shift"]["is_significant"]) is bool
        # the generator is where the reference's two draws leave it: the second draw happens only with more than 1000 CSF voxels
        n_t, n_csf = case["facts"]["n_tumour"], case["facts"]["n_csf"]
        ref = np.random.RandomState(case["rng_seed"])
        if n_t and n_csf:
            mx.draws(n_t, n_csf, ref)
        assert all(np.array_equal(a, b) for a, b in zip(ref.get_state()[1:3], np.random.get_state()[1:3])), case["name"]
        # an explicit generator gives the same result and leaves the global one alone
        if n_t and n_csf and n_csf <= 1000:
            state = np.random.get_state()
            again = me.mass_effect(*dev, case["voxel_dims"], rng=np.random.RandomState(case["rng_seed"]))
            assert json.dumps(again) == json.dumps(got)
            assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))
    print(f"mass_effect: largest relative error of a float that contains a std {cmp.worst:.3g} at {cmp.where}")


def test_exact_distance_is_never_above_the_sampled_one_and_draws_nothing(me, gpu):
    larger = equal_small = 0
    for case in mx.load_fixture()["cases"]:
        np.random.seed(1234)
        state = np.random.get_state()
        got = _run_case_exact(me, gpu, case)
        assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state())), case["name"]  # the generator is untouched
        want = dict(case["expected"]["ventricular_compression"])
        exact, sampled = got["ventricular_compression"].get("tumor_to_ventricle_distance_mm"), want.get("tumor_to_ventricle_distance_mm")
        assert exact == case["facts"]["exact_distance_mm"], case["name"]
        if exact is None:
            assert sampled is None
            continue
        assert type(exact) is float and exact <= sampled, (case["name"], exact, sampled)
        larger += exact < sampled
        if case["facts"]["n_tumour"] <= 1000 and case["facts"]["n_csf"] <= 1000:
            assert exact == sampled, case["name"]
            equal_small += 1
        want["tumor_to_ventricle_distance_mm"] = exact  # nothing else depends on the distance
        mx.Comparer().same(got["ventricular_compression"], want, case["name"])
    assert larger >= 1 and equal_small >= 1


def _run_case_exact(me, gpu, case):
    seg, t1 = mx.fixture_data(case)
    return me.mass_effect(_dev(seg, gpu), _dev(t1, gpu), case["voxel_dims"], distance="exact")


def test_repeats_are_bit_equal_and_bad_inputs_are_refused(me, gpu):
    case = mx.case("shift_severe")
    one, two = _run_case(me, gpu, case), _run_case(me, gpu, case)
    assert json.dumps(one) == json.dumps(two)  # every float bit for bit, every key in the same place
    assert json.dumps(_run_case_exact(me, gpu, case)) == json.dumps(_run_case_exact(me, gpu, case))
    seg, t1 = mx.fixture_data(case)
    bad = seg.copy()
    bad[0, 0, 0] = 5
    with pytest.raises(ValueError, match="above 4"):
        me.mass_effect(_dev(bad, gpu), _dev(t1, gpu), case["voxel_dims"])
    with pytest.raises(ValueError, match="differ in shape"):
        me.mass_effect(_dev(seg, gpu), _dev(t1[:-1], gpu), case["voxel_dims"])
    with pytest.raises(ValueError, match="distance 'nearest'"):
        me.mass_effect(_dev(seg, gpu), _dev(t1, gpu), case["voxel_dims"], distance="nearest")
    plateau = np.where(t1 > 0, 500.0, 0.0).astype(np.float32)  # every positive voxel at the 5th percentile: no voxel above it
    with pytest.raises(ValueError, match="plateau"):
        me.mass_effect(_dev(seg, gpu), _dev(plateau, gpu), case["voxel_dims"])


@pytest.mark.parametrize("scheme,case_name", [("brats2021", "shift_moderate_negative"), ("brats2025", "csf_left_only")])
def test_mass_effect_command_writes_the_json(amd, gpu, tmp_path, scheme, case_name):
    case = mx.case(case_name)
    seg, t1 = mx.fixture_data(case)
    zooms = tuple(case["voxel_dims"])
    case_id = "BraTS2021_00042" if scheme == "brats2021" else "BraTS-GLI-00042-000"
    names = ("_t1", "_t1ce", "_t2", "_flair") if scheme == "brats2021" else ("-t1n", "-t1c", "-t2w", "-t2f")
    case_dir = tmp_path / "some_folder"
    case_dir.mkdir()
    for suffix in names:  # (step 2 reads T1 only; the case folder holds all four sequences)
        amd.nifti.save_like(case_dir / f"{case_id}{suffix}.nii.gz", t1.astype(np.int16), amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.int16))
    amd.nifti.save_like(tmp_path / "seg.nii.gz", seg, amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.uint8))
    out = tmp_path / "results" / "step2.json"
    env = dict(os.environ, PYTHONPATH=mx.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "brats_amd.mass_effect", "--input", str(case_dir), "--segmentation", str(tmp_path / "seg.nii.gz"),
                          "--output", str(out), "--seed", str(case["rng_seed"])], capture_output=True, text=True, env=env, cwd=mx.ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert len(res.stdout.strip().splitlines()) == 1 and res.stdout.startswith(case_id + ": "), res.stdout
    got = json.loads(out.read_text())
    assert list(got) == ["case_id", "step", "voxel_info", *mx.SECTIONS]
    assert got["case_id"] == case_id and got["step"] == "Step 2 - Mass effect metrics"
    assert got["voxel_info"]["dimensions_mm"] == [float(np.float32(v)) for v in zooms]
    mx.Comparer().same({k: got[k] for k in mx.SECTIONS}, case["expected"], case_name)
