"""Quality control (the reference's step 5) on the MI355X: the four kernels of csrc/quality.hip against scipy and numpy, the dicts
against what the reference's step 5 returned (tests/golden/quality.json; a float that contains a std within 1e-9 relative,
everything else exactly).  The child processes this file starts run under a time limit of their own; nothing is retried."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
from scipy import ndimage

import quality_util as qu

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def q(amd):
    return qu.module("quality")


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)  # (a copy: the cached arrays are read-only)


# ---- fill holes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(qu.fill_cases()))
def test_fill_holes_is_scipy_bit_for_bit(q, gpu, name):
    mask = qu.fill_cases()[name]
    want = ndimage.binary_fill_holes(mask).astype(np.uint8)
    out, filled = q.binary_fill_holes(_dev(mask, gpu))
    got = out.cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want), (name, int((got != want).sum()))
    assert filled == int(want.sum()) - int((mask != 0).sum())
    if name == "diagonal gap":
        assert filled == 27
    if name == "winding channel":
        assert filled == 0 and got[5, 5, 5] == 0


def test_fill_holes_takes_any_nonzero_as_foreground_and_refuses_aliasing(q, amd, gpu):
    mask = qu.fill_cases()["ball inside a shell"]
    seg = (mask * np.random.RandomState(2).randint(1, 5, mask.shape)).astype(np.uint8)
    out, filled = q.binary_fill_holes(_dev(seg, gpu))
    assert np.array_equal(out.cpu().numpy(), ndimage.binary_fill_holes(mask).astype(np.uint8)) and filled > 0
    m = _dev(mask, gpu)
    import ctypes
    n = ctypes.c_int64(0)
    rc = amd._lib.load().mi355_binary_fill_holes(m.data_ptr(), *mask.shape, m.data_ptr(), ctypes.byref(n), None)
    assert rc < 0 and b"out must not be the input" in amd._lib.load().mi355_last_error()


# ---- Sobel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", qu.SOBEL_SHAPES)
def test_sobel_magnitude_at_single_voxels_is_scipy_bit_for_bit(q, gpu, shape):
    x = qu.integer_volume(shape)
    want = qu.scipy_sobel_magnitude(x)
    xd = _dev(x, gpu)
    picks = qu.sobel_single_voxels(shape)
    assert len(picks) >= 8 if min(shape) > 1 else len(picks) >= 4
    for idx in picks:
        flags = torch.zeros(shape, dtype=torch.uint8, device=gpu)
        flags[idx] = 4
        n, mean, std = q.sobel_magnitude_stats(xd, flags, 4)
        assert (n, mean, std) == (1, float(want[idx]), 0.0), (idx, mean, float(want[idx]))
        assert q.sobel_magnitude_stats(xd, flags, 3) == (0, 0.0, 0.0)  # the bit is not among the selected ones


@pytest.mark.parametrize("shape", qu.SOBEL_SHAPES)
def test_sobel_statistics_over_everything_and_over_a_subset(q, gpu, shape):
    x = qu.integer_volume(shape)
    mag = qu.scipy_sobel_magnitude(x)
    rs = np.random.RandomState(3)
    for name, flags in (("everything", np.full(shape, 255, np.uint8)), ("subset", (rs.random_sample(shape) < 0.3).astype(np.uint8) * 16)):
        want = qu.stats_of(mag[flags != 0])
        n, mean, std = q.sobel_magnitude_stats(_dev(x, gpu), _dev(flags, gpu), 255 if name == "everything" else 16)
        err_mean, err_std = abs(mean - want[1]) / want[1], abs(std - want[2]) / want[2] if want[2] else abs(std)
        print(f"sobel {shape} {name}: n {n}, mean off by {err_mean:.3g} (bound {n * EPS:.3g}), std off by {err_std:.3g}")
        assert n == want[0] and n > 0
        assert err_mean <= n * EPS  # the reordering bound of a sum of n non-negative doubles
        assert err_std <= qu.RTOL_STD


def test_sobel_refuses_a_select_outside_1_255(q, amd, gpu):
    x = _dev(qu.integer_volume((2, 3, 4)), gpu)
    flags = torch.ones((2, 3, 4), dtype=torch.uint8, device=gpu)
    for select in (0, 256, -1):
        with pytest.raises(amd._lib.Mi355Error, match="select"):
            q.sobel_magnitude_stats(x, flags, select)


# ---- radial shells ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", qu.SHELL_SHAPES)
def test_radial_shells_equal_numpy_exactly(q, gpu, shape):
    x = qu.integer_volume(shape, seed=13)
    rs = np.random.RandomState(4)
    selected = rs.random_sample(shape) < 0.6 if shape != (1, 1, 1) else np.ones(shape, bool)
    flags = (selected.astype(np.uint8) * 5) | (rs.random_sample(shape) < 0.5).astype(np.uint8) * 2  # bits 0 and 2 select, bit 1 is noise
    centre = [np.float64(int(s)) / 7 for s in (rs.randint(0, 7 * n - 6) for n in shape)]  # of the form sum / n with n = 7, inside the volume
    want = qu.radial_shell(x, selected, centre)
    got = q.radial_shell_moments(_dev(x, gpu), _dev(flags, gpu), 5, centre)
    print(f"radial shells {shape}: max_dist {got[0]!r}, inner {got[1]} voxels, outer {got[3]} voxels")
    assert got[0] == want[0], (got[0], want[0])  # bit-equal: a fused multiply-add in the distance would show here
    assert got[1:] == want[1:]
    if shape == (1, 1, 1):
        assert got == (0.0, 0, 0.0, 0, 0.0)
    else:
        assert got[1] > 0 and got[3] > 0


def test_radial_shells_of_an_empty_selection_are_zero(q, gpu):
    x = _dev(qu.integer_volume((9, 10, 11)), gpu)
    flags = torch.full((9, 10, 11), 2, dtype=torch.uint8, device=gpu)
    assert q.radial_shell_moments(x, flags, 1, (4.0, 4.5, 5.0)) == (0.0, 0, 0.0, 0, 0.0)


# ---- face slabs -------------------------------------------------------------------------------------------------------
def test_face_slabs(q, amd, gpu):
    shape = (7, 9, 4)
    hi = [n - 1 for n in shape]
    picks = [tuple(hi[k] if (c >> k) & 1 else 0 for k in range(3)) for c in range(8)]
    picks += [tuple(end if j == k else shape[j] // 2 for j in range(3)) for k in range(3) for end in (0, hi[k])]
    for idx in picks:  # a single positive voxel at each corner and on each face, in turn, among negative values
        x = np.full(shape, -3.0, np.float32)
        x[idx] = 2.0
        for margin in (1, 2, 5, 100):  # 5 and 100: above the length of axis 2 / of every axis
            got = q.face_slab_counts(_dev(x, gpu), margin)
            assert got.dtype == np.int64 and np.array_equal(got, qu.face_slab_counts(x, margin)), (idx, margin, got)
    x = qu.integer_volume(shape) - 16000.0  # about half of the values negative
    for margin in (1, 3, 5):
        assert np.array_equal(q.face_slab_counts(_dev(x, gpu), margin), qu.face_slab_counts(x, margin))
    for margin in (0, -2):
        with pytest.raises(amd._lib.Mi355Error, match="margin"):
            q.face_slab_counts(_dev(x, gpu), margin)


# ---- end to end -------------------------------------------------------------------------------------------------------
def _run_case(q, gpu, case):
    seg, vols = qu.fixture_data(case)
    return q.quality_control(_dev(seg, gpu), *(_dev(v, gpu) for v in vols), case["voxel_dims"])


def test_quality_control_equals_the_reference(q, gpu):
    cmp = qu.Comparer()
    for case in qu.load_fixture()["cases"]:
        if case["args"]["shape"] == [240, 240, 155]:
            seg, vols = qu.fixture_data(case)
            dev = [_dev(seg, gpu)] + [_dev(v, gpu) for v in vols]
            q.quality_control(*dev, case["voxel_dims"])  # warm: scratch buffers at their final size
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = q.quality_control(*dev, case["voxel_dims"])
            print(f"quality_control, 240 x 240 x 155, warm: {(time.perf_counter() - t0) * 1e3:.1f} ms wall")
        else:
            got = _run_case(q, gpu, case)
        assert tuple(got) == qu.SECTIONS
        cmp.same(got, case["expected"], case["name"])
    print(f"quality_control: largest relative error of a float that contains a std {cmp.worst:.3g} at {cmp.where}")


def test_repeats_are_bit_equal_and_bad_inputs_are_refused(q, gpu):
    case = qu.case("issues_poor_t2")
    one, two = _run_case(q, gpu, case), _run_case(q, gpu, case)
    assert json.dumps(one) == json.dumps(two)  # every float bit for bit, every key in the same place
    seg, vols = qu.fixture_data(case)
    bad = seg.copy()
    bad[0, 0, 0] = 5
    with pytest.raises(ValueError, match="above 4"):
        q.quality_control(_dev(bad, gpu), *(_dev(v, gpu) for v in vols), case["voxel_dims"])
    with pytest.raises(ValueError, match="differ in shape"):
        q.quality_control(_dev(seg, gpu), *(_dev(v[:-1], gpu) for v in vols), case["voxel_dims"])
    chans = [_dev(v, gpu) for v in vols]
    chans[2] = torch.zeros_like(chans[2])
    with pytest.raises(ValueError, match="T2 has no positive voxel"):
        q.quality_control(_dev(seg, gpu), *chans, case["voxel_dims"])


@pytest.mark.parametrize("scheme,case_name", [("brats2021", "good_segmentation"), ("brats2025", "bias_severe_ghost")])
def test_quality_command_writes_the_json(amd, gpu, tmp_path, scheme, case_name):
    case = qu.case(case_name)
    seg, vols = qu.fixture_data(case)
    zooms = tuple(case["voxel_dims"])
    case_id = "BraTS2021_00042" if scheme == "brats2021" else "BraTS-GLI-00042-000"
    names = ("_t1", "_t1ce", "_t2", "_flair") if scheme == "brats2021" else ("-t1n", "-t1c", "-t2w", "-t2f")
    case_dir = tmp_path / "some_folder"
    case_dir.mkdir()
    for v, suffix in zip(vols, names):
        amd.nifti.save_like(case_dir / f"{case_id}{suffix}.nii.gz", v.astype(np.int16), amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.int16))
    amd.nifti.save_like(tmp_path / "seg.nii.gz", seg, amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.uint8))
    out = tmp_path / "results" / "step5.json"
    env = dict(os.environ, PYTHONPATH=qu.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "brats_amd.quality", "--input", str(case_dir), "--segmentation", str(tmp_path / "seg.nii.gz"),
                          "--output", str(out)], capture_output=True, text=True, env=env, cwd=qu.ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert len(res.stdout.strip().splitlines()) == 1 and res.stdout.startswith(case_id + ": "), res.stdout
    got = json.loads(out.read_text())
    assert list(got) == ["case_id", "step", *qu.SECTIONS]
    assert got["case_id"] == case_id and got["step"] == "Step 5 - Quality control and confidence metrics"
    qu.Comparer().same({k: got[k] for k in qu.SECTIONS}, case["expected"], case_name)
