"""Connected-component labelling, per-component statistics and lesion multiplicity on the MI355X:
bit-equal to scipy.ndimage.label / numpy on every volume, and equal to what the reference's step 3 returned
(tests/golden/multiplicity.json)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import components_util as cu

pytestmark = pytest.mark.gpu

NOISE_SHAPE = (45, 70, 150)
# name -> builder of a uint8 mask; fixed list
VOLUMES = {
    "one_voxel_on": lambda: np.ones((1, 1, 1), np.uint8),
    "one_voxel_off": lambda: np.zeros((1, 1, 1), np.uint8),
    "line_last_axis": lambda: cu.noise(11, (1, 1, 301), 0.6),
    "line_first_axis": lambda: cu.noise(12, (301, 1, 1), 0.6),
    "ragged_small": lambda: cu.noise(13, (5, 9, 70), 0.4),
    "ragged_medium": lambda: cu.noise(14, (7, 17, 130), 0.3),
    "ragged_thin": lambda: cu.noise(15, (13, 3, 65), 0.5),
    "all_zeros": lambda: np.zeros((9, 20, 100), np.uint8),
    "all_ones": lambda: np.ones((9, 20, 100), np.uint8),
    "checkerboard": lambda: cu.checkerboard((16, 24, 96)),
    "serpentine": lambda: cu.serpentine((13, 37, 200)),
    "noise_0.05": lambda: cu.noise(21, NOISE_SHAPE, 0.05),
    "noise_0.2": lambda: cu.noise(22, NOISE_SHAPE, 0.2),
    "noise_0.31": lambda: cu.noise(23, NOISE_SHAPE, 0.31),
    "noise_0.5": lambda: cu.noise(24, NOISE_SHAPE, 0.5),
    "noise_0.7": lambda: cu.noise(25, NOISE_SHAPE, 0.7),
    "noise_0.31_full_size": lambda: cu.noise(26, (240, 240, 155), 0.31),
}


def _label(amd, gpu, mask, connectivity):
    labels, n = amd.components.label_components(torch.from_numpy(np.ascontiguousarray(mask)).to(gpu), connectivity)
    return labels.cpu().numpy(), n


def _check_labels(amd, gpu, mask, connectivity, what):
    want, n_want = cu.scipy_labels(mask, connectivity)
    got, n = _label(amd, gpu, mask, connectivity)
    assert got.dtype == np.int32 and got.shape == mask.shape
    print(f"{what} connectivity {connectivity}: {n} components (scipy {n_want}), {int((got != want).sum())} voxels differ")
    assert n == n_want, what
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("connectivity", [1, 3])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_labels_equal_scipy(amd, gpu, name, connectivity):
    mask = VOLUMES[name]()
    if name == "checkerboard":
        want_n = mask.size // 2 if connectivity == 1 else 1
        assert cu.scipy_labels(mask, connectivity)[1] == want_n
    _check_labels(amd, gpu, mask, connectivity, name)


@pytest.mark.parametrize("connectivity", [1, 3])
def test_labels_equal_scipy_on_the_fixture_maps(amd, gpu, connectivity):
    for case in cu.load_fixture()["cases"]:
        seg = cu.fixture_label_map(amd, case)
        _check_labels(amd, gpu, (seg > 0).astype(np.uint8), connectivity, case["name"] + " tumour")
        _check_labels(amd, gpu, (seg == 3).astype(np.uint8), connectivity, case["name"] + " enhancing")
        _check_labels(amd, gpu, seg, connectivity, case["name"] + " raw labels as mask")  # foreground = nonzero, not == 1


def test_bad_connectivity_is_refused(amd, gpu):
    mask = torch.ones((4, 4, 4), dtype=torch.uint8, device=gpu)
    for c in (0, 2, 6, 26):
        with pytest.raises(amd._lib.Mi355Error, match="connectivity"):
            amd.components.label_components(mask, c)
    assert amd.components.label_components(mask, 1)[1] == 1


@pytest.mark.parametrize("name,connectivity", [("noise_0.05", 1), ("noise_0.05", 3), ("noise_0.2", 3), ("noise_0.31", 1), ("noise_0.7", 1),
                                               ("serpentine", 1), ("checkerboard", 1), ("all_ones", 3), ("line_first_axis", 1),
                                               ("ragged_medium", 3), ("one_voxel_on", 1)])
def test_component_stats_equal_numpy(amd, gpu, name, connectivity):
    mask = VOLUMES[name]()
    seg = np.random.RandomState(5).randint(0, 6, mask.shape).astype(np.uint8)  # values 0..5: 5 is counted nowhere
    want_lab, n = cu.scipy_labels(mask, connectivity)
    assert 0 < n <= 65536
    labels, n_got = amd.components.label_components(torch.from_numpy(mask).to(gpu), connectivity)
    assert n_got == n
    got = amd.components.component_stats(labels, n, torch.from_numpy(seg).to(gpu))
    assert got.dtype == np.int64 and np.array_equal(got, cu.numpy_stats(want_lab, n, seg)), name
    got = amd.components.component_stats(labels, n)
    assert np.array_equal(got, cu.numpy_stats(want_lab, n)), name
    assert not got[:, 10:].any()


def test_component_stats_on_the_fixture_maps(amd, gpu):
    for case in cu.load_fixture()["cases"]:
        seg = cu.fixture_label_map(amd, case)
        want_lab, n = cu.scipy_labels(seg > 0, 3)
        labels, n_got = amd.components.label_components(torch.from_numpy(seg).to(gpu), 3)
        assert n_got == n
        got = amd.components.component_stats(labels, n, torch.from_numpy(seg).to(gpu))
        assert got.shape == (n, 14) and np.array_equal(got, cu.numpy_stats(want_lab, n, seg)), case["name"]


def test_component_stats_cap_and_empty(amd, gpu):
    empty = torch.zeros((8, 8, 64), dtype=torch.uint8, device=gpu)
    labels, n = amd.components.label_components(empty, 1)
    assert n == 0 and amd.components.component_stats(labels, 0).shape == (0, 14)
    board = cu.checkerboard((64, 64, 64))
    labels, n = amd.components.label_components(torch.from_numpy(board).to(gpu), 1)   # the labelling itself has no cap
    assert n == 131072
    assert np.array_equal(labels.cpu().numpy(), cu.scipy_labels(board, 1)[0])
    with pytest.raises(amd._lib.Mi355Error, match="131072 components"):
        amd.components.component_stats(labels, n)
    small = cu.noise(3, (10, 20, 70), 0.2)     # ... and the next call works
    want_lab, n = cu.scipy_labels(small, 1)
    labels, n_got = amd.components.label_components(torch.from_numpy(small).to(gpu), 1)
    assert n_got == n and np.array_equal(amd.components.component_stats(labels, n), cu.numpy_stats(want_lab, n))


def test_lesion_multiplicity_equals_the_reference(amd, gpu):
    for case in cu.load_fixture()["cases"]:
        seg = cu.fixture_label_map(amd, case)
        got = amd.components.lesion_multiplicity(torch.from_numpy(seg).to(gpu), case["voxel_dims"])
        cu.assert_same(got, case["expected"], case["name"])


def test_repeated_calls_and_scratch_reuse(amd, gpu):
    a = torch.from_numpy(cu.noise(31, (40, 50, 130), 0.3)).to(gpu)
    b = torch.from_numpy(cu.noise(32, (9, 200, 70), 0.25)).to(gpu)
    la1, na1 = amd.components.label_components(a, 1)
    sa1 = amd.components.component_stats(la1, na1, a)
    la2, na2 = amd.components.label_components(a, 1)
    sa2 = amd.components.component_stats(la2, na2, a)
    assert na1 == na2 and torch.equal(la1, la2) and np.array_equal(sa1, sa2)
    lb, nb = amd.components.label_components(b, 3)       # another shape, another connectivity, then the first again
    sb = amd.components.component_stats(lb, nb)
    la3, na3 = amd.components.label_components(a, 1)
    sa3 = amd.components.component_stats(la3, na3, a)
    assert na3 == na1 and torch.equal(la3, la1) and np.array_equal(sa3, sa1)
    want_lab, n = cu.scipy_labels(b.cpu().numpy(), 3)
    assert nb == n and np.array_equal(lb.cpu().numpy(), want_lab) and np.array_equal(sb, cu.numpy_stats(want_lab, n))


def _blobby_seg(seed=41, shape=(40, 64, 72)):
    """label map with several objects per class: smoothed noise thresholded into classes 1..3, plus fragments"""
    from scipy.ndimage import gaussian_filter
    rs = np.random.RandomState(seed)
    f = gaussian_filter(rs.standard_normal(shape), 3.0)
    f = (f - f.mean()) / f.std()
    seg = np.zeros(shape, np.uint8)
    seg[f > 0.8] = 1
    seg[f > 1.3] = 2
    seg[f < -1.2] = 3
    idx = rs.choice(seg.size, 60, replace=False)
    seg.reshape(-1)[idx] = rs.randint(1, 4, 60)
    return seg


def test_component_filter_equals_numpy(amd, gpu):
    seg = _blobby_seg()
    mask = (seg == 1).astype(np.uint8)
    want_lab, n = cu.scipy_labels(mask, 1)
    labels, n_got = amd.components.label_components(torch.from_numpy(mask).to(gpu), 1)
    assert n_got == n and n > 3
    keep = np.random.RandomState(1).rand(n + 1) < 0.5
    keep[0] = False  # ignored: background voxels keep their seg value
    got = amd.components.component_filter(labels, torch.from_numpy(seg).to(gpu), keep).cpu().numpy()
    want = np.where((want_lab > 0) & ~keep[want_lab], 0, seg).astype(np.uint8)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("classes,vol,least", [([1], 1.0, None), ([2, 3], 0.5, None), ([(1, 2)], 1.0, None), ([1, 2, 3], 1.5, 30.0),
                                               ([(1, 2), 3], 1.0, {(1, 2): 40.0, 3: 5.0}), ([4], 1.0, None)])
def test_largest_component_equals_the_scipy_restatement(amd, gpu, classes, vol, least):
    seg = _blobby_seg()
    want, want_removed, want_kept = cu.largest_component_ref(seg, classes, vol, least)
    got, removed, kept = amd.components.remove_all_but_the_largest_connected_component(torch.from_numpy(seg).to(gpu), classes, vol, least)
    assert np.array_equal(got.cpu().numpy(), want)
    assert removed == want_removed and kept == want_kept
    if classes != [4]:
        assert not np.array_equal(want, seg), "the case removes nothing"


def _write_seg(amd, path, seg, zooms):
    like = amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.uint8)
    amd.nifti.save_like(path, seg, like)


def test_postprocess_front_end_with_and_without_largest_component(amd, gpu, tmp_path):
    src, plain, today, flagged = (tmp_path / d for d in ("src", "plain", "today", "flagged"))
    for d in (src, today):
        d.mkdir()
    seg = _blobby_seg(seed=43)
    zooms = (1.0, 1.0, 2.0)
    _write_seg(amd, src / "case.nii.gz", seg, zooms)
    front_end = importlib.import_module("brats_amd.nnunet_predict")
    assert front_end.main(["--postprocess", str(src), "-o", str(plain)]) == 0
    # today's path, step by step: threshold, label convention, save
    like = amd.nifti.load(src / "case.nii.gz")
    t, _ = amd.evaluate.apply_brats_threshold(torch.from_numpy(np.ascontiguousarray(like.data.astype(np.uint8))).to(gpu), 200, 2)
    amd.nifti.save_like(today / "case.nii.gz", amd.evaluate.convert_labels(t, "brats2021").cpu().numpy(), like)
    assert (plain / "case.nii.gz").read_bytes() == (today / "case.nii.gz").read_bytes()
    assert front_end.main(["--postprocess", str(src), "-o", str(flagged), "--largest_component", "1", "3",
                                    "--min_object_size", "50", "--label_format", "nnunet", "--threshold", "0"]) == 0
    want, _, _ = cu.largest_component_ref(seg, [1, 3], 2.0, 50.0)
    got = amd.nifti.load(flagged / "case.nii.gz").data
    assert np.array_equal(got, want) and not np.array_equal(want, seg)


def test_multiplicity_command_writes_the_json(amd, gpu, tmp_path):
    case = [c for c in cu.load_fixture()["cases"] if c["name"] == "aniso"][0]
    seg = cu.fixture_label_map(amd, case)
    case_dir = tmp_path / "BraTS-GLI-00042-000"
    case_dir.mkdir()
    _write_seg(amd, tmp_path / "seg.nii.gz", seg, tuple(case["voxel_dims"]))
    out = tmp_path / "results" / "step3.json"
    env = dict(os.environ, PYTHONPATH=cu.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "brats_amd.multiplicity", "--input", str(case_dir), "--segmentation", str(tmp_path / "seg.nii.gz"),
                          "--output", str(out)], capture_output=True, text=True, env=env, cwd=cu.ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = json.loads(out.read_text())
    assert got["case_id"] == "BraTS-GLI-00042-000" and got["voxel_info"]["dimensions_mm"] == case["voxel_dims"]
    cu.assert_same({k: got[k] for k in case["expected"]}, case["expected"], "aniso")
