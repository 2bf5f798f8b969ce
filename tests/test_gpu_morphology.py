"""Binary morphology, squared distance transform, mask reductions and tumour morphology on the MI355X:
masks and distance maps bit-equal to scipy.ndimage, integer moments bit-equal to numpy, fp64 statistics within 1e-9 relative,
and the dicts equal to what the reference's step 4 returned (tests/golden/morphology.json).  The one child process this file
starts runs under a time limit of its own; nothing is retried."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import components_util as cu
import morphology_util as mu
from test_gpu_components import VOLUMES

pytestmark = pytest.mark.gpu

RTOL = mu.RTOL
GRADIENT_VOLUMES = ("ragged_small", "ragged_medium", "checkerboard", "serpentine", "noise_0.05", "noise_0.31", "noise_0.7")


@pytest.fixture(scope="module")
def morph(amd):
    return mu.morphology_module()


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _has_background(mask):
    return bool((mask == 0).any())


@pytest.mark.parametrize("iterations", [1, 2, 5, 10])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_erosion_and_dilation_equal_scipy(morph, gpu, name, iterations):
    mask = VOLUMES[name]()
    dev = _dev(mask, gpu)
    for ours, theirs in ((morph.binary_erosion, mu.erode), (morph.binary_dilation, mu.dilate)):
        got = ours(dev, iterations).cpu().numpy()
        want = theirs(mask, iterations)
        assert got.dtype == np.uint8 and got.shape == mask.shape
        assert np.array_equal(got, want), (name, iterations, ours.__name__, int((got != want).sum()))


def test_morphology_reads_nonzero_as_foreground_and_refuses_bad_calls(amd, morph, gpu):
    seg = np.random.RandomState(4).randint(0, 5, (9, 11, 70)).astype(np.uint8) * (cu.noise(5, (9, 11, 70), 0.7))
    assert np.array_equal(morph.binary_erosion(_dev(seg, gpu), 2).cpu().numpy(), mu.erode(seg, 2))
    assert np.array_equal(morph.binary_dilation(_dev(seg, gpu), 3).cpu().numpy(), mu.dilate(seg, 3))
    with pytest.raises(amd._lib.Mi355Error, match="iterations"):
        morph.binary_erosion(_dev(seg, gpu), 0)
    with pytest.raises(amd._lib.Mi355Error, match="iterations"):
        morph.binary_dilation(_dev(seg, gpu), -1)


@pytest.mark.parametrize("inverted", [False, True])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_squared_edt_equals_scipy(amd, morph, gpu, name, inverted):
    mask = VOLUMES[name]()
    if inverted:
        mask = (mask == 0).astype(np.uint8)
    if not _has_background(mask):
        with pytest.raises(amd._lib.Mi355Error, match="no background"):
            morph.distance_transform_edt_sq(_dev(mask, gpu))
        return
    got = morph.distance_transform_edt_sq(_dev(mask, gpu)).cpu().numpy()
    want = mu.edt_sq(mask)
    assert got.dtype == np.int32 and got.shape == mask.shape
    assert np.array_equal(got, want), (name, inverted, int((got != want).sum()), int(np.abs(got.astype(np.int64) - want).max()))


def test_squared_edt_on_the_fixture_maps(amd, morph, gpu):
    for case in mu.load_fixture()["cases"]:
        seg, _ = mu.fixture_data(amd, case)
        if not seg.any():
            continue
        assert np.array_equal(morph.distance_transform_edt_sq(_dev(seg, gpu)).cpu().numpy(), mu.edt_sq(seg)), case["name"]
        inv = (seg == 0).astype(np.uint8)
        assert np.array_equal(morph.distance_transform_edt_sq(_dev(inv, gpu)).cpu().numpy(), mu.edt_sq(inv)), case["name"]


@pytest.mark.parametrize("shape,match", [((46342, 1, 1), "squared diagonal"), ((2, 1025, 2), "1024 entries"), ((2, 2, 1025), "1024 entries")])
def test_squared_edt_refuses_shapes_before_launching(amd, gpu, shape, match):
    mask = torch.zeros(shape, dtype=torch.uint8, device=gpu)  # all background: only the shape can be the reason
    out = torch.full(shape, -7, dtype=torch.int32, device=gpu)
    lib = amd._lib.load()
    rc = lib.mi355_edt_squared(mask.data_ptr(), shape[0], shape[1], shape[2], out.data_ptr(), torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and match in lib.mi355_last_error().decode()
    assert bool((out == -7).all()), "a refused call wrote to its output"


def test_squared_edt_without_background_writes_nothing(amd, morph, gpu):
    shape = (6, 7, 70)
    mask = torch.ones(shape, dtype=torch.uint8, device=gpu)
    out = torch.full(shape, -7, dtype=torch.int32, device=gpu)
    lib = amd._lib.load()
    rc = lib.mi355_edt_squared(mask.data_ptr(), shape[0], shape[1], shape[2], out.data_ptr(), torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and "no background" in lib.mi355_last_error().decode()
    assert bool((out == -7).all())
    # the longest lines the tile takes, and a first axis beyond them
    for shape in ((3, 1024, 5), (2, 3, 1024), (1500, 4, 3)):
        m = cu.noise(51, shape, 0.9)
        got = morph.distance_transform_edt_sq(_dev(m, gpu)).cpu().numpy()
        assert np.array_equal(got, mu.edt_sq(m)), shape


@pytest.mark.parametrize("name", list(VOLUMES))
def test_second_moments_equal_numpy(morph, gpu, name):
    mask = VOLUMES[name]()
    got = morph.second_moments(_dev(mask, gpu))
    assert got.dtype == np.int64 and np.array_equal(got, mu.second_moments(mask)), name


@pytest.mark.parametrize("integers", [True, False])
def test_masked_moments_equal_numpy(morph, gpu, integers):
    rs = np.random.RandomState(8)
    shape = (37, 41, 150)
    flags = (rs.randint(0, 256, shape) * (rs.random_sample(shape) < 0.3)).astype(np.uint8)
    flags[..., :40] &= 0x0F  # bits that are absent from whole chunks
    vols = rs.uniform(0, 4000, (4,) + shape)
    vols = (np.rint(vols) if integers else vols).astype(np.float32)
    got = morph.masked_moments(_dev(vols, gpu), _dev(flags, gpu))
    want = mu.masked_moments(vols, flags)
    assert got.shape == (8, 4, 3) and np.array_equal(got[:, :, 0], want[:, :, 0])
    err = np.abs(got[:, :, 1:] - want[:, :, 1:]) / want[:, :, 1:]
    print(f"masked moments ({'integer' if integers else 'fractional'} intensities): largest relative error {err.max():.3g}")
    assert err.max() <= RTOL
    if integers:  # integer sums below 2^53 are exact in any order
        assert np.array_equal(got, want)
    one = morph.masked_moments(_dev(vols[:1], gpu), _dev(np.zeros(shape, np.uint8), gpu))
    assert one.shape == (8, 1, 3) and not one.any()


def test_flag_helpers_build_the_region_map(amd, morph, gpu):
    for case in mu.load_fixture()["cases"]:
        if case["args"]["shape"] == [240, 240, 155]:
            continue  # (the end-to-end test covers it)
        seg, vols = mu.fixture_data(amd, case)
        got = morph.region_flags(_dev(seg, gpu), *(_dev(vols[c], gpu) for c in (morph.T1, morph.T2, morph.FLAIR))).cpu().numpy()
        assert np.array_equal(got, mu.flag_map(morph, seg, vols)), case["name"]
    flags = _dev(np.full((3, 4, 70), 0xFF, np.uint8), gpu)
    x = _dev(np.arange(840, dtype=np.float32).reshape(3, 4, 70), gpu)
    morph.flag_from_flags(flags, 7, require=0x01, x=x, lo=99.5, hi=float("inf"))  # strict comparisons, +inf allowed
    assert np.array_equal(flags.cpu().numpy().ravel() >> 7, (np.arange(840) > 99.5).astype(np.uint8))
    morph.flag_from_flags(flags, 7, x=x, lo=100.0, hi=102.0)
    assert np.flatnonzero(flags.cpu().numpy().ravel() >> 7).tolist() == [101]
    assert bool(((flags & 0x7F) == 0x7F).all()), "another bit changed"
    with pytest.raises(amd._lib.Mi355Error, match="NaN"):
        morph.flag_from_flags(flags, 7, x=x, lo=float("nan"))


@pytest.mark.parametrize("name", GRADIENT_VOLUMES)
def test_gradient_statistics_equal_the_numpy_restatement(morph, gpu, name):
    mask = VOLUMES[name]()
    surface = (mask != 0) & (mu.erode(mask) == 0)
    d2_in, d2_out = mu.edt_sq(mask), mu.edt_sq(mask == 0)
    n, mean, std = morph.surface_gradient_stats(_dev(d2_in, gpu), _dev(d2_out, gpu), _dev(surface.astype(np.uint8), gpu))
    wn, wmean, wstd = mu.gradient_stats(d2_in, d2_out, surface)
    print(f"{name}: n {n}, mean {mean!r} (numpy {wmean!r}), std {std!r} (numpy {wstd!r})")
    assert n == wn and n > 0
    assert abs(mean - wmean) <= RTOL * wmean and abs(std - wstd) <= RTOL * wstd
    # the select mask picks bits of a flag byte
    both = surface.astype(np.uint8) << 3 | 0x01
    assert morph.surface_gradient_stats(_dev(d2_in, gpu), _dev(d2_out, gpu), _dev(both, gpu), 1 << 3) == (n, mean, std)


def test_gradient_statistics_refusals_and_empty_surface(amd, morph, gpu):
    z = torch.zeros((4, 5, 70), dtype=torch.int32, device=gpu)
    assert morph.surface_gradient_stats(z, z, torch.zeros((4, 5, 70), dtype=torch.uint8, device=gpu)) == (0, 0.0, 0.0)
    flat = torch.zeros((1, 5, 70), dtype=torch.int32, device=gpu)
    with pytest.raises(amd._lib.Mi355Error, match="at least 2"):
        morph.surface_gradient_stats(flat, flat, torch.ones((1, 5, 70), dtype=torch.uint8, device=gpu))


def _run_case(amd, morph, gpu, case):
    seg, vols = mu.fixture_data(amd, case)
    return morph.tumor_morphology(_dev(seg, gpu), *(_dev(v, gpu) for v in vols), case["voxel_dims"])


def test_tumor_morphology_equals_the_reference(amd, morph, gpu):
    cmp = mu.Comparer()
    for case in mu.load_fixture()["cases"]:
        got = _run_case(amd, morph, gpu, case)
        assert tuple(got) == mu.SECTIONS
        cmp.same(got, case["expected"], case["name"])
    print(f"tumor_morphology: largest relative error of a float {cmp.worst:.3g} at {cmp.where}")


def test_repeated_calls_and_scratch_reuse(amd, morph, gpu):
    a = _dev(cu.noise(31, (40, 50, 130), 0.6), gpu)
    b = _dev(cu.noise(32, (9, 200, 70), 0.25), gpu)
    first = (morph.binary_erosion(a, 5), morph.binary_dilation(a, 5), morph.distance_transform_edt_sq(a), morph.second_moments(a))
    morph.binary_dilation(b, 10), morph.distance_transform_edt_sq(b)     # another shape on the same stream and scratch
    again = (morph.binary_erosion(a, 5), morph.binary_dilation(a, 5), morph.distance_transform_edt_sq(a), morph.second_moments(a))
    for x, y in zip(first[:3], again[:3]):
        assert torch.equal(x, y)
    assert np.array_equal(first[3], again[3])
    case = [c for c in mu.load_fixture()["cases"] if c["name"] == "noise20"][0]
    one, two = _run_case(amd, morph, gpu, case), _run_case(amd, morph, gpu, case)
    assert json.dumps(one, sort_keys=True) == json.dumps(two, sort_keys=True)  # every float bit for bit
    rs = np.random.RandomState(9)
    vols, flags = _dev(rs.uniform(0, 1, (4, 20, 30, 90)).astype(np.float32), gpu), _dev(rs.randint(0, 256, (20, 30, 90)).astype(np.uint8), gpu)
    assert np.array_equal(morph.masked_moments(vols, flags), morph.masked_moments(vols, flags))


@pytest.mark.parametrize("scheme,case_name", [("brats2021", "aniso"), ("brats2025", "eccentric")])
def test_morphology_command_writes_the_json(amd, gpu, tmp_path, scheme, case_name):
    case = [c for c in mu.load_fixture()["cases"] if c["name"] == case_name][0]
    seg, vols = mu.fixture_data(amd, case)
    zooms = tuple(case["voxel_dims"])
    case_id = "BraTS2021_00042" if scheme == "brats2021" else "BraTS-GLI-00042-000"
    names = ("_t1", "_t1ce", "_t2", "_flair") if scheme == "brats2021" else ("-t1n", "-t1c", "-t2w", "-t2f")
    case_dir = tmp_path / "some_folder"
    case_dir.mkdir()
    for v, suffix in zip(vols, names):
        amd.nifti.save_like(case_dir / f"{case_id}{suffix}.nii.gz", v.astype(np.int16), amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.int16))
    amd.nifti.save_like(tmp_path / "seg.nii.gz", seg, amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.uint8))
    out = tmp_path / "results" / "step4.json"
    env = dict(os.environ, PYTHONPATH=mu.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "brats_amd.morphology", "--input", str(case_dir), "--segmentation", str(tmp_path / "seg.nii.gz"),
                          "--output", str(out)], capture_output=True, text=True, env=env, cwd=mu.ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = json.loads(out.read_text())
    assert list(got) == ["case_id", "step", "voxel_info", *mu.SECTIONS]
    assert got["case_id"] == case_id and got["voxel_info"]["dimensions_mm"] == case["voxel_dims"]
    mu.Comparer().same({k: got[k] for k in mu.SECTIONS}, case["expected"], case_name)
