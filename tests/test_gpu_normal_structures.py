"""Normal-structures assessment (the reference's step 6) on the MI355X: the kernels of csrc/normal_structures.hip and the
18-neighbour labelling against scipy and numpy, off the cube and at the smallest shapes where they can still go wrong, and the
dicts against what the reference's step 6 returned or raised (tests/golden/normal_structures.json; every value exactly).  The child
processes this file starts run under a time limit of their own; nothing is retried."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
from scipy import ndimage

import components_util as cu
import normal_structures_util as nu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ns(amd):
    return nu.module("normal_structures")


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)  # (a copy: the cached arrays are read-only)


# ---- city-block distance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(nu.cityblock_cases()))
def test_cityblock_distance_is_scipy_bit_for_bit(ns, gpu, name):
    mask = nu.cityblock_cases()[name]
    fg = mask != 0
    m = _dev(mask, gpu)
    to_fg, to_bg = ns.cityblock_distance(m, True).cpu().numpy(), ns.cityblock_distance(m, False).cpu().numpy()
    assert to_fg.dtype == np.int32 and to_bg.dtype == np.int32 and to_fg.shape == mask.shape
    want = nu.scipy_taxicab(mask, True)  # distance_transform_cdt(metric='taxicab'); None: no foreground to measure to
    if want is None:
        far = nu.module("volume_ops").CITYBLOCK_FAR
        assert np.all(to_fg == far) and far == nu.FAR >= 2 ** 30
    else:
        assert np.array_equal(to_fg, want), (name, int((to_fg != want).sum()))
        assert np.all(to_fg[fg] == 0)
    assert np.array_equal(to_bg, nu.scipy_taxicab(mask, False)), name  # on a copy zero-padded by one
    for n in nu.ITERATIONS:
        assert np.array_equal(to_fg <= n, ndimage.binary_dilation(fg, iterations=n)), (name, n)
        assert np.array_equal(to_bg > n, ndimage.binary_erosion(fg, iterations=n)), (name, n)
    if name.startswith("all foreground"):
        d = np.indices(mask.shape)
        assert np.array_equal(to_bg, np.min([np.minimum(d[k], mask.shape[k] - 1 - d[k]) for k in range(3)], axis=0) + 1)  # distances to the faces only


def test_cityblock_distance_refuses_what_it_cannot_hold(ns, amd, gpu):
    with pytest.raises(amd._lib.Mi355Error, match="axis 2"):
        ns.cityblock_distance(torch.zeros((1, 1, 16384), dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match="uint8"):
        ns.cityblock_distance(torch.zeros((2, 2, 2), dtype=torch.int32, device=gpu))
    line = np.zeros((1, 1, 16383), np.uint8)  # the longest line: one workgroup, one line in LDS
    line[0, 0, 5] = 1
    got = ns.cityblock_distance(_dev(line, gpu)).cpu().numpy()
    assert np.array_equal(got[0, 0], np.abs(np.arange(16383) - 5))


# ---- 18-neighbour labels ----------------------------------------------------------------------------------------------
def _labels(amd, gpu, mask, neighbours):
    labels, n = amd.components.label_components_neighbours(_dev(mask, gpu), neighbours)
    return labels.cpu().numpy(), n


@pytest.mark.parametrize("p", [0.05, 0.2, 0.31, 0.5])
def test_labels_with_18_neighbours_equal_scipy(amd, gpu, p):
    mask = cu.noise(int(p * 100), (23, 41, 150), p)
    for neighbours, connectivity in ((18, 2), (6, 1), (26, 3)):
        want, n_want = cu.scipy_labels(mask, connectivity)
        got, n = _labels(amd, gpu, mask, neighbours)
        print(f"noise {p}, {neighbours} neighbours: {n} components (scipy {n_want}), {int((got != want).sum())} voxels differ")
        assert n == n_want and got.dtype == np.int32 and np.array_equal(got, want), (p, neighbours)
    assert cu.scipy_labels(mask, 1)[1] > cu.scipy_labels(mask, 2)[1] > cu.scipy_labels(mask, 3)[1]  # the three really differ here


@pytest.mark.parametrize("name,shape,a,b,kind", nu.seam_pairs(), ids=[p[0] for p in nu.seam_pairs()])
def test_edge_and_corner_pairs_across_every_brick_seam(amd, gpu, name, shape, a, b, kind):
    mask = np.zeros(shape, np.uint8)
    mask[a] = mask[b] = 1
    counts = [_labels(amd, gpu, mask, neighbours)[1] for neighbours in (6, 18, 26)]
    assert counts == ([2, 1, 1] if kind == "edge" else [2, 2, 1]), (name, counts)
    mirrored = np.ascontiguousarray(mask[:, ::-1, :])  # the other diagonal of the same seam
    assert [_labels(amd, gpu, mirrored, neighbours)[1] for neighbours in (6, 18, 26)] == counts, name


def test_bad_neighbour_counts_are_refused_and_the_old_entry_point_is_unchanged(amd, gpu):
    mask = torch.ones((4, 4, 4), dtype=torch.uint8, device=gpu)
    for neighbours in (0, 2, 3, 27):
        with pytest.raises(amd._lib.Mi355Error, match="neighbours"):
            amd.components.label_components_neighbours(mask, neighbours)
    assert amd.components.label_components_neighbours(mask, 18)[1] == 1
    with pytest.raises(amd._lib.Mi355Error, match="connectivity 2"):
        amd.components.label_components(mask, 2)


# ---- int32 order statistics -------------------------------------------------------------------------------------------
QS = (0, 5, 40, 50, 60, 75, 99.9, 100)


@pytest.mark.parametrize("n", [1, 2, 5, 4097])
def test_order_statistics_equal_a_sort(ns, gpu, n):
    rs = np.random.RandomState(n)
    for name, values in (("spread", rs.randint(0, 2 ** 31 - 1, n)), ("ties", rs.randint(0, 3, n) * 70000), ("ends", rs.choice([0, 2 ** 31 - 1, 12345], n))):
        values = values.astype(np.int32)
        if name == "ends" and n >= 2:
            values[0], values[-1] = 0, 2 ** 31 - 1
        got = ns.masked_order_stats_i32(_dev(values, gpu), QS)  # 8 percentiles in one call
        want = nu.order_stats(values, QS)
        assert got[0] == want[0] == n and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (name, n, got, want)
        assert got[1].dtype == np.int32


def test_order_statistics_with_flags_and_refusals(ns, amd, gpu):
    rs = np.random.RandomState(9)
    shape = (9, 10, 47)
    values = (rs.randint(0, 50, shape) ** 2).astype(np.int32)  # squared distances: heavy ties
    flags = rs.randint(0, 8, shape).astype(np.uint8)
    for require, forbid in ((1, 0), (1, 4), (3, 4), (0, 7), (0, 0)):
        got = ns.masked_order_stats_i32(_dev(values, gpu), (60, 40), _dev(flags, gpu), require, forbid)
        want = nu.order_stats(values[nu.selected(flags, require, forbid)], (60, 40))
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (require, forbid)
    got = ns.masked_order_stats_i32(_dev(values, gpu), (60, 40), _dev(flags, gpu), 8, 0)  # bit 3 is never set: nothing selected
    assert got[0] == 0 and not got[1].any() and not got[2].any()
    values[3, 3, 3] = -1
    with pytest.raises(amd._lib.Mi355Error, match="negative"):
        ns.masked_order_stats_i32(_dev(values, gpu), 50)
    assert ns.masked_order_stats_i32(_dev(values, gpu), 50, _dev((values >= 0).astype(np.uint8), gpu), 1)[0] == values.size - 1
    with pytest.raises(amd._lib.Mi355Error, match="percentiles"):
        ns.masked_order_stats_i32(_dev(np.abs(values), gpu), list(range(9)))


# ---- flag predicates and the column maximum ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", nu.FLAG_SHAPES)
def test_flag_from_i32_equals_numpy(ns, gpu, shape):
    rs = np.random.RandomState(shape[2])
    values = rs.randint(-3, 12, shape).astype(np.int32)
    values.reshape(-1)[:2] = (-2 ** 31, 2 ** 31 - 1)
    flags = rs.randint(0, 256, shape).astype(np.uint8)
    for bit, lo, hi, require, forbid in ((7, 0, 5, 0, 0), (0, 6, 2 ** 31 - 1, 2, 0), (3, -2 ** 31, 4, 8, 1), (2, 3, 3, 0, 4), (5, 4, 2, 0, 0), (1, 0, 10, 6, 48)):
        got = ns.flag_from_i32(_dev(flags, gpu), bit, _dev(values, gpu), lo, hi, require, forbid).cpu().numpy()
        assert np.array_equal(got, nu.flag_i32(flags, bit, values, lo, hi, require, forbid)), (shape, bit, lo, hi)
    f, v = _dev(flags, gpu).reshape(-1), _dev(values, gpu).reshape(-1)
    for cut in (1, 2, 3):  # pointers off the 4- and 16-byte grid, a length that is no multiple of 4
        got = ns.flag_from_i32(f[cut:].clone(), 4, v[cut:], 0, 5).cpu().numpy()   # (the clone starts on the grid again, the values do not)
        assert np.array_equal(got, nu.flag_i32(flags.reshape(-1)[cut:], 4, values.reshape(-1)[cut:], 0, 5, 0, 0)), cut
        part = f.clone()[cut:]
        got = ns.flag_from_i32(part, 4, v[cut:].clone(), 0, 5).cpu().numpy()      # (and the other way round)
        assert np.array_equal(got, nu.flag_i32(flags.reshape(-1)[cut:], 4, values.reshape(-1)[cut:], 0, 5, 0, 0)), cut
    assert np.array_equal(ns.flag_from_i32(_dev(flags, gpu), 6, _dev(values, gpu), 2 ** 40, 2 ** 41).cpu().numpy(), flags & ~np.uint8(64))  # clamped: empty


@pytest.mark.parametrize("shape", nu.FLAG_SHAPES)
def test_flag_from_box_equals_numpy(ns, gpu, shape):
    rs = np.random.RandomState(shape[0])
    flags = rs.randint(0, 256, shape).astype(np.uint8)
    d0, d1, d2 = shape
    boxes = [(0, d0, 0, d1, 0, d2 // 3), (0, d0, 0, d1, 0, d2), (0, 1, 0, d1, 0, d2), (d0 - 1, d0, 0, d1, 0, d2), (0, d0, 0, 1, 0, d2), (0, d0, d1 - 1, d1, 0, d2),
             (0, d0, 0, d1, 0, 1), (0, d0, 0, d1, d2 - 1, d2), (-3, d0 + 3, -1, d1 + 9, -2, d2 + 1), (2, 5, 3, 7, 1, 3), (3, 3, 0, d1, 0, d2), (4, 2, 0, d1, 0, d2),
             (0, d0, 0, d1, d2, d2 + 5), (-5, 0, 0, d1, 0, d2)]
    for k, box in enumerate(boxes):
        bit, require, forbid = k % 8, (0, 1, 6)[k % 3], (0, 8, 0, 16)[k % 4]
        got = ns.flag_from_box(_dev(flags, gpu), bit, box, require, forbid).cpu().numpy()
        assert np.array_equal(got, nu.flag_box(flags, bit, box, require, forbid)), (shape, box)


@pytest.mark.parametrize("shape", nu.FLAG_SHAPES)
def test_column_count_max_equals_numpy(ns, amd, gpu, shape):
    rs = np.random.RandomState(shape[1])
    flags = rs.randint(0, 4, shape).astype(np.uint8)
    d1 = shape[1]
    for i1_from in (0, 1, d1 // 2, d1 - 1, d1, d1 + 3):
        for require, forbid in ((1, 0), (1, 2), (0, 3), (3, 0)):
            got = ns.column_count_max(_dev(flags, gpu), i1_from, require, forbid)
            assert got == nu.column_count_max(flags, i1_from, require, forbid), (shape, i1_from, require, forbid)
    assert ns.column_count_max(torch.full(shape, 5, dtype=torch.uint8, device=gpu), 0, 4) == shape[0]
    assert ns.column_count_max(torch.zeros(shape, dtype=torch.uint8, device=gpu), 0, 1) == 0
    with pytest.raises(amd._lib.Mi355Error, match="i1_from"):
        ns.column_count_max(_dev(flags, gpu), -1, 1)


# ---- end to end -------------------------------------------------------------------------------------------------------
def _run_case(ns, gpu, case):
    seg, vols = nu.fixture_data(case)
    return ns.normal_structures(_dev(seg, gpu), *(_dev(v, gpu) for v in vols), case["voxel_dims"])


def _timed(fn, repeats=5):
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best * 1e3


def test_normal_structures_equal_the_reference(ns, amd, gpu):
    raised = 0
    for case in nu.load_fixture()["cases"]:
        if case["args"]["shape"] == [240, 240, 155]:
            seg, vols = nu.fixture_data(case)
            dev = [_dev(seg, gpu)] + [_dev(v, gpu) for v in vols]
            ns.normal_structures(*dev, case["voxel_dims"])  # warm: scratch buffers at their final size
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nu.check_case(ns, case, lambda: ns.normal_structures(*dev, case["voxel_dims"]))
            print(f"normal_structures, 240 x 240 x 155, warm: {(time.perf_counter() - t0) * 1e3:.1f} ms wall")
            # the tumour's two dilations: one city-block transform against 10 + 5 steps of the existing erosion / dilation kernel
            both = _timed(lambda: ns.cityblock_distance(dev[0]))
            steps = _timed(lambda: (amd.morphology.binary_dilation(dev[0], 10), amd.morphology.binary_dilation(dev[0], 5)))
            print(f"tumour at 240 x 240 x 155, best of 5 warm wall times: cityblock_distance {both:.3f} ms, binary_dilation(10) + binary_dilation(5) {steps:.3f} ms")
            dist = ns.cityblock_distance(dev[0]).cpu().numpy()
            for n in (5, 10):
                assert np.array_equal(dist <= n, amd.morphology.binary_dilation(dev[0], n).cpu().numpy() != 0), n
        else:
            raised += nu.check_case(ns, case, lambda: _run_case(ns, gpu, case)) is None
    assert raised == 2


def test_repeats_are_bit_equal_and_bad_inputs_are_refused(ns, gpu):
    case = nu.case("marked_right_communicating")
    one, two = _run_case(ns, gpu, case), _run_case(ns, gpu, case)
    assert json.dumps(one) == json.dumps(two)  # every float bit for bit, every key in the same place
    seg, vols = nu.fixture_data(case)
    bad = seg.copy()
    bad[0, 0, 0] = 5
    with pytest.raises(ValueError, match="above 4"):
        ns.normal_structures(_dev(bad, gpu), *(_dev(v, gpu) for v in vols), case["voxel_dims"])
    with pytest.raises(ValueError, match="differ in shape"):
        ns.normal_structures(_dev(seg, gpu), *(_dev(v[:-1], gpu) for v in vols), case["voxel_dims"])
    with pytest.raises(ValueError, match="float32"):
        ns.normal_structures(_dev(seg, gpu), *(_dev(v.astype(np.float64), gpu) for v in vols), case["voxel_dims"])
    chans = [_dev(v, gpu) for v in vols]
    chans[0] = torch.full_like(chans[0], 7.0)  # a plateau: no voxel exceeds the 5th percentile
    with pytest.raises(ValueError, match="brain mask .* is empty"):
        ns.normal_structures(_dev(seg, gpu), *chans, case["voxel_dims"])


def test_too_many_components_are_refused_with_their_count(ns, gpu, monkeypatch):
    case = nu.case("mild_symmetric")
    seg, vols = nu.fixture_data(case)
    monkeypatch.setattr(nu.module("components"), "MAX_COMPONENTS", 0)
    with pytest.raises(ValueError, match="falls into 1 components"):
        ns.normal_structures(_dev(seg, gpu), *(_dev(v, gpu) for v in vols), case["voxel_dims"])


@pytest.mark.parametrize("scheme,case_name", [("brats2021", "moderate_left_adjacent"), ("brats2025", "edge_joined_pair")])
def test_normal_structures_command_writes_the_json(amd, gpu, tmp_path, scheme, case_name):
    case = nu.case(case_name)
    seg, vols = nu.fixture_data(case)
    zooms = tuple(case["voxel_dims"])
    case_id = "BraTS2021_00042" if scheme == "brats2021" else "BraTS-GLI-00042-000"
    names = ("_t1", "_t1ce", "_t2", "_flair") if scheme == "brats2021" else ("-t1n", "-t1c", "-t2w", "-t2f")
    case_dir = tmp_path / "some_folder"
    case_dir.mkdir()
    for v, suffix in zip(vols, names):
        amd.nifti.save_like(case_dir / f"{case_id}{suffix}.nii.gz", v.astype(np.int16), amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.int16))
    amd.nifti.save_like(tmp_path / "seg.nii.gz", seg, amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.uint8))
    out = tmp_path / "results" / "step6.json"
    env = dict(os.environ, PYTHONPATH=nu.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "brats_amd.normal_structures", "--input", str(case_dir), "--segmentation", str(tmp_path / "seg.nii.gz"),
                          "--output", str(out)], capture_output=True, text=True, env=env, cwd=nu.ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert len(res.stdout.strip().splitlines()) == 1 and res.stdout.startswith(case_id + ": "), res.stdout
    got = json.loads(out.read_text())
    assert list(got) == ["case_id", "step", *nu.SECTIONS]
    assert got["case_id"] == case_id and got["step"] == "Step 6 - Normal structures assessment"
    nu.compare({k: got[k] for k in nu.SECTIONS}, case["expected"], case_name)
