"""Lesion-wise scoring on the MI355X (csrc/lesionwise.hip, brats_amd.evaluate.lesionwise_*): the 6- / 18- / 26-neighbour morphology
bit-equal to scipy on the in-LDS path and on the multi-launch path, the joint histogram of two label maps equal to np.add.at on its LDS
and its global path, the table lookup in both widths, every refusal with its message and an untouched output, and lesionwise_metrics
end to end against the scipy restatement of lesionwise_util.py: every integer exact, hd95 and both aggregates within the 1e-12 relative
that test_gpu_surface_distance.py reasons for the fp64 distance map.  The end-to-end tests print the largest relative difference seen.
The child processes this file starts run under a time limit of their own; nothing is retried."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

import lesionwise_util as lu
import surface_distance_util as su

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRICK = (8, 16, 64)     # MI355_MORPH_NB_BRICK0 / 1 / 2
LDS_STEPS = 4           # MI355_MORPH_NB_LDS_STEPS
PAIR_CHUNK = 16384      # voxels per workgroup of the histogram (PC_CHUNK in lesionwise.hip)
LDS_BINS = 8192         # MI355_PAIR_LDS_BINS
TABLE_MAX = 1 << 20     # MI355_PAIR_TABLE_MAX
U8P, I32P, I64P = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _stream(gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


def _err(lib):
    return lib.mi355_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- morphology
# the last shape spans several bricks of 8 x 16 x 64 along every axis with a ragged tail: 2 bricks + 3, 2 bricks + 5, 2 bricks + 7
MORPH_SHAPES = [(1, 1, 1), (1, 1, 301), (301, 1, 1), (5, 9, 70), (13, 3, 65), (7, 17, 130), (2 * BRICK[0] + 3, 2 * BRICK[1] + 5, 2 * BRICK[2] + 7)]


def morph_nb(amd, gpu, mask, dilate, neighbours, iterations, with_tmp=True):
    """-> (rc, out as left on the device); out and tmp hold 0xA5 on entry"""
    lib = amd._lib.load()
    dm = _dev(mask, gpu)
    out = torch.full(mask.shape, 0xA5, dtype=torch.uint8, device=gpu)
    tmp = torch.full(mask.shape, 0xA5, dtype=torch.uint8, device=gpu) if with_tmp else None
    rc = lib.mi355_binary_morphology_nb(dm.data_ptr(), *mask.shape, int(dilate), neighbours, iterations, out.data_ptr(),
                                        None if tmp is None else tmp.data_ptr(), 0 if tmp is None else tmp.numel(), _stream(gpu))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def morph_inputs(shape):
    rs = np.random.RandomState(11)
    field = ndimage.gaussian_filter(rs.standard_normal(shape), 1.5, mode="nearest")
    blobs = (field > np.quantile(field, 0.6)).astype(np.uint8) * 7 if field.size > 1 else np.full(shape, 9, np.uint8)   # foreground = nonzero
    corner, centre = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    corner[0, 0, 0] = 1
    centre[tuple(s // 2 for s in shape)] = 255
    return {"blobs": blobs, "ones": np.ones(shape, np.uint8), "zeros": np.zeros(shape, np.uint8), "corner": corner, "centre": centre}


@pytest.mark.parametrize("neighbours", [6, 18, 26])
@pytest.mark.parametrize("shape", MORPH_SHAPES)
def test_morphology_equals_scipy(amd, gpu, shape, neighbours):
    iterations = [1, 3, min(shape) + 1]            # the last one is larger than the shortest axis
    if shape == MORPH_SHAPES[-1]:
        iterations += [LDS_STEPS, LDS_STEPS + 1, 2 * LDS_STEPS + 1]   # the most one launch takes, then two launches, then three
    assert any(k > LDS_STEPS for k in iterations) == (min(shape) >= LDS_STEPS), "shapes with a short axis stay on one launch"
    for name, mask in morph_inputs(shape).items():
        for dilate in (True, False):
            for k in iterations:
                rc, got = morph_nb(amd, gpu, mask, dilate, neighbours, k, with_tmp=k > LDS_STEPS)   # one launch needs no second buffer
                assert rc == 0, _err(amd._lib.load())
                want = lu.morph(mask, dilate, neighbours, k)
                assert np.array_equal(got, want), (shape, neighbours, name, dilate, k, int((got != want).sum()))


def test_a_seed_grows_into_the_263_voxels_of_three_18_neighbour_steps(amd, gpu):
    shape = MORPH_SHAPES[-1]
    mask = morph_inputs(shape)["centre"]
    for k, count in ((1, 19), (2, 93), (3, 263), (4, 569)):
        rc, got = morph_nb(amd, gpu, mask, True, 18, k)
        assert rc == 0 and int(got.sum()) == count and set(np.unique(got)) == {0, 1}
    rc, got = morph_nb(amd, gpu, morph_inputs(shape)["corner"], True, 18, 3)
    g = np.indices(shape)
    assert rc == 0 and np.array_equal(got != 0, (g.max(axis=0) <= 3) & (g.sum(axis=0) <= 6)), "outside the volume nothing carries the dilation on"


@pytest.mark.parametrize("shape", [(5, 9, 70), MORPH_SHAPES[-1]])
def test_six_neighbours_equal_the_existing_cross_morphology(amd, gpu, shape):
    vo = amd.volume_ops
    mask = _dev(morph_inputs(shape)["blobs"], gpu)
    for k in (1, 3, 6):
        assert torch.equal(vo.binary_dilation_nb(mask, 6, k), vo.binary_dilation(mask, k))
        assert torch.equal(vo.binary_erosion_nb(mask, 6, k), vo.binary_erosion(mask, k))
    for nb in (18, 26):
        assert np.array_equal(vo.binary_dilation_nb(mask, nb, 5).cpu().numpy(), lu.morph(mask.cpu().numpy(), True, nb, 5))
        assert np.array_equal(vo.binary_erosion_nb(mask, nb).cpu().numpy(), lu.morph(mask.cpu().numpy(), False, nb, 1))


def test_morphology_refuses_bad_calls(amd, gpu):
    lib = amd._lib.load()
    mask = np.ones((3, 4, 5), np.uint8)
    for neighbours, k, with_tmp, match in ((7, 1, True, "neighbours"), (18, 0, True, "iterations"), (18, LDS_STEPS + 1, False, "second buffer")):
        rc, out = morph_nb(amd, gpu, mask, True, neighbours, k, with_tmp)
        assert rc == -1 and match in _err(lib) and (out == 0xA5).all(), (neighbours, k)
    dm = _dev(mask, gpu)
    out = torch.full(mask.shape, 0xA5, dtype=torch.uint8, device=gpu)
    tmp = torch.full(mask.shape, 0xA5, dtype=torch.uint8, device=gpu)
    calls = ((dm.data_ptr(), dm.data_ptr(), tmp.data_ptr(), 60, 1, "aliased"), (dm.data_ptr(), out.data_ptr(), tmp.data_ptr(), 59, 5, "needs 60"),
             (dm.data_ptr(), out.data_ptr(), out.data_ptr(), 60, 5, "second buffer"))
    for src, dst, scratch, nbytes, k, match in calls:
        rc = lib.mi355_binary_morphology_nb(src, 3, 4, 5, 1, 18, k, dst, scratch, nbytes, _stream(gpu))
        torch.cuda.synchronize()
        assert rc == -1 and match in _err(lib), match
    assert bool((out == 0xA5).all()) and bool((tmp == 0xA5).all()), "a refused call wrote to a buffer"


# ---------------------------------------------------------------------------------------------------------------- joint histogram
def pair_counts(amd, gpu, a, n_a, b, n_b, words=None, fill=-1):
    """-> (rc, counts as left on the host); the device table holds `fill` words on entry, the host array -7"""
    lib = amd._lib.load()
    entries = (n_a + 1) * (n_b + 1)
    words = entries + 1 if words is None else words
    table = torch.full((max(words, 1),), fill, dtype=torch.int64, device=gpu)
    counts = np.full(min(entries, TABLE_MAX + 4096), -7, dtype=np.int64)
    da, db = _dev(a, gpu), _dev(b, gpu)
    rc = lib.mi355_label_pair_counts(da.data_ptr(), n_a, db.data_ptr(), n_b, a.size, table.data_ptr(), words, counts.ctypes.data_as(I64P), _stream(gpu))
    torch.cuda.synchronize()
    return rc, counts


def label_patterns(n_a, n_b, V):
    rs = np.random.RandomState(5)
    entries = (n_a + 1) * (n_b + 1)
    uniform = (rs.randint(0, n_a + 1, V).astype(np.int32), rs.randint(0, n_b + 1, V).astype(np.int32))
    a, b = np.full(V, n_a, np.int32), np.full(V, n_b // 2, np.int32)      # one pair holds almost every voxel
    a[::997], b[::991] = 0, n_b
    keys = (np.arange(V, dtype=np.int64) * 7919 + 13) % entries if entries < V else rs.permutation(entries)[:V]   # every voxel another pair where the table allows it
    distinct = ((keys // (n_b + 1)).astype(np.int32), (keys % (n_b + 1)).astype(np.int32))
    return {"uniform": uniform, "one_pair": (a, b), "distinct": distinct}


# (3, 700) and (90, 89) are counted in LDS, (90, 90) is the first table past its bins, (1023, 1023) is the cap itself
@pytest.mark.parametrize("n_a,n_b", [(0, 0), (1, 1), (3, 700), (90, 89), (90, 90), (900, 900), (1023, 1023)])
def test_pair_counts_equal_numpy(amd, gpu, n_a, n_b):
    entries = (n_a + 1) * (n_b + 1)
    assert entries <= TABLE_MAX and ((n_a, n_b) not in ((3, 700), (90, 89)) or entries <= LDS_BINS) and ((n_a, n_b) != (90, 90) or entries > LDS_BINS)
    for V in (PAIR_CHUNK + 777, 5000):             # one chunk and a tail; a single partial chunk
        for name, (a, b) in label_patterns(n_a, n_b, V).items():
            if name == "distinct" and entries >= V:
                assert len(np.unique(a.astype(np.int64) * (n_b + 1) + b)) == V
            want = lu.pair_table(a, n_a, b, n_b)
            for fill in (-1, 0):
                rc, got = pair_counts(amd, gpu, a, n_a, b, n_b, fill=fill)
                assert rc == 0, _err(amd._lib.load())
                assert np.array_equal(got.reshape(n_a + 1, n_b + 1), want) and int(got.sum()) == V, (n_a, n_b, V, name)


def test_pair_counts_refusals_write_nothing(amd, gpu):
    lib = amd._lib.load()
    a, b = np.zeros(5000, np.int32), np.zeros(5000, np.int32)
    rc, got = pair_counts(amd, gpu, a, 1024, b, 1023, words=8)
    assert rc == -1 and "1024 and 1023 labels" in _err(lib) and str(1025 * 1024) in _err(lib) and (got == -7).all()
    rc, got = pair_counts(amd, gpu, a, 3, b, 4, words=20)
    assert rc == -1 and "needs 21" in _err(lib) and (got == -7).all()
    for n_a, n_b in ((3, 4), (200, 200)):          # the LDS path and the global path
        for bad_a, bad_b in ((n_a + 1, 0), (0, n_b + 1), (-1, 0), (0, 2 ** 31 - 1)):
            a2, b2 = a.copy(), b.copy()
            a2[4321], b2[4321] = bad_a, bad_b
            rc, got = pair_counts(amd, gpu, a2, n_a, b2, n_b)
            assert rc == -1 and "1 voxels carry a label outside" in _err(lib) and (got == -7).all(), (n_a, n_b, bad_a, bad_b)
    with pytest.raises(ValueError, match="1024 components in the first map and 1023 in the second"):
        amd.components.pair_counts(_dev(a.reshape(10, 20, 25), gpu), 1024, _dev(b.reshape(10, 20, 25), gpu), 1023)
    got = amd.components.pair_counts(_dev(a.reshape(10, 20, 25), gpu), 2, _dev(b.reshape(10, 20, 25), gpu), 1)
    assert got.dtype == np.int64 and got.shape == (3, 2) and got[0, 0] == 5000 and got.sum() == 5000


# ---------------------------------------------------------------------------------------------------------------- lookup
@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_lookup_equals_numpy_and_refuses_a_label_out_of_range(amd, gpu, dtype):
    lib = amd._lib.load()
    rs = np.random.RandomState(9)
    n, shape = 300, (7, 17, 130)
    labels = rs.randint(0, n + 1, shape).astype(np.int32)
    labels[0, 0, :3] = (0, n, 0)
    table = rs.randint(1, 250, n + 1).astype(dtype) if dtype == np.uint8 else rs.randint(-2 ** 31, 2 ** 31 - 1, n + 1).astype(np.int32)
    assert table[0] != 0
    got = amd.components.lookup(_dev(labels, gpu), n, table)
    assert got.dtype == (torch.uint8 if dtype == np.uint8 else torch.int32) and np.array_equal(got.cpu().numpy(), table[labels])
    zero = amd.components.lookup(_dev(np.zeros((1, 1, 1), np.int32), gpu), 0, table[:1])
    assert zero.cpu().numpy().tolist() == [[[int(table[0])]]]
    # raw calls: a label one past n, a negative one, a short work buffer - refused, the poisoned output untouched
    fn, ptr = (lib.mi355_label_lookup, U8P) if dtype == np.uint8 else (lib.mi355_label_lookup_i32, I32P)
    out = torch.full(shape, 0x5A, dtype=torch.uint8 if dtype == np.uint8 else torch.int32, device=gpu)
    work = torch.zeros(16 + table.nbytes, dtype=torch.uint8, device=gpu)
    for bad in (n + 1, -1):
        wrong = labels.copy()
        wrong[3, 9, 77] = bad
        dl = _dev(wrong, gpu)
        rc = fn(dl.data_ptr(), wrong.size, n, table.ctypes.data_as(ptr), work.data_ptr(), work.numel(), out.data_ptr(), _stream(gpu))
        torch.cuda.synchronize()
        assert rc == -1 and f"1 voxels carry a label outside 0..{n}" in _err(lib) and bool((out == 0x5A).all())
    dl = _dev(labels, gpu)
    rc = fn(dl.data_ptr(), labels.size, n, table.ctypes.data_as(ptr), work.data_ptr(), work.numel() - 1, out.data_ptr(), _stream(gpu))
    torch.cuda.synchronize()
    assert rc == -1 and "working memory" in _err(lib) and bool((out == 0x5A).all())
    rc = fn(dl.data_ptr(), labels.size, n, table.ctypes.data_as(ptr), work.data_ptr(), work.numel(), out.data_ptr(), _stream(gpu))
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(out.cpu().numpy(), table[labels])
    with pytest.raises(ValueError, match="table"):
        amd.components.lookup(dl, n, table[:-1])
    with pytest.raises(ValueError, match="table"):
        amd.components.lookup(dl, n, table.astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------- end to end
SPACINGS = ((1.0, 1.0, 1.0), (1.5, 1.0, 0.8))


def same_case(got, want, what):
    assert list(got) == list(want)
    return max(lu.same(got[name], want[name], (what, name)) for name in want)


@functools.lru_cache(maxsize=None)
def scene_oracle(spacing):
    return lu.case_lesionwise(*lu.scene_labels(), spacing)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_the_scene_end_to_end(amd, gpu, spacing):
    pred, gt = lu.scene_labels()
    want = scene_oracle(spacing)
    assert [r["pred_components"] for r in want["WT"]["lesions"]] == [[1], [2], [2, 3], []] and want["WT"]["fp_components"] == [{"id": 4, "voxels": 27}]
    got = amd.evaluate.lesionwise_metrics(_dev(pred, gpu), _dev(gt, gpu), spacing)
    worst = same_case(got, want, spacing)
    print(f"scene spacing {spacing}: worst relative difference {worst:.3g}")
    assert got["WT"]["lesionwise_dice"] == 0.1901620623466239
    again = amd.evaluate.lesionwise_metrics(_dev(pred, gpu), _dev(gt, gpu), spacing)
    assert again == got, "two runs are bit-equal"
    merged = amd.evaluate.evaluate_lesionwise(_dev(pred, gpu), _dev(gt, gpu), spacing)
    base = amd.evaluate.evaluate_with_surfaces(_dev(pred, gpu), _dev(gt, gpu), spacing)
    for key in base:
        if key in su.REGIONS:
            assert merged[key]["lesionwise"] == got[key] and {k: v for k, v in merged[key].items() if k != "lesionwise"} == base[key]
        else:
            assert merged[key] == base[key]
    # other parameters reach the device path and the host arithmetic alike
    kw = dict(dilation=1, min_volume_mm3=20.0, penalty_mm=100.0)
    same_case(amd.evaluate.lesionwise_metrics(_dev(pred, gpu), _dev(gt, gpu), spacing, regions={"all": (3,)}, **kw),
              lu.case_lesionwise(pred, gt, spacing, regions={"all": (3,)}, **kw), "dilation 1")


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", [(33, 17, 29), (40, 48, 56)])
def test_smooth_label_maps_end_to_end(amd, gpu, shape, spacing):
    pred, gt = lu.noise_pair(2, shape)
    want = lu.case_lesionwise(pred, gt, spacing)
    assert any(r["num_lesions"] >= 2 for r in want.values()) and any(r["num_fp"] >= 1 for r in want.values()) and any(r["num_fn"] >= 1 for r in want.values()), \
        "the seed no longer gives two lesions, a false positive and a false negative: the comparison would be vacuous"
    got = amd.evaluate.lesionwise_metrics(_dev(pred, gpu), _dev(gt, gpu), spacing)
    worst = same_case(got, want, (shape, spacing))
    print(f"smooth maps {shape} spacing {spacing}: worst relative difference {worst:.3g}")
    assert amd.evaluate.lesionwise_metrics(_dev(pred, gpu), _dev(gt, gpu), spacing) == got, "two runs are bit-equal"


def test_empty_maps_and_an_absent_region(amd, gpu):
    pred, gt = lu.noise_pair(2, (33, 17, 29))
    zeros = np.zeros_like(pred)
    spacing = (1.5, 1.0, 0.8)
    for what, p, g in (("empty prediction", zeros, gt), ("empty ground truth", pred, zeros), ("both empty", zeros, zeros)):
        got = amd.evaluate.lesionwise_metrics(_dev(p, gpu), _dev(g, gpu), spacing)
        same_case(got, lu.case_lesionwise(p, g, spacing), what)
        for m in got.values():
            if what == "empty prediction":
                assert m["num_fp"] == 0 and m["num_tp"] == 0 and all(r["hd95"] == 374.0 and r["dice"] == 0.0 for r in m["lesions"])
                assert m["lesionwise_dice"] == (0.0 if m["num_counted"] else 1.0)
            elif what == "empty ground truth":
                assert m["num_lesions"] == 0 and m["num_fp"] > 0 and m["lesionwise_dice"] == 0.0 and m["lesionwise_hd95"] == 374.0
            else:
                assert (m["num_lesions"], m["num_fp"], m["lesionwise_dice"], m["lesionwise_hd95"]) == (0, 0, 1.0, 0.0)
    # label 2 only: TC and ET are absent from both maps, WT is there
    p2, g2 = (pred > 0).astype(np.uint8) * 2, (gt > 0).astype(np.uint8) * 2
    got = amd.evaluate.lesionwise_metrics(_dev(p2, gpu), _dev(g2, gpu), spacing)
    same_case(got, lu.case_lesionwise(p2, g2, spacing), "label 2 only")
    assert got["WT"]["num_lesions"] >= 1 and got["TC"]["num_lesions"] == got["ET"]["num_lesions"] == 0 and got["ET"]["lesionwise_dice"] == 1.0
    with pytest.raises(ValueError, match="dilation"):
        amd.evaluate.lesionwise_metrics(_dev(p2, gpu), _dev(g2, gpu), spacing, dilation=17)


def test_too_many_components_and_too_large_a_pair_table_are_value_errors(amd, gpu):
    """isolated voxels on a lattice: 41^3 = 68 921 components of the prediction (more than MAX_COMPONENTS = 65 536); 11^3 = 1331 lesions
    eight voxels apart, which three dilation steps leave apart, against 1331 components: a 1332 x 1332 table, above 2^20 entries"""
    many = np.zeros((82, 82, 82), np.uint8)
    many[::2, ::2, ::2] = 1
    one = np.zeros_like(many)
    one[40, 40, 40] = 1
    with pytest.raises(ValueError, match=r"region 'WT' of the prediction has 68921 components \(65536 at most\)"):
        amd.evaluate.lesionwise_metrics(_dev(many, gpu), _dev(one, gpu), (1, 1, 1))
    with pytest.raises(ValueError, match=r"region 'WT' of the ground truth has 68921 components"):
        amd.evaluate.lesionwise_metrics(_dev(one, gpu), _dev(many, gpu), (1, 1, 1))
    sparse = np.zeros((88, 88, 88), np.uint8)
    sparse[::8, ::8, ::8] = 1
    with pytest.raises(ValueError, match=r"1331 components in region 'WT' of the ground truth and 1331 in its dilation make a table of 1774224 entries"):
        amd.evaluate.lesionwise_metrics(_dev(sparse, gpu), _dev(sparse, gpu), (1, 1, 1))


# ---------------------------------------------------------------------------------------------------------------- command
def run_command(args, timeout=240):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "brats_amd.evaluate", *args], capture_output=True, text=True, env=env, cwd=ROOT, timeout=timeout)


def test_command_reports_and_writes_the_lesionwise_block(amd, gpu, tmp_path):
    from test_lesionwise_cpu import check_lesionwise_lines
    from test_surface_distance_cpu import check_report_contract
    zooms = (1.5, 1.0, 0.75)     # exact in the header's float32
    pred, gt = lu.noise_pair(2, (33, 17, 29))
    for name, seg in (("pred", pred), ("gt", gt)):
        amd.nifti.save_like(tmp_path / f"{name}.nii.gz", seg, amd.nifti.make_header(seg.shape, zooms=zooms, dtype=np.uint8))
    out = tmp_path / "metrics.json"
    common = ["--pred", str(tmp_path / "pred.nii.gz"), "--gt", str(tmp_path / "gt.nii.gz"), "--output", str(out)]
    res = run_command(common + ["--lesionwise", "--dilation", "2", "--min-lesion-mm3", "10", "--lesion-penalty-mm", "100"])
    assert res.returncode == 0, res.stdout + res.stderr
    written = json.loads(out.read_text())
    api = amd.evaluate.evaluate_lesionwise(_dev(pred, gpu), _dev(gt, gpu), zooms, dilation=2, min_volume_mm3=10.0, penalty_mm=100.0)
    assert written == json.loads(json.dumps(api))
    for key in su.REGIONS:
        m = written[key]["lesionwise"]
        assert set(m) == {"lesionwise_dice", "lesionwise_hd95", "num_lesions", "num_counted", "num_tp", "num_fn", "num_fp", "fp_components", "lesions",
                          "dilation", "min_volume_mm3", "penalty_mm"}
        assert (m["dilation"], m["min_volume_mm3"], m["penalty_mm"]) == (2, 10.0, 100.0) and "hd95" in written[key]
    lines = res.stdout.splitlines()
    check_report_contract(lines, {"mean_dice": api["mean_dice"], "WT": api["WT"]["dice"], "TC": api["TC"]["dice"], "ET": api["ET"]["dice"]})
    check_lesionwise_lines(lines, api)
    res = run_command(common + ["--lesionwise", "--dilation", "0"])
    assert res.returncode == 1 and "dilation" in res.stderr and "Lesion-wise" not in res.stdout


# ---------------------------------------------------------------------------------------------------------------- full size
def test_full_size_case_against_scipy(amd, gpu):
    """A 120 x 120 x 78 crop of the 240 x 240 x 155 grid (the scipy side of the full grid takes over ten seconds per region): four lesions,
    one of which the prediction misses, and three hundred specks in the prediction - a few hundred components per region."""
    shape, spacing = (120, 120, 78), (1.0, 1.0, 1.0)
    pred, gt = lu.blob_case(shape)
    want = lu.case_lesionwise(pred, gt, spacing)
    assert want["WT"]["num_fp"] > 200 and want["TC"]["num_fn"] >= 1 and all(m["num_lesions"] == 4 for m in want.values())
    got = amd.evaluate.lesionwise_metrics(_dev(pred, gpu), _dev(gt, gpu), spacing)
    worst = same_case(got, want, "full size")
    print(f"full size {shape}: worst relative difference {worst:.3g}")
