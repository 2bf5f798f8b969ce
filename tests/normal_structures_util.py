"""CPU restatements shared by test_normal_structures_cpu.py and test_gpu_normal_structures.py (scipy / numpy only): what
csrc/normal_structures.hip, the 18-neighbour labelling and the flag, moment and percentile kernels deliver for the reference's
step 6, computed on the host, the primitive test shapes, the fixture loader and the comparer."""
import functools
import hashlib
import importlib
import importlib.util
import json
import os

import numpy as np
from scipy import ndimage

import morphology_util as mu

ROOT = mu.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "normal_structures.json")
SECTIONS = ("ventricular_system", "parenchyma", "major_vessels")
FAR = 1 << 30  # MI355_CITYBLOCK_FAR


def module(name):
    return importlib.import_module("brats_amd." + name)


def generator_tool():
    spec = importlib.util.spec_from_file_location("_gen_normal_structures_golden", os.path.join(ROOT, "tools", "gen_normal_structures_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@functools.lru_cache(maxsize=None)
def load_fixture():
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


def case(name):
    return [c for c in load_fixture()["cases"] if c["name"] == name][0]


@functools.lru_cache(maxsize=None)
def _case_data(name):
    synthetic = module("synthetic")
    a = case(name)["args"]
    seg = synthetic.shapes_map(a["seed"], tuple(a["shape"]), a["parts"])
    vols = synthetic.mri_for_normal_structures(a["seed"] + 1, seg, ventricles=a["ventricles"], brain_axes=a["brain_axes"], outside=a["outside"],
                                               contrast=a["contrast"], pv_gain=a["pv_gain"], voids=a["voids"], enhancement=a["enhancement"], cuts=a["cuts"],
                                               zero=a["zero"], sigma=a["sigma"])
    seg.setflags(write=False)
    vols.setflags(write=False)
    return seg, vols


def fixture_data(c):
    """(label map, [4, ...] float32 volumes) of a fixture case, regenerated from its arguments once (read-only) and checked
    against its hashes"""
    seg, vols = _case_data(c["name"])
    assert hashlib.sha256(seg.tobytes()).hexdigest() == c["sha256"]["seg"], f"label map of case {c['name']} is not the one the fixture was made from"
    assert hashlib.sha256(vols.tobytes()).hexdigest() == c["sha256"]["vols"], f"volumes of case {c['name']} are not the ones the fixture was made from"
    return seg, vols


# ---- the primitives, restated -----------------------------------------------------------------------------------------
def cityblock(mask, to_foreground):
    """The exact L1 distance by brute force over the three axes: running minima along each axis of a copy padded by one voxel
    (a source when the distance is measured to the background, far otherwise).  Written without scipy on purpose: the tests
    compare it, and the device, with scipy's chamfer transform and with its iterated dilations and erosions."""
    fg = np.asarray(mask) != 0
    src = fg if to_foreground else ~fg
    g = np.where(np.pad(src, 1, constant_values=not to_foreground), 0, FAR).astype(np.int64)
    for axis in range(3):
        g = np.moveaxis(g, axis, 0)
        for k in range(1, g.shape[0]):
            g[k] = np.minimum(g[k], g[k - 1] + 1)
        for k in range(g.shape[0] - 2, -1, -1):
            g[k] = np.minimum(g[k], g[k + 1] + 1)
        g = np.moveaxis(g, 0, axis)
    return np.minimum(g[1:-1, 1:-1, 1:-1], FAR).astype(np.int32)


def scipy_taxicab(mask, to_foreground):
    """scipy's own taxicab transform of the same thing (None where scipy has nothing to measure to)"""
    fg = np.asarray(mask) != 0
    if to_foreground:
        return ndimage.distance_transform_cdt(~fg, metric="taxicab").astype(np.int32) if fg.any() else None
    return ndimage.distance_transform_cdt(np.pad(fg, 1), metric="taxicab")[1:-1, 1:-1, 1:-1].astype(np.int32)


def order_stats(values, qs):
    """(count, below, above) from a sorted copy"""
    v = np.sort(np.asarray(values).reshape(-1))
    q = np.atleast_1d(np.asarray(qs, dtype=np.float64))
    if v.size == 0:
        return 0, np.zeros(q.size, np.int32), np.zeros(q.size, np.int32)
    r = np.floor((v.size - 1) * np.true_divide(q, 100)).astype(np.int64)
    return int(v.size), v[r].astype(np.int32), v[np.minimum(r + 1, v.size - 1)].astype(np.int32)


def selected(flags, require, forbid):
    return ((flags & require) == require) & ((flags & forbid) == 0)


def flag_i32(flags, bit, values, lo, hi, require, forbid):
    on = selected(flags, require, forbid) & (values >= lo) & (values <= hi)
    return ((flags & ~np.uint8(1 << bit)) | (on.astype(np.uint8) << bit)).astype(np.uint8)


def flag_box(flags, bit, box, require, forbid):
    inside = np.zeros(flags.shape, dtype=bool)
    inside[tuple(slice(max(int(box[2 * k]), 0), max(int(box[2 * k + 1]), 0)) for k in range(3))] = True
    on = selected(flags, require, forbid) & inside
    return ((flags & ~np.uint8(1 << bit)) | (on.astype(np.uint8) << bit)).astype(np.uint8)


def column_count_max(flags, i1_from, require, forbid):
    slab = selected(flags, require, forbid)[:, i1_from:, :]
    return int(np.max(np.sum(slab, axis=0))) if slab.any() else 0  # step6_normal_structures.py:130-131


# ---- the primitive test shapes ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cityblock_cases():
    """name -> uint8 mask"""
    rs = np.random.RandomState(7)
    cases = {"1x1x1 foreground": np.ones((1, 1, 1), np.uint8), "1x1x1 background": np.zeros((1, 1, 1), np.uint8),
             "1x7x9": (rs.random_sample((1, 7, 9)) < 0.3).astype(np.uint8)}
    shape = (5, 6, 7)
    hi, mid = [n - 1 for n in shape], [n // 2 for n in shape]
    picks = [tuple(hi[k] if (c >> k) & 1 else 0 for k in range(3)) for c in range(8)]
    picks += [tuple(end if j == k else mid[j] for j in range(3)) for k in range(3) for end in (0, hi[k])]
    for idx in picks:
        m = np.zeros(shape, np.uint8)
        m[idx] = 3  # any nonzero value is foreground
        cases[f"5x6x7 single voxel at {idx}"] = m
    cases["all foreground 6x5x4"] = np.ones((6, 5, 4), np.uint8)
    cases["all background 6x5x4"] = np.zeros((6, 5, 4), np.uint8)
    for shape in ((33, 34, 35), (70, 3, 129)):
        for p in (0.02, 0.5, 0.98):
            cases[f"noise {p} {shape[0]}x{shape[1]}x{shape[2]}"] = (rs.random_sample(shape) < p).astype(np.uint8)
    for v in cases.values():
        v.setflags(write=False)
    return cases


ITERATIONS = (1, 2, 3, 5, 10)
FLAG_SHAPES = ((7, 9, 4), (17, 19, 65))


def seam_pairs():
    """(name, shape, voxel a, voxel b, kind): two voxels that touch across an edge only / a corner only, placed across each seam
    of the 4 x 8 x 64 bricks of the labelling (axis 2 at 63 | 64, axis 1 at 7 | 8, axis 0 at 3 | 4)"""
    shape = (9, 18, 130)
    base = {"x": (1, 2, 63), "y": (1, 7, 20), "z": (3, 2, 20)}
    out = []
    for seam, a in base.items():
        k = {"z": 0, "y": 1, "x": 2}[seam]
        other = [j for j in range(3) if j != k]
        for o in other:  # edge: one step across the seam and one along another axis
            b = list(a)
            b[k] += 1
            b[o] += 1
            out.append((f"edge across the {seam} seam and axis {o}", shape, a, tuple(b), "edge"))
        out.append((f"corner across the {seam} seam", shape, a, tuple(v + 1 for v in a), "corner"))
    return out


# ---- the statistics of a case, restated -------------------------------------------------------------------------------
def host_stats(ns, seg, vols):
    """what ``normal_structures.normal_structures_stats`` collects on the device, with scipy and numpy on the host, following
    step6_normal_structures.py's own expressions (the ventricles are found once)"""
    t1, t1ce, t2, flair = (v.astype(np.float64) for v in vols)
    d0, d1, d2 = seg.shape
    brain = t1 > np.percentile(t1[t1 > 0], 5) if t1.max() > 0 else t1 > 0
    stats = {"shape": seg.shape, "n_brain": int(brain.sum())}
    if not brain.any():
        return stats
    tumour = seg > 0
    normal = brain & ~tumour
    csf = brain & (t1 < np.percentile(t1[brain], 15)) & (t2 > np.percentile(t2[brain], 85)) & (flair < np.percentile(flair[brain], 25)) & ~tumour
    csf = ndimage.binary_dilation(ndimage.binary_erosion(csf, iterations=1), iterations=1)
    labeled, n = ndimage.label(csf, structure=ndimage.generate_binary_structure(3, 2))
    vent = np.zeros_like(csf)
    for i in range(1, n + 1):
        component = labeled == i
        if component.sum() > 1000 and abs(np.mean(np.where(component)[0]) - d0 / 2) < d0 * 0.3:
            vent |= component
    stats.update(n_normal=int(normal.sum()), n_ventricle=int(vent.sum()), n_ventricle_left=int(vent[:d0 // 2].sum()),
                 n_ventricle_right=int(vent[d0 // 2:].sum()))
    if vent.any():
        frontal_y = np.percentile(np.where(vent)[1], 75)
        stats["frontal_width"] = int(np.max(np.sum(vent[:, int(frontal_y):, :], axis=0)))
    stats["n_obstructed"] = int((vent & ndimage.binary_dilation(tumour, iterations=5)).sum())
    dist = ndimage.distance_transform_edt(brain)
    deep = normal & (dist > np.percentile(dist[brain], 60))
    cortical = normal & (dist < np.percentile(dist[brain], 40))
    pv = ndimage.binary_dilation(vent, iterations=10) & normal & ~vent
    stats["periventricular"] = (int(pv.sum()), float(flair[pv].sum()))
    stats["cortical"] = (int(cortical.sum()), float(flair[cortical].sum()), float(t1[cortical].sum()))
    stats["deep"] = (int(deep.sum()), float(t1[deep].sum()))
    inferior = brain.copy()
    inferior[:, :, d2 // 3:] = False
    stats["n_inferior"] = int(inferior.sum())
    stats["n_flow_void"] = int((inferior & (t1 < np.percentile(t1[inferior], 5)) & ~tumour).sum()) if inferior.any() else 0
    peri = ndimage.binary_dilation(tumour, iterations=10) & ~tumour & brain
    stats["peritumoral"] = (int(peri.sum()), float(t1[peri].sum()), float(t1ce[peri].sum()))
    return stats


def compare(got, want, path=""):
    """every value exactly equal: strings, integers, booleans, None, floats bit for bit, keys and their order, list order"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (path, list(got) if isinstance(got, dict) else got, list(want))
        for k in want:
            compare(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (path, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            compare(g, w, f"{path}[{i}]")
    else:
        assert want is None or isinstance(want, (bool, int, float, str)), (path, want)
        assert type(got) is type(want) and got == want, (path, got, want)


def check_case(ns, case, run):
    """``run()`` returns the three dicts, or raises what the fixture says the case raises"""
    import pytest
    if "raises" in case:  # the reference's UnboundLocalError, or whatever numpy makes of a percentile of nothing
        with pytest.raises(ValueError, match="UnboundLocalError" if case["raises"] == "UnboundLocalError" else "brain mask .* is empty"):
            run()
        return None
    got = run()
    assert tuple(got) == SECTIONS
    compare(got, case["expected"], case["name"])
    return got
