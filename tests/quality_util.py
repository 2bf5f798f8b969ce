"""CPU restatements shared by test_quality_cpu.py and test_gpu_quality.py (scipy / numpy only): what csrc/quality.hip and the flag,
moment and percentile kernels deliver for the reference's step 5, computed on the host the way the kernels compute it (the
complement labelled and its face components marked, a 27-point gather on a padded copy, ...), the primitive test shapes, the
fixture loader and the comparer."""
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "quality.json")
SECTIONS = ("segmentation_quality", "image_quality", "artifact_detection", "measurement_confidence", "limitations_and_caveats")
RTOL_STD = 1e-9  # the reference's std is numpy's two-pass formula, ours comes from sums in a fixed order: the cap steps 1 and 4 use
STD_KEYS = ("std_intensity", "snr_estimate", "background_cv", "edge_gradient_cv")  # the floats that contain a standard deviation


def module(name):
    return importlib.import_module("brats_amd." + name)


def generator_tool():
    spec = importlib.util.spec_from_file_location("_gen_quality_golden", os.path.join(ROOT, "tools", "gen_quality_golden.py"))
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
    vols = synthetic.mri_for_quality(a["seed"] + 1, seg, levels=a["levels"], brain_axes=a["brain_axes"], radial_gain=a["radial_gain"], plateau=a["plateau"],
                                     ghost=a["ghost"], dropout=a["dropout"], spikes=a["spikes"], edge_noise=a["edge_noise"], zero_channel=a["zero_channel"],
                                     sigma=a["sigma"])
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


# ---- the four primitives, restated ------------------------------------------------------------------------------------
def fill_holes(mask):
    """(0 / 1 map, voxels added): the complement labelled with 6 neighbours, the components with a face voxel kept open"""
    fg = np.asarray(mask) != 0
    labels, _ = ndimage.label(~fg)
    faces = [labels[0], labels[-1], labels[:, 0], labels[:, -1], labels[:, :, 0], labels[:, :, -1]]
    open_labels = np.unique(np.concatenate([f.reshape(-1) for f in faces]))
    hole = (labels > 0) & ~np.isin(labels, open_labels)
    return (fg | hole).astype(np.uint8), int(hole.sum())


def sobel_magnitude(x):
    """sqrt(gx^2 + gy^2 + gz^2) of the whole volume in float64: 27 shifted views of a copy padded by repeating the border"""
    p = np.pad(np.asarray(x, dtype=np.float64), 1, mode="edge")
    d, s = (-1.0, 0.0, 1.0), (1.0, 2.0, 1.0)
    n0, n1, n2 = x.shape
    g = [np.zeros(x.shape), np.zeros(x.shape), np.zeros(x.shape)]
    for a in range(3):
        for b in range(3):
            for c in range(3):
                v = p[a:a + n0, b:b + n1, c:c + n2]
                g[0] += d[a] * s[b] * s[c] * v
                g[1] += s[a] * d[b] * s[c] * v
                g[2] += s[a] * s[b] * d[c] * v
    return np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)


def scipy_sobel_magnitude(x):
    x = np.asarray(x).astype(float)  # step5_quality.py:413-416
    return np.sqrt(ndimage.sobel(x, axis=0) ** 2 + ndimage.sobel(x, axis=1) ** 2 + ndimage.sobel(x, axis=2) ** 2)


def stats_of(values):
    """(n, mean, population std) as the entry points return them"""
    return (int(values.size), float(values.mean()), float(values.std())) if values.size else (0, 0.0, 0.0)


def radial_shell(x, selected, centre, inner_frac=0.3, outer_frac=0.7):
    """(max_dist, n_inner, sum_inner, n_outer, sum_outer), step5_quality.py:280-297 on a boolean selection"""
    coords = np.where(selected)
    if len(coords[0]) == 0:
        return 0.0, 0, 0.0, 0, 0.0
    distances = np.sqrt((coords[0] - centre[0])**2 + (coords[1] - centre[1])**2 + (coords[2] - centre[2])**2)
    max_dist = distances.max()
    values = np.asarray(x, dtype=np.float64)[selected]
    inner, outer = values[distances < max_dist * inner_frac], values[distances > max_dist * outer_frac]
    return float(max_dist), int(inner.size), float(inner.sum()), int(outer.size), float(outer.sum())


def face_slab_counts(x, margin):
    pos = np.asarray(x) > 0
    return np.array([pos[:margin].sum(), pos[-margin:].sum(), pos[:, :margin].sum(), pos[:, -margin:].sum(), pos[:, :, :margin].sum(),
                     pos[:, :, -margin:].sum()], dtype=np.int64)


# ---- the primitive test shapes ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fill_cases():
    """name -> uint8 mask, the cases of the hole-filling tests"""
    rs = np.random.RandomState(5)
    cases = {"1x1x1 background": np.zeros((1, 1, 1), np.uint8), "1x1x1 foreground": np.ones((1, 1, 1), np.uint8)}
    m = (rs.random_sample((1, 7, 9)) < 0.5).astype(np.uint8)
    m[0, 2:5, 3:6] = 1
    m[0, 3, 4] = 0  # enclosed in the plane, but every voxel of a 1 x 7 x 9 volume lies on a face
    cases["1x7x9 all on a face"] = m
    m = np.zeros((5, 6, 7), np.uint8)
    m[1:4, 1:4, 1:4] = 1
    m[2, 2, 2] = 0
    cases["5x6x7 one enclosed voxel"] = m
    m = np.zeros((9, 10, 11), np.uint8)
    m[2:7, 2:7, 2:7] = 1
    m[3:6, 3:6, 3:6] = 0
    m[2, 2, 2] = 0  # the corner of the shell: the cavity's corner (3, 3, 3) touches it only diagonally
    cases["diagonal gap"] = m
    m = np.zeros((12, 13, 14), np.uint8)
    m[1:11, 1:12, 1:13] = 1
    m[4:7, 4:7, 4:7] = 0  # the cavity, then a channel with five right-angle turns to the face c0 = 0
    for sl in ((5, 5, slice(7, 10)), (5, slice(5, 10), 9), (slice(5, 9), 9, 9), (8, 9, slice(3, 10)), (8, slice(2, 10), 3), (slice(0, 9), 2, 3)):
        m[sl] = 0
    cases["winding channel"] = m
    g = np.ogrid[0:21, 0:21, 0:21]
    r2 = sum((v - 10.0) ** 2 for v in g)
    cases["ball inside a shell"] = (((r2 <= 81) & (r2 > 49)) | (r2 <= 9)).astype(np.uint8)
    cases["all foreground"] = np.ones((6, 5, 4), np.uint8)
    cases["all background"] = np.zeros((6, 5, 4), np.uint8)
    cases["noise 33x34x35"] = (rs.random_sample((33, 34, 35)) < 0.5).astype(np.uint8)
    cases["noise 70x3x129"] = (rs.random_sample((70, 3, 129)) < 0.5).astype(np.uint8)
    for v in cases.values():
        v.setflags(write=False)
    return cases


SOBEL_SHAPES = ((2, 3, 4), (5, 1, 7), (17, 19, 65))
SHELL_SHAPES = ((1, 1, 1), (9, 10, 11), (40, 41, 70))


@functools.lru_cache(maxsize=None)
def integer_volume(shape, seed=11):
    """integer-valued float32 volume below 2^15, read-only"""
    v = np.random.RandomState(seed).randint(0, 2 ** 15, shape).astype(np.float32)
    v.setflags(write=False)
    return v


def sobel_single_voxels(shape):
    """the 8 corners, one voxel on each face and one interior voxel (where the shape has one), as a list of index tuples"""
    hi = [n - 1 for n in shape]
    mid = [n // 2 for n in shape]
    picks = [tuple(hi[k] if (c >> k) & 1 else 0 for k in range(3)) for c in range(8)]
    for k in range(3):
        for end in (0, hi[k]):
            picks.append(tuple(end if j == k else mid[j] for j in range(3)))
    picks.append(tuple(mid))
    return list(dict.fromkeys(picks))


# ---- the statistics of a case, restated -------------------------------------------------------------------------------
def _moments(values):
    v = np.asarray(values, dtype=np.float64)
    return np.array([v.size, v.sum(), (v * v).sum()])


def host_stats(q, seg, vols):
    """what ``quality.quality_stats`` collects on the device, with scipy and numpy on the host"""
    wt = seg > 0
    data = [v.astype(np.float64) for v in vols]
    t1 = data[0]
    stats = {"shape": seg.shape, "label_stats": mu.label_stats(seg, 8)}
    if wt.any():
        stats["num_components"] = int(ndimage.label(wt, structure=ndimage.generate_binary_structure(3, 3))[1])
        stats["filled"] = fill_holes(wt)[1]
    brain = t1 > np.percentile(t1[t1 > 0], 5) if t1.max() > 0 else t1 > 0
    n_brain = stats["n_brain"] = int(brain.sum())
    stats["sequences"] = {}
    for name, x in zip(q.SEQUENCES, data):
        s = {"ghost": _moments(x[~brain & (x > 0)]), "brain": _moments(x[brain]), "background": np.zeros(3), "zeros": 0, "outliers_high": 0,
             "outliers_low": 0}
        if n_brain:
            values = x[brain]
            s["background"] = _moments(x[~brain & (x > 0) & (x < np.percentile(x[x > 0], 10))])
            s["zeros"] = int(((x == 0) & brain).sum())
            q01, q25, q75, q99 = np.percentile(values, (1, 25, 75, 99))
            iqr = q75 - q25
            s["outliers_high"], s["outliers_low"] = int((values > q99 + 3 * iqr).sum()), int((values < q01 - 3 * iqr).sum())
        stats["sequences"][name] = s
    if n_brain:
        coords = np.where(brain)
        stats["shell"] = radial_shell(t1, brain, [np.mean(coords[i]) for i in range(3)])
    stats["face_counts"] = face_slab_counts(t1, q.EDGE_MARGIN)
    edge = wt & (mu.erode(wt, 2) == 0)
    stats["n_edge"] = int(edge.sum())
    if wt.any() and stats["n_edge"] > 100:
        stats["edge_gradient"] = stats_of(sobel_magnitude(vols[0])[edge])
    return stats


class Comparer:
    """strings, integers, booleans, None, keys and their order and list order equal; floats equal, except those that contain a
    standard deviation (STD_KEYS), which may differ by RTOL_STD relative; keeps the largest relative error of such a float seen"""

    def __init__(self):
        self.worst, self.where = 0.0, ""

    def same(self, got, want, path=""):
        if isinstance(want, dict):
            assert isinstance(got, dict) and list(got) == list(want), (path, list(got) if isinstance(got, dict) else got, list(want))
            for k in want:
                self.same(got[k], want[k], f"{path}/{k}")
        elif isinstance(want, list):
            assert isinstance(got, list) and len(got) == len(want), (path, got, want)
            for i, (g, w) in enumerate(zip(got, want)):
                self.same(g, w, f"{path}[{i}]")
        elif isinstance(want, float):
            assert isinstance(got, float), (path, got, want)
            if path.rsplit("/", 1)[-1] in STD_KEYS:
                err = abs(got - want) / abs(want) if want != 0 else abs(got)
                if err > self.worst:
                    self.worst, self.where = err, path
                assert err <= RTOL_STD, (path, got, want, err)
            else:
                assert got == want, (path, got, want)
        else:
            assert want is None or isinstance(want, (bool, int, str)), (path, want)
            assert type(got) is type(want) and got == want, (path, got, want)
