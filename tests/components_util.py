"""CPU restatements shared by test_components_cpu.py and test_gpu_components.py (scipy / numpy only)."""
import hashlib
import json
import os

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "multiplicity.json")


def scipy_labels(mask, connectivity):
    lab, n = ndimage.label(mask != 0, structure=ndimage.generate_binary_structure(3, connectivity))
    return lab.astype(np.int32), int(n)


def numpy_stats(lab, n, seg=None):
    """The [n, 14] integer table from a label map: count, coordinate sums, minima, maxima, voxels with seg value 1..4."""
    out = np.zeros((n, 14), dtype=np.int64)
    if n == 0:
        return out
    idx = np.flatnonzero(lab.ravel() > 0)
    comp = lab.ravel()[idx].astype(np.int64) - 1
    coords = np.unravel_index(idx, lab.shape)
    out[:, 0] = np.bincount(comp, minlength=n)
    for k in range(3):
        c = coords[k].astype(np.int64)
        np.add.at(out[:, 1 + k], comp, c)
        lo, hi = np.full(n, 1 << 40, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        np.minimum.at(lo, comp, c)
        np.maximum.at(hi, comp, c)
        out[:, 4 + k], out[:, 7 + k] = lo, hi
    if seg is not None:
        s = seg.ravel()[idx]
        for v in (1, 2, 3, 4):
            out[:, 9 + v] = np.bincount(comp[s == v], minlength=n)
    return out


def load_fixture():
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


def fixture_label_map(amd, case):
    a = case["args"]
    seg = amd.synthetic.label_map(a["seed"], tuple(a["shape"]), [(tuple(c), r) for c, r in a["lesions"]], a["fragments"], enhancing=a["enhancing"])
    assert hashlib.sha256(seg.tobytes()).hexdigest() == case["sha256"], f"label map of case {case['name']} is not the one the fixture was made from"
    return seg


def assert_same(got, want, path=""):
    """integers, booleans, strings, None, keys and list order equal; floats to 1e-12 relative, centroids to 1e-9 absolute"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), (path, sorted(got) if isinstance(got, dict) else got, sorted(want))
        for k in want:
            assert_same(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (path, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, f"{path}[{i}]")
    elif isinstance(want, float):
        assert isinstance(got, float), (path, got, want)
        if "centroid" in path:
            assert abs(got - want) <= 1e-9, (path, got, want)
        else:
            assert abs(got - want) <= 1e-12 * abs(want), (path, got, want)
    else:
        assert want is None or isinstance(want, (bool, int, str)), (path, want)
        assert type(got) is type(want) and got == want, (path, got, want)


def largest_component_ref(image, for_which_classes, volume_per_voxel, minimum_valid_object_size=None):
    """nnU-Net v1 remove_all_but_the_largest_connected_component restated with scipy.ndimage.label (default structure:
    6 neighbours).  minimum_valid_object_size: None, one number or {class: number}."""
    image = image.copy()
    largest_removed, kept_size = {}, {}
    for c in for_which_classes:
        if isinstance(c, (list, tuple)):
            c = tuple(c)
            mask = np.isin(image, c)
        else:
            mask = image == c
        lmap, n = ndimage.label(mask.astype(int))
        sizes = {i: (lmap == i).sum() * volume_per_voxel for i in range(1, n + 1)}
        largest_removed[c], kept_size[c] = None, None
        if n > 0:
            maximum = max(sizes.values())
            kept_size[c] = maximum
            for i in range(1, n + 1):
                if sizes[i] != maximum:
                    remove = True
                    if minimum_valid_object_size is not None:
                        least = minimum_valid_object_size[c] if isinstance(minimum_valid_object_size, dict) else minimum_valid_object_size
                        remove = sizes[i] < least
                    if remove:
                        image[(lmap == i) & mask] = 0
                        largest_removed[c] = sizes[i] if largest_removed[c] is None else max(largest_removed[c], sizes[i])
    return image, largest_removed, kept_size


def checkerboard(shape):
    return (np.indices(shape).sum(axis=0) % 2 == 0).astype(np.uint8)


def serpentine(shape):
    """One path that runs along the last axis in every other row of every other slab and turns at alternating ends: it
    crosses every brick seam many times and its pieces merge late (a row meets the next one only at its far end)."""
    d0, d1, d2 = shape
    m = np.zeros(shape, dtype=np.uint8)
    rows = list(range(0, d1, 2))
    for zi, z in enumerate(range(0, d0, 2)):
        for yi, y in enumerate(rows):
            m[z, y, :] = 1
            if yi + 1 < len(rows):
                m[z, y + 1, d2 - 1 if yi % 2 == 0 else 0] = 1
        if z + 2 < d0:
            m[z + 1, rows[-1] if zi % 2 == 0 else 0, zi % (d2)] = 1
    return m


def noise(seed, shape, p):
    return (np.random.RandomState(seed).random_sample(shape) < p).astype(np.uint8)
