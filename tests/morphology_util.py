"""CPU restatements shared by test_morphology_cpu.py and test_gpu_morphology.py (scipy / numpy only): what the device kernels of
csrc/morphology.hip deliver, computed from the same inputs on the host."""
import hashlib
import importlib
import importlib.util
import json
import os

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "morphology.json")
SECTIONS = ("shape_descriptors", "border_regularity", "margin_definition", "necrosis_pattern", "cystic_solid_classification")
RTOL = 1e-9  # ratios of fp64 sums over fewer than 2^24 terms: the bound DESIGN.md's test table already uses for centroids


def morphology_module():
    return importlib.import_module("brats_amd.morphology")


def generator_tool():
    spec = importlib.util.spec_from_file_location("_gen_morphology_golden", os.path.join(ROOT, "tools", "gen_morphology_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def load_fixture():
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


def fixture_data(amd, case):
    """(label map, [4, ...] float32 volumes) of a fixture case, regenerated from its arguments and checked against its hashes"""
    a = case["args"]
    seg = amd.synthetic.shapes_map(a["seed"], tuple(a["shape"]), a["parts"])
    vols = amd.synthetic.mri_for_label_map(a["seed"] + 1, seg, gain=a["gain"], cystic=a["cystic"], sigma=a["sigma"], brain=a["brain"])
    assert hashlib.sha256(seg.tobytes()).hexdigest() == case["sha256"]["seg"], f"label map of case {case['name']} is not the one the fixture was made from"
    assert hashlib.sha256(vols.tobytes()).hexdigest() == case["sha256"]["vols"], f"volumes of case {case['name']} are not the ones the fixture was made from"
    return seg, vols


def erode(mask, iterations=1):
    return ndimage.binary_erosion(mask != 0, iterations=iterations).astype(np.uint8)


def dilate(mask, iterations=1):
    return ndimage.binary_dilation(mask != 0, iterations=iterations).astype(np.uint8)


def edt_sq(mask):
    return np.rint(ndimage.distance_transform_edt(mask != 0) ** 2).astype(np.int32)


def second_moments(mask):
    c = [v.astype(np.int64) for v in np.nonzero(mask)]
    return np.array([len(c[0]), c[0].sum(), c[1].sum(), c[2].sum(), (c[0] * c[0]).sum(), (c[1] * c[1]).sum(), (c[2] * c[2]).sum(),
                     (c[0] * c[1]).sum(), (c[0] * c[2]).sum(), (c[1] * c[2]).sum()], dtype=np.int64)


def label_stats(seg, K=8):
    out = np.zeros((K, 10), dtype=np.int64)
    out[:, 4:7], out[:, 7:10] = 1 << 40, -1
    out[0] = [int((seg == 0).sum() + (seg >= K).sum()), 0, 0, 0, 0, 0, 0, -1, -1, -1]
    for l in range(1, K):
        c = [v.astype(np.int64) for v in np.nonzero(seg == l)]
        if len(c[0]):
            out[l] = [len(c[0])] + [v.sum() for v in c] + [v.min() for v in c] + [v.max() for v in c]
    return out


def gradient_stats(d2_in, d2_out, surface):
    """(n, mean, population std) of |np.gradient(sqrt(d2_in) - sqrt(d2_out))| at the surface voxels"""
    signed = np.sqrt(d2_in.astype(np.float64)) - np.sqrt(d2_out.astype(np.float64))
    g = np.sqrt(sum(np.gradient(signed, axis=k) ** 2 for k in range(3)))[surface != 0]
    return (int(g.size), float(g.mean()), float(g.std())) if g.size else (0, 0.0, 0.0)


def masked_moments(vols, flags):
    out = np.zeros((8, vols.shape[0], 3), dtype=np.float64)
    for b in range(8):
        m = (flags >> b) & 1 != 0
        for c in range(vols.shape[0]):
            v = vols[c][m].astype(np.float64)
            out[b, c] = [v.size, v.sum(), (v * v).sum()]
    return out


def flag_map(morph, seg, vols):
    """the flag byte per voxel that tumor_morphology builds on the device"""
    wt = seg > 0
    flags = np.zeros(seg.shape, dtype=np.uint8)
    flags |= wt.astype(np.uint8) << morph.WT
    if wt.any():
        flags |= ((dilate(wt, 5) != 0) & ~wt).astype(np.uint8) << morph.BAND
        flags |= (wt & (erode(wt) == 0)).astype(np.uint8) << morph.INNER
        flags |= ((dilate(wt) != 0) & ~wt).astype(np.uint8) << morph.OUTER
        ncr = seg == 1
        flags |= ncr.astype(np.uint8) << morph.NCR
        t1, t2, flair = (vols[c].astype(np.float64) for c in (morph.T1, morph.T2, morph.FLAIR))
        t1_hi, t2_lo, flair_hi = morph.csf_thresholds(t1, t2, flair)
        flags |= (ncr & (t1 < t1_hi) & (t2 > t2_lo) & (flair < flair_hi)).astype(np.uint8) << morph.CYSTIC
    return flags


def host_stats(morph, seg, vols):
    """the five arguments of morphology_from_stats but the voxel sizes, from scipy and numpy"""
    flags = flag_map(morph, seg, vols)
    surface = (flags >> morph.INNER) & 1
    gradient = None
    if surface.sum() >= 10:
        gradient = gradient_stats(edt_sq(seg > 0), edt_sq(seg == 0), surface)
    return label_stats(seg), second_moments(seg > 0), gradient, masked_moments(vols, flags)


class Comparer:
    """strings, integers, booleans, keys and list order equal; floats within RTOL relative; keeps the largest relative error seen"""

    def __init__(self):
        self.worst, self.where = 0.0, ""

    def same(self, got, want, path=""):
        if isinstance(want, dict):
            assert isinstance(got, dict) and set(got) == set(want), (path, sorted(got) if isinstance(got, dict) else got, sorted(want))
            for k in want:
                self.same(got[k], want[k], f"{path}/{k}")
        elif isinstance(want, list):
            assert isinstance(got, list) and len(got) == len(want), (path, got, want)
            for i, (g, w) in enumerate(zip(got, want)):
                self.same(g, w, f"{path}[{i}]")
        elif isinstance(want, float):
            assert isinstance(got, float), (path, got, want)
            err = abs(got - want) / abs(want) if want != 0 else abs(got)
            if err > self.worst:
                self.worst, self.where = err, path
            assert err <= RTOL, (path, got, want, err)
        else:
            assert isinstance(want, (bool, int, str)), (path, want)
            assert type(got) is type(want) and got == want, (path, got, want)
