"""CPU restatements shared by test_mass_effect_cpu.py and test_gpu_mass_effect.py (scipy / numpy only): what csrc/mass_effect.hip
and the flag, moment and percentile kernels deliver for the reference's step 2, computed on the host; the cases of the primitive
tests (both files run the same ones), the wrong variants the CPU tests hold against them, the fixture loader and the comparer."""
import functools
import hashlib
import importlib
import importlib.util
import json
import os

import numpy as np
from scipy import ndimage

import morphology_util as mu
import quality_util as qu

ROOT = mu.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "mass_effect.json")
SECTIONS = ("anatomical_location", "midline_shift", "ventricular_compression", "sulcal_effacement", "herniation_risk")
RTOL_STD = qu.RTOL_STD  # the project's cap for a float that contains a standard deviation (steps 1, 4 and 5)
STD_KEYS = ("variance_ratio", "peritumoral_intensity_std", "normal_brain_intensity_std")
AXIS_MAX = 4096


def module(name="mass_effect"):
    return importlib.import_module("brats_amd." + name)


def generator_tool():
    spec = importlib.util.spec_from_file_location("_gen_mass_effect_golden", os.path.join(ROOT, "tools", "gen_mass_effect_golden.py"))
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
    t1 = synthetic.mri_for_mass_effect(a["seed"] + 1, seg, brain_axes=a["brain_axes"], cuts=a["cuts"], dark=a["dark"], noise=a["noise"],
                                       peri_scale=a["peri_scale"], zero=a["zero"], sigma=a["sigma"])
    seg.setflags(write=False)
    t1.setflags(write=False)
    return seg, t1


def fixture_data(c):
    """(label map, float32 T1) of a fixture case, regenerated from its arguments once (read-only) and checked against its hashes"""
    seg, t1 = _case_data(c["name"])
    assert hashlib.sha256(seg.tobytes()).hexdigest() == c["sha256"]["seg"], f"label map of case {c['name']} is not the one the fixture was made from"
    assert hashlib.sha256(t1.tobytes()).hexdigest() == c["sha256"]["t1"], f"volume of case {c['name']} is not the one the fixture was made from"
    return seg, t1


class Comparer(qu.Comparer):
    """quality_util.Comparer's rule - everything equal in value and type, except the floats that contain a standard deviation,
    gated at RTOL_STD relative - with the float names of step 2"""

    def same(self, got, want, path=""):
        if isinstance(want, float) and path.rsplit("/", 1)[-1] in STD_KEYS:
            assert isinstance(got, float), (path, got, want)
            err = abs(got - want) / abs(want) if want != 0 else abs(got)
            if err > self.worst:
                self.worst, self.where = err, path
            assert err <= RTOL_STD, (path, got, want, err)
        elif isinstance(want, float):
            assert isinstance(got, float) and got == want, (path, got, want)
        else:
            super().same(got, want, path)


# ---- the five primitives, restated ------------------------------------------------------------------------------------
def selected(flags, require=0, forbid=0):
    f = np.asarray(flags)
    return ((f & require) == require) & ((f & forbid) == 0)


def axis_counts(flags, require=0, forbid=0):
    s = selected(flags, require, forbid)
    return tuple(s.sum(axis=tuple(k for k in range(3) if k != a)).astype(np.int64) for a in range(3))


def box_counts(flags, boxes, require=0, forbid=0, closed=False):
    """``closed=True`` is the wrong variant that takes hi as the last index"""
    s = selected(flags, require, forbid)
    e = 1 if closed else 0
    return np.array([s[max(b[0], 0):max(b[1] + e, 0), max(b[2], 0):max(b[3] + e, 0), max(b[4], 0):max(b[5] + e, 0)].sum() for b in boxes], dtype=np.int64)


def select_ranked(flags, ranks, require=0, forbid=0, base=0, order="C"):
    """``base=1`` (ranks counted from 1) and ``order='F'`` are the wrong variants"""
    s = selected(flags, require, forbid)
    r = np.asarray(ranks, dtype=np.int64) - base
    if order == "C":
        return np.flatnonzero(s)[r]
    c = np.nonzero(s.T)  # Fortran order: axis 0 fastest
    return np.ravel_multi_index(c[::-1], s.shape)[r]


def min_pair_dist2(a, b, shape):
    pa = np.stack(np.unravel_index(np.asarray(a, dtype=np.int64), shape), axis=1)
    pb = np.stack(np.unravel_index(np.asarray(b, dtype=np.int64), shape), axis=1)
    best = None
    for lo in range(0, len(pa), 256):
        d = ((pa[lo:lo + 256, None, :] - pb[None, :, :]) ** 2).sum(axis=2).min()
        best = int(d) if best is None else min(best, int(d))
    return best


def masked_min(values, flags, require=0, forbid=0):
    v = np.asarray(values)[selected(flags, require, forbid)]
    return (int(v.min()) if v.size else None), int(v.size)


# ---- the cases of the primitive tests ---------------------------------------------------------------------------------
AXIS_SHAPES = ((1, 1, 1), (3, 5, 130), (67, 2, 3), (5, 70, 9))
SELECTIONS = ((0, 0), (1, 0), (0, 4), (5, 2), (129, 66))  # (require, forbid)
RANK_SIZES = (1, 63, 65)
RANK_SHAPES = ((3, 5, 130), (17, 33, 65), (129, 131, 67))
RANK_DENSITIES = (0.01, 0.5, 1.0)
BOX_SHAPE = (9, 20, 35)


@functools.lru_cache(maxsize=None)
def random_flags(shape, seed=3):
    f = np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def density_flags(shape, density, seed=7):
    """bit 2 set with the given density among random other bits (bit 0 never set: require 4, forbid 1 selects the density)"""
    rs = np.random.RandomState(seed)
    f = (rs.randint(0, 128, shape).astype(np.uint8) << 1) & 0xFA
    f |= (rs.random_sample(shape) < density).astype(np.uint8) << 2
    f.setflags(write=False)
    return f


def rank_set(m, seed=11):
    """every rank when there are at most 4096, else the first, the last and an unsorted random set with repeats"""
    if m <= 4096:
        return np.random.RandomState(seed).permutation(m).astype(np.int64)
    r = np.random.RandomState(seed).randint(0, m, 1500).astype(np.int64)
    r[:4] = [0, m - 1, r[10], r[10]]
    return r


def box_cases(shape=BOX_SHAPE):
    """name -> list of boxes (lo0, hi0, lo1, hi1, lo2, hi2), all inside the volume"""
    d0, d1, d2 = shape
    faces = [(0, 1, 0, d1, 0, d2), (d0 - 1, d0, 0, d1, 0, d2), (0, d0, 0, 1, 0, d2), (0, d0, d1 - 1, d1, 0, d2), (0, d0, 0, d1, 0, 1), (0, d0, 0, d1, d2 - 1, d2)]
    rs = np.random.RandomState(5)
    overlapping = []
    for _ in range(16):
        lo = [rs.randint(0, n) for n in shape]
        hi = [rs.randint(l, n + 1) for l, n in zip(lo, shape)]
        overlapping.append((lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
    overlapping[0] = (0, d0, 0, d1, 0, d2)
    return {"faces": faces, "empty": [(3, 3, 0, d1, 0, d2), (0, d0, 7, 2, 0, d2), (0, 0, 0, 0, 0, 0), (d0, d0, d1, d1, d2, d2)],
            "single voxel": [(4, 5, 11, 12, 17, 18), (0, 1, 0, 1, 0, 1), (d0 - 1, d0, d1 - 1, d1, d2 - 1, d2)], "whole volume": [(0, d0, 0, d1, 0, d2)],
            "16 overlapping": overlapping}


BAD_BOXES = ([(-1, 3, 0, 5, 0, 5)], [(0, 10, 0, 5, 0, 5)], [(0, 9, 0, 21, 0, 5)], [(0, 9, 0, 5, -2, 5)], [(0, 9, 0, 5, 0, 36)])


# ---- the reference's expressions on the masks -------------------------------------------------------------------------
def masks(seg, t1):
    """(tumour, brain, csf) as step 2 forms them, utils.py:63-68 and step2_mass_effect.py:165-181"""
    x = t1.astype(np.float64)
    tumour = seg > 0
    brain = x > np.percentile(x[x > 0], 5) if x.max() > 0 else x > 0
    csf = (x < np.percentile(x[brain], 15)) & (x > 0) & ~tumour if brain.any() else np.zeros_like(brain)
    return tumour, brain, csf


def shift_mm(brain, vd0, split="midline"):
    """step2_mass_effect.py:66-105 on the brain mask; ``split='dims'`` is the wrong variant that cuts at ``dims[0] // 2``"""
    x = np.where(brain)[0]
    lo, hi = x.min(), x.max()
    midline, width = (lo + hi) / 2, hi - lo
    k = int(midline) if split == "midline" else brain.shape[0] // 2
    left, right = brain.copy(), brain.copy()
    left[k:], right[:k] = 0, 0
    if left.sum() == 0 or right.sum() == 0:
        return 0.0
    left_shift = (ndimage.center_of_mass(left)[0] - (midline - width / 4)) * np.float32(vd0)
    right_shift = (ndimage.center_of_mass(right)[0] - (midline + width / 4)) * np.float32(vd0)
    return float(abs((left_shift + right_shift) / 2))


def draws(n_tumour, n_csf, gen=np.random, unconditional=False):
    """the ranks step2_mass_effect.py:214-225 draws; ``unconditional=True`` is the wrong variant that always draws twice"""
    tumour = gen.choice(n_tumour, min(1000, n_tumour), replace=False)
    if n_csf > 1000 or unconditional:
        csf = gen.choice(n_csf, min(1000, n_csf), replace=False)
    else:
        csf = np.arange(n_csf)
    return tumour, csf


def _moments(values):
    v = np.asarray(values, dtype=np.float64)
    return np.array([v.size, v.sum(), (v * v).sum()])


def host_stats(me, seg, t1, gen=np.random, distance="sampled"):
    """what ``mass_effect.mass_effect_stats`` collects on the device, with scipy and numpy on the host"""
    x = t1.astype(np.float64)
    tumour, brain, csf = masks(seg, t1)
    stats = {"shape": seg.shape, "label_stats": mu.label_stats(seg, 8), "n_brain": int(brain.sum()), "dist2": None}
    if brain.any():
        stats["brain_counts0"] = axis_counts(brain.astype(np.uint8), 1)[0]
        stats["csf_counts0"] = axis_counts(csf.astype(np.uint8), 1)[0]
    if tumour.any():
        dilated = ndimage.binary_dilation(tumour, iterations=me.DILATIONS)
        stats["peritumoral"], stats["distant"] = _moments(x[dilated & ~tumour & brain]), _moments(x[brain & ~dilated])
        stats["tumour_counts0"] = axis_counts(tumour.astype(np.uint8), 1)[0]
        stats["box_counts"] = box_counts(tumour.astype(np.uint8), me.lobe_boxes(seg.shape), 1)
    if tumour.any() and csf.any():
        if distance == "sampled":
            rt, rc = draws(int(tumour.sum()), int(csf.sum()), gen)
            stats["dist2"] = min_pair_dist2(np.flatnonzero(tumour)[rt], np.flatnonzero(csf)[rc], seg.shape)
        else:
            stats["dist2"] = int(mu.edt_sq(~csf)[tumour].min())
    return stats
