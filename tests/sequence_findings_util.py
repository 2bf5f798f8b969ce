"""CPU restatements shared by test_sequence_findings_cpu.py, test_gpu_percentile.py and test_gpu_sequence_findings.py (scipy / numpy
only): what csrc/percentile.hip and the flag and moment kernels deliver for the reference's step 1, computed on the host."""
import functools
import hashlib
import importlib
import importlib.util
import json
import os

import numpy as np

import morphology_util as mu

ROOT = mu.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "sequence_findings.json")
SECTIONS = ("region_signal_analysis", "contrast_enhancement", "t2_flair_mismatch", "volumes")
RTOL_STD = 1e-9  # the reference's std is numpy's two-pass formula, ours the exact difference of two squares: the cap step 4 uses
PERCENTILES = (0, 1, 5, 10, 15, 20, 25, 40, 50, 60, 75, 85, 99, 100, 33.3)


def module(name):
    return importlib.import_module("brats_amd." + name)


def generator_tool():
    spec = importlib.util.spec_from_file_location("_gen_sequence_findings_golden", os.path.join(ROOT, "tools", "gen_sequence_findings_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@functools.lru_cache(maxsize=None)
def load_fixture():
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _case_data(name):
    synthetic = module("synthetic")
    case = [c for c in load_fixture()["cases"] if c["name"] == name][0]
    a = case["args"]
    seg = synthetic.shapes_map(a["seed"], tuple(a["shape"]), a["parts"])
    vols = synthetic.mri_with_region_gains(a["seed"] + 1, seg, a["gains"], et_noise=a["et_noise"], zero_channel=a["zero_channel"], sigma=a["sigma"],
                                           brain=a["brain"])
    seg.setflags(write=False)
    vols.setflags(write=False)
    return seg, vols


def fixture_data(case):
    """(label map, [4, ...] float32 volumes) of a fixture case, regenerated from its arguments once (read-only) and checked
    against its hashes"""
    seg, vols = _case_data(case["name"])
    assert hashlib.sha256(seg.tobytes()).hexdigest() == case["sha256"]["seg"], f"label map of case {case['name']} is not the one the fixture was made from"
    assert hashlib.sha256(vols.tobytes()).hexdigest() == case["sha256"]["vols"], f"volumes of case {case['name']} are not the ones the fixture was made from"
    return seg, vols


def flag_map(sf, seg, vols):
    """the flag byte per voxel that sequence_findings builds on the device (utils.py:54-60, :167-178; step1_sequence_findings.py:225-226)"""
    ncr, ed, et = seg == 1, seg == 2, (seg == 3) | (seg == 4)
    flags = (ncr.astype(np.uint8) << sf.NCR) | (ed.astype(np.uint8) << sf.ED) | (et.astype(np.uint8) << sf.ET)
    for c, bit in enumerate(sf.NORMAL):
        data = vols[c].astype(np.float64)
        brain = data > np.percentile(data[data > 0], 5) if data.max() > 0 else data > 0
        flags |= (brain & (seg == 0)).astype(np.uint8) << bit
    flags |= ((mu.dilate(ncr, 2) != 0) & et).astype(np.uint8) << sf.RING
    return flags


def masked_moments(vols, flags):
    out = np.zeros((8, vols.shape[0], 3), dtype=np.float64)
    flat = vols.reshape(vols.shape[0], -1)
    for b in range(8):
        idx = np.flatnonzero((flags.reshape(-1) >> b) & 1)
        for c in range(vols.shape[0]):
            v = flat[c][idx].astype(np.float64)
            out[b, c] = [v.size, v.sum(), (v * v).sum()]
    return out


def order_stats(selected, qs):
    """(below, above, percentiles) of a float32 array as numpy gives them: sorted values at floor(v) and min(floor(v) + 1, m - 1) of
    the virtual index v = (m - 1) * q / 100, and np.percentile of the float64 copy"""
    s = np.sort(selected)
    m = s.size
    v = (m - 1) * np.true_divide(np.asarray(qs, dtype=np.float64), 100)
    lo = np.floor(v).astype(np.int64)
    return s[lo], s[np.minimum(lo + 1, m - 1)], np.percentile(selected.astype(np.float64), qs)


def same_floats(got, want):
    """equal as float32 bits, zeros of either sign equal"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))))


class Comparer:
    """strings, integers, booleans, None, keys and list order equal; floats equal, except a ``std``, which may differ by RTOL_STD
    relative; keeps the largest relative error of a std seen"""

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
            if path.endswith("/std"):
                err = abs(got - want) / abs(want) if want != 0 else abs(got)
                if err > self.worst:
                    self.worst, self.where = err, path
                assert err <= RTOL_STD, (path, got, want, err)
            else:
                assert got == want, (path, got, want)
        else:
            assert want is None or isinstance(want, (bool, int, str)), (path, want)
            assert type(got) is type(want) and got == want, (path, got, want)
