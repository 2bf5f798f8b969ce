"""No GPU: the ensemble-uncertainty symbols are declared, bound and built; ``uncertainty.summarize`` on hand-made counts; the drop-in's
parser; the restatements of tests/uncertainty_util.py and the measured constants the GPU gates of test_gpu_uncertainty_kernels.py use."""
import importlib
import os
import re

import numpy as np
import pytest

import plumbing_util as pu
import uncertainty_util as uu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mi355_sw_partial_folds_moments", "mi355_sw_finish_moments", "mi355_logits_aggregate_m2", "mi355_logits_aggregate_tiles_m2",
               "mi355_head_aggregate_m2", "mi355_uncertainty_maps", "mi355_uncertainty_stats")


@pytest.fixture(scope="module")
def unc(amd):
    return importlib.import_module(amd.__name__ + ".uncertainty")


def test_new_symbols_are_declared_bound_and_built(amd, unc):
    with open(os.path.join(ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    pkg = os.path.dirname(amd._lib.__file__)
    with open(os.path.join(pkg, "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    lib = amd._lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym
        assert sym in amd._lib.EXPORTS, sym
        assert f"lib.{sym}.argtypes" in binding, sym
        assert hasattr(lib, sym), sym
    assert "uncertainty.hip" in amd._build.SOURCES
    for mod, names in ((amd.ops, ("logits_aggregate_m2_", "logits_aggregate_tiles_m2_", "head_aggregate_m2_")),
                       (amd.predictor, ("predict_folds_moments", "finish_sharded_moments")),
                       (unc, ("maps", "region_stats", "summarize", "member_agreement"))):
        for name in names:
            assert callable(getattr(mod, name)), name
    # the reference lines the header names, and the kernels the issue names
    assert "run_brats2021_inference_singlethread.py:97-128" in header and "step5_quality.py:457-500" in header
    with open(os.path.join(pkg, "csrc", "aggregate.hip"), encoding="utf-8") as f:
        src = f.read()
    # (the M2 instantiations of the per-tile kernel, of the tiles kernel and of the one term both add)
    assert "template <bool M2, int NM, typename Source>\n__global__ void head_aggregate_kernel" in src and "mirror_step<M2>" in src
    assert "logits_aggregate_tiles_kernel<decltype(m2)::value>" in src and "finish_moments_kernel" in src


def test_the_package_does_not_import_the_module_by_itself():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import brats_amd; "
            "print(any(k.endswith('.uncertainty') for k in sys.modules))" % ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "False", res.stdout + res.stderr


def test_summarize_on_hand_made_counts(unc):
    # thresholds 0.25, 0.5, 0.75, then |F|; columns of sums: unc.SUM_COLUMNS
    counts = np.array([[1200, 1000, 700, 1000], [10, 0, 0, 0], [0, 0, 0, 0]])
    sums = np.array([[1100.0, 30.0, 400.0, 900.0, 10.0, 250.0, 0.16],
                     [4.0, 0.5, 9.0, 0.0, 0.0, 0.0, 0.04],
                     [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    out = unc.summarize(counts, sums, 1000.0, ("a", "b", "c"))   # 1 cm3 per voxel: every product below is exact
    a = out["a"]
    assert a["voxels"] == 1000 and a["volume_cm3"] == 1000.0 and a["volume_interval_cm3"] == [700.0, 1200.0] and a["expected_volume_cm3"] == 1100.0
    assert a["mean_confidence"] == 0.9 and a["mean_std"] == 0.1 and a["mean_entropy_bits"] == 0.25 and a["boundary_fraction"] == 0.5
    assert a["max_std"] == 0.4
    b = out["b"]   # |F| = 0: no confidence, nothing at the boundary of nothing... the 10 voxels above 0.25 count against max(n50, 1)
    assert b["mean_confidence"] is None and b["mean_std"] is None and b["mean_entropy_bits"] is None
    assert b["volume_cm3"] == 0.0 and b["volume_interval_cm3"] == [0.0, 10.0] and b["boundary_fraction"] == 10.0 and b["max_std"] == 0.2
    c = out["c"]
    assert c["mean_confidence"] is None and c["boundary_fraction"] == 0 and c["volume_interval_cm3"] == [0.0, 0.0] and c["max_std"] == 0.0
    import json
    assert json.loads(json.dumps(out)) == out
    for a in out.values():
        assert a["volume_interval_cm3"][0] <= a["volume_cm3"] <= a["volume_interval_cm3"][1]
    with pytest.raises(ValueError, match="region names"):
        unc.summarize(counts, sums, 2.0, ("a", "b"))
    with pytest.raises(ValueError, match="0.25, 0.5 and 0.75"):
        unc.summarize(counts[:, :3], sums, 2.0, ("a", "b", "c"), thresholds=(0.1, 0.5))
    with pytest.raises(ValueError, match="no probabilities"):
        unc.maps(None, None, nonlin="identity")


def test_the_parser_accepts_and_refuses(amd, capsys):
    parse = amd.driver.parse_args
    base = ["--input", "in", "--output", "out"]
    assert "uncertainty" not in vars(parse(base))   # without the flag the namespace is what it was (tests/test_pipeline_cpu.py pins it)
    assert parse(base + ["--uncertainty"]).uncertainty is True
    a = parse(base + ["--uncertainty", "--analyze", "--dtype", "f16", "--label-format", "nnunet"])
    assert a.uncertainty and a.analyze
    assert parse(base + ["--uncertainty", "--label-format", "brats2021"]).label_format == "brats2021"
    with pytest.raises(SystemExit) as e:
        parse(base + ["--uncertainty", "--sequential"])
    assert e.value.code == 2 and "--uncertainty" in capsys.readouterr().err
    assert parse(base + ["--sequential"]).sequential    # (still accepted alone)


def test_the_measured_constants_are_what_the_restatements_give():
    """T_STD_MEASURED / T_ENT_MEASURED: the float32 restatement against the float64 one on the inputs of the GPU test; the constants
    sit at or just above the measurement (within 5 %), and the special voxels give exact values in both."""
    worst_s = worst_e = 0.0
    for nonlin in ("sigmoid", "softmax"):
        a, b = uu.maps_case(10, nonlin), uu.maps_case(11, nonlin, True)
        for second in ((None, None), b):
            m32, m64 = uu.maps32(*a, *second, nonlin=nonlin), uu.maps64(*a, *second, nonlin=nonlin)
            assert all(np.isfinite(v).all() for v in m32.values())
            worst_s = max(worst_s, float(np.abs(m32["std"] - m64["std"]).max()))
            worst_e = max(worst_e, float(np.abs(m32["entropy"] - m64["entropy"]).max()))
            if second[0] is None:
                assert (m32["var"].reshape(3, -1)[:, :45] == 0).all() and (m64["var"].reshape(3, -1)[:, :5] == 0).all()
    print(f"measured: std {worst_s:.3e}, entropy {worst_e:.3e}")
    assert 0.95 * uu.T_STD_MEASURED <= worst_s <= uu.T_STD_MEASURED and 0.95 * uu.T_ENT_MEASURED <= worst_e <= uu.T_ENT_MEASURED
    m = uu.maps64(*uu.maps_case(10, "sigmoid"))
    e = m["entropy"].reshape(3, -1)
    assert (e[:, :2] == 0).all() and (e[:, 2] == 1).all() and np.allclose(e[:, 3:5], 0.8112781244591328)


def test_tile_moments_are_the_moments_of_the_mirror_samples():
    """res = the float64 tile_result of plumbing_util, res2 - res^2 = the variance over the mirror list, voxel by voxel"""
    mirrors = pu.MIRROR_LISTS["zyx"]
    lg = pu.logits_case(8, 3, pu.AGG_PATCH, 5)[pu.AGG_FIRST:]
    for nonlin in ("sigmoid", "softmax"):
        res, res2 = uu.tile_moments(lg, mirrors, pu.AGG_PATCH, nonlin)
        assert np.allclose(res, pu.tile_result(lg, mirrors, pu.AGG_PATCH, nonlin, np.float64), rtol=0, atol=1e-15)
        samples = np.stack([pu.flip_tile(pu.nonlin64(lg[i], nonlin).reshape(res.shape), m) for i, m in enumerate(mirrors)])
        assert np.allclose(res2 - res * res, samples.var(0), rtol=0, atol=1e-14) and (res2 - res * res).max() > 1e-3


def test_stats_restatement_counts_strictly():
    mean = np.array([[0.25, 0.5, 0.75, 0.7500001, 0.2, 1.0]], np.float32)
    counts, sums, _ = uu.stats64(mean, mean * 0 + np.float32(0.1), mean * 0 + 1)
    assert counts.tolist() == [[4, 3, 2, 3]] and np.isclose(sums[0, 3], 0.75 + 0.7500001 + 1.0) and sums[0, 6] == np.float32(0.1)
