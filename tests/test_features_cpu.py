"""The batch planner of the batched percentile select, and that the new entry point, module and keyword are where the six
steps and ``brats_amd.features`` expect them.  No device."""
import importlib
import inspect
import os
import re

import numpy as np

import morphology_util as mu

NEW_SYMBOLS = ("mi355_masked_percentiles_multi",)
T1, T1CE, T2, FLAIR = "t1", "t1ce", "t2", "flair"   # the planner compares volumes by identity only
BRAIN = 1


def _mod(name):
    return importlib.import_module("brats_amd." + name)


def the_22_requests():
    """What the six steps ask per case: 14 selects over the positive voxels, 8 over the brain mask"""
    pos = lambda x, q: (x, q, 0, 0, 0.0, np.inf)
    brain = lambda x, q: (x, q, BRAIN, 0, -np.inf, np.inf)
    reqs = [pos(T1, 5)] * 4 + [pos(T1, 10)] * 2                               # steps 1, 2, 5, 6; steps 4, 5
    reqs += [pos(T1CE, 5), pos(T1CE, 10)]                                     # steps 1, 5
    reqs += [pos(T2, 5), pos(T2, 10), pos(T2, 85)]                            # steps 1, 5, 4
    reqs += [pos(FLAIR, 5), pos(FLAIR, 10), pos(FLAIR, 20)]
    reqs += [brain(T1, 15)] * 2 + [brain(T2, 85), brain(FLAIR, 25)]           # steps 2, 6; step 6
    reqs += [brain(x, (1, 25, 75, 99)) for x in (T1, T1CE, T2, FLAIR)]        # step 5
    assert len(reqs) == 22
    return reqs


def _fake_results(batches):
    """(count, values) per entry with a value that names its volume, predicate and percentile"""
    return [[(7, np.array([hash((x, require, q)) % 1000 + q / 1000 for q in qs], dtype=np.float64)) for x, qs, require, _, _, _ in batch] for batch in batches]


def test_the_22_requests_of_a_case_collapse_to_two_batches(amd):
    reqs = the_22_requests()
    batches, back = _mod("percentile").plan_percentile_batches(reqs)
    assert len(batches) == 2 and [len(b) for b in batches] == [4, 4]
    assert all(len(qs) <= 8 and len(set(qs)) == len(qs) for b in batches for _, qs, *_ in b)
    assert sorted((x, qs) for x, qs, *_ in batches[0]) == [(FLAIR, (5.0, 10.0, 20.0)), (T1, (5.0, 10.0)), (T1CE, (5.0, 10.0)), (T2, (5.0, 10.0, 85.0))]
    assert all(require == BRAIN for _, _, require, *_ in batches[1])
    assert sum(len(qs) for _, qs, *_ in batches[1]) == 18
    got = _mod("percentile").gather_planned(_fake_results(batches), back)
    assert len(got) == len(reqs)
    for (x, qs, require, *_), (count, values) in zip(reqs, got):
        assert count == 7
        assert values.tolist() == [hash((x, require, float(q))) % 1000 + float(q) / 1000 for q in np.atleast_1d(qs)]


def test_batches_hold_four_volumes_and_eight_percentiles_at_most(amd):
    plan = _mod("percentile").plan_percentile_batches
    vols = [object() for _ in range(9)]
    batches, back = plan([(v, (50, 25)) for v in vols])
    assert [len(b) for b in batches] == [4, 4, 1]
    assert [p[0][:2] for p in back] == [(k // 4, k % 4) for k in range(9)]
    # the same volume under another predicate is another entry
    batches, _ = plan([(vols[0], 5, 0, 0, 0.0, np.inf), (vols[0], 5, 1, 0), (vols[0], 5, 0, 2), (vols[0], 5, 0, 0, 0.0, 9.0), (vols[0], 5, 0, 0, 0.0, np.inf)])
    assert [len(b) for b in batches] == [4]
    # a ninth distinct percentile for one volume opens a new batch; a repeated one does not
    batches, back = plan([(vols[0], (1, 2, 3, 4, 5, 6, 7, 8)), (vols[0], 8), (vols[0], 9), (vols[1], 50), (vols[0], (9, 1))])
    assert len(batches) == 2 and batches[0][0][1] == (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0) and batches[1][0][:2] == (vols[0], (9.0,))
    assert batches[0][1][:2] == (vols[1], (50.0,))
    assert back[1] == [(0, 0, 7)] and back[2] == [(1, 0, 0)] and back[4] == [(1, 0, 0), (0, 0, 0)]
    got = _mod("percentile").gather_planned([[(3, np.arange(8.0)), (4, np.array([50.0]))], [(3, np.array([90.0]))]], back)
    assert [g[1].tolist() for g in got] == [list(np.arange(8.0)), [7.0], [90.0], [50.0], [90.0, 0.0]] and [g[0] for g in got] == [3, 3, 3, 4, 3]
    assert plan([]) == ([], [])


def test_the_context_asks_for_what_the_steps_ask(amd):
    f = _mod("features")
    reqs = the_22_requests()
    names = {T1: 0, T1CE: 1, T2: 2, FLAIR: 3}
    for x, qs, require, *_ in reqs:
        have = (f.BRAIN_QS if require else f.POSITIVE_QS)[names[x]]
        assert all(q in have for q in np.atleast_1d(qs)), (x, qs, require)
    assert all(len(v) <= 8 for v in list(f.POSITIVE_QS.values()) + list(f.BRAIN_QS.values()))
    assert sum(len(v) for v in f.POSITIVE_QS.values()) == 10 and sum(len(v) for v in f.BRAIN_QS.values()) == 18


def test_symbol_is_declared_exported_and_bound(amd):
    with open(os.path.join(mu.ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(amd._lib.__file__), "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    import ctypes
    lib = ctypes.CDLL(str(amd._lib.lib_path()))
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint " + sym + r"\(", header), sym
        assert sym in amd._lib.EXPORTS and f"lib.{sym}.argtypes" in binding, sym
        assert hasattr(lib, sym), sym
    assert "run_all.py:411-446" in header and "step5_quality.py:210-212" in header
    for name in ("masked_percentiles_multi", "masked_order_stats_multi", "plan_percentile_batches", "gather_planned"):
        assert callable(getattr(_mod("percentile"), name)), name
    for name in ("CaseContext", "extract_all", "run_all_steps", "main"):
        assert callable(getattr(_mod("features"), name)), name


def test_the_six_resident_functions_take_a_context(amd):
    fns = (_mod("sequence_findings").sequence_findings, _mod("mass_effect").mass_effect, _mod("components").lesion_multiplicity, _mod("morphology").tumor_morphology,
           _mod("quality").quality_control, _mod("normal_structures").normal_structures, _mod("sequence_findings").region_flags, _mod("mass_effect").mass_effect_stats,
           _mod("morphology").region_flags, _mod("quality").quality_stats, _mod("normal_structures").normal_structures_stats)
    for fn in fns:
        p = inspect.signature(fn).parameters
        assert "ctx" in p and p["ctx"].default is None, fn.__name__
    p = inspect.signature(_mod("mass_effect").mass_effect).parameters
    assert list(p)[:5] == ["seg", "t1", "voxel_dims", "rng", "distance"] and p["distance"].default == "sampled"
    p = inspect.signature(_mod("features").extract_all).parameters
    assert list(p) == ["seg", "t1", "t1ce", "t2", "flair", "voxel_dims", "rng", "distance"] and p["rng"].default is None and p["distance"].default == "sampled"


def test_features_does_not_import_the_oracle(amd):
    with open(_mod("features").__file__, encoding="utf-8") as f:
        text = f.read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M)


def test_the_command_takes_the_arguments_of_the_reference(amd, capsys):
    import pytest
    with pytest.raises(SystemExit):
        _mod("features").main(["--input", "x"])
    err = capsys.readouterr().err
    assert "--segmentation" in err and "--output" in err
    assert _mod("features").STEP_KEYS == ("step1_sequence_findings", "step2_mass_effect", "step3_multiplicity", "step4_morphology", "step5_quality",
                                          "step6_normal_structures")
