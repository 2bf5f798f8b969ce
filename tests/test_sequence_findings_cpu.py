"""Device percentiles and sequence findings (the reference's step 1) without a device.

tests/golden/sequence_findings.json holds what the reference's own step 1 (feature_extraction/step1_sequence_findings.py,
imported unmodified by tools/gen_sequence_findings_golden.py) returned for seeded synthetic cases.  Here what the device would
deliver is computed with scipy and numpy, so these tests pin the host arithmetic - numpy's percentile interpolation and the
dict building -, the fixture and the interface declarations."""
import os
import re

import numpy as np
import pytest

import sequence_findings_util as su
from oracle import ref_shim


def _values(rs, kind, n):
    if kind == "integers":
        return rs.randint(1, 4000, n).astype(np.float32)
    if kind == "gaussian":
        return (rs.standard_normal(n) * 300 + 500).astype(np.float32)
    return rs.randint(1, 6, n).astype(np.float32)  # five distinct values, heavy ties


def test_percentile_from_order_stats_is_np_percentile_bit_for_bit(amd):
    pct = su.module("percentile")
    rs = np.random.RandomState(0)
    lengths = [1, 2, 3] + [int(v) for v in rs.randint(1, 5001, 117)]
    checked = 0
    for i, n in enumerate(lengths):
        for kind in ("integers", "gaussian", "ties"):
            v = _values(rs, kind, n)
            below, above, want = su.order_stats(v, su.PERCENTILES)
            got = pct.percentile_from_order_stats(n, su.PERCENTILES, below, above)
            assert got.dtype == np.float64 and got.shape == want.shape
            assert np.array_equal(got, want), (n, kind, got, want)
            for q, b, a, w in zip(su.PERCENTILES[::4], below[::4], above[::4], want[::4]):  # scalars too
                assert float(pct.percentile_from_order_stats(n, q, b, a)) == w
            checked += got.size
    assert checked == len(lengths) * 3 * len(su.PERCENTILES)


def test_sequence_findings_from_stats_reproduces_the_reference(amd):
    sf = su.module("sequence_findings")
    cmp = su.Comparer()
    for case in su.load_fixture()["cases"]:
        seg, vols = su.fixture_data(case)
        got = sf.sequence_findings_from_stats(su.masked_moments(vols, su.flag_map(sf, seg, vols)), case["voxel_dims"])
        assert tuple(got) == su.SECTIONS
        cmp.same(got, case["expected"], case["name"])
    print(f"largest relative error of a std: {cmp.worst:.3g} at {cmp.where}")


def test_fixture_reaches_the_branch_table():
    cases = {c["name"]: c for c in su.load_fixture()["cases"]}
    exp = {k: c["expected"] for k, c in cases.items()}
    regions = [r for e in exp.values() for r in e["region_signal_analysis"]["regions"].values()]
    assert {r[s]["signal_label"] for r in regions for s in ("T1", "T2", "FLAIR", "T1ce")} == {
        "markedly hypointense", "hypointense", "isointense", "hyperintense", "markedly hyperintense"}
    ce = [e["contrast_enhancement"] for e in exp.values()]
    assert {c["heterogeneity"] for c in ce} == {"Not applicable", "Homogeneous", "Mildly heterogeneous", "Heterogeneous", "Markedly heterogeneous"}
    assert {c["enhancement_strength"] for c in ce if "enhancement_strength" in c} == {
        "Marked enhancement", "Strong enhancement", "Moderate enhancement", "Mild enhancement", "Minimal/equivocal enhancement"}
    assert {c["pattern"] for c in ce} == {"Ring-enhancing", "Solid/nodular enhancing", "Non-enhancing"}
    solid = [k for k, e in exp.items() if e["contrast_enhancement"]["pattern"] == "Solid/nodular enhancing"]
    assert [k for k in solid if "ncr" in exp[k]["region_signal_analysis"]["regions"]], "no solid enhancement with a necrotic core"
    assert [k for k in solid if "ncr" not in exp[k]["region_signal_analysis"]["regions"]], "no solid enhancement without a necrotic core"
    assert {e["t2_flair_mismatch"]["mismatch_detected"] for e in exp.values()} == {True, False}
    assert {e["t2_flair_mismatch"].get("region") for e in exp.values()} >= {"ncr", "ed"}  # found in the first region and in a later one
    assert [e for e in exp.values() if 0 < len(e["region_signal_analysis"]["regions"]) < 3], "no case with a missing region"
    none = [e for e in exp.values() if not e["region_signal_analysis"]["regions"]]
    assert none and all(v == 0.0 for v in none[0]["volumes"].values()) and none[0]["contrast_enhancement"]["pattern"] == "Non-enhancing"
    zero = [e for e in exp.values() if e["region_signal_analysis"]["normal_brain_reference"]["T1_mean"] is None]
    assert zero and all(r["T1"]["ratio_to_normal"] == 1.0 for r in zero[0]["region_signal_analysis"]["regions"].values())
    assert zero[0]["region_signal_analysis"]["normal_brain_reference"]["voxel_count"] == 0
    assert [c for c in cases.values() if any(p[1] == 4 for p in c["args"]["parts"])], "no case with label 4"
    assert [c for c in cases.values() if c["args"]["shape"] == [240, 240, 155]]
    assert [c for c in cases.values() if len(set(c["voxel_dims"])) > 1]


def test_fixture_keeps_clear_of_every_threshold_and_rounding_boundary():
    tool = su.generator_tool()
    data = su.load_fixture()
    assert tool.too_close(data) == []
    assert sum(len(tool.scores(c["expected"])) for c in data["cases"]) >= 100
    assert sum(len(tool.rounded(c["expected"])) for c in data["cases"]) >= 80
    assert os.path.getsize(su.FIXTURE) < 100 * 1024


def test_fixture_is_what_the_reference_returns_today():
    if not ref_shim.reference_available():
        pytest.skip("the reference tree is not on this machine")
    assert su.generator_tool().generate() == su.load_fixture()


def test_fixture_volumes_match_their_hashes_and_are_integers_below_2_24(amd):
    for case in su.load_fixture()["cases"]:
        if case["args"]["shape"] == [240, 240, 155]:
            continue  # (regenerated and hashed by the comparison above)
        _, vols = su.fixture_data(case)
        assert vols.dtype == np.float32 and np.array_equal(vols, np.rint(vols)) and 0 <= vols.min() and vols.max() < 2 ** 24


def test_new_symbol_is_declared_exported_and_bound(amd):
    with open(os.path.join(su.ROOT, "include", "mi355_nnunet.h"), encoding="utf-8") as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(amd._lib.__file__), "_lib.py"), encoding="utf-8") as f:
        binding = f.read()
    sym = "mi355_masked_percentiles"
    assert re.search(r"\bint " + sym + r"\(", header)
    assert sym in amd._lib.EXPORTS and f"lib.{sym}.argtypes" in binding
    assert "percentile.hip" in amd._build.SOURCES
    import ctypes
    lib = ctypes.CDLL(str(amd._lib.lib_path()))
    assert hasattr(lib, sym) and lib.mi355_version() >= 102
    pct, sf = su.module("percentile"), su.module("sequence_findings")
    for mod, names in ((pct, ("percentile_from_order_stats", "masked_percentiles", "masked_order_stats", "intensity_stats")),
                       (sf, ("sequence_findings", "sequence_findings_from_stats", "region_flags", "analyze", "main")),
                       (su.module("synthetic"), ("mri_with_region_gains",))):
        for name in names:
            assert callable(getattr(mod, name)), name


def test_new_modules_do_not_import_the_oracle(amd):
    pkg = os.path.dirname(su.module("percentile").__file__)
    for name in ("percentile.py", "sequence_findings.py"):
        with open(os.path.join(pkg, name), encoding="utf-8") as f:
            text = f.read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), name
        assert "reference" not in [m.group(1) for m in re.finditer(r"^\s*(?:from|import)\s+(\w+)", text, flags=re.M)], name
