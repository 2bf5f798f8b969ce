"""``brats_amd.case_io``: what ``load_case`` reads, the document each of the six step records makes ``run_step`` assemble, and
the layering of the package's imports.  No device: the upload and the resident functions are replaced."""
import ast
import importlib
import json
from pathlib import Path

import numpy as np
import pytest

SHAPE = (3, 4, 5)
SCHEMES = {"underscore": ("BraTS2021_00000", {"t1": "_t1", "t1ce": "_t1ce", "t2": "_t2", "flair": "_flair"}),
           "hyphen": ("BraTS-GLI-00000-000", {"t1": "-t1n", "t1ce": "-t1c", "t2": "-t2w", "flair": "-t2f"})}
STEP_MODULES = ("sequence_findings", "mass_effect", "multiplicity", "morphology", "quality", "normal_structures")
ALL, T1_ONLY, NONE = ("t1", "t1ce", "t2", "flair"), ("t1",), ()
LOADED = dict(zip(STEP_MODULES, (ALL, T1_ONLY, NONE, ALL, ALL, ALL)))


def _mod(name):
    return importlib.import_module("brats_amd." + name)


def _write_case(folder, scheme, zooms=(1.0, 1.0, 1.0), seg_zooms=None):
    """A 3 x 4 x 5 case in ``folder / 'case_dir'``; the stored label map holds a 2.6.  Returns (case folder, segmentation path, paths)."""
    nifti = _mod("nifti")
    case_dir = folder / "case_dir"
    case_dir.mkdir()
    case_id, suffix = SCHEMES[scheme]
    rng = np.random.RandomState(3)
    paths = {}
    for k, sfx in suffix.items():
        paths[k] = case_dir / f"{case_id}{sfx}.nii.gz"
        nifti.save_like(paths[k], rng.rand(*SHAPE).astype(np.float32), nifti.make_header(SHAPE, zooms, dtype=np.float32))
    seg = np.zeros(SHAPE, dtype=np.float32)
    seg[1, 1, 1], seg[1, 2, 3], seg[2, 0, 0] = 2.6, 1.4, 4.0
    seg_path = folder / "seg.nii.gz"
    nifti.save_like(seg_path, seg, nifti.make_header(SHAPE, seg_zooms or zooms, dtype=np.float32))
    return case_dir, seg_path, paths


@pytest.fixture
def counted_loads(monkeypatch):
    nifti = _mod("nifti")
    seen, real = [], nifti.load
    monkeypatch.setattr(nifti, "load", lambda path: (seen.append(Path(path)), real(path))[1])
    return seen


# ---- load_case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_load_case_loads_exactly_the_files_a_step_names_once_each(tmp_path, counted_loads, scheme):
    case_io = _mod("case_io")
    case_dir, seg_path, paths = _write_case(tmp_path, scheme)
    for name in STEP_MODULES:
        spec = _mod(name).STEP_SPEC
        assert spec.modalities == LOADED[name], name
        del counted_loads[:]
        case = case_io.load_case(case_dir, seg_path, spec.modalities)
        assert sorted(counted_loads) == sorted([paths[k] for k in LOADED[name]] + [seg_path]), name   # 4 + 1, T1 + 1, the segmentation alone
        assert list(case.images) == list(LOADED[name])
        assert case.case_id == (SCHEMES[scheme][0] if LOADED[name] else "case_dir")
        assert case.labels.dtype == np.uint8 and case.labels.flags["C_CONTIGUOUS"] and case.labels.shape == SHAPE
        assert case.labels[1, 1, 1] == 3 and case.labels[1, 2, 3] == 1 and case.labels[2, 0, 0] == 4 and int(case.labels.sum()) == 8   # 2.6 -> 3
        assert case.segmentation.zooms == (1.0, 1.0, 1.0)


def test_load_case_without_modalities_does_not_look_into_the_folder(tmp_path, counted_loads, monkeypatch):
    case_io = _mod("case_io")
    _, seg_path, _ = _write_case(tmp_path, "underscore")
    monkeypatch.setattr(case_io, "case_id_and_paths", lambda folder: pytest.fail("step 3 names the case after the folder"))
    case = case_io.load_case(tmp_path / "no_such_folder", seg_path, ())
    assert case.case_id == "no_such_folder" and case.images == {} and counted_loads == [seg_path]


def test_a_folder_without_modalities_is_refused(tmp_path):
    case_io = _mod("case_io")
    _, seg_path, _ = _write_case(tmp_path, "hyphen")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="Could not find MRI files in "):
        case_io.load_case(empty, seg_path, ("t1",))
    with pytest.raises(ValueError) as err:
        case_io.case_id_and_paths(empty)
    assert str(err.value) == f"Could not find MRI files in {empty}"


# ---- the six records --------------------------------------------------------------------------------------------------
FAKE = {"alpha": 1, "beta": {"x": 2.5, "y": [True, None]}}
RESIDENT = {"sequence_findings": ("sequence_findings", "sequence_findings"), "mass_effect": ("mass_effect", "mass_effect"),
            "multiplicity": ("components", "lesion_multiplicity"), "morphology": ("morphology", "tumor_morphology"),
            "quality": ("quality", "quality_control"), "normal_structures": ("normal_structures", "normal_structures")}
# (T1 zooms, segmentation zooms) -> voxel_info as the float steps write it, as step 2 writes it (float32 products), as step 3
# writes it (the segmentation's header)
ZOOMS = [((1.0, 1.0, 1.0), (1.0, 1.0, 1.0)), ((0.5, 1.25, 2.0), (2.0, 1.25, 0.5))]
VOXEL_INFO = {ZOOMS[0]: {"float": {"dimensions_mm": [1.0, 1.0, 1.0], "volume_mm3": 1.0, "volume_cm3": 0.001},
                         "float32": {"dimensions_mm": [1.0, 1.0, 1.0], "volume_mm3": 1.0, "volume_cm3": 0.0010000000474974513},
                         "segmentation": {"dimensions_mm": [1.0, 1.0, 1.0], "volume_mm3": 1.0, "volume_cm3": 0.001}},
              ZOOMS[1]: {"float": {"dimensions_mm": [0.5, 1.25, 2.0], "volume_mm3": 1.25, "volume_cm3": 0.00125},
                         "float32": {"dimensions_mm": [0.5, 1.25, 2.0], "volume_mm3": 1.25, "volume_cm3": 0.0012499999720603228},
                         "segmentation": {"dimensions_mm": [2.0, 1.25, 0.5], "volume_mm3": 1.25, "volume_cm3": 0.00125}}}
CASE_ID = SCHEMES["underscore"][0]


def expected_documents(zooms):
    """What the six ``analyze`` functions returned and wrote before they shared ``run_step``, for the resident result FAKE"""
    v = VOXEL_INFO[zooms]
    return {"sequence_findings": {"case_id": CASE_ID, "step": "Step 1 - Sequence-specific findings", "voxel_info": v["float"], "alpha": 1,
                                  "beta": {"x": 2.5, "y": [True, None]}, "sequences_analyzed": ["T1", "T1ce", "T2", "FLAIR"], "diffusion_available": False,
                                  "diffusion_note": "DWI/ADC not available in standard BraTS dataset"},
            "mass_effect": {"case_id": CASE_ID, "step": "Step 2 - Mass effect metrics", "voxel_info": v["float32"], "alpha": 1,
                            "beta": {"x": 2.5, "y": [True, None]}},
            "multiplicity": {"case_id": "case_dir", "step": "Step 3 - Lesion multiplicity and distribution", "voxel_info": v["segmentation"], "alpha": 1,
                             "beta": {"x": 2.5, "y": [True, None]}},
            "morphology": {"case_id": CASE_ID, "step": "Step 4 - Tumor morphology and margins", "voxel_info": v["float"], "alpha": 1,
                           "beta": {"x": 2.5, "y": [True, None]}},
            "quality": {"case_id": CASE_ID, "step": "Step 5 - Quality control and confidence metrics", "alpha": 1, "beta": {"x": 2.5, "y": [True, None]}},
            "normal_structures": {"case_id": CASE_ID, "step": "Step 6 - Normal structures assessment", "alpha": 1, "beta": {"x": 2.5, "y": [True, None]}}}


def _same_types(a, b):
    assert type(a) is type(b), (a, b)
    if isinstance(a, dict):
        assert list(a) == list(b)
        for k in a:
            _same_types(a[k], b[k])
    elif isinstance(a, list):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same_types(x, y)


@pytest.mark.parametrize("zooms", ZOOMS, ids=["unit", "anisotropic"])
def test_each_record_assembles_the_document_its_command_has_always_written(tmp_path, monkeypatch, zooms):
    case_io = _mod("case_io")
    case_dir, seg_path, _ = _write_case(tmp_path, "underscore", zooms[0], zooms[1])
    monkeypatch.setattr(case_io, "to_device", lambda array, dtype: np.ascontiguousarray(array.astype(dtype)))
    calls = {}
    for name, (module, function) in RESIDENT.items():
        monkeypatch.setattr(_mod(module), function, lambda *args, _name=name, **kwargs: (calls.__setitem__(_name, (args, kwargs)), dict(FAKE))[1])
    rng = np.random.RandomState(5)
    for name, want in expected_documents(zooms).items():
        out = tmp_path / "results" / name / "step.json"   # (the writer makes the folders)
        more = {"rng": rng, "distance": "exact"} if name == "mass_effect" else {}
        got = _mod(name).analyze(case_dir, seg_path, out, **more)
        assert got == want and list(got) == list(want), name
        _same_types(got, want)
        assert out.read_text() == json.dumps(want, indent=2), name
        args, kwargs = calls[name]
        assert args[0].dtype == np.uint8 and args[0][1, 1, 1] == 3 and kwargs in ({}, {"ctx": None})
        voxel_dims = args[1] if name == "multiplicity" else args[2] if name == "mass_effect" else args[5]
        assert len(args) == {"multiplicity": 2, "mass_effect": 5}.get(name, 6)
        assert all(a.dtype == np.float32 and a.shape == SHAPE for a in args[1:-1 if name != "mass_effect" else 2])
        if name == "mass_effect":   # np.float32 of zooms[:3], then rng and distance
            assert [type(z) for z in voxel_dims] == [np.float32] * 3 and [float(z) for z in voxel_dims] == list(zooms[0])
            assert args[3] is rng and args[4] == "exact"
        else:
            assert [type(z) for z in voxel_dims] == [float] * 3 and voxel_dims == list(zooms[1] if name == "multiplicity" else zooms[0])
    assert _mod("mass_effect").analyze(case_dir, seg_path) == expected_documents(zooms)["mass_effect"]   # rng None, distance 'sampled'
    assert calls["mass_effect"][0][3] is None and calls["mass_effect"][0][4] == "sampled"


def test_the_records_are_the_six_steps_of_features_in_order():
    features = _mod("features")
    assert [spec.key for spec in features.SPECS] == ["step1_sequence_findings", "step2_mass_effect", "step3_multiplicity", "step4_morphology", "step5_quality",
                                                     "step6_normal_structures"]
    assert [spec is _mod(name).STEP_SPEC for spec, name in zip(features.SPECS, STEP_MODULES)] == [True] * 6


def test_a_command_prints_its_one_line_and_takes_its_own_arguments(tmp_path, monkeypatch, capsys):
    case_io = _mod("case_io")
    case_dir, seg_path, _ = _write_case(tmp_path, "underscore")
    monkeypatch.setattr(case_io, "to_device", lambda array, dtype: np.ascontiguousarray(array.astype(dtype)))
    seen = {}
    result = {"component_analysis": {"description": "Single lesion"}, "distribution_pattern": {"pattern": "Unifocal"}, "enhancing_analysis": {"pattern": "None"}}
    monkeypatch.setattr(_mod("components"), "lesion_multiplicity", lambda seg, zooms, ctx=None: dict(result))
    assert _mod("multiplicity").main(["--input", str(case_dir), "--segmentation", str(seg_path)]) == 0
    assert capsys.readouterr().out == "case_dir: Single lesion; Unifocal; None\n"
    result = {"anatomical_location": {"laterality": "Unilateral (left hemisphere)", "primary_lobe": "frontal"}, "midline_shift": {"severity": "None"},
              "ventricular_compression": {"severity": "Mild"}, "sulcal_effacement": {"severity": "None/Minimal"}, "herniation_risk": {"risk_level": "Low"}}
    monkeypatch.setattr(_mod("mass_effect"), "mass_effect", lambda seg, t1, zooms, rng, distance, ctx=None: (seen.update(rng=rng, distance=distance), dict(result))[1])
    assert _mod("mass_effect").main(["--input", str(case_dir), "--segmentation", str(seg_path), "--distance", "exact", "--seed", "7"]) == 0
    assert capsys.readouterr().out == (f"{CASE_ID}: Unilateral (left hemisphere), frontal; midline shift None; ventricles Mild; sulci None/Minimal; "
                                       "herniation risk Low\n")
    assert seen["distance"] == "exact" and seen["rng"].randint(1 << 30) == np.random.RandomState(7).randint(1 << 30)
    with pytest.raises(SystemExit):
        _mod("multiplicity").main(["--input", str(case_dir), "--segmentation", str(seg_path), "--seed", "7"])


# ---- layering ---------------------------------------------------------------------------------------------------------
def _package_sources():
    folder = Path(_mod("case_io").__file__).parent
    return {p.name: ast.parse(p.read_text()) for p in sorted(folder.glob("*.py"))}


def test_no_module_imports_an_underscore_name_from_a_sibling():
    found = []
    for name, tree in _package_sources().items():
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level >= 1 and node.module:
                found += [f"{name}:{node.lineno}: from .{node.module} import {a.name}" for a in node.names if a.name.startswith("_")]
    assert not found, found


def test_features_imports_normal_structures_at_the_top_only():
    tree = _package_sources()["features.py"]
    local = []
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
            for node in ast.walk(fn):
                if isinstance(node, ast.ImportFrom) and ((node.module or "").endswith("normal_structures") or any(a.name == "normal_structures" for a in node.names)):
                    local.append(node.lineno)
                if isinstance(node, ast.Import) and any(a.name.endswith("normal_structures") for a in node.names):
                    local.append(node.lineno)
    assert not local, local
