"""Case I/O of the feature-extraction steps: one loader, one writer and one command for all six.

A step module declares a ``StepSpec`` - what its command loads, where its voxel sizes come from, what its JSON file holds around
the step's result - and its ``analyze`` / ``main`` are ``run_step`` / ``step_main`` on that record.  ``features.run_all_steps``
assembles each step's file from the same records (``document``), so the file of a step is stated once.
"""
from __future__ import annotations

import argparse
import json
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

import numpy as np

from . import nifti

MODALITIES = ('t1', 't1ce', 't2', 'flair')
#: channels of the stacked volumes, in that order
T1, T1CE, T2, FLAIR = range(4)


@dataclass(frozen=True)
class StepSpec:
    key: str                     # the step's key in ``features`` and the stem of its file there
    title: str                   # the value of 'step'
    description: str             # of the command
    call: Callable               # call(seg, chans, zooms, ctx=None, **step_args): the resident function on device tensors, chans by modality
    summary: Callable            # summary(res): what ``main`` prints after the case id
    modalities: tuple = MODALITIES   # the files the command loads beside the segmentation
    zooms: str = 't1'            # voxel sizes: 't1' (float), 't1_float32' (np.float32 of zooms[:3]) or 'segmentation' (float, its own header)
    voxel_info: bool = True      # whether the file holds 'voxel_info'
    case_id: str = 'files'       # 'files': the prefix of the modality files; 'folder': the name of the input folder
    tail: dict = field(default_factory=dict)   # keys appended after the result
    step_args: tuple = ()        # the keyword arguments ``call`` takes beyond ``ctx``
    input_help: str = 'Input folder containing MRI sequences'


@dataclass
class Case:
    """Host data of a case: nothing here touches the device"""
    case_id: str
    images: dict                 # modality -> NiftiImage, the requested ones
    segmentation: nifti.NiftiImage
    labels: np.ndarray           # uint8 (x, y, z), contiguous


def case_id_and_paths(input_folder):
    """utils.py:71-114: the case id and the T1, T1ce, T2 and FLAIR files of a case folder, in either naming scheme."""
    folder = Path(input_folder)
    files = sorted(folder.glob("*_t1.nii.gz"))
    if files:
        case_id = files[0].name.split('_t1')[0]
    else:
        files = sorted(folder.glob("*-t1n.nii.gz"))
        case_id = files[0].name.split('-t1')[0] if files else folder.name
    for names in ({'t1': '_t1', 't1ce': '_t1ce', 't2': '_t2', 'flair': '_flair'}, {'t1': '-t1n', 't1ce': '-t1c', 't2': '-t2w', 'flair': '-t2f'}):
        if (folder / f"{case_id}{names['t1']}.nii.gz").exists():
            return case_id, {k: folder / f"{case_id}{v}.nii.gz" for k, v in names.items()}
    raise ValueError(f"Could not find MRI files in {folder}")


def load_case(input_folder, segmentation_path, modalities=MODALITIES):
    """Loads the named modalities and the segmentation, each file once.  Without modalities the folder is not looked into and
    only names the case."""
    if modalities:
        case_id, paths = case_id_and_paths(input_folder)
    else:
        case_id, paths = Path(input_folder).name, {}
    images = {k: nifti.load(paths[k]) for k in modalities}
    seg = nifti.load(segmentation_path)
    labels = np.ascontiguousarray(np.round(seg.data).astype(np.uint8))   # (x, y, z) as nibabel hands it to the reference
    return Case(case_id, images, seg, labels)


def to_device(array, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array.astype(dtype))).cuda()


def step_zooms(spec, t1_zooms, segmentation_zooms):
    """The voxel sizes a step works with, in the number type its command has always handed it"""
    if spec.zooms == 'segmentation':
        return [float(v) for v in segmentation_zooms]
    if spec.zooms == 't1_float32':
        return [np.float32(v) for v in tuple(t1_zooms)[:3]]   # header.get_zooms(), utils.py:119
    return [float(v) for v in t1_zooms]


def voxel_info(zooms):
    return {'dimensions_mm': [float(v) for v in zooms], 'volume_mm3': float(np.prod(zooms)), 'volume_cm3': float(np.prod(zooms) / 1000)}


def document(spec, case_id, input_folder, zooms, result):
    """The dict a step's file holds: head, the step's result, tail"""
    res = {'case_id': Path(input_folder).name if spec.case_id == 'folder' else case_id, 'step': spec.title}
    if spec.voxel_info:
        res['voxel_info'] = voxel_info(zooms)
    res.update(result)
    res.update(spec.tail)
    return res


def write_json(path, res):
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    with open(path, 'w') as f:
        json.dump(res, f, indent=2)


def run_step(spec, input_folder, segmentation_path, output_path=None, **step_args):
    """A step as its command runs it: load what the record names, upload, call the resident function, write the file."""
    case = load_case(input_folder, segmentation_path, spec.modalities)
    zooms = step_zooms(spec, case.images['t1'].zooms if 't1' in case.images else None, case.segmentation.zooms)
    chans = {k: to_device(img.data, np.float32) for k, img in case.images.items()}
    res = document(spec, case.case_id, input_folder, zooms, spec.call(to_device(case.labels, np.uint8), chans, zooms, **step_args))
    if output_path:
        write_json(output_path, res)
    return res


def step_main(spec, argv=None, extra_args=None):
    """The command of a step.  ``extra_args(parser)`` adds the step's own arguments and returns ``parsed -> step_args``."""
    ap = argparse.ArgumentParser(description=spec.description)
    ap.add_argument('--input', required=True, help=spec.input_help)
    ap.add_argument('--segmentation', required=True, help='Path to segmentation mask (NIfTI)')
    ap.add_argument('--output', default=None, help='Output path for JSON results')
    step_args = extra_args(ap) if extra_args else (lambda args: {})
    args = ap.parse_args(argv)
    res = run_step(spec, args.input, args.segmentation, args.output, **step_args(args))
    print(f"{res['case_id']}: {spec.summary(res)}")
    return 0
