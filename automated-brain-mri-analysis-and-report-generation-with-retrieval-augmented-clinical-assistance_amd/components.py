"""Connected components on the device and the reference's lesion multiplicity.

``feature_extraction/step3_multiplicity.py`` labels the tumour mask once with ``scipy.ndimage.label`` and then, per
component, compares the whole labelled volume with the component id and runs ``np.where`` on the result (:63-121,
:227-242).  Here one labelling pass and one statistics pass on the device give an integer table per component (voxel
count, coordinate sums, bounding box, voxels per label value), and everything step 3 reports is host arithmetic on those
integers, in the reference's order of operations (``multiplicity_from_stats``: a pure function, testable without a device).
The report prose of step 3 (clinical implication, differentials, enhancement note, text summary) is out of scope.

``remove_all_but_the_largest_connected_component`` is nnU-Net v1's post-processing function of that name; its source is
not part of the reference tree (parity unpinned).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .volume_ops import check_volume

#: columns of the per-component table (mi355_component_stats)
COUNT, SUM0, MIN0, MAX0, SEG1 = 0, 1, 4, 7, 10
NCOL = 14
MAX_COMPONENTS = 65536

# step3_multiplicity.py:33-38
SATELLITE_DISTANCE_MM = 20
SEPARATE_DISTANCE_MM = 40
MIN_LESION_VOLUME_CM3 = 0.1


def label_components(mask, connectivity=1):
    """mask: CUDA uint8 [d0, d1, d2], foreground = nonzero.  connectivity 1 (6 neighbours, scipy's default structure) or 3
    (26 neighbours, ``generate_binary_structure(3, 3)``).  Returns (int32 CUDA label map, n): components numbered 1..n in
    raster order of their first voxel, exactly as ``scipy.ndimage.label`` numbers them."""
    import torch
    mask = check_volume(mask, torch.uint8, "label_components")
    labels = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    n = C.c_int32(0)
    stream = torch.cuda.current_stream(mask.device).cuda_stream
    _lib.check(_lib.load().mi355_label_components(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2], int(connectivity),
                                                  labels.data_ptr(), C.byref(n), stream), "mi355_label_components")
    return labels, int(n.value)


def label_components_neighbours(mask, neighbours):
    """``label_components`` with the neighbourhood named by its size: 6, 18 (faces and edges, ``generate_binary_structure(3, 2)``:
    what ``feature_extraction/step6_normal_structures.py:66-67`` labels with) or 26."""
    import torch
    mask = check_volume(mask, torch.uint8, "label_components_neighbours")
    labels = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    n = C.c_int32(0)
    stream = torch.cuda.current_stream(mask.device).cuda_stream
    _lib.check(_lib.load().mi355_label_components_nb(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2], int(neighbours),
                                                     labels.data_ptr(), C.byref(n), stream), "mi355_label_components_nb")
    return labels, int(n.value)


def component_stats(labels, n, seg=None):
    """labels: the map of ``label_components``, n its component count, seg: optional CUDA uint8 map of the same shape.
    Returns int64 [n, 14]: count, coordinate sums (3), minima (3), maxima (3), voxels with seg value 1, 2, 3, 4."""
    import torch
    labels = check_volume(labels, torch.int32, "component_stats")
    seg_ptr = None
    if seg is not None:
        seg = check_volume(seg, torch.uint8, "component_stats")
        if seg.shape != labels.shape:
            raise ValueError("component_stats: seg and labels differ in shape")
        seg_ptr = seg.data_ptr()
    out = np.zeros((max(int(n), 0), NCOL), dtype=np.int64)
    stream = torch.cuda.current_stream(labels.device).cuda_stream
    _lib.check(_lib.load().mi355_component_stats(labels.data_ptr(), seg_ptr, labels.shape[0], labels.shape[1], labels.shape[2], int(n),
                                                 out.ctypes.data_as(C.POINTER(C.c_int64)), stream), "mi355_component_stats")
    return out


def component_filter(labels, seg, keep):
    """out[i] = seg[i] where keep[labels[i]] (or labels[i] == 0), else 0.  keep: n + 1 booleans, keep[0] ignored."""
    import torch
    labels = check_volume(labels, torch.int32, "component_filter")
    seg = check_volume(seg, torch.uint8, "component_filter")
    if seg.shape != labels.shape:
        raise ValueError("component_filter: seg and labels differ in shape")
    keep = np.ascontiguousarray(np.asarray(keep, dtype=bool).astype(np.uint8))
    out = torch.empty_like(seg)
    stream = torch.cuda.current_stream(seg.device).cuda_stream
    _lib.check(_lib.load().mi355_component_filter(labels.data_ptr(), seg.data_ptr(), seg.numel(), keep.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  len(keep) - 1, out.data_ptr(), stream), "mi355_component_filter")
    return out


PAIR_TABLE_MAX = 1 << 20     # MI355_PAIR_TABLE_MAX
_LOOKUP_TABLE_OFFSET = 16    # bytes in front of the table's copy in the work buffer of mi355_label_lookup


def pair_counts(a, n_a, b, n_b, names=("the first map", "the second map")):
    """a, b: CUDA int32 label maps of one shape with labels 0..n_a and 0..n_b -> int64 [n_a + 1, n_b + 1], entry [i, j] = the voxels
    with a == i and b == j (row 0 and column 0 = label 0 included; the table sums to the voxel count): ``np.add.at(t, (a, b), 1)``.
    ValueError: a table of more than ``PAIR_TABLE_MAX`` entries.  A label outside its range is refused by the library."""
    import torch
    a = check_volume(a, torch.int32, "pair_counts")
    b = check_volume(b, torch.int32, "pair_counts")
    if a.shape != b.shape:
        raise ValueError("pair_counts: the two label maps differ in shape")
    n_a, n_b = int(n_a), int(n_b)
    if n_a < 0 or n_b < 0:
        raise ValueError(f"pair_counts: {n_a} and {n_b} labels")
    entries = (n_a + 1) * (n_b + 1)
    if entries > PAIR_TABLE_MAX:
        raise ValueError(f"pair_counts: {n_a} components in {names[0]} and {n_b} in {names[1]} make a table of {entries} entries "
                         f"({PAIR_TABLE_MAX} at most)")
    table = torch.empty(entries + 1, dtype=torch.int64, device=a.device)
    out = np.zeros(entries, dtype=np.int64)
    stream = torch.cuda.current_stream(a.device).cuda_stream
    _lib.check(_lib.load().mi355_label_pair_counts(a.data_ptr(), n_a, b.data_ptr(), n_b, a.numel(), table.data_ptr(), table.numel(),
                                                   out.ctypes.data_as(C.POINTER(C.c_int64)), stream), "mi355_label_pair_counts")
    return out.reshape(n_a + 1, n_b + 1)


def lookup(labels, n, table):
    """labels: CUDA int32 label map with labels 0..n; table: n + 1 entries of uint8 or int32 (numpy) -> ``table[labels]`` as a CUDA tensor
    of the table's dtype; ``table[0]`` is honoured.  A label outside 0..n is refused by the library and nothing is written."""
    import torch
    labels = check_volume(labels, torch.int32, "lookup")
    table = np.ascontiguousarray(table)
    n = int(n)
    if table.dtype not in (np.uint8, np.int32) or table.shape != (n + 1,):
        raise ValueError(f"lookup: a uint8 or int32 table of n + 1 = {n + 1} entries expected, got {table.dtype} {table.shape}")
    if n > MAX_COMPONENTS:
        raise ValueError(f"lookup: {n} components, {MAX_COMPONENTS} at most")
    wide = table.dtype == np.int32
    out = torch.empty(labels.shape, dtype=torch.int32 if wide else torch.uint8, device=labels.device)
    work = torch.empty(_LOOKUP_TABLE_OFFSET + table.nbytes, dtype=torch.uint8, device=labels.device)
    stream = torch.cuda.current_stream(labels.device).cuda_stream
    lib = _lib.load()
    if wide:
        _lib.check(lib.mi355_label_lookup_i32(labels.data_ptr(), labels.numel(), n, table.ctypes.data_as(_lib.c_int32_p), work.data_ptr(), work.numel(),
                                              out.data_ptr(), stream), "mi355_label_lookup_i32")
    else:
        _lib.check(lib.mi355_label_lookup(labels.data_ptr(), labels.numel(), n, table.ctypes.data_as(C.POINTER(C.c_uint8)), work.data_ptr(), work.numel(),
                                          out.data_ptr(), stream), "mi355_label_lookup")
    return out


def _indicator(seg, values):
    """uint8 map that is 1 where seg takes one of `values` (the remap kernel with a 0/1 table)."""
    import torch
    table = np.zeros(256, dtype=np.uint8)
    table[list(values)] = 1
    out = torch.empty_like(seg)
    stream = torch.cuda.current_stream(seg.device).cuda_stream
    _lib.check(_lib.load().mi355_label_remap(seg.data_ptr(), out.data_ptr(), seg.numel(), table.ctypes.data_as(C.POINTER(C.c_uint8)), stream),
               "mi355_label_remap")
    return out


# ---- step3_multiplicity.py:41-374 on the integer tables ---------------------------------------------------------------
def _centroid(row):
    n = int(row[COUNT])
    return [float(np.float64(int(row[SUM0 + k])) / n) for k in range(3)]  # np.mean of integer coordinates: exact sum, one division


def _distance(c1, c2):
    return np.sqrt((c1['x'] - c2['x'])**2 + (c1['y'] - c2['y'])**2 + (c1['z'] - c2['z'])**2)  # :174-178, :286-290


def _relationship(distance_mm):  # :197-204
    if distance_mm < SATELLITE_DISTANCE_MM:
        return 'Satellite/adjacent'
    if distance_mm < SEPARATE_DISTANCE_MM:
        return 'Regional spread'
    return 'Distant/separate'


def _component_analysis(stats, voxel_dims):  # detect_connected_components, :41-152
    if len(stats) == 0:
        return {'num_components': 0, 'components': [], 'is_single_lesion': True, 'description': 'No tumor detected'}
    components = []
    for comp_id, row in enumerate(stats, 1):
        volume_cm3 = row[COUNT] * np.prod(voxel_dims) / 1000
        c = _centroid(row)
        centroid = {'x': c[0], 'y': c[1], 'z': c[2]}
        centroid_mm = {k: centroid[k] * voxel_dims[i] for i, k in enumerate('xyz')}
        bbox = {}
        for i, k in enumerate('xyz'):
            bbox[f'{k}_min'] = int(row[MIN0 + i])
            bbox[f'{k}_max'] = int(row[MAX0 + i])
        max_diameter_mm = max((bbox[f'{k}_max'] - bbox[f'{k}_min']) * voxel_dims[i] for i, k in enumerate('xyz'))
        composition = {'ncr': int(row[SEG1]), 'ed': int(row[SEG1 + 1]), 'et': int(row[SEG1 + 2])}
        components.append({'id': comp_id, 'voxel_count': int(row[COUNT]), 'volume_cm3': float(volume_cm3), 'centroid_voxel': centroid,
                           'centroid_mm': centroid_mm, 'bounding_box': bbox, 'max_diameter_mm': float(max_diameter_mm),
                           'composition': composition, 'has_enhancement': composition['et'] > 0})
    significant = [c for c in components if c['volume_cm3'] >= MIN_LESION_VOLUME_CM3]
    excluded = len(components) - len(significant)
    significant.sort(key=lambda x: x['volume_cm3'], reverse=True)  # stable: equal volumes keep the order of their ids
    for i, comp in enumerate(significant):
        comp['rank'] = i + 1
        comp['classification'] = 'Primary lesion' if i == 0 else f'Secondary lesion #{i}'
    note = f' ({excluded} sub-threshold fragments excluded, <{MIN_LESION_VOLUME_CM3} cm³)' if excluded else ''
    return {'num_components': len(significant), 'components': significant, 'is_single_lesion': len(significant) == 1,
            'description': f'{len(significant)} lesion(s) detected{note}', 'excluded_fragments': excluded,
            'minimum_volume_threshold_cm3': MIN_LESION_VOLUME_CM3}


def _distance_analysis(components):  # calculate_inter_lesion_distances, :155-194
    if len(components) < 2:
        return {'distances': [], 'min_distance_mm': None, 'max_distance_mm': None, 'mean_distance_mm': None}
    distances = []
    for i in range(len(components)):
        for j in range(i + 1, len(components)):
            dist = _distance(components[i]['centroid_mm'], components[j]['centroid_mm'])
            distances.append({'component_1': components[i]['id'], 'component_2': components[j]['id'], 'distance_mm': float(dist),
                              'relationship': _relationship(dist)})
    values = [d['distance_mm'] for d in distances]
    return {'distances': distances, 'min_distance_mm': float(min(values)), 'max_distance_mm': float(max(values)),
            'mean_distance_mm': float(np.mean(values))}


def _satellite_analysis(components):  # detect_satellite_lesions, :266-311; the no-tumour dict of analyze_multiplicity, :500-505
    if not components:
        return {'satellite_count': 0, 'satellites': [], 'has_satellites': False, 'description': 'No tumor detected'}
    if len(components) < 2:
        return {'satellite_count': 0, 'satellites': [], 'has_satellites': False, 'description': 'Single lesion, no satellites'}
    primary = components[0]['centroid_mm']
    satellites = []
    for comp in components[1:]:
        dist = _distance(primary, comp['centroid_mm'])
        if dist < SATELLITE_DISTANCE_MM:
            satellites.append({'component_id': comp['id'], 'volume_cm3': comp['volume_cm3'], 'distance_from_primary_mm': float(dist),
                               'has_enhancement': comp['has_enhancement']})
    description = (f'{len(satellites)} satellite lesion(s) within {SATELLITE_DISTANCE_MM}mm of primary tumor' if satellites
                   else 'No satellite lesions detected')
    return {'satellite_count': len(satellites), 'satellites': satellites, 'has_satellites': len(satellites) > 0,
            'satellite_threshold_mm': SATELLITE_DISTANCE_MM, 'description': description}


def _enhancing_analysis(stats, voxel_dims):  # analyze_enhancing_components, :207-263
    n = len(stats)
    if n == 0:
        return {'num_enhancing_foci': 0, 'enhancing_components': [], 'pattern': 'Non-enhancing',
                'description': 'No enhancing tumor components detected'}
    foci = []
    for comp_id, row in enumerate(stats, 1):
        volume_cm3 = row[COUNT] * np.prod(voxel_dims) / 1000
        c = _centroid(row)
        foci.append({'id': comp_id, 'volume_cm3': float(volume_cm3),
                     'centroid_mm': {k: float(np.float64(c[i]) * voxel_dims[i]) for i, k in enumerate('xyz')}})
    foci.sort(key=lambda x: x['volume_cm3'], reverse=True)
    pattern = 'Single enhancing focus' if n == 1 else ('Few enhancing foci' if n <= 3 else 'Multiple/scattered enhancing foci')
    return {'num_enhancing_foci': n, 'enhancing_components': foci, 'pattern': pattern,
            'total_enhancing_volume_cm3': float(sum(c['volume_cm3'] for c in foci)),
            'description': f'{n} separate enhancing focus/foci detected'}


def _distribution_pattern(comp, dist, sat, enh):  # classify_distribution_pattern, :314-374, without its prose fields
    n = comp['num_components']
    if n == 0:
        return {'pattern': 'No tumor', 'classification': 'No lesion detected'}
    if n == 1:
        pattern, classification = 'Solitary', 'Single contiguous lesion'
    elif sat['has_satellites']:
        pattern, classification = 'Primary with satellites', 'Main lesion with satellite nodules'
    elif n <= 3:
        if dist['max_distance_mm'] and dist['max_distance_mm'] < SEPARATE_DISTANCE_MM:
            pattern, classification = 'Regional multifocal', 'Few lesions in regional distribution'
        else:
            pattern, classification = 'Distant multifocal', 'Separate lesions in different brain regions'
    else:
        pattern, classification = 'Diffuse/scattered', 'Multiple lesions throughout brain'
    return {'pattern': pattern, 'classification': classification, 'lesion_count': n, 'enhancing_foci_count': enh['num_enhancing_foci']}


def multiplicity_from_stats(tumour_stats, enhancing_stats, voxel_dims):
    """The dicts of step 3 from the two integer tables ([n, 14] each: components of ``seg > 0`` with the seg values counted,
    components of ``seg == 3``; both 26-connected, numbered as scipy numbers them) and the voxel sizes along axis 0, 1, 2
    (called x, y, z as in the reference).  Pure host arithmetic in float64."""
    voxel_dims = [float(v) for v in voxel_dims]
    tumour_stats = np.asarray(tumour_stats, dtype=np.int64).reshape(-1, NCOL)
    enhancing_stats = np.asarray(enhancing_stats, dtype=np.int64).reshape(-1, NCOL)
    comp = _component_analysis(tumour_stats, voxel_dims)
    dist = _distance_analysis(comp['components'])
    sat = _satellite_analysis(comp['components'])
    enh = _enhancing_analysis(enhancing_stats, voxel_dims)
    return {'component_analysis': comp, 'distance_analysis': dist, 'satellite_analysis': sat, 'enhancing_analysis': enh,
            'distribution_pattern': _distribution_pattern(comp, dist, sat, enh)}


def lesion_multiplicity(seg, voxel_dims, ctx=None):
    """seg: CUDA uint8 label map [d0, d1, d2] (1 = ncr, 2 = ed, 3 = et, as step 3 reads them) -> the dict of
    ``multiplicity_from_stats``.  Two labellings and two statistics passes on the device.  ``ctx``: the ``features.CaseContext`` of
    ``seg``, which has the tumour's labelling, or None."""
    import torch
    if ctx is not None:
        seg = ctx.volumes(seg, (), "lesion_multiplicity")[0]
    seg = check_volume(seg, torch.uint8, "lesion_multiplicity")
    labels, n = label_components(seg, 3) if ctx is None else ctx.tumour_components  # tumour = seg > 0
    tumour = component_stats(labels, n, seg)
    labels, n = label_components(_indicator(seg, (3,)), 3)    # enhancing = seg == 3
    enhancing = component_stats(labels, n)
    return multiplicity_from_stats(tumour, enhancing, voxel_dims)


def remove_all_but_the_largest_connected_component(seg, for_which_classes, volume_per_voxel, minimum_valid_object_size=None):
    """nnU-Net v1's post-processing step on the device.  seg: CUDA uint8 label map; for_which_classes: labels, or tuples of
    labels that form one region; every object of a class (6-connectivity) that is not of the maximum size is set to 0, unless
    minimum_valid_object_size ({class: size} or one number, in the unit of volume_per_voxel) is given and the object reaches
    it.  Returns (new seg, largest_removed {class: size or None}, kept_size {class: size or None})."""
    import torch
    seg = check_volume(seg, torch.uint8, "remove_all_but_the_largest_connected_component").clone()
    largest_removed, kept_size = {}, {}
    for c in for_which_classes:
        members = tuple(c) if isinstance(c, (list, tuple)) else (c,)
        c = tuple(c) if isinstance(c, (list, tuple)) else c
        if 0 in members:
            raise ValueError("remove_all_but_the_largest_connected_component: class 0 is the background")
        labels, n = label_components(_indicator(seg, members), 1)
        largest_removed[c], kept_size[c] = None, None
        if n == 0:
            continue
        sizes = component_stats(labels, n)[:, COUNT] * volume_per_voxel
        maximum = sizes.max()
        kept_size[c] = float(maximum)
        remove = sizes != maximum
        if minimum_valid_object_size is not None:
            least = minimum_valid_object_size[c] if isinstance(minimum_valid_object_size, dict) else minimum_valid_object_size
            remove &= sizes < least
        if remove.any():
            largest_removed[c] = float(sizes[remove].max())
            seg = component_filter(labels, seg, np.concatenate([[True], ~remove]))
    return seg, largest_removed, kept_size
