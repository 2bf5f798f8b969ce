"""The volume primitives that belong to no single feature-extraction step: thin ctypes wrappers over the entry points of
csrc/morphology.hip, csrc/quality.hip, csrc/mass_effect.hip and csrc/normal_structures.hip (and the morphology of
csrc/lesionwise.hip and the axis reversal of csrc/resident_case.hip), and the tensor checks they share.

A step module (``sequence_findings``, ``mass_effect``, ``morphology``, ``quality``, ``normal_structures``) and ``features`` import
what they need from here; the primitives with one subject of their own stay in ``percentile``, ``components`` and ``evaluate``.
``torch`` is imported inside the functions: the host arithmetic of the steps is tested on machines without a device.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np

from . import _lib

NBITS = 8
#: longest axis-1 / axis-2 line of ``distance_transform_edt_sq`` (one line per 64 KiB LDS tile)
EDT_MAX_LINE = 1024
CITYBLOCK_FAR = 1 << 30                        # MI355_CITYBLOCK_FAR
_I32_MAX = 2 ** 31 - 1
_I64P = C.POINTER(C.c_int64)


# ---- the shared checks ------------------------------------------------------------------------------------------------
def check_volume(t, dtype, what):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or t.dim() != 3:
        raise ValueError(f"{what}: CUDA {dtype} [d0, d1, d2] tensor expected")
    return t.contiguous()


def stream_of(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def mean_std(row):
    """(mean, population std) from (n, sum, sum of squares): the difference of the two squares is taken exactly"""
    n = int(row[0])
    s1, s2 = Fraction(float(row[1])), Fraction(float(row[2]))
    var = s2 / n - (s1 / n) ** 2
    return np.float64(float(s1 / n)), np.float64(np.sqrt(float(var)) if var > 0 else 0.0)


def _flags(t, what, dim=None):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or (dim is not None and t.dim() != dim):
        raise ValueError(f"{what}: CUDA uint8 {'[d0, d1, d2] ' if dim == 3 else ''}tensor expected")
    return t.contiguous()


def _check_values(values, flags, what):
    import torch
    if not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or not flags.is_cuda:
        raise ValueError(f"{what}: CUDA uint8 flags expected")
    if not isinstance(values, torch.Tensor) or values.dtype != torch.int32 or not values.is_cuda or values.shape != flags.shape:
        raise ValueError(f"{what}: CUDA int32 values of the shape of the flags expected")
    if not values.is_contiguous() or not flags.is_contiguous():
        raise ValueError(f"{what}: contiguous tensors expected")


# ---- csrc/resident_case.hip -------------------------------------------------------------------------------------------
def reverse_axes(t):
    """t: contiguous CUDA uint8 or float32 tensor [d0, d1, d2] or [C, d0, d1, d2] -> a new tensor [d2, d1, d0] or [C, d2, d1, d0],
    ``out[c, k, j, i] = t[c, i, j, k]`` bit for bit, in one launch on the current stream: a volume in file order ([Z, Y, X], what
    the inference driver holds) becomes the (x, y, z) volume the evaluator and the feature steps take, and back."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.uint8, torch.float32) or t.dim() not in (3, 4):
        raise ValueError("reverse_axes: CUDA uint8 or float32 tensor [d0, d1, d2] or [C, d0, d1, d2] expected")
    if not t.is_contiguous():
        raise ValueError("reverse_axes: contiguous tensor expected")
    lead = tuple(t.shape[:-3])
    d0, d1, d2 = (int(v) for v in t.shape[-3:])
    out = torch.empty(lead + (d2, d1, d0), dtype=t.dtype, device=t.device)
    _lib.check(_lib.load().mi355_reverse_axes(t.data_ptr(), out.data_ptr(), int(lead[0]) if lead else 1, d0, d1, d2, t.element_size(), stream_of(t)),
               "mi355_reverse_axes")
    return out


# ---- csrc/morphology.hip ----------------------------------------------------------------------------------------------
def _morph(mask, iterations, dilate, what):
    import torch
    mask = check_volume(mask, torch.uint8, what)
    out = torch.empty_like(mask)
    _lib.check(_lib.load().mi355_binary_morphology(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2], int(dilate), int(iterations),
                                                   out.data_ptr(), stream_of(mask)), "mi355_binary_morphology")
    return out


def binary_erosion(mask, iterations=1):
    """mask: CUDA uint8 [d0, d1, d2], foreground = nonzero -> uint8 0 / 1 map, bit-equal to
    ``scipy.ndimage.binary_erosion(mask, iterations=iterations)`` (6-neighbour cross, border_value 0); iterations >= 1."""
    return _morph(mask, iterations, 0, "binary_erosion")


def binary_dilation(mask, iterations=1):
    """As ``binary_erosion`` for ``scipy.ndimage.binary_dilation``."""
    return _morph(mask, iterations, 1, "binary_dilation")


# ---- csrc/lesionwise.hip: the same two with the 6-, 18- or 26-neighbourhood -------------------------------------------------
MORPH_NB_LDS_STEPS = 4                         # MI355_MORPH_NB_LDS_STEPS


def _morph_nb(mask, neighbours, iterations, dilate, what):
    import torch
    mask = check_volume(mask, torch.uint8, what)
    out = torch.empty_like(mask)
    tmp = torch.empty_like(mask) if int(iterations) > MORPH_NB_LDS_STEPS else None   # the second buffer of a run of several launches
    _lib.check(_lib.load().mi355_binary_morphology_nb(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2], int(dilate), int(neighbours),
                                                      int(iterations), out.data_ptr(), None if tmp is None else tmp.data_ptr(),
                                                      0 if tmp is None else tmp.numel(), stream_of(mask)), "mi355_binary_morphology_nb")
    return out


def binary_erosion_nb(mask, neighbours, iterations=1):
    """mask: CUDA uint8 [d0, d1, d2], foreground = nonzero -> uint8 0 / 1 map, bit-equal to ``scipy.ndimage.binary_erosion(mask,
    generate_binary_structure(3, c), iterations)`` with c = 1, 2, 3 for ``neighbours`` = 6, 18, 26 (border_value 0); iterations >= 1."""
    return _morph_nb(mask, neighbours, iterations, 0, "binary_erosion_nb")


def binary_dilation_nb(mask, neighbours, iterations=1):
    """As ``binary_erosion_nb`` for ``scipy.ndimage.binary_dilation``."""
    return _morph_nb(mask, neighbours, iterations, 1, "binary_dilation_nb")


def distance_transform_edt_sq(mask):
    """mask: CUDA uint8 [d0, d1, d2] -> int32 map of the squared distance, in voxels, to the nearest background voxel
    (0 on the background): ``rint(scipy.ndimage.distance_transform_edt(mask) ** 2)`` bit for bit.  Refused: a mask without
    background, a squared diagonal beyond int32, more than 1024 entries along axis 1 or 2."""
    import torch
    mask = check_volume(mask, torch.uint8, "distance_transform_edt_sq")
    out = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().mi355_edt_squared(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2], out.data_ptr(), stream_of(mask)),
               "mi355_edt_squared")
    return out


def surface_gradient_stats(d2_in, d2_out, surface, select=255):
    """d2_in, d2_out: the int32 maps of ``distance_transform_edt_sq`` of a mask and of its complement; surface: CUDA uint8 map,
    a voxel counts where ``surface & select`` is nonzero.  Returns (n, mean, std) of ``|grad(sqrt(d2_in) - sqrt(d2_out))|``
    over those voxels, the gradient being ``np.gradient``'s, the std the population one; fp64."""
    import torch
    d2_in = check_volume(d2_in, torch.int32, "surface_gradient_stats")
    d2_out = check_volume(d2_out, torch.int32, "surface_gradient_stats")
    surface = check_volume(surface, torch.uint8, "surface_gradient_stats")
    if not (d2_in.shape == d2_out.shape == surface.shape):
        raise ValueError("surface_gradient_stats: the three maps differ in shape")
    out = (C.c_double * 3)()
    _lib.check(_lib.load().mi355_surface_gradient_stats(d2_in.data_ptr(), d2_out.data_ptr(), surface.data_ptr(), int(select), surface.shape[0],
                                                        surface.shape[1], surface.shape[2], out, stream_of(surface)), "mi355_surface_gradient_stats")
    return int(out[0]), float(out[1]), float(out[2])


def second_moments(mask):
    """mask: CUDA uint8 [d0, d1, d2] -> int64 [10]: n, the sums of the coordinates c0 c1 c2, of their squares, and of c0 c1,
    c0 c2, c1 c2 over the foreground.  Exact."""
    import torch
    mask = check_volume(mask, torch.uint8, "second_moments")
    out = np.zeros(10, dtype=np.int64)
    _lib.check(_lib.load().mi355_mask_second_moments(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2],
                                                     out.ctypes.data_as(C.POINTER(C.c_int64)), stream_of(mask)), "mi355_mask_second_moments")
    return out


def masked_moments(vols, flags):
    """vols: CUDA float32 [C, ...], flags: CUDA uint8 of the shape of one channel, bit b = region b.  Returns float64
    [8, C, 3]: per (bit, channel) the number of voxels with the bit, the sum and the sum of squares of the channel over them,
    accumulated in fp64 in a fixed order."""
    import torch
    if not isinstance(vols, torch.Tensor) or vols.dtype != torch.float32 or not vols.is_cuda or vols.dim() < 2:
        raise ValueError("masked_moments: CUDA float32 [C, ...] tensor expected")
    if not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or not flags.is_cuda or flags.shape != vols.shape[1:]:
        raise ValueError("masked_moments: CUDA uint8 flags of the shape of one channel expected")
    vols, flags = vols.contiguous(), flags.contiguous()
    out = np.zeros((NBITS, vols.shape[0], 3), dtype=np.float64)
    _lib.check(_lib.load().mi355_masked_moments(vols.data_ptr(), vols.shape[0], flags.data_ptr(), flags.numel(),
                                                out.ctypes.data_as(C.POINTER(C.c_double)), stream_of(flags)), "mi355_masked_moments")
    return out


def flag_from_labels(labels, values, bit, flags):
    """Bit ``bit`` of ``flags`` (in place) = ``labels`` takes one of ``values``; with a 0 / 1 mask and ``(1,)`` a mask becomes a bit."""
    table = np.zeros(256, dtype=np.uint8)
    table[list(values)] = 1
    _lib.check(_lib.load().mi355_flag_from_labels(labels.data_ptr(), table.ctypes.data_as(C.POINTER(C.c_uint8)), int(bit), flags.data_ptr(),
                                                  flags.numel(), stream_of(flags)), "mi355_flag_from_labels")
    return flags


def flag_from_flags(flags, bit, require=0, forbid=0, x=None, lo=-np.inf, hi=np.inf):
    """Bit ``bit`` of ``flags`` (in place) = all bits of the mask ``require`` set, none of ``forbid``, and ``lo < x < hi`` (fp64
    comparison of the float32 volume ``x``, when given)."""
    _lib.check(_lib.load().mi355_flag_from_flags(flags.data_ptr(), int(bit), int(require), int(forbid), None if x is None else x.data_ptr(),
                                                 float(lo), float(hi), flags.numel(), stream_of(flags)), "mi355_flag_from_flags")
    return flags


# ---- csrc/quality.hip -------------------------------------------------------------------------------------------------
def binary_fill_holes(mask):
    """mask: CUDA uint8 [d0, d1, d2], foreground = nonzero -> (uint8 0 / 1 map bit-equal to
    ``scipy.ndimage.binary_fill_holes(mask)``, number of voxels added)."""
    import torch
    mask = check_volume(mask, torch.uint8, "binary_fill_holes")
    out = torch.empty_like(mask)
    filled = C.c_int64(0)
    _lib.check(_lib.load().mi355_binary_fill_holes(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2], out.data_ptr(), C.byref(filled),
                                                   stream_of(mask)), "mi355_binary_fill_holes")
    return out, int(filled.value)


def sobel_magnitude_stats(x, flags, select=255):
    """x: CUDA float32 [d0, d1, d2]; flags: CUDA uint8 map of that shape, a voxel counts where ``flags & select`` is nonzero.
    Returns (n, mean, std) of ``sqrt(sobel(x, 0)**2 + sobel(x, 1)**2 + sobel(x, 2)**2)`` over those voxels (scipy's defaults,
    float64, population std)."""
    import torch
    x = check_volume(x, torch.float32, "sobel_magnitude_stats")
    flags = check_volume(flags, torch.uint8, "sobel_magnitude_stats")
    if flags.shape != x.shape:
        raise ValueError("sobel_magnitude_stats: the volume and the flags differ in shape")
    out = (C.c_double * 3)()
    _lib.check(_lib.load().mi355_sobel_magnitude_stats(x.data_ptr(), flags.data_ptr(), int(select), x.shape[0], x.shape[1], x.shape[2], out, stream_of(x)),
               "mi355_sobel_magnitude_stats")
    return int(out[0]), float(out[1]), float(out[2])


def radial_shell_moments(x, flags, require, centre, inner_frac=0.3, outer_frac=0.7):
    """Over the voxels whose flag byte has every bit of ``require``: (max_dist, n_inner, sum_inner, n_outer, sum_outer) - the
    largest distance from ``centre`` (voxel units, numpy's float64 arithmetic bit for bit), and count and sum of ``x`` over the
    voxels nearer than ``max_dist * inner_frac`` and over those farther than ``max_dist * outer_frac``."""
    import torch
    x = check_volume(x, torch.float32, "radial_shell_moments")
    flags = check_volume(flags, torch.uint8, "radial_shell_moments")
    if flags.shape != x.shape:
        raise ValueError("radial_shell_moments: the volume and the flags differ in shape")
    c = (C.c_double * 3)(*[float(v) for v in centre])
    out = (C.c_double * 5)()
    _lib.check(_lib.load().mi355_radial_shell_moments(x.data_ptr(), flags.data_ptr(), int(require), x.shape[0], x.shape[1], x.shape[2], c, float(inner_frac),
                                                      float(outer_frac), out, stream_of(x)), "mi355_radial_shell_moments")
    return float(out[0]), int(out[1]), float(out[2]), int(out[3]), float(out[4])


def face_slab_counts(x, margin):
    """x: CUDA float32 [d0, d1, d2] -> int64 [6]: the voxels with ``x > 0`` in the first and in the last ``margin`` indices of
    axis 0, 1, 2 (``x[:margin]``, ``x[-margin:]``, ``x[:, :margin]``, ...)."""
    import torch
    x = check_volume(x, torch.float32, "face_slab_counts")
    out = np.zeros(6, dtype=np.int64)
    _lib.check(_lib.load().mi355_face_slab_counts(x.data_ptr(), x.shape[0], x.shape[1], x.shape[2], int(margin), out.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  stream_of(x)), "mi355_face_slab_counts")
    return out


# ---- csrc/mass_effect.hip ---------------------------------------------------------------------------------------------
def axis_counts(flags, require=0, forbid=0):
    """flags: CUDA uint8 [d0, d1, d2]; a voxel is selected when its byte has every bit of ``require`` and no bit of ``forbid``.
    Returns three int64 arrays: the selected voxels at each index of axis 0, 1, 2 (``sel.sum(axis=(1, 2))``, ...).  No axis may
    be longer than 4096."""
    flags = _flags(flags, "axis_counts", 3)
    d0, d1, d2 = flags.shape
    out = np.zeros(d0 + d1 + d2, dtype=np.int64)
    _lib.check(_lib.load().mi355_axis_counts(flags.data_ptr(), int(require), int(forbid), d0, d1, d2, out.ctypes.data_as(_I64P), stream_of(flags)),
               "mi355_axis_counts")
    return out[:d0], out[d0:d0 + d1], out[d0 + d1:]


def box_counts(flags, boxes, require=0, forbid=0):
    """The selected voxels inside each of 1..16 boxes ``(lo0, hi0, lo1, hi1, lo2, hi2)``, half-open, inside the volume; boxes may
    overlap, an empty one counts 0.  int64 [len(boxes)]."""
    flags = _flags(flags, "box_counts", 3)
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 6))
    out = np.zeros(len(b), dtype=np.int64)
    _lib.check(_lib.load().mi355_box_counts(flags.data_ptr(), int(require), int(forbid), flags.shape[0], flags.shape[1], flags.shape[2],
                                            b.ctypes.data_as(_lib.c_int32_p), len(b), out.ctypes.data_as(_I64P), stream_of(flags)), "mi355_box_counts")
    return out


def select_ranked(flags, ranks, require=0, forbid=0):
    """``np.flatnonzero(selected)[ranks]`` as a CUDA int64 tensor, and the number of selected voxels: the linear C-order indices
    of the selected voxels of the given 0-based ranks (1..65 536 of them, any order, repeats allowed).  A rank outside the
    selection raises and writes nothing."""
    import torch
    flags = _flags(flags, "select_ranked")
    r = np.ascontiguousarray(np.asarray(ranks, dtype=np.int64).reshape(-1))
    index = torch.empty(max(len(r), 1), dtype=torch.int64, device=flags.device)
    count = C.c_int64(0)
    _lib.check(_lib.load().mi355_select_ranked(flags.data_ptr(), int(require), int(forbid), flags.numel(), r.ctypes.data_as(_I64P), len(r), index.data_ptr(),
                                               C.byref(count), stream_of(flags)), "mi355_select_ranked")
    return index[:len(r)], int(count.value)


def min_pair_dist2(a, b, shape):
    """a, b: CUDA int64 lists (1..65 536 entries each) of linear C-order indices into a volume of ``shape`` -> the smallest
    squared distance, in voxel units, between a voxel of a and a voxel of b (an int)."""
    import torch
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_cuda or t.dim() != 1:
            raise ValueError("min_pair_dist2: CUDA int64 [k] tensors expected")
    a, b = a.contiguous(), b.contiguous()
    out = C.c_int64(0)
    _lib.check(_lib.load().mi355_min_pair_dist2(a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), int(shape[0]), int(shape[1]), int(shape[2]), C.byref(out),
                                                stream_of(a)), "mi355_min_pair_dist2")
    return int(out.value)


def masked_min(values, flags, require=0, forbid=0):
    """values: CUDA int32 tensor, flags: CUDA uint8 tensor of its shape -> (the minimum over the selected voxels or None, their
    number)."""
    import torch
    flags = _flags(flags, "masked_min")
    if not isinstance(values, torch.Tensor) or values.dtype != torch.int32 or not values.is_cuda or values.shape != flags.shape:
        raise ValueError("masked_min: CUDA int32 values of the shape of the flags expected")
    values = values.contiguous()
    lowest, count = C.c_int32(0), C.c_int64(0)
    _lib.check(_lib.load().mi355_masked_min_i32(values.data_ptr(), flags.data_ptr(), int(require), int(forbid), flags.numel(), C.byref(lowest), C.byref(count),
                                                stream_of(flags)), "mi355_masked_min_i32")
    return (int(lowest.value) if count.value else None), int(count.value)


# ---- csrc/normal_structures.hip ---------------------------------------------------------------------------------------
def cityblock_distance(mask, to_foreground=True):
    """mask: CUDA uint8 [d0, d1, d2], foreground = nonzero -> int32 map of the exact city-block (taxicab) distance.
    ``to_foreground``: to the nearest foreground voxel (0 on the mask, ``CITYBLOCK_FAR`` = 2^30 everywhere when the mask is empty);
    ``dist <= n`` is ``scipy.ndimage.binary_dilation(mask, iterations=n)``.  Otherwise: to the nearest background voxel, every
    position outside the volume being background; ``dist > n`` is ``scipy.ndimage.binary_erosion(mask, iterations=n)``."""
    import torch
    mask = check_volume(mask, torch.uint8, "cityblock_distance")
    out = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().mi355_cityblock_distance(mask.data_ptr(), mask.shape[0], mask.shape[1], mask.shape[2], int(bool(to_foreground)), out.data_ptr(),
                                                    stream_of(mask)), "mi355_cityblock_distance")
    return out


def flag_from_i32(flags, bit, values, lo=0, hi=_I32_MAX, require=0, forbid=0):
    """Bit ``bit`` of ``flags`` (in place) = all bits of the mask ``require`` set, none of ``forbid``, and ``lo <= values <= hi``
    (int32 map of the shape of the flags; bounds beyond int32 are clamped, an empty range clears the bit)."""
    _check_values(values, flags, "flag_from_i32")
    lo, hi = max(int(lo), -_I32_MAX - 1), min(int(hi), _I32_MAX)
    if lo > hi:
        lo, hi = 1, 0
    _lib.check(_lib.load().mi355_flag_from_i32(flags.data_ptr(), int(bit), int(require), int(forbid), values.data_ptr(), lo, hi, flags.numel(), stream_of(flags)),
               "mi355_flag_from_i32")
    return flags


def flag_from_box(flags, bit, box, require=0, forbid=0):
    """Bit ``bit`` of ``flags`` [d0, d1, d2] (in place) = all bits of ``require`` set, none of ``forbid``, and the voxel inside the
    half-open index box ``(lo0, hi0, lo1, hi1, lo2, hi2)``, clipped to the volume."""
    import torch
    if not flags.is_contiguous():
        raise ValueError("flag_from_box: contiguous flags expected")
    check_volume(flags, torch.uint8, "flag_from_box")
    b = np.ascontiguousarray(np.clip(np.asarray(box, dtype=np.int64).reshape(6), -_I32_MAX, _I32_MAX).astype(np.int32))
    _lib.check(_lib.load().mi355_flag_from_box(flags.data_ptr(), int(bit), int(require), int(forbid), flags.shape[0], flags.shape[1], flags.shape[2],
                                               b.ctypes.data_as(_lib.c_int32_p), stream_of(flags)), "mi355_flag_from_box")
    return flags


def masked_order_stats_i32(values, qs, flags=None, require=0, forbid=0):
    """values: CUDA int32 tensor with nothing below 0; flags: CUDA uint8 tensor of its shape or None.  Returns ``(count, below,
    above)``: the number of selected voxels and per percentile the two int32 order statistics that bracket it (ranks ``floor(v)``
    and ``min(floor(v) + 1, count - 1)``, ``v = (count - 1) * q / 100``); zeros when nothing is selected."""
    import torch
    if not isinstance(values, torch.Tensor) or values.dtype != torch.int32 or not values.is_cuda:
        raise ValueError("masked_order_stats_i32: CUDA int32 tensor expected")
    if flags is not None and (not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or not flags.is_cuda or flags.shape != values.shape):
        raise ValueError("masked_order_stats_i32: CUDA uint8 flags of the shape of the values expected")
    values = values.contiguous()
    flags = None if flags is None else flags.contiguous()
    q = np.ascontiguousarray(np.atleast_1d(np.asarray(qs, dtype=np.float64)))
    count = C.c_int64(0)
    below, above = np.zeros(q.size, dtype=np.int32), np.zeros(q.size, dtype=np.int32)
    _lib.check(_lib.load().mi355_masked_order_stats_i32(values.data_ptr(), values.numel(), None if flags is None else flags.data_ptr(), int(require), int(forbid),
                                                        q.ctypes.data_as(C.POINTER(C.c_double)), q.size, C.byref(count), below.ctypes.data_as(_lib.c_int32_p),
                                                        above.ctypes.data_as(_lib.c_int32_p), stream_of(values)), "mi355_masked_order_stats_i32")
    return int(count.value), below, above


def column_count_max(flags, i1_from, require=0, forbid=0):
    """``np.max(np.sum(selected[:, i1_from:, :], axis=0))`` of the voxels of ``flags`` [d0, d1, d2] with every bit of ``require`` and
    no bit of ``forbid``; 0 when that slab selects nothing."""
    import torch
    flags = check_volume(flags, torch.uint8, "column_count_max")
    out = C.c_int64(0)
    _lib.check(_lib.load().mi355_column_count_max(flags.data_ptr(), int(require), int(forbid), flags.shape[0], flags.shape[1], flags.shape[2], int(i1_from),
                                                  C.byref(out), stream_of(flags)), "mi355_column_count_max")
    return int(out.value)
