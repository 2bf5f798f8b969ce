"""``np.percentile`` of a masked float32 volume without leaving the device.

The reference takes percentiles of ``data[mask]`` in a dozen places (``feature_extraction/utils.py:48-49, :57, :67``,
``step2_mass_effect.py:179``, ``step4_morphology.py:317-320``, ``step5_quality.py:194-212``, ``step6_normal_structures.py``).
numpy partitions a copy of the selected values; here ``csrc/percentile.hip`` radix-selects the two order statistics that
bracket each percentile straight from the volume and its flag byte, and numpy's interpolation between the two is host
arithmetic (``percentile_from_order_stats``: a pure function, testable without a device).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def percentile_from_order_stats(count, q, below, above):
    """numpy's ``method='linear'`` (``np.percentile``'s default) in float64, bit for bit: ``count`` values were selected, ``below``
    and ``above`` are their ascending order statistics of rank ``floor(v)`` and ``min(floor(v) + 1, count - 1)`` for the virtual
    index ``v = (count - 1) * q / 100``.  ``q``, ``below`` and ``above`` broadcast; returns float64 of their shape."""
    q = np.asarray(q, dtype=np.float64)
    below, above = np.asarray(below, dtype=np.float64), np.asarray(above, dtype=np.float64)
    v = (int(count) - 1) * np.true_divide(q, 100)
    g = v - np.floor(v)
    d = above - below
    r = np.asarray(below + d * g)
    hi = np.asarray(above - d * (1 - g))
    return np.where(g >= 0.5, hi, r)


def masked_order_stats(x, qs, flags=None, require=0, forbid=0, lo=-np.inf, hi=np.inf):
    """The entry point as it is: ``(count, nan_count, below, above)`` - the number of selected voxels, the number of NaN among the
    voxels the flags select, and per percentile the two float32 order statistics that bracket it (NaN when nothing is
    selected).  Selection as in ``masked_percentiles``."""
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("masked_percentiles: CUDA float32 tensor expected")
    if flags is not None and (not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or not flags.is_cuda or flags.shape != x.shape):
        raise ValueError("masked_percentiles: CUDA uint8 flags of the shape of the volume expected")
    x = x.contiguous()
    flags = None if flags is None else flags.contiguous()
    q = np.ascontiguousarray(np.atleast_1d(np.asarray(qs, dtype=np.float64)))
    count = (C.c_int64 * 2)()
    below, above = np.full(q.size, np.nan, dtype=np.float32), np.full(q.size, np.nan, dtype=np.float32)
    rc = _lib.load().mi355_masked_percentiles(x.data_ptr(), x.numel(), None if flags is None else flags.data_ptr(), int(require), int(forbid), float(lo),
                                              float(hi), q.ctypes.data_as(C.POINTER(C.c_double)), q.size, count, _lib.fptr(below), _lib.fptr(above),
                                              torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, "mi355_masked_percentiles")
    return int(count[0]), int(count[1]), below, above


def masked_percentiles(x, qs, flags=None, require=0, forbid=0, lo=-np.inf, hi=np.inf):
    """x: CUDA float32 tensor; flags: CUDA uint8 tensor of its shape or None.  A voxel is selected when every bit of ``require``
    is set in its flag byte, no bit of ``forbid`` is, and ``lo < x < hi`` (``x[x > 0]`` is ``lo=0``).  Returns ``(count,
    float64 array)``: the number of selected voxels and ``np.percentile(selected.astype(float64), qs)``, bit for bit; the array
    is all NaN when nothing is selected.  Up to 8 percentiles per call share every pass over the volume.  Raises when a voxel
    the flags select is NaN (numpy would have returned NaN)."""
    count, nans, below, above = masked_order_stats(x, qs, flags, require, forbid, lo, hi)
    if nans:
        raise ValueError(f"masked_percentiles: {nans} of the voxels the flags select are NaN")
    if count == 0:
        return 0, np.full(below.shape, np.nan)
    return count, percentile_from_order_stats(count, np.atleast_1d(np.asarray(qs, dtype=np.float64)), below, above)


def intensity_stats(x, flags, bit):
    """``utils.get_intensity_stats(data, mask)`` (utils.py:27-51) for the region bit ``bit`` of the flag byte: minimum, maximum,
    median and quartiles from one ``masked_percentiles`` call, mean, std and count from ``masked_moments``."""
    from . import morphology
    count, p = masked_percentiles(x, (0, 100, 50, 25, 75), flags, require=1 << bit)
    if count == 0:
        return {'mean': None, 'std': None, 'min': None, 'max': None, 'median': None, 'q25': None, 'q75': None, 'voxel_count': 0}
    row = morphology.masked_moments(x.reshape((1,) + tuple(x.shape)), flags)[bit][0]
    mean, std = morphology._mean_std(row)
    return {'mean': float(mean), 'std': float(std), 'min': float(p[0]), 'max': float(p[1]), 'median': float(p[2]), 'q25': float(p[3]),
            'q75': float(p[4]), 'voxel_count': int(row[0])}
