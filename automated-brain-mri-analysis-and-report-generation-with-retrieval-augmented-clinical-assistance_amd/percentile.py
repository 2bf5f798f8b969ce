"""``np.percentile`` of a masked float32 volume without leaving the device.

The reference takes percentiles of ``data[mask]`` in a dozen places (``feature_extraction/utils.py:48-49, :57, :67``,
``step2_mass_effect.py:179``, ``step4_morphology.py:317-320``, ``step5_quality.py:194-212``, ``step6_normal_structures.py``).
numpy partitions a copy of the selected values; here ``csrc/percentile.hip`` radix-selects the two order statistics that
bracket each percentile straight from the volume and its flag byte, and numpy's interpolation between the two is host
arithmetic (``percentile_from_order_stats``: a pure function, testable without a device).

The six steps of one case ask for the same percentiles again and again; ``masked_percentiles_multi`` selects in up to four volumes
that share the flag byte in the four passes one volume takes, and ``plan_percentile_batches`` (pure) merges any list of requests
into such batches.
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


#: volumes per batched call and percentiles per volume (PCT_MAX_VOLUMES, PCT_MAX_Q of csrc/radix_select.h)
MAX_VOLUMES, MAX_Q = 4, 8


def masked_order_stats_multi(requests, flags=None, info=None):
    """``masked_order_stats`` for up to 4 volumes of one shape that share ``flags``, in four passes over the voxels for all of them
    (``mi355_masked_percentiles_multi``).  ``requests``: tuples ``(x, qs, require, forbid, lo, hi)``, the last four optional with the
    defaults of ``masked_order_stats``.  Returns one ``(count, nan_count, below, above)`` per request, bit-equal to the single
    call's.  ``info``: a dict that receives ``launches``, the kernel launches of the call (4 unless a pass was split by volume or
    nothing is selected at all)."""
    import torch
    lib = _lib.load()
    reqs = [tuple(r) + (0, 0, -np.inf, np.inf)[len(r) - 2:] for r in requests]
    nvol = len(reqs)
    for x, _, _, _, _, _ in reqs:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError("masked_percentiles_multi: CUDA float32 tensors expected")
    if nvol and any(r[0].numel() != reqs[0][0].numel() for r in reqs):
        raise _lib.Mi355Error(f"masked_percentiles_multi: the volumes differ in length ({', '.join(str(r[0].numel()) for r in reqs)} voxels)")
    if flags is not None and (not isinstance(flags, torch.Tensor) or flags.dtype != torch.uint8 or not flags.is_cuda or
                              (nvol and flags.shape != reqs[0][0].shape)):
        raise ValueError("masked_percentiles_multi: CUDA uint8 flags of the shape of the volumes expected")
    xs = [r[0].contiguous() for r in reqs]
    flags = None if flags is None else flags.contiguous()
    qs = [np.ascontiguousarray(np.atleast_1d(np.asarray(r[1], dtype=np.float64)).reshape(-1)) for r in reqs]
    x_ptrs = (C.c_void_p * max(nvol, 1))(*[x.data_ptr() for x in xs])
    q_ptrs = (C.POINTER(C.c_double) * max(nvol, 1))(*[q.ctypes.data_as(C.POINTER(C.c_double)) for q in qs])
    ints = lambda k: (C.c_int32 * max(nvol, 1))(*[int(r[k]) for r in reqs])
    doubles = lambda k: (C.c_double * max(nvol, 1))(*[float(r[k]) for r in reqs])
    nq = (C.c_int32 * max(nvol, 1))(*[q.size for q in qs])
    count = (C.c_int64 * (2 * max(nvol, 1)))()
    below = np.full((max(nvol, 1), MAX_Q), np.nan, dtype=np.float32)
    above = np.full((max(nvol, 1), MAX_Q), np.nan, dtype=np.float32)
    launches = C.c_int32(0)
    stream = torch.cuda.current_stream(xs[0].device).cuda_stream if nvol else None
    rc = lib.mi355_masked_percentiles_multi(x_ptrs, nvol, xs[0].numel() if nvol else 0, None if flags is None else flags.data_ptr(), ints(2), ints(3),
                                            doubles(4), doubles(5), q_ptrs, nq, count, _lib.fptr(below), _lib.fptr(above), C.byref(launches), stream)
    _lib.check(rc, "mi355_masked_percentiles_multi")
    if info is not None:
        info['launches'] = int(launches.value)
    return [(int(count[2 * v]), int(count[2 * v + 1]), below[v, :qs[v].size].copy(), above[v, :qs[v].size].copy()) for v in range(nvol)]


def percentiles_from_order_stats(stats, qs):
    """What ``masked_percentiles`` makes of one ``(count, nan_count, below, above)``: its NaN refusal, NaN values for an empty
    selection, numpy's interpolation otherwise."""
    count, nans, below, above = stats
    if nans:
        raise ValueError(f"masked_percentiles: {nans} of the voxels the flags select are NaN")
    if count == 0:
        return 0, np.full(below.shape, np.nan)
    return count, percentile_from_order_stats(count, np.atleast_1d(np.asarray(qs, dtype=np.float64)), below, above)


def masked_percentiles_multi(requests, flags=None):
    """``masked_percentiles`` for up to 4 requests ``(x, qs, require, forbid, lo, hi)`` (the last four optional) on volumes of one
    shape that share ``flags``: a list of ``(count, float64 array)``, each what ``masked_percentiles(x, qs, flags, require, forbid,
    lo, hi)`` returns, bit for bit, from four passes over the voxels for all of them.  Raises, as the single call, when a voxel the
    flags select for one of the requests is NaN."""
    requests = [tuple(r) for r in requests]
    return [percentiles_from_order_stats(st, r[1]) for st, r in zip(masked_order_stats_multi(requests, flags), requests)]


def plan_percentile_batches(requests):
    """Any number of requests ``(x, qs, require, forbid, lo, hi)`` (the last four optional) -> ``(batches, back)``.  Pure: nothing
    is launched and ``x`` is only compared by identity.

    ``batches``: lists of at most 4 merged requests ``(x, qs, require, forbid, lo, hi)`` with at most 8 distinct percentiles each,
    each list one ``masked_percentiles_multi`` call.  Requests for the same volume and predicate share one entry and a
    percentile asked twice is selected once; a ninth distinct percentile for one volume and predicate opens an entry in a later
    batch.  ``back[i]``: one ``(batch, entry, place)`` per percentile of request i, in its own order, so that
    ``results[batch][entry][1][place]`` is its value (``gather_planned``)."""
    reqs = [tuple(r) + (0, 0, -np.inf, np.inf)[len(r) - 2:] for r in requests]
    batches = []      # batch -> entries [x, [q...], require, forbid, lo, hi]
    entries = {}      # (volume, predicate) -> [(batch, entry)] in batch order
    back = []
    for x, qs, require, forbid, lo, hi in reqs:
        key = (id(x), int(require), int(forbid), float(lo), float(hi))
        places = []
        for q in np.atleast_1d(np.asarray(qs, dtype=np.float64)).reshape(-1):
            q = float(q)
            mine = entries.setdefault(key, [])
            hit = next(((b, e) for b, e in mine if q in batches[b][e][1]), None) or next(((b, e) for b, e in mine if len(batches[b][e][1]) < MAX_Q), None)
            if hit is None:
                first = mine[-1][0] + 1 if mine else 0
                b = next((k for k in range(first, len(batches)) if len(batches[k]) < MAX_VOLUMES), None)
                if b is None:
                    batches.append([])
                    b = len(batches) - 1
                batches[b].append([x, [], int(require), int(forbid), float(lo), float(hi)])
                hit = (b, len(batches[b]) - 1)
                mine.append(hit)
            chosen = batches[hit[0]][hit[1]][1]
            if q not in chosen:
                chosen.append(q)
            places.append((hit[0], hit[1], chosen.index(q)))
        back.append(places)
    return [[(e[0], tuple(e[1]), e[2], e[3], e[4], e[5]) for e in batch] for batch in batches], back


def gather_planned(results, back):
    """``results[batch][entry] = (count, values)`` of the batches of ``plan_percentile_batches`` -> one ``(count, float64 array)`` per
    original request, its values in its own order."""
    out = []
    for places in back:
        out.append((results[places[0][0]][places[0][1]][0], np.array([results[b][e][1][k] for b, e, k in places], dtype=np.float64)))
    return out


def intensity_stats(x, flags, bit):
    """``utils.get_intensity_stats(data, mask)`` (utils.py:27-51) for the region bit ``bit`` of the flag byte: minimum, maximum,
    median and quartiles from one ``masked_percentiles`` call, mean, std and count from ``masked_moments``."""
    from .volume_ops import masked_moments, mean_std
    count, p = masked_percentiles(x, (0, 100, 50, 25, 75), flags, require=1 << bit)
    if count == 0:
        return {'mean': None, 'std': None, 'min': None, 'max': None, 'median': None, 'q25': None, 'q75': None, 'voxel_count': 0}
    row = masked_moments(x.reshape((1,) + tuple(x.shape)), flags)[bit][0]
    mean, std = mean_std(row)
    return {'mean': float(mean), 'std': float(std), 'min': float(p[0]), 'max': float(p[1]), 'median': float(p[2]), 'q25': float(p[3]),
            'q75': float(p[4]), 'voxel_count': int(row[0])}
