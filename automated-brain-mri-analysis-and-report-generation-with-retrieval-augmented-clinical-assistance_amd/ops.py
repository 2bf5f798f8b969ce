"""Thin torch-CUDA wrappers over the single-purpose C-ABI entry points.

torch is used for device memory and streams only; every computation happens in the HIP
library.  All functions raise ``Mi355Error`` if the library is missing or no GPU is present.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .volume_ops import stream_of


def _require_cuda(t, dtype, name):
    if not t.is_cuda or t.dtype != dtype:
        raise ValueError(f"{name}: expected a CUDA tensor of dtype {dtype}")
    return t.contiguous()


def regions_to_labels(probs, order=(1, 2, 3), bbox_lo=(0, 0, 0), full_shape=None):
    """seg = 0; seg[probs[i] > 0.5] = order[i] in order; pasted at bbox_lo of a zero uint8 volume of
    full_shape (reference driver :144-156, region_class_order=(1,2,3)).  ``order=None``: seg = argmax over channels
    (the same export for trainers without regions)."""
    import torch
    probs = _require_cuda(probs, torch.float32, "probs")
    c, z, y, x = probs.shape
    full = tuple(full_shape) if full_shape is not None else (z, y, x)
    out = torch.empty(full, dtype=torch.uint8, device=probs.device)
    order_a = None if order is None else (C.c_int32 * len(order))(*[int(v) for v in order])
    lo = (C.c_int32 * 3)(*[int(v) for v in bbox_lo])
    fu = (C.c_int32 * 3)(*[int(v) for v in full])
    _lib.check(_lib.load().mi355_regions_to_labels(probs.data_ptr(), c, z, y, x, order_a, lo, fu, out.data_ptr(),
                                                   stream_of(probs)), "mi355_regions_to_labels")
    return out


def label_ensemble(a, b):
    """uint8(np.round((a + b) / 2.0)) - the reference's 2-model label ensemble (driver :305)."""
    import torch
    a = _require_cuda(a, torch.uint8, "a")
    b = _require_cuda(b, torch.uint8, "b")
    if a.shape != b.shape:
        raise ValueError("label_ensemble: shape mismatch")
    out = torch.empty_like(a)
    _lib.check(_lib.load().mi355_label_ensemble(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), stream_of(a)),
               "mi355_label_ensemble")
    return out


def prob_mean(a, b):
    import torch
    a = _require_cuda(a, torch.float32, "a")
    b = _require_cuda(b, torch.float32, "b")
    if a.shape != b.shape:
        raise ValueError("prob_mean: shape mismatch")
    out = torch.empty_like(a)
    _lib.check(_lib.load().mi355_prob_mean(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), stream_of(a)),
               "mi355_prob_mean")
    return out


def crop_mask(vol):
    """Nonzero mask with holes filled and its bounding box, on the device (nnU-Net v1 ``crop_to_nonzero`` as the
    reference's ``trainer.preprocess_patient`` runs it, driver :89).  vol: CUDA fp32 [C, Z, Y, X].
    Returns (mask uint8 [Z, Y, X], bbox [[z_lo, z_hi], [y_lo, y_hi], [x_lo, x_hi]])."""
    import torch
    _require_cuda(vol, torch.float32, "vol")
    if vol.dim() != 4:
        raise ValueError("crop_mask expects [C, Z, Y, X]")
    vol = vol.contiguous()
    c, z, y, x = vol.shape
    mask = torch.empty((z, y, x), dtype=torch.uint8, device=vol.device)
    box = (C.c_int32 * 6)()
    _lib.check(_lib.load().mi355_crop_mask(vol.data_ptr(), c, z, y, x, mask.data_ptr(), box, stream_of(vol)), "mi355_crop_mask")
    return mask, [[int(box[0]), int(box[1])], [int(box[2]), int(box[3])], [int(box[4]), int(box[5])]]


def zscore_masked_(vol, mask):
    """In place: per channel x[m] = (x[m]-mean)/(std+1e-8), x[~m] = 0 (nonCT + use_mask_for_norm)."""
    import torch
    if not (vol.is_cuda and vol.dtype == torch.float32 and vol.is_contiguous()):
        raise ValueError("zscore_masked_: vol must be a contiguous CUDA fp32 tensor")
    mask = _require_cuda(mask, torch.uint8, "mask")
    c = vol.shape[0]
    v = vol[0].numel()
    if mask.numel() != v:
        raise ValueError("zscore_masked_: mask shape mismatch")
    _lib.check(_lib.load().mi355_zscore_masked(vol.data_ptr(), mask.data_ptr(), c, v, stream_of(vol)),
               "mi355_zscore_masked")
    return vol


def resize_axis(x, axis: int, n_out: int, order: int):
    """One 1-D resampling pass along ``axis`` of a contiguous CUDA fp32 tensor (``mi355_resize_axis``): half-pixel-centred grid,
    edge replication, interpolation order 0 / 1 / 3 - skimage.transform.resize(order, mode='edge', anti_aliasing=False) along one
    axis, before its clipping."""
    import torch
    x = _require_cuda(x, torch.float32, "x")
    axis = axis % x.dim()
    n_in = int(x.shape[axis])
    if int(n_out) == n_in:
        return x
    outer = int(np.prod(x.shape[:axis], dtype=np.int64)) if axis > 0 else 1
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64)) if axis + 1 < x.dim() else 1
    out = torch.empty(tuple(x.shape[:axis]) + (int(n_out),) + tuple(x.shape[axis + 1:]), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().mi355_resize_axis(x.data_ptr(), out.data_ptr(), outer, n_in, int(n_out), inner, int(order), stream_of(x)),
               "mi355_resize_axis")
    return out


def clip_to_range_of_(x, ref, group_dims: int):
    """In place: every group of ``x`` (its first ``group_dims`` axes index the groups) clipped to [min, max] of the same group of
    ``ref`` (skimage's resize clips its output to the range of its input)."""
    import torch
    x = _require_cuda(x, torch.float32, "x")
    ref = _require_cuda(ref, torch.float32, "ref")
    if tuple(x.shape[:group_dims]) != tuple(ref.shape[:group_dims]):
        raise ValueError("clip_to_range_of_: group shapes differ")
    groups = int(np.prod(x.shape[:group_dims], dtype=np.int64)) if group_dims else 1
    _lib.check(_lib.load().mi355_clip_to_range_of(x.data_ptr(), groups, x.numel() // groups, ref.data_ptr(), ref.numel() // groups,
                                                  stream_of(x)), "mi355_clip_to_range_of")
    return x


def mask_to_float(mask):
    """fp32 indicator (1.0 / 0.0) of a uint8 mask (``mi355_mask_to_float``)."""
    import torch
    mask = _require_cuda(mask, torch.uint8, "mask")
    out = torch.empty(mask.shape, dtype=torch.float32, device=mask.device)
    _lib.check(_lib.load().mi355_mask_to_float(mask.data_ptr(), out.data_ptr(), mask.numel(), stream_of(mask)), "mi355_mask_to_float")
    return out


def threshold_ge(x, thr: float):
    """uint8 mask ``x >= thr`` (``mi355_threshold_ge``)."""
    import torch
    x = _require_cuda(x, torch.float32, "x")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().mi355_threshold_ge(x.data_ptr(), float(thr), out.data_ptr(), x.numel(), stream_of(x)), "mi355_threshold_ge")
    return out


def conv3d_ndhwc(x, weight, bias=None, stride=1, act=0, slope=0.01, impl="mfma"):
    """Single conv (test entry point). x: CUDA fp32 or fp16 [N,D,H,W,Cin]; weight: numpy [Cout,Cin,3,3,3]."""
    import torch
    if x.dtype == torch.float16:
        x = _require_cuda(x, torch.float16, "x")
        n, d, h, w, cin = x.shape
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        cout = weight.shape[0]
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        do, ho, wo = (d - 1) // stride + 1, (h - 1) // stride + 1, (w - 1) // stride + 1
        y = torch.full((n, do, ho, wo, cout), float("nan"), dtype=torch.float16, device=x.device)
        _lib.check(_lib.load().mi355_conv3d_ndhwc_f16(x.data_ptr(), n, d, h, w, cin, _lib.fptr(weight), _lib.fptr(b), cout,
                                                      stride, act, slope, y.data_ptr(), stream_of(x)), "mi355_conv3d_ndhwc_f16")
        return y
    x = _require_cuda(x, torch.float32, "x")
    n, d, h, w, cin = x.shape
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    cout = weight.shape[0]
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    do, ho, wo = (d - 1) // stride + 1, (h - 1) // stride + 1, (w - 1) // stride + 1
    y = torch.full((n, do, ho, wo, cout), float("nan"), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().mi355_conv3d_ndhwc(x.data_ptr(), n, d, h, w, cin, _lib.fptr(weight), _lib.fptr(b), cout,
                                              stride, act, slope, {"mfma": 0, "direct": 1}[impl], y.data_ptr(),
                                              stream_of(x)), "mi355_conv3d_ndhwc")
    return y


def conv3d_sums_ndhwc(x, weight, bias=None, stride=1, act=0, slope=0.01):
    """Single conv with the run-time-norm statistics epilogue (test entry point): returns (y, sums) with
    sums[n, cout] = (sum of y, sum of y^2) over the voxels, fp64 - what InstanceNorm / GroupNorm reduce y to
    (generic_UNet.py:62-72).  x: CUDA fp32 or fp16 [N,D,H,W,Cin]; weight: numpy [Cout,Cin,3,3,3]."""
    import torch
    f16 = x.dtype == torch.float16
    x = _require_cuda(x, torch.float16 if f16 else torch.float32, "x")
    n, d, h, w, cin = x.shape
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    cout = weight.shape[0]
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    do, ho, wo = (d - 1) // stride + 1, (h - 1) // stride + 1, (w - 1) // stride + 1
    y = torch.full((n, do, ho, wo, cout), float("nan"), dtype=x.dtype, device=x.device)
    sums = torch.full((n, cout, 2), float("nan"), dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().mi355_conv3d_sums_ndhwc(x.data_ptr(), 1 if f16 else 0, n, d, h, w, cin, _lib.fptr(weight), _lib.fptr(b),
                                                   cout, stride, act, slope, y.data_ptr(), sums.data_ptr(), stream_of(x)),
               "mi355_conv3d_sums_ndhwc")
    return y, sums


#: NaN elements every conv3d_fused_ndhwc output carries behind its end (a kernel that stores past the end shows there)
FUSED_GUARD = 64


def conv3d_fused_ndhwc(x0, weight, bias=None, x1=None, in_scale=None, in_shift=None, in_act=0, head_w=None, head_b=None,
                       stats=False, stride=1, act=0, slope=0.01, impl="mfma"):
    """One conv with the fused operands of a network conv (test entry point, ``mi355_conv3d_fused_ndhwc``).
    x0: CUDA fp32 or fp16 [N,D,H,W,C0]; x1: the same dtype [N,D,H,W,C1] or None (virtual concat, x0 first); weight: numpy
    [Cout,C0+C1,3,3,3]; in_scale / in_shift: CUDA fp32 [N,C0] (producer norm applied to x0 while staging, LeakyReLU when
    in_act = 1); head_w / head_b: CUDA fp32 [ncls,Cout] / [ncls] (fused 1x1x1 head: the result is fp32 logits [N,ncls,Do,Ho,Wo]
    instead of the NDHWC feature map).  Returns (y or logits, sums [N,Cout,2] fp64 or None).  Outputs start as NaN and are
    the front of a buffer with FUSED_GUARD more NaN elements."""
    import torch
    f16 = x0.dtype == torch.float16
    dt = torch.float16 if f16 else torch.float32
    x0 = _require_cuda(x0, dt, "x0")
    n, d, h, w, c0 = x0.shape
    c1 = 0
    if x1 is not None:
        x1 = _require_cuda(x1, dt, "x1")
        assert tuple(x1.shape[:4]) == (n, d, h, w), (x1.shape, x0.shape)
        c1 = x1.shape[4]
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    cout = weight.shape[0]
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    in_scale, in_shift, head_w, head_b = (None if t is None else _require_cuda(t, torch.float32, name) for t, name in (
        (in_scale, "in_scale"), (in_shift, "in_shift"), (head_w, "head_w"), (head_b, "head_b")))
    do, ho, wo = (d - 1) // stride + 1, (h - 1) // stride + 1, (w - 1) // stride + 1
    head = head_w is not None
    ncls = head_w.shape[0] if head else 0
    shape = (n, ncls, do, ho, wo) if head else (n, do, ho, wo, cout)
    numel = int(np.prod(shape))
    out = torch.full((numel + FUSED_GUARD,), float("nan"), dtype=torch.float32 if head else dt, device=x0.device)[:numel].view(shape)
    sums = torch.full((n, cout, 2), float("nan"), dtype=torch.float64, device=x0.device) if stats else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(_lib.load().mi355_conv3d_fused_ndhwc(
        x0.data_ptr(), ptr(x1), 1 if f16 else 0, n, d, h, w, c0, c1, _lib.fptr(weight), _lib.fptr(b), cout, stride, act, slope,
        {"mfma": 0, "direct": 1}[impl], ptr(in_scale), ptr(in_shift), in_act, ptr(head_w), ptr(head_b), ncls,
        out.data_ptr() if head else None, None if head else out.data_ptr(), ptr(sums), stream_of(x0)), "mi355_conv3d_fused_ndhwc")
    return out, sums


def conv3d_plan(dtype, shape, c0, cout, c1=0, stride=1, impl="mfma", stats=False, in_norm=False, head_ncls=0, s2_least_padding=False):
    """Dry run of ``conv3d_fused_ndhwc`` (test aid, ``mi355_conv3d_plan``; no GPU needed): the kernel a call of ``shape`` =
    (N, D, H, W) with C0 (+ C1) input channels would be dispatched to.  dtype: "f32" | "f16".  Returns a dict (rc, kernel, grid,
    lds_bytes, splitk, tile, fuses_in_norm, error); a refused call has rc < 0 and the dispatcher's message in ``error``.
    s2_least_padding: the call carries the stride-2 planner's least-padding hint (``mi355_conv3d_plan_hinted``)."""
    p = _lib.ConvPlan()
    n, d, h, w = (int(v) for v in shape)
    lib = _lib.load()
    args = ({"f32": 0, "f16": 1}[dtype], n, d, h, w, int(c0), int(c1), int(cout), int(stride),
            {"mfma": 0, "direct": 1}[impl], int(bool(stats)), int(bool(in_norm)), int(head_ncls))
    rc = lib.mi355_conv3d_plan_hinted(*args, 1, C.byref(p)) if s2_least_padding else lib.mi355_conv3d_plan(*args, C.byref(p))
    return {"rc": rc, "kernel": p.kernel.decode(), "grid": tuple(p.grid), "lds_bytes": int(p.lds_bytes), "splitk": int(p.splitk),
            "tile": tuple(p.tile), "fuses_in_norm": bool(p.fuses_in_norm), "error": (lib.mi355_last_error() or b"").decode() if rc < 0 else ""}


def tconv_plan(dtype, shape, cin, cout):
    """Dry run of ``tconv3d_ndhwc`` (test aid, ``mi355_tconv3d_plan``; no GPU needed): the transposed-conv kernel a call of
    ``shape`` = (N, D, H, W) input voxels with Cin -> Cout channels is sent to.  dtype: "f32" | "f16".  Returns a dict (rc, kernel,
    grid, lds_bytes, error); a refused call has rc < 0 and the launcher's message in ``error``."""
    p = _lib.ConvPlan()
    lib = _lib.load()
    rc = lib.mi355_tconv3d_plan({"f32": 0, "f16": 1}[dtype], *(int(v) for v in shape), int(cin), int(cout), C.byref(p))
    return {"rc": rc, "kernel": p.kernel.decode(), "grid": tuple(p.grid), "lds_bytes": int(p.lds_bytes),
            "error": (lib.mi355_last_error() or b"").decode() if rc < 0 else ""}


def conv_kernel_names():
    """Every kernel instantiation the 3x3x3 conv dispatch can launch (test aid, ``mi355_conv_kernel_names``; no GPU needed): a list
    of (table, name), one per row of the four row tables, names as ``conv3d_plan`` reports them (without " split-K")."""
    lib = _lib.load()
    need = lib.mi355_conv_kernel_names(None, 0)
    _lib.check(need, "mi355_conv_kernel_names")
    buf = C.create_string_buffer(int(need))
    _lib.check(lib.mi355_conv_kernel_names(buf, need), "mi355_conv_kernel_names")
    return [tuple(line.split(" | ", 1)) for line in buf.value.decode().splitlines()]


def stage0_plan(volume, patch, step_size=0.5, mirror_axes=(), r=2):
    """Dry run of the sliding window's shared stage 0 (``mi355_stage0_plan``; no GPU needed) for a volume (Z, Y, X), a patch and
    the mirror axes (a subset of (0, 1, 2)); ``r`` = blocks of encoder stage 0 (0: the network does not qualify).  Returns a dict:
    shared, n_tiles, n_mirrors, padded, volume (the whole-volume pass, padded to whole 4 x 8 x 8 tiles), slab_thickness and
    samples - one dict per (tile, mirror), tile-major, in the coordinates of its mirrored pass: tile, mirror (tuple of flipped
    axes), origin, face (six flags: z lo, z hi, y lo, y hi, x lo, x hi) and slabs {face index: (origin, shape)}."""
    lib = _lib.load()
    g = _lib.Stage0Geom()
    p3 = (C.c_int32 * 3)(*(int(v) for v in patch))
    z, y, x = (int(v) for v in volume)
    mask = sum(1 << int(a) for a in mirror_axes)
    n = lib.mi355_stage0_plan(z, y, x, p3, float(step_size), mask, int(r), C.byref(g), None, 0)
    _lib.check(n, "mi355_stage0_plan")
    buf = (_lib.Stage0Sample * max(n, 1))()
    _lib.check(lib.mi355_stage0_plan(z, y, x, p3, float(step_size), mask, int(r), C.byref(g), buf, n), "mi355_stage0_plan")
    samples = []
    for i in range(n):
        s = buf[i]
        samples.append({"tile": int(s.tile), "mirror": tuple(a for a in range(3) if s.mirror >> a & 1), "origin": tuple(s.origin),
                        "face": tuple(int(f) for f in s.face),
                        "slabs": {f: (tuple(s.slab_origin[f]), tuple(s.slab_shape[f])) for f in range(6) if s.face[f]}})
    return {"shared": bool(g.shared), "n_tiles": int(g.n_tiles), "n_mirrors": int(g.n_mirrors), "padded": tuple(g.padded),
            "volume": tuple(g.volume), "slab_thickness": tuple(g.slab_thickness), "samples": samples}


def stage0_merge_plan(volume, patch, step_size=0.5, mirror_axes=(), r=2, skip_half=True):
    """Dry run of the merged stage-0 slabs (``mi355_stage0_merge_plan``; no GPU needed).  Returns a dict: shared, r, rs (the shell
    depths of the level-0 features and of the slab chain), n_tiles, n_mirrors, padded, volume, slab_thickness, n_slabs / slab_shape /
    voxels per axis (z per tile; y, x per key), voxels_per_tile (what per-tile slabs on all axes hold), slabs {1: [...], 2: [...]} of
    dicts mirror (tuple of flipped axes), side, origin - in key order -, and samples: one dict per (tile, mirror), tile-major, with
    tile, mirror, origin, slab (six entries: z faces 0 = per-tile slab, y / x faces the index in slabs[axis], -1 = a volume face)
    and offset {face: (z, y, x)} of the tile's part inside the slab."""
    lib = _lib.load()
    g = _lib.Stage0MergeGeom()
    p3 = (C.c_int32 * 3)(*(int(v) for v in patch))
    z, y, x = (int(v) for v in volume)
    mask = sum(1 << int(a) for a in mirror_axes)
    args = (z, y, x, p3, float(step_size), mask, int(r), int(bool(skip_half)), C.byref(g))
    n = lib.mi355_stage0_merge_plan(*args, None, 0, None, 0)
    _lib.check(n, "mi355_stage0_merge_plan")
    nk = int(g.n_slabs[1]) + int(g.n_slabs[2])
    kbuf, sbuf = (_lib.Stage0MergeSlab * max(nk, 1))(), (_lib.Stage0MergeSample * max(n, 1))()
    _lib.check(lib.mi355_stage0_merge_plan(*args, kbuf, nk, sbuf, n), "mi355_stage0_merge_plan")
    axes = lambda m: tuple(a for a in range(3) if m >> a & 1)
    slabs = {1: [], 2: []}
    for i in range(nk):
        k = kbuf[i]
        slabs[int(k.axis)].append({"mirror": axes(k.mirror), "side": int(k.side), "origin": tuple(k.origin)})
    samples = []
    for i in range(n):
        q = sbuf[i]
        samples.append({"tile": int(q.tile), "mirror": axes(q.mirror), "origin": tuple(q.origin), "slab": tuple(int(v) for v in q.slab),
                        "offset": {f: tuple(q.offset[f]) for f in range(2, 6) if q.slab[f] >= 0}})
    return {"shared": bool(g.shared), "r": int(g.r), "rs": int(g.rs), "n_tiles": int(g.n_tiles), "n_mirrors": int(g.n_mirrors),
            "padded": tuple(g.padded), "volume": tuple(g.volume), "slab_thickness": tuple(g.slab_thickness), "n_slabs": tuple(g.n_slabs),
            "slab_shape": tuple(tuple(v) for v in g.slab_shape), "voxels": tuple(int(v) for v in g.voxels),
            "voxels_per_tile": int(g.voxels_per_tile), "slabs": slabs, "samples": samples}


def skip_share_plan(volume, patch, step_size=0.5, mirror_axes=(), dtype="f32", norm="batch", nonlin_first=False, enc0_blocks=2,
                    stride=1, skip_is_enc0=True, c_up=32, c_skip=32, cout=32, head_ncls=0, batch_tiles=0, rank=0, world=1):
    """Dry run of the shared skip half (``mi355_skip_share_plan``; no GPU needed): whether the last decoder stage's first conv takes
    its skip half from the shared stage-0 pass, for a volume (Z, Y, X), a patch, the mirror axes and a description of the network
    (defaults: model A).  Returns a dict: stage0_shared, skip_shared, r, skip_shell (r + 1 when on, else 0), n_tiles, n_mirrors,
    volume and slab_thickness.  batch_tiles, rank and world are passed through; the result does not depend on them."""
    nd = _lib.SkipShareNet({"f32": 0, "f16": 1}[dtype], {"none": 0, "batch": 1, "instance": 2, "group": 3}[norm], int(bool(nonlin_first)),
                           int(enc0_blocks), int(stride), int(bool(skip_is_enc0)), int(c_up), int(c_skip), int(cout), int(head_ncls))
    g = _lib.SkipShareGeom()
    z, y, x = (int(v) for v in volume)
    mask = sum(1 << int(a) for a in mirror_axes)
    _lib.check(_lib.load().mi355_skip_share_plan(z, y, x, _i3(patch), float(step_size), mask, C.byref(nd), int(batch_tiles), int(rank),
                                                 int(world), C.byref(g)), "mi355_skip_share_plan")
    return {"stage0_shared": bool(g.stage0_shared), "skip_shared": bool(g.skip_shared), "r": int(g.r), "skip_shell": int(g.skip_shell),
            "n_tiles": int(g.n_tiles), "n_mirrors": int(g.n_mirrors), "volume": tuple(g.volume), "slab_thickness": tuple(g.slab_thickness)}


def conv3d_wino3_ndhwc(x0, weight, bias=None, x1=None, addend=None, act=0, slope=0.01):
    """One stride-1 conv on ``conv3_f32_wino3_kernel<0, false>`` whatever the size (test entry point, ``mi355_conv3d_wino3_ndhwc``):
    act(bias + conv(cat(x0, x1)) + addend).  x0 / x1: CUDA fp32 [N,D,H,W,C]; addend: CUDA fp32 [N,D,H,W,Cout] or None; weight:
    numpy [Cout,C0+C1,3,3,3]."""
    import torch
    x0 = _require_cuda(x0, torch.float32, "x0")
    n, d, h, w, c0 = x0.shape
    c1 = 0
    if x1 is not None:
        x1 = _require_cuda(x1, torch.float32, "x1")
        if tuple(x1.shape[:4]) != (n, d, h, w):
            raise ValueError("conv3d_wino3_ndhwc: x1 must cover the same voxels as x0")
        c1 = int(x1.shape[4])
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    cout = weight.shape[0]
    if weight.shape[1] != c0 + c1:
        raise ValueError(f"conv3d_wino3_ndhwc: weight takes {weight.shape[1]} channels, the inputs hold {c0} + {c1}")
    if addend is not None:
        addend = _require_cuda(addend, torch.float32, "addend")
        if tuple(addend.shape) != (n, d, h, w, cout):
            raise ValueError("conv3d_wino3_ndhwc: addend must be [N,D,H,W,Cout]")
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    y = torch.full((n, d, h, w, cout), float("nan"), dtype=torch.float32, device=x0.device)
    _lib.check(_lib.load().mi355_conv3d_wino3_ndhwc(x0.data_ptr(), None if x1 is None else x1.data_ptr(), n, d, h, w, c0, c1,
                                                    _lib.fptr(weight), _lib.fptr(b), cout, act, slope,
                                                    None if addend is None else addend.data_ptr(), y.data_ptr(), stream_of(x0)),
               "mi355_conv3d_wino3_ndhwc")
    return y


def stage0_view_plan(volume, patch, step_size=0.5, mirror_axes=(), dtype="f32", norm="batch", nonlin_first=False, enc0_blocks=2,
                     stride=1, skip_is_enc0=True, c_up=32, c_skip=32, cout=32, head_ncls=0, c_level1=64, batch_samples=0):
    """Dry run of the stage-0 views (``mi355_stage0_view_plan``; no GPU needed) for a volume (Z, Y, X), a patch, the mirror axes and
    a description of the network (defaults: model A; ``c_level1`` = output channels of the first stride-2 conv, ``batch_samples`` =
    (tile, mirror) samples per forward, 0 = the default).  Returns a dict: enc0_viewed, half_viewed (which tile tensor is read
    through a view), depth (shell depths of the two), n_tiles, n_mirrors, volume and samples - one dict per (tile, mirror), tile-major
    as ``stage0_plan`` lists them: offset (voxel index of the tile's origin in the whole-volume tensor), faces (six flags) and
    shell_voxels (what the gather still writes, per tensor)."""
    nd = _lib.SkipShareNet({"f32": 0, "f16": 1}[dtype], {"none": 0, "batch": 1, "instance": 2, "group": 3}[norm], int(bool(nonlin_first)),
                           int(enc0_blocks), int(stride), int(bool(skip_is_enc0)), int(c_up), int(c_skip), int(cout), int(head_ncls))
    lib = _lib.load()
    g = _lib.Stage0ViewGeom()
    z, y, x = (int(v) for v in volume)
    mask = sum(1 << int(a) for a in mirror_axes)
    args = (z, y, x, _i3(patch), float(step_size), mask, C.byref(nd), int(c_level1), int(batch_samples), C.byref(g))
    n = lib.mi355_stage0_view_plan(*args, None, 0)
    _lib.check(n, "mi355_stage0_view_plan")
    buf = (_lib.Stage0ViewSample * max(n, 1))()
    _lib.check(lib.mi355_stage0_view_plan(*args, buf, n), "mi355_stage0_view_plan")
    samples = [{"offset": int(buf[i].offset), "faces": tuple(buf[i].faces >> f & 1 for f in range(6)),
                "shell_voxels": tuple(int(v) for v in buf[i].shell_voxels)} for i in range(n)]
    return {"enc0_viewed": bool(g.enc0_viewed), "half_viewed": bool(g.half_viewed), "depth": tuple(g.depth), "n_tiles": int(g.n_tiles),
            "n_mirrors": int(g.n_mirrors), "volume": tuple(g.volume), "samples": samples}


def level1_share_plan(volume, patch, step_size=0.5, mirror_axes=(), mode=1, dtype="f32", norm="batch", nonlin_first=False, enc0_blocks=2,
                      c_level0=32, num_pool=5, enc1_blocks=2, c_level1=64, skip_is_enc1=True, dec1_blocks=2):
    """Dry run of the shared level 1 (``mi355_level1_share_plan``; no GPU needed: the decision a sliding window runs under ``MI355_SHARE_LEVEL1``) for a volume
    (Z, Y, X), a patch, the mirror axes and a description of the network (defaults: model A).  mode: 0 off, 1 the default rule,
    2 wherever it is structurally possible.  Returns a dict: possible, on, r0, k1, d1, dS, n_tiles, n_mirrors, padded, volume,
    stage0_slab_thickness, merged (per axis), region (level-0 extent), slab_thickness (level 1), n_slabs, region_voxels /
    slab_voxels / tile_voxels (level-1 voxels), regions - dicts (mirror, origin, faces) - and samples, tile-major - dicts (tile,
    mirror, region, origin, origin1, faces and slabs: face -> (offset, shape) of the level-0 sub-box of the tile)."""
    last = _lib.SkipShareNet({"f32": 0, "f16": 1}[dtype], {"none": 0, "batch": 1, "instance": 2, "group": 3}[norm], int(bool(nonlin_first)),
                             int(enc0_blocks), 1, 1, int(c_level0), int(c_level0), int(c_level0), 0)
    nd = _lib.Level1ShareNet(last, int(num_pool), int(enc1_blocks), int(c_level1), int(bool(skip_is_enc1)), int(dec1_blocks),
                             int(c_level1), int(c_level1))
    lib = _lib.load()
    g = _lib.Level1ShareGeom()
    z, y, x = (int(v) for v in volume)
    mask = sum(1 << int(a) for a in mirror_axes)
    head = (z, y, x, _i3(patch), float(step_size), mask, C.byref(nd), int(mode), C.byref(g))
    n = lib.mi355_level1_share_plan(*head, None, 0, None, 0)
    _lib.check(n, "mi355_level1_share_plan")
    regs = (_lib.Level1ShareRegion * max(int(g.n_regions), 1))()
    smp = (_lib.Level1ShareSample * max(n, 1))()
    _lib.check(lib.mi355_level1_share_plan(*head, regs, int(g.n_regions), smp, n), "mi355_level1_share_plan")
    axes = lambda m: tuple(a for a in range(3) if m >> a & 1)  # noqa: E731
    bits = lambda v: tuple(v >> f & 1 for f in range(6))  # noqa: E731
    out = {k: int(getattr(g, k)) for k in ("r0", "k1", "d1", "dS", "n_tiles", "n_mirrors", "region_voxels", "slab_voxels", "tile_voxels")}
    out.update({k: bool(getattr(g, k)) for k in ("possible", "on")})
    out.update({k: tuple(int(v) for v in getattr(g, k)) for k in ("padded", "volume", "stage0_slab_thickness", "region", "slab_thickness", "n_slabs")})
    out["merged"] = tuple(bool(v) for v in g.merged)
    out["regions"] = [{"mirror": axes(regs[i].mirror), "origin": tuple(regs[i].origin), "faces": bits(regs[i].faces)} for i in range(int(g.n_regions))]
    out["samples"] = [{"tile": int(s.tile), "mirror": axes(s.mirror), "region": int(s.region), "origin": tuple(s.origin), "origin1": tuple(s.origin1),
                       "faces": bits(s.faces),
                       "slabs": {f: (tuple(s.slab_offset[f]), tuple(s.slab_shape[f])) for f in range(6) if s.slab[f]}} for s in smp[:n]]
    return out


def _stage0_view(src, samples, depth):
    """src: CUDA fp32 [n_wv, Ve0, Ve1, Ve2, C]; samples: dicts {wv, origin, faces: six flags} -> (Stage0View, keep-alive)"""
    import torch
    src = _require_cuda(src, torch.float32, "view source")
    if src.dim() != 5 or len(samples) > 64:
        raise ValueError("stage-0 view: source must be [n_wv, Ve0, Ve1, Ve2, C], at most 64 samples")
    v = _lib.Stage0View()
    v.src_dev, v.n_wv, v.depth, v.n_samples = src.data_ptr(), int(src.shape[0]), int(depth), len(samples)
    for k in range(3):
        v.volume[k] = int(src.shape[1 + k])
    for i, sm in enumerate(samples):
        v.samples[i].wv = int(sm["wv"])
        for k in range(3):
            v.samples[i].origin[k] = int(sm["origin"][k])
        v.samples[i].faces = sum(1 << f for f in range(6) if sm["faces"][f])
    return v, src


def conv3d_s2dma_view_ndhwc(x, weight, bias=None, view=None, act=0, slope=0.01, force=True, s2_least_padding=False, x1=None):
    """One stride-2 conv on ``conv3_f32_s2dma_kernel`` or, with ``view`` = (src, samples, depth), on its view twin (test entry point,
    ``mi355_conv3d_s2dma_view_ndhwc``).  x: CUDA fp32 [N,D,H,W,Cin], the dense tile tensor - with a view only its shell voxels are
    read; src: CUDA fp32 [n_wv,Ve0,Ve1,Ve2,Cin]; samples: one dict {wv, origin, faces} per sample of x; weight: numpy [Cout,Cin,3,3,3].
    s2_least_padding: the call carries the planner's least-padding hint (``mi355_conv3d_s2dma_hinted_ndhwc``).
    x1: the second half of a virtual concat [x | x1] (``mi355_conv3d_s2dma_concat_ndhwc``; no view then)."""
    import torch
    x = _require_cuda(x, torch.float32, "x")
    n, d, h, w, cin = x.shape
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    cout = weight.shape[0]
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    if x1 is not None:
        x1 = _require_cuda(x1, torch.float32, "x1")
        if view is not None or tuple(x1.shape[:4]) != (n, d, h, w):
            raise ValueError("conv3d_s2dma_view_ndhwc: x1 needs x's [N,D,H,W] and comes without a view")
        y = torch.full((n, (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cout), float("nan"), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().mi355_conv3d_s2dma_concat_ndhwc(x.data_ptr(), x1.data_ptr(), n, d, h, w, cin, int(x1.shape[4]), _lib.fptr(weight),
                                                                _lib.fptr(b), cout, act, slope, int(bool(force)), int(bool(s2_least_padding)),
                                                                y.data_ptr(), stream_of(x)), "mi355_conv3d_s2dma_concat_ndhwc")
        return y
    v, keep = (None, None) if view is None else _stage0_view(view[0], view[1], view[2])
    if keep is not None and keep.shape[4] != cin:
        raise ValueError("conv3d_s2dma_view_ndhwc: the view's source must have the input's channels")
    y = torch.full((n, (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1, cout), float("nan"), dtype=torch.float32, device=x.device)
    head = (x.data_ptr(), None if v is None else C.byref(v), n, d, h, w, cin, _lib.fptr(weight), _lib.fptr(b), cout, act, slope, int(bool(force)))
    if s2_least_padding:
        _lib.check(_lib.load().mi355_conv3d_s2dma_hinted_ndhwc(*head, 1, y.data_ptr(), stream_of(x)), "mi355_conv3d_s2dma_hinted_ndhwc")
    else:
        _lib.check(_lib.load().mi355_conv3d_s2dma_view_ndhwc(*head, y.data_ptr(), stream_of(x)), "mi355_conv3d_s2dma_view_ndhwc")
    return y


def conv_s2_split_pack(weight, cin_pad=None):
    """The split-bf16 weight pack of an fp32 stride-2 layer (test aid, ``mi355_conv_s2_split_pack``; no GPU needed).  weight: numpy
    [Cout,Cin,3,3,3], Cout a multiple of 64; cin_pad (default: Cin rounded up to 8) the padded channel count.  Returns a uint16 array
    [Cout/64, cin_pad/8, 3 (dz), 3 (hi, mid, lo), 4608] of bf16 bit patterns; within a piece: group 0 (tap dz*9 alone) is
    [nf 2][lane 64][4], groups g = 1..4 (taps dz*9 + 2g-1, 2g) follow at 512 + (g-1)*1024 as [nf 2][lane 64][tap 2][4]."""
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    cin_pad = (cin + 7) // 8 * 8 if cin_pad is None else int(cin_pad)
    lib = _lib.load()
    n = lib.mi355_conv_s2_split_pack(_lib.fptr(weight), cin, cin_pad, cout, None, 0)
    if n < 0:
        _lib.check(int(n), "mi355_conv_s2_split_pack")
    out = np.zeros(int(n), dtype=np.uint16)
    lib.mi355_conv_s2_split_pack(_lib.fptr(weight), cin, cin_pad, cout, out.ctypes.data_as(C.POINTER(C.c_uint16)), int(n))
    return out.reshape(cout // 64, cin_pad // 8, 3, 3, 4608)


def conv3d_wino3_view_ndhwc(x0, weight, bias, addend, view=None, act=0, slope=0.01):
    """``conv3d_wino3_ndhwc`` with an addend that is read through ``view`` = (src, samples, depth) (test entry point,
    ``mi355_conv3d_wino3_view_ndhwc``): addend CUDA fp32 [N,D,H,W,Cout], the dense tile tensor - with a view only its shell voxels
    are read; src: CUDA fp32 [n_wv,Ve0,Ve1,Ve2,Cout]."""
    import torch
    x0 = _require_cuda(x0, torch.float32, "x0")
    n, d, h, w, c0 = x0.shape
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    cout = weight.shape[0]
    addend = _require_cuda(addend, torch.float32, "addend")
    if tuple(addend.shape) != (n, d, h, w, cout):
        raise ValueError("conv3d_wino3_view_ndhwc: addend must be [N,D,H,W,Cout]")
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    v, keep = (None, None) if view is None else _stage0_view(view[0], view[1], view[2])
    if keep is not None and keep.shape[4] != cout:
        raise ValueError("conv3d_wino3_view_ndhwc: the view's source must have the addend's channels")
    y = torch.full((n, d, h, w, cout), float("nan"), dtype=torch.float32, device=x0.device)
    _lib.check(_lib.load().mi355_conv3d_wino3_view_ndhwc(x0.data_ptr(), n, d, h, w, c0, _lib.fptr(weight), _lib.fptr(b), cout, act, slope,
                                                         addend.data_ptr(), None if v is None else C.byref(v), y.data_ptr(), stream_of(x0)),
               "mi355_conv3d_wino3_view_ndhwc")
    return y


def last_conv_kernel() -> str:
    """Kernel instantiation the last ``conv3d_ndhwc`` call of this thread ran on (test aid)."""
    return (_lib.load().mi355_last_conv_kernel() or b"").decode()


def tconv3d_ndhwc(x, weight):
    """Single ConvTranspose3d k=2 s=2 (test entry point). weight: numpy [Cin,Cout,2,2,2]."""
    import torch
    if x.dtype == torch.float16:
        x = _require_cuda(x, torch.float16, "x")
        n, d, h, w, cin = x.shape
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        cout = weight.shape[1]
        y = torch.full((n, 2 * d, 2 * h, 2 * w, cout), float("nan"), dtype=torch.float16, device=x.device)
        _lib.check(_lib.load().mi355_tconv3d_ndhwc_f16(x.data_ptr(), n, d, h, w, cin, _lib.fptr(weight), cout, y.data_ptr(),
                                                       stream_of(x)), "mi355_tconv3d_ndhwc_f16")
        return y
    x = _require_cuda(x, torch.float32, "x")
    n, d, h, w, cin = x.shape
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    cout = weight.shape[1]
    y = torch.full((n, 2 * d, 2 * h, 2 * w, cout), float("nan"), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().mi355_tconv3d_ndhwc(x.data_ptr(), n, d, h, w, cin, _lib.fptr(weight), cout, y.data_ptr(),
                                               stream_of(x)), "mi355_tconv3d_ndhwc")
    return y


def compute_steps(patch, image, step_size):
    buf = (C.c_int32 * 256)()
    n = _lib.load().mi355_compute_steps(int(patch), int(image), float(step_size), buf, 256)
    _lib.check(n, "mi355_compute_steps")
    return [int(buf[i]) for i in range(n)]


# ---- the kernels around the convolutions, one launch each (test entry points; every call waits for the stream).  fp32 tensors
# are plain NDHWC, fp16 tensors channel-blocked [N, C / 8, V, 8], passed as they are.
def _i3(v):
    v = [int(k) for k in v]
    if len(v) != 3:
        raise ValueError(f"expected three extents, got {v}")
    return (C.c_int32 * 3)(*v)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _f32(t, name, numel=None):
    import torch
    if t is None:
        return None
    t = _require_cuda(t, torch.float32, name)
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name}: {t.numel()} elements, expected {numel}")
    return t


def norm_finalize(stats, count, kind="instance", groups=1, eps=1e-5, gamma=None, beta=None):
    """``mi355_norm_finalize``: stats CUDA fp64 [N, C, 2] (sum, sum of squares over ``count`` voxels) -> (scale, shift) CUDA fp32
    [N, C]; gamma / beta CUDA fp32 [C] or None."""
    import torch
    stats = _require_cuda(stats, torch.float64, "stats")
    n, c, two = stats.shape
    if two != 2:
        raise ValueError("stats must be [N, C, 2]")
    gamma, beta = _f32(gamma, "gamma", c), _f32(beta, "beta", c)
    scale = torch.full((n, c), float("nan"), dtype=torch.float32, device=stats.device)
    shift = torch.full((n, c), float("nan"), dtype=torch.float32, device=stats.device)
    _lib.check(_lib.load().mi355_norm_finalize(stats.data_ptr(), n, c, int(count), {"instance": _lib.NORM_INSTANCE, "group": _lib.NORM_GROUP}[kind],
                                               int(groups), float(eps), _ptr(gamma), _ptr(beta), scale.data_ptr(), shift.data_ptr(),
                                               stream_of(stats)), "mi355_norm_finalize")
    return scale, shift


def norm_apply_(x, scale, shift, act=0, slope=0.01):
    """``mi355_norm_apply``, in place.  x: contiguous CUDA fp32 [N, V, C] or fp16 channel-blocked [N, C / 8, V, 8]; scale / shift
    CUDA fp32 [N, C]."""
    import torch
    if not (x.is_cuda and x.is_contiguous() and x.dtype in (torch.float32, torch.float16)):
        raise ValueError("norm_apply_: x must be a contiguous CUDA fp32 / fp16 tensor")
    if x.dtype == torch.float16:
        n, cb, v, eight = x.shape
        if eight != 8:
            raise ValueError("norm_apply_: fp16 tensors are [N, C / 8, V, 8]")
        c = cb * 8
    else:
        n, v, c = x.shape
    scale, shift = _f32(scale, "scale", n * c), _f32(shift, "shift", n * c)
    _lib.check(_lib.load().mi355_norm_apply(x.data_ptr(), int(x.dtype == torch.float16), n, v, c, scale.data_ptr(), shift.data_ptr(), int(act),
                                            float(slope), stream_of(x)), "mi355_norm_apply")
    return x


def extract_tiles(vol, pad, tiles, patch, cpad, dtype="f32"):
    """``mi355_extract_tiles``.  vol: CUDA fp32 [C, Z, Y, X]; pad: its offset (z, y, x) in the padded volume; tiles: (z0, y0, x0,
    mirror mask) per sample.  Returns [n, PV, cpad] (fp32, and fp16 when cpad % 8 != 0) or the blocked [n, cpad / 8, PV, 8] fp16."""
    import torch
    vol = _require_cuda(vol, torch.float32, "vol")
    c, z, y, x = vol.shape
    tiles = [tuple(int(k) for k in t) for t in tiles]
    if not tiles or any(len(t) != 4 for t in tiles):
        raise ValueError("extract_tiles: tiles are (z0, y0, x0, mirror)")
    n, cpad = len(tiles), int(cpad)
    pv = int(np.prod([int(p) for p in patch]))
    f16 = {"f32": False, "f16": True}[dtype]
    shape = (n, cpad // 8, pv, 8) if f16 and cpad % 8 == 0 else (n, pv, cpad)
    out = torch.full(shape, float("nan"), dtype=torch.float16 if f16 else torch.float32, device=vol.device)
    flat = (C.c_int32 * (4 * n))(*[k for t in tiles for k in t])
    _lib.check(_lib.load().mi355_extract_tiles(vol.data_ptr(), c, z, y, x, _i3(pad), flat, n, _i3(patch), cpad, out.data_ptr(), int(f16),
                                               stream_of(vol)), "mi355_extract_tiles")
    return out


def _feat_dims(feat):
    """(f16, samples, voxels, channels) of a feature tensor in the network's layout."""
    import torch
    if not (feat.is_cuda and feat.is_contiguous() and feat.dtype in (torch.float32, torch.float16)):
        raise ValueError("feat must be a contiguous CUDA fp32 / fp16 tensor")
    if feat.dtype == torch.float16:
        n, cb, v, eight = feat.shape
        if eight != 8:
            raise ValueError("fp16 features are [N, C / 8, V, 8]")
        return True, n, v, cb * 8
    n, v, c = feat.shape
    return False, n, v, c


def _head_operands(weight, bias, cin):
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    if weight.ndim != 2 or weight.shape[1] != cin:
        raise ValueError(f"head weight must be [ncls, {cin}]")
    bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    if bias is not None and bias.shape != (weight.shape[0],):
        raise ValueError("head bias must be [ncls]")
    return weight, bias


def head_logits(feat, weight, bias=None, scale=None, shift=None, slope=1.0):
    """``mi355_head_logits``.  feat: CUDA fp32 [N, V, C] or fp16 blocked [N, C / 8, V, 8]; weight numpy [ncls, C]; scale / shift CUDA
    fp32 [N, C] or None.  Returns logits CUDA fp32 [N, ncls, V]."""
    import torch
    f16, n, v, c = _feat_dims(feat)
    weight, bias = _head_operands(weight, bias, c)
    scale, shift = _f32(scale, "scale", n * c), _f32(shift, "shift", n * c)
    ncls = weight.shape[0]
    out = torch.full((n, ncls, v), float("nan"), dtype=torch.float32, device=feat.device)
    _lib.check(_lib.load().mi355_head_logits(feat.data_ptr(), int(f16), n, v, c, _lib.fptr(weight), _lib.fptr(bias), ncls, _ptr(scale),
                                             _ptr(shift), float(slope), out.data_ptr(), stream_of(feat)), "mi355_head_logits")
    return out


def _tile_operands(agg, cnt, gauss, ncls, patch, origin, name):
    import torch
    agg = _require_cuda(agg, torch.float32, "agg")
    if not agg.is_contiguous() or agg.dim() != 4 or agg.shape[0] != ncls:
        raise ValueError(f"{name}: agg must be a contiguous [ncls, Zp, Yp, Xp]")
    padded = tuple(int(k) for k in agg.shape[1:])
    if cnt is not None and (not cnt.is_cuda or cnt.dtype != torch.float32 or not cnt.is_contiguous() or tuple(cnt.shape) != padded):
        raise ValueError(f"{name}: cnt must be a contiguous CUDA fp32 [Zp, Yp, Xp]")
    pv = int(np.prod([int(p) for p in patch]))
    gauss = _f32(gauss, "gauss", pv)
    if any(int(o) < 0 or int(o) + int(p) > q for o, p, q in zip(origin, patch, padded)):
        raise ValueError(f"{name}: the tile leaves the padded grid")
    return gauss, padded, pv


def _agg2_operand(agg, agg2, name):
    import torch
    if agg2 is None or not agg2.is_cuda or agg2.dtype != torch.float32 or not agg2.is_contiguous() or agg2.shape != agg.shape:
        raise ValueError(f"{name}: agg2 must be a contiguous CUDA fp32 tensor of agg's shape")
    if agg2.data_ptr() == agg.data_ptr():
        raise ValueError(f"{name}: agg2 must not be agg")
    return agg2


# The aggregation wrappers and their _m2 twins: one implementation per pair.  m2: the call is the twin - it takes agg2 and calls the
# entry point's _m2 twin, which has agg2 behind agg in its arguments; the public function's name, for the messages, follows from it.
def _aggregate_call(symbol, m2, src, head, mirrors, patch, nonlin, gauss, agg, agg2, cnt, padded, where):
    from .predictor import NONLIN
    symbol += "_m2" if m2 else ""
    moments = [agg2.data_ptr()] if m2 else []
    _lib.check(getattr(_lib.load(), symbol)(*head, (C.c_int32 * max(len(mirrors), 1))(*mirrors), len(mirrors), _i3(patch), NONLIN[nonlin], _ptr(gauss),
                                            agg.data_ptr(), *moments, _ptr(cnt), _i3(padded), *where, stream_of(src)), symbol)


def _head_aggregate(m2, feat, weight, bias, mirrors, patch, nonlin, agg, agg2, cnt, origin, gauss, first_sample, scale, shift, slope):
    name = "head_aggregate_m2_" if m2 else "head_aggregate_"
    f16, n, v, c = _feat_dims(feat)
    weight, bias = _head_operands(weight, bias, c)
    mirrors = [int(m) for m in mirrors]
    gauss, padded, pv = _tile_operands(agg, cnt, gauss, weight.shape[0], patch, origin, name)
    if m2:
        agg2 = _agg2_operand(agg, agg2, name)
    if v != pv or first_sample < 0 or first_sample + len(mirrors) > n:
        raise ValueError(f"{name}: feat does not hold the tile's samples")
    scale, shift = _f32(scale, "scale", n * c), _f32(shift, "shift", n * c)
    head = (feat.data_ptr(), int(f16), c, _lib.fptr(weight), _lib.fptr(bias), weight.shape[0], _ptr(scale), _ptr(shift), float(slope), int(first_sample))
    _aggregate_call("mi355_head_aggregate", m2, feat, head, mirrors, patch, nonlin, gauss, agg, agg2, cnt, padded, (_i3(origin),))


def _logits_aggregate(m2, logits, mirrors, patch, nonlin, agg, agg2, cnt, origin, gauss, first_sample):
    import torch
    name = "logits_aggregate_m2_" if m2 else "logits_aggregate_"
    logits = _require_cuda(logits, torch.float32, "logits")
    n, ncls, v = logits.shape
    mirrors = [int(m) for m in mirrors]
    gauss, padded, pv = _tile_operands(agg, cnt, gauss, ncls, patch, origin, name)
    if m2:
        agg2 = _agg2_operand(agg, agg2, name)
    if v != pv or first_sample < 0 or first_sample + len(mirrors) > n:
        raise ValueError(f"{name}: logits do not hold the tile's samples")
    _aggregate_call("mi355_logits_aggregate", m2, logits, (logits.data_ptr(), ncls, int(first_sample)), mirrors, patch, nonlin, gauss, agg, agg2, cnt, padded, (_i3(origin),))


def _logits_aggregate_tiles(m2, logits, mirrors, patch, nonlin, agg, agg2, cnt, origins, gauss, first_sample):
    import torch
    name = "logits_aggregate_tiles_m2_" if m2 else "logits_aggregate_tiles_"
    logits = _require_cuda(logits, torch.float32, "logits")
    n, ncls, v = logits.shape
    mirrors = [int(m) for m in mirrors]
    origins = [[int(k) for k in o] for o in origins]
    if not origins:
        raise ValueError(f"{name}: no tile")
    for o in origins:
        gauss_dev, padded, pv = _tile_operands(agg, cnt, gauss, ncls, patch, o, name)
    if m2:
        agg2 = _agg2_operand(agg, agg2, name)
    if v != pv or first_sample < 0 or first_sample + len(origins) * len(mirrors) > n:
        raise ValueError(f"{name}: logits do not hold the tiles' samples")
    flat = [k for o in origins for k in o]
    _aggregate_call("mi355_logits_aggregate_tiles", m2, logits, (logits.data_ptr(), ncls, int(first_sample)), mirrors, patch, nonlin, gauss_dev, agg, agg2, cnt, padded,
                    ((C.c_int32 * len(flat))(*flat), len(origins)))


def head_aggregate_(feat, weight, bias, mirrors, patch, nonlin, agg, cnt, origin, gauss=None, first_sample=0, scale=None, shift=None,
                    slope=1.0):
    """``mi355_head_aggregate``: one tile into agg [ncls, Zp, Yp, Xp] / cnt [Zp, Yp, Xp] (CUDA fp32, in place; cnt may be None).
    feat: every sample of the forward ([S, PV, C] fp32 or blocked fp16), of which first_sample .. + len(mirrors) - 1 are this tile's;
    mirrors: masks, bit0 z; nonlin "identity" | "sigmoid" | "softmax"; gauss CUDA fp32 [patch] or None."""
    _head_aggregate(False, feat, weight, bias, mirrors, patch, nonlin, agg, None, cnt, origin, gauss, first_sample, scale, shift, slope)


def logits_aggregate_(logits, mirrors, patch, nonlin, agg, cnt, origin, gauss=None, first_sample=0):
    """``mi355_logits_aggregate``: as ``head_aggregate_`` from logits CUDA fp32 [S, ncls, PV]."""
    _logits_aggregate(False, logits, mirrors, patch, nonlin, agg, None, cnt, origin, gauss, first_sample)


def logits_aggregate_tiles_(logits, mirrors, patch, nonlin, agg, cnt, origins, gauss=None, first_sample=0):
    """``mi355_logits_aggregate_tiles``: the tiles at ``origins`` (tile i: samples first_sample + i * len(mirrors) ..) in one launch,
    bit-identical to ``logits_aggregate_`` tile by tile in that order."""
    _logits_aggregate_tiles(False, logits, mirrors, patch, nonlin, agg, None, cnt, origins, gauss, first_sample)


def head_aggregate_m2_(feat, weight, bias, mirrors, patch, nonlin, agg, agg2, cnt, origin, gauss=None, first_sample=0, scale=None, shift=None,
                       slope=1.0):
    """``mi355_head_aggregate_m2``: ``head_aggregate_`` that also adds the tile's second moment (mean over the mirrors of p^2, times
    gauss) into agg2 [ncls, Zp, Yp, Xp]; agg and cnt receive what the plain call gives them, bit for bit.  "identity" is refused."""
    _head_aggregate(True, feat, weight, bias, mirrors, patch, nonlin, agg, agg2, cnt, origin, gauss, first_sample, scale, shift, slope)


def logits_aggregate_m2_(logits, mirrors, patch, nonlin, agg, agg2, cnt, origin, gauss=None, first_sample=0):
    """``mi355_logits_aggregate_m2``: as ``head_aggregate_m2_`` from logits CUDA fp32 [S, ncls, PV]."""
    _logits_aggregate(True, logits, mirrors, patch, nonlin, agg, agg2, cnt, origin, gauss, first_sample)


def logits_aggregate_tiles_m2_(logits, mirrors, patch, nonlin, agg, agg2, cnt, origins, gauss=None, first_sample=0):
    """``mi355_logits_aggregate_tiles_m2``: the tiles at ``origins`` in one launch with the second moment kept; agg2 is bit-identical to
    ``logits_aggregate_m2_`` tile by tile in that order, and a voxel no tile covers is not written."""
    _logits_aggregate_tiles(True, logits, mirrors, patch, nonlin, agg, agg2, cnt, origins, gauss, first_sample)


def cnt_add_tile_(cnt, patch, origin, gauss=None):
    """``mi355_cnt_add_tile``: cnt [Zp, Yp, Xp] (CUDA fp32, in place) += gauss [patch] (None: 1) at origin."""
    gauss, padded, _ = _tile_operands(cnt[None], cnt, gauss, 1, patch, origin, "cnt_add_tile_")
    _lib.check(_lib.load().mi355_cnt_add_tile(_ptr(gauss), _i3(patch), cnt.data_ptr(), _i3(padded), _i3(origin), stream_of(cnt)),
               "mi355_cnt_add_tile")


def stage0_gather(wv, slabs, samples, patch, r, shells_only=False, out=None):
    """``mi355_stage0_gather``.  wv: CUDA fp32 [mirrors, Ve0, Ve1, Ve2, C]; slabs: per axis a CUDA fp32 [n, S0, S1, S2, C] (S[a] = the
    slab thickness, S[k] = patch[k] otherwise) or None; samples: dicts {wv, origin, slab: six indices or -1}.  Returns
    [len(samples), P0, P1, P2, C].  Slab and whole-volume indices are checked against the tensors here.
    shells_only: ``mi355_stage0_gather_shells`` - only the voxels within r of a face with a slab are written, into ``out`` (CUDA fp32
    of the result's shape, otherwise left as it is) when given."""
    import torch
    wv = _require_cuda(wv, torch.float32, "wv")
    nwv, c = int(wv.shape[0]), int(wv.shape[4])
    patch = [int(p) for p in patch]
    a = _lib.Stage0GatherArgs()
    a.wv_dev = wv.data_ptr()
    keep = [wv]
    for k in range(3):
        a.patch[k], a.volume[k] = patch[k], int(wv.shape[1 + k])
        a.slab_thickness[k] = 2 * int(r)
    for k, sl in enumerate(slabs):
        if sl is None:
            continue
        sl = _require_cuda(sl, torch.float32, f"slabs[{k}]")
        keep.append(sl)
        want = [int(sl.shape[1 + j]) if j == k else patch[j] for j in range(3)]
        if sl.dim() != 5 or list(sl.shape[1:4]) != want or sl.shape[4] != c:
            raise ValueError(f"slabs[{k}]: shape {tuple(sl.shape)}")
        a.slab_dev[k] = sl.data_ptr()
        a.slab_thickness[k] = int(sl.shape[1 + k])
    if len(samples) > 64:
        raise ValueError("stage0_gather: more than 64 samples")
    for i, sm in enumerate(samples):
        if not 0 <= int(sm["wv"]) < nwv:
            raise ValueError(f"stage0_gather: sample {i}: whole-volume index")
        a.samples[i].wv = int(sm["wv"])
        for k in range(3):
            a.samples[i].origin[k] = int(sm["origin"][k])
        for f in range(6):
            idx = int(sm["slab"][f])
            if idx >= 0 and (slabs[f >> 1] is None or idx >= slabs[f >> 1].shape[0]):
                raise ValueError(f"stage0_gather: sample {i}: face {f} has no slab {idx}")
            a.samples[i].slab[f] = idx
    a.r, a.channels, a.n_samples = int(r), c, len(samples)
    shape = (max(len(samples), 1), patch[0], patch[1], patch[2], c)
    if out is None:
        out = torch.full(shape, float("nan"), dtype=torch.float32, device=wv.device)
    elif not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == shape):
        raise ValueError(f"stage0_gather: out must be a contiguous CUDA fp32 {shape}")
    a.out_dev = out.data_ptr()
    if shells_only:
        _lib.check(_lib.load().mi355_stage0_gather_shells(C.byref(a), stream_of(wv)), "mi355_stage0_gather_shells")
    else:
        _lib.check(_lib.load().mi355_stage0_gather(C.byref(a), stream_of(wv)), "mi355_stage0_gather")
    return out


def stage0_gather_merged(wv, slabs, samples, patch, r, spans, shells_only=False, out=None, second=None, tile=None, by_box=False):
    """``mi355_stage0_gather_merged``: ``stage0_gather`` with slabs that may span the volume.  slabs[a]: CUDA fp32 [n, S0, S1, S2, C] or
    None; spans[a][k] truthy: the slabs of axis a span the volume along k (S[k] = volume[k], the tile at its origin) instead of
    holding the tile's extent (S[k] = patch[k]).  second: None or a dict wv, slabs, r and optionally out - a second tensor gathered
    for the same samples.  Returns (out, out2); out / out2 given are written in place (shells_only: the shell voxels alone).
    tile: ``mi355_stage0_gather_boxes`` - the samples are sub-boxes (each dict also has ``sub``, its offset in its tile) of tiles of
    ``tile`` voxels, which is what a slab holds along an axis it does not span; by_box: the dense gather of one tensor is launched
    over the boxes (``stage0_gather_box_kernel``) instead of over the whole volume's rows."""
    import torch
    wv = _require_cuda(wv, torch.float32, "wv")
    nwv = int(wv.shape[0])
    patch = [int(p) for p in patch]
    boxes = _lib.Stage0GatherBoxesArgs() if tile is not None else None
    m = _lib.Stage0GatherMergedArgs() if boxes is None else boxes.merged
    held = patch if tile is None else [int(t) for t in tile]  # what a slab holds along an axis it does not span
    a = m.base
    keep = [wv]
    vol = [int(wv.shape[1 + k]) for k in range(3)]
    counts = [0, 0, 0]

    def bind(t, sl_list, name):
        c = int(t.shape[4])
        if list(t.shape[1:4]) != vol or t.shape[0] != nwv:
            raise ValueError(f"{name}: shape {tuple(t.shape)}")
        ptrs = [None, None, None]
        for k, sl in enumerate(sl_list):
            if sl is None:
                continue
            sl = _require_cuda(sl, torch.float32, f"{name} slabs[{k}]")
            keep.append(sl)
            thick = int(sl.shape[1 + k])
            want = [thick if j == k else (vol[j] if spans[k][j] else held[j]) for j in range(3)]
            if sl.dim() != 5 or list(sl.shape[1:4]) != want or sl.shape[4] != c or (counts[k] and counts[k] != sl.shape[0]):
                raise ValueError(f"{name} slabs[{k}]: shape {tuple(sl.shape)}, expected [n, {want}, {c}]")
            if a.slab_thickness[k] not in (0, thick):
                raise ValueError(f"{name} slabs[{k}]: thickness {thick}")
            a.slab_thickness[k], counts[k] = thick, int(sl.shape[0])
            for j in range(3):
                m.slab_shape[k][j], m.spans_volume[k][j] = want[j], int(bool(spans[k][j]))
            ptrs[k] = sl.data_ptr()
        return c, ptrs

    c, ptrs = bind(wv, slabs, "first")
    a.wv_dev, a.r, a.channels, a.n_samples = wv.data_ptr(), int(r), c, len(samples)
    for k in range(3):
        a.patch[k], a.volume[k] = patch[k], vol[k]
        a.slab_dev[k] = ptrs[k]
    c2 = 0
    if second is not None:
        wv2 = _require_cuda(second["wv"], torch.float32, "second wv")
        keep.append(wv2)
        c2, ptrs2 = bind(wv2, second["slabs"], "second")
        if any((p is None) != (q is None) for p, q in zip(ptrs, ptrs2)):
            raise ValueError("stage0_gather_merged: the two tensors need slabs on the same axes")
        m.wv2_dev, m.r2, m.channels2 = wv2.data_ptr(), int(second["r"]), c2
        for k in range(3):
            m.slab2_dev[k] = ptrs2[k]
    for k in range(3):
        if ptrs[k] is None:   # an axis without slabs: the per-tile form, never indexed
            a.slab_thickness[k] = 2 * int(second["r"] if second is not None else r)
            for j in range(3):
                m.slab_shape[k][j], m.spans_volume[k][j] = (a.slab_thickness[k] if j == k else held[j]), 0
    if len(samples) > 64:
        raise ValueError("stage0_gather_merged: more than 64 samples")
    for i, sm in enumerate(samples):
        if not 0 <= int(sm["wv"]) < nwv:
            raise ValueError(f"stage0_gather_merged: sample {i}: whole-volume index")
        a.samples[i].wv = int(sm["wv"])
        for k in range(3):
            a.samples[i].origin[k] = int(sm["origin"][k])
        for f in range(6):
            idx = int(sm["slab"][f])
            if idx >= counts[f >> 1]:
                raise ValueError(f"stage0_gather_merged: sample {i}: face {f} has no slab {idx}")
            a.samples[i].slab[f] = idx
        if boxes is not None:
            for k in range(3):
                boxes.sub[i][k] = int(sm["sub"][k])

    def result(given, ch):
        shape = (max(len(samples), 1), patch[0], patch[1], patch[2], ch)
        if given is None:
            return torch.full(shape, float("nan"), dtype=torch.float32, device=wv.device)
        if not (given.is_cuda and given.is_contiguous() and given.dtype == torch.float32 and tuple(given.shape) == shape):
            raise ValueError(f"stage0_gather_merged: out must be a contiguous CUDA fp32 {shape}")
        return given

    out = result(out, c)
    a.out_dev = out.data_ptr()
    out2 = None
    if second is not None:
        out2 = result(second.get("out"), c2)
        m.out2_dev = out2.data_ptr()
    if boxes is not None:
        for k in range(3):
            boxes.tile[k] = held[k]
        _lib.check(_lib.load().mi355_stage0_gather_boxes(C.byref(boxes), int(bool(shells_only)), int(bool(by_box)), stream_of(wv)),
                   "mi355_stage0_gather_boxes")
    elif by_box:
        raise ValueError("stage0_gather_merged: by_box needs the sub-box form (tile)")
    else:
        _lib.check(_lib.load().mi355_stage0_gather_merged(C.byref(m), int(bool(shells_only)), stream_of(wv)), "mi355_stage0_gather_merged")
    return out, out2


def stage0_mask_(x, keep):
    """``mi355_stage0_mask``, in place: x CUDA fp32 [N, Ve0, Ve1, Ve2, C], zero outside [0, keep)."""
    import torch
    if not (x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 5):
        raise ValueError("stage0_mask_: x must be a contiguous CUDA fp32 [N, Ve0, Ve1, Ve2, C]")
    _lib.check(_lib.load().mi355_stage0_mask(x.data_ptr(), int(x.shape[0]), _i3(x.shape[1:4]), _i3(keep), int(x.shape[4]), stream_of(x)),
               "mi355_stage0_mask")
    return x


# Device scratch, for tests (include/mi355_nnunet.h; DESIGN.md "Scratch holds no state").
#: the slots of csrc/common.h's enum ScratchSlot, in its order
SCRATCH_SLOTS = ("SCR_ARENA", "SCR_SW_AGG", "SCR_SPLITK_F32", "SCR_SPLITK_F16", "SCR_ZEROS", "SCR_ZERO_BIAS", "SCR_SMALL", "SCR_TOPK",
                 "SCR_CROP", "SCR_ZSCORE", "SCR_RESAMPLE", "SCR_RESAMPLE_MM", "SCR_COMPONENTS", "SCR_MORPHOLOGY", "SCR_QUALITY",
                 "SCR_MASS_EFFECT")
#: the slots every lane shares (the zero pages): never filled, never released
SCRATCH_SHARED = ("SCR_ZEROS", "SCR_ZERO_BIAS")
#: MI355_SCRATCH_LANES: streams that hold scratch of their own at one time
SCRATCH_LANES = 4


def _scratch_stream(stream):
    """A raw stream handle, a torch stream, or None for torch's current stream."""
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return int(getattr(stream, "cuda_stream", stream))


def scratch_slot_count() -> int:
    """The library's number of scratch slots (host code: needs no GPU)."""
    return int(_lib.load().mi355_scratch_sizes(None, None, 0))


def scratch_sizes(stream=None) -> dict:
    """{slot name: bytes allocated} for the lane of ``stream``; claims no lane and allocates nothing."""
    n = len(SCRATCH_SLOTS)
    buf = (C.c_int64 * n)()
    rc = _lib.load().mi355_scratch_sizes(_scratch_stream(stream), buf, n)
    _lib.check(rc, "mi355_scratch_sizes")
    if rc != n:
        raise _lib.Mi355Error(f"the library has {rc} scratch slots, ops.SCRATCH_SLOTS names {n}")
    return {name: int(buf[i]) for i, name in enumerate(SCRATCH_SLOTS)}


def scratch_fill(slot, word: int, stream=None) -> int:
    """Fill the whole buffer of ``slot`` (a name of SCRATCH_SLOTS; None: every lane-owned slot) of the lane of ``stream`` with
    the 32-bit ``word``, on that stream.  Returns the bytes filled."""
    idx = -1 if slot is None else SCRATCH_SLOTS.index(slot)
    rc = int(_lib.load().mi355_scratch_fill(_scratch_stream(stream), idx, int(word) & 0xFFFFFFFF))
    _lib.check(rc, "mi355_scratch_fill")
    return rc


def scratch_release(stream=None) -> None:
    """Free the lane-owned scratch of the lane of ``stream`` and forget the lane."""
    _lib.check(_lib.load().mi355_scratch_release(_scratch_stream(stream)), "mi355_scratch_release")


def scratch_zero_pages() -> tuple:
    """Non-zero bytes in (SCR_ZEROS, SCR_ZERO_BIAS); 0 for a page that does not exist yet."""
    out = (C.c_int64 * 2)()
    _lib.check(_lib.load().mi355_scratch_zero_pages(out), "mi355_scratch_zero_pages")
    return int(out[0]), int(out[1])


def live_allocations() -> tuple:
    """(count, bytes) of the device memory the library's owners hold now: weights and Gaussian maps of live handles, the buffers
    of a single-op call while it runs; scratch is not counted (host code: needs no GPU)."""
    count, nbytes = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().mi355_live_allocations(C.byref(count), C.byref(nbytes)), "mi355_live_allocations")
    return int(count.value), int(nbytes.value)
