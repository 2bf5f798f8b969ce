"""Seeded synthetic checkpoints and BraTS-shaped volumes.

Neither the KAIST checkpoints nor BraTS data exist in the build or GPU containers
(reference .gitignore:12,20,28-29), so tests, smoke and bench all use these generators
(SURVEY.md 8d).  ``np.random.RandomState`` streams are frozen across numpy versions, so the same
seed gives the same weights here, on the GPU box and in the committed golden fixtures.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np


def unet_widths(in_ch, base, num_classes, num_pool, max_feat=320, encoder_scale=1, convs_per_stage=2):
    """Channel plan of Generic_UNet.__init__ (reference generic_UNet.py:280-375) for
    convolutional_pooling=True, convolutional_upsampling=True.  Returns
    (enc[(cin,cout)...] per stage incl. bottleneck, tu[(cin,cout)], dec[[(cin,cout)...]], head_cin)."""
    enc = []
    out_f = base * encoder_scale
    in_f = in_ch
    for _ in range(num_pool):
        enc.append([(in_f, out_f)] + [(out_f, out_f)] * (convs_per_stage - 1))
        in_f = out_f
        out_f = min(int(np.round(out_f * 2)), max_feat)
    final = out_f
    enc.append([(in_f, out_f)] + [(out_f, out_f)] * (convs_per_stage - 2) + [(out_f, final)])
    tu, dec = [], []
    head_cin = None
    for u in range(num_pool):
        from_down = final if u == 0 else int(final / encoder_scale)
        from_skip = enc[-(2 + u)][-1][1]
        final = from_skip
        tu.append((from_down, from_skip))
        last = int(final / encoder_scale)
        dec.append([(2 * from_skip, from_skip)] + [(from_skip, from_skip)] * (convs_per_stage - 2) + [(from_skip, last)])
        head_cin = last
    return enc, tu, dec, head_cin


def make_state_dict(norm: str = "batch", seed: int = 7, in_ch: int = 4, base: int = 32, num_classes: int = 3,
                    num_pool: int = 5, max_feat: int = 320, encoder_scale: int = 1, head_scale: float = 12.0,
                    all_heads: bool = False) -> "OrderedDict[str, np.ndarray]":
    """He-normal (a=0.01) conv weights, zero conv bias, gamma~U(.5,1.5), beta~N(0,.1); BatchNorm
    running mean~N(0,.1), var~U(.5,1.5).  The segmentation head is scaled by ``head_scale`` so the
    logits are confidently bimodal like a trained model's (threshold sensitivity)."""
    rs = np.random.RandomState(seed)
    enc, tu, dec, head_cin = unet_widths(in_ch, base, num_classes, num_pool, max_feat, encoder_scale)
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    a = 0.01

    def conv_block(prefix, cin, cout):
        std = np.sqrt(2.0 / ((1 + a * a) * cin * 27))
        sd[prefix + ".conv.weight"] = (rs.standard_normal((cout, cin, 3, 3, 3)) * std).astype(np.float32)
        sd[prefix + ".conv.bias"] = (rs.standard_normal(cout) * 0.05).astype(np.float32)
        if norm != "none":
            sd[prefix + ".instnorm.weight"] = rs.uniform(0.5, 1.5, cout).astype(np.float32)
            sd[prefix + ".instnorm.bias"] = (rs.standard_normal(cout) * 0.1).astype(np.float32)
        if norm == "batch":
            sd[prefix + ".instnorm.running_mean"] = (rs.standard_normal(cout) * 0.1).astype(np.float32)
            sd[prefix + ".instnorm.running_var"] = rs.uniform(0.5, 1.5, cout).astype(np.float32)
            sd[prefix + ".instnorm.num_batches_tracked"] = np.asarray(1000, dtype=np.int64)

    for d in range(num_pool):
        for i, (ci, co) in enumerate(enc[d]):
            conv_block(f"conv_blocks_context.{d}.blocks.{i}", ci, co)
    # bottleneck = Sequential(StackedConvLayers(n-1 convs), StackedConvLayers(1 conv))  (:329-335)
    bott = enc[num_pool]
    for i, (ci, co) in enumerate(bott[:-1]):
        conv_block(f"conv_blocks_context.{num_pool}.0.blocks.{i}", ci, co)
    conv_block(f"conv_blocks_context.{num_pool}.1.blocks.0", *bott[-1])
    for u in range(num_pool):
        ci, co = tu[u]
        std = np.sqrt(2.0 / ((1 + a * a) * co * 8))  # torch fan_in of a ConvTranspose weight [cin,cout,k]
        sd[f"tu.{u}.weight"] = (rs.standard_normal((ci, co, 2, 2, 2)) * std).astype(np.float32)
        blocks = dec[u]
        for i, (bi, bo) in enumerate(blocks[:-1]):
            conv_block(f"conv_blocks_localization.{u}.0.blocks.{i}", bi, bo)
        conv_block(f"conv_blocks_localization.{u}.1.blocks.0", *blocks[-1])
        if all_heads or u == num_pool - 1:
            hc = blocks[-1][1]
            std = np.sqrt(2.0 / ((1 + a * a) * hc))
            sd[f"seg_outputs.{u}.weight"] = (rs.standard_normal((num_classes, hc, 1, 1, 1)) * std * head_scale).astype(np.float32)
    return sd


#: the named synthetic models of SURVEY 8d ("model A" = base BN net, "model B" = large GroupNorm-16 net)
MODEL_PRESETS = {
    "A": dict(norm="batch", base=32, max_feat=320, encoder_scale=1),
    "A_in": dict(norm="instance", base=32, max_feat=320, encoder_scale=1),
    "B": dict(norm="group", base=32, max_feat=512, encoder_scale=2),
}


def make_model(name: str, seed: int = 7, **overrides) -> Tuple["OrderedDict[str, np.ndarray]", Dict]:
    cfg = dict(MODEL_PRESETS[name])
    cfg.update(overrides)
    sd = make_state_dict(seed=seed, **cfg)
    meta = dict(norm=cfg["norm"], num_groups=16)
    return sd, meta


def make_volume(seed: int = 1000, shape=(155, 240, 240), dense: bool = False, channels: int = 4,
                semi_axes: Optional[Tuple[float, float, float]] = None) -> np.ndarray:
    """Synthetic ``[4, Z, Y, X]`` float32 'MRI': smooth field x ellipsoidal brain mask (exact zeros
    outside, a few interior zero holes), MR-like intensities 0..~4000.  The default
    mask gives a nonzero crop of about (140,172,138) -> 8 tiles of 128^3; ``dense`` -> 18 tiles."""
    from scipy.ndimage import gaussian_filter

    rs = np.random.RandomState(seed)
    Z, Y, X = shape
    vol = np.empty((channels, Z, Y, X), dtype=np.float32)
    for c in range(channels):
        noise = rs.standard_normal((Z, Y, X)).astype(np.float32)
        smooth = gaussian_filter(noise, sigma=6.0, mode="nearest")
        smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min() + 1e-12)
        vol[c] = (200.0 + 400.0 * c) + smooth * (1500.0 + 500.0 * c)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    cz, cy, cx = (Z - 1) / 2.0, (Y - 1) / 2.0, (X - 1) / 2.0
    # bright "tumour" blobs
    for _ in range(rs.randint(1, 4)):
        bz, by, bx = cz + rs.uniform(-25, 25), cy + rs.uniform(-35, 35), cx + rs.uniform(-30, 30)
        r = rs.uniform(8, 18)
        blob = np.exp(-(((zz - bz) ** 2 + (yy - by) ** 2 + (xx - bx) ** 2) / (2 * r * r))).astype(np.float32)
        vol += blob[None] * rs.uniform(500, 1500, size=(channels, 1, 1, 1)).astype(np.float32)
    if not dense:
        if semi_axes is None:
            semi_axes = (70.0 * Z / 155.0, 86.0 * Y / 240.0, 69.0 * X / 240.0)
        mask = (((zz - cz) / semi_axes[0]) ** 2 + ((yy - cy) / semi_axes[1]) ** 2 + ((xx - cx) / semi_axes[2]) ** 2) <= 1.0
        vol *= mask[None]
        # interior zero holes (exercise binary_fill_holes in the preprocessing)
        for _ in range(3):
            hz, hy, hx = int(cz + rs.uniform(-15, 15)), int(cy + rs.uniform(-20, 20)), int(cx + rs.uniform(-20, 20))
            vol[:, max(hz - 2, 0):hz + 2, max(hy - 2, 0):hy + 2, max(hx - 2, 0):hx + 2] = 0.0
    return vol


def label_map(seed: int, shape, lesions, fragments: int = 0, enhancing: bool = True, speckle: float = 0.6) -> np.ndarray:
    """Synthetic uint8 label map ``[d0, d1, d2]`` for the connected-component path: per lesion ``(centre, radius)`` a ball
    of label 1 (shell), label 2 inside 0.7 radius (core) and, if ``enhancing``, label 3 on a ``speckle`` share of the voxels
    inside 0.5 radius; then ``fragments`` isolated voxels of a random label 1..3 anywhere in the volume."""
    rs = np.random.RandomState(seed)
    seg = np.zeros(tuple(shape), dtype=np.uint8)
    for centre, radius in lesions:
        lo = [max(int(np.floor(c - radius)), 0) for c in centre]
        hi = [min(int(np.ceil(c + radius)) + 1, s) for c, s in zip(centre, shape)]
        g = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        d2 = sum((g[k] - float(centre[k])) ** 2 for k in range(3))
        box = seg[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        box[d2 <= radius * radius] = 1
        box[d2 <= (0.7 * radius) ** 2] = 2
        if enhancing:
            box[(d2 <= (0.5 * radius) ** 2) & (rs.random_sample(d2.shape) < speckle)] = 3
    if fragments:
        idx = rs.choice(seg.size, fragments, replace=False)
        seg.reshape(-1)[idx] = rs.randint(1, 4, fragments).astype(np.uint8)
    return seg


def shapes_map(seed: int, shape, parts) -> np.ndarray:
    """Synthetic uint8 label map ``[d0, d1, d2]`` painted part by part, later parts over earlier ones (the morphology path:
    shapes whose sphericity, elongation and contour class are known in advance).  A part is ``["ball", label, centre, radius]``,
    ``["box", label, lo, hi]`` (hi exclusive) or ``["noise", label, lo, hi, p]`` (each voxel of the box with probability p);
    everything is clipped to the volume."""
    rs = np.random.RandomState(seed)
    seg = np.zeros(tuple(shape), dtype=np.uint8)
    for part in parts:
        kind, label = part[0], int(part[1])
        if kind == "ball":
            centre, radius = part[2], float(part[3])
            lo = [max(int(np.floor(c - radius)), 0) for c in centre]
            hi = [min(int(np.ceil(c + radius)) + 1, s) for c, s in zip(centre, shape)]
            g = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
            d2 = sum((g[k] - float(centre[k])) ** 2 for k in range(3))
            seg[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][d2 <= radius * radius] = label
        elif kind in ("box", "noise"):
            lo = [max(int(v), 0) for v in part[2]]
            hi = [min(int(v), s) for v, s in zip(part[3], shape)]
            box = seg[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
            if kind == "box":
                box[...] = label
            else:
                box[rs.random_sample(box.shape) < float(part[4])] = label
        else:
            raise ValueError(f"shapes_map: unknown part {kind!r}")
    return seg


def mri_for_label_map(seed: int, seg: np.ndarray, gain: float = 0.0, cystic: float = 0.0, sigma: float = 3.0, brain: bool = True) -> np.ndarray:
    """Four float32 volumes ``[4, d0, d1, d2]`` (T1, T1ce, T2, FLAIR) on the grid of ``seg`` with integer values below 2^24,
    as BraTS files hold: a smooth field per channel, zero outside an ellipsoidal 'brain' (``brain``), multiplied by
    ``1 + gain`` inside the tumour (``seg > 0``), and with a CSF-like signal (T1 and FLAIR dark, T2 bright) on a ``cystic``
    share of the voxels of label 1."""
    from scipy.ndimage import gaussian_filter

    rs = np.random.RandomState(seed)
    shape = seg.shape
    vols = np.empty((4,) + shape, dtype=np.float32)
    for c in range(4):
        smooth = gaussian_filter(rs.standard_normal(shape).astype(np.float32), sigma=sigma, mode="nearest")
        smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min() + 1e-12)
        vols[c] = (400.0 + 200.0 * c) + smooth * (1200.0 + 300.0 * c)
    if brain:
        g = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
        inside = sum(((g[k] - (shape[k] - 1) / 2.0) / (0.47 * shape[k])) ** 2 for k in range(3)) <= 1.0
        vols *= inside[None]
    vols[:, seg > 0] *= np.float32(1.0 + gain)
    ncr = seg == 1
    pick = ncr & (rs.random_sample(shape) < cystic)
    vols[0][pick], vols[2][pick], vols[3][pick] = 50.0, 6000.0, 60.0
    return np.rint(vols).astype(np.float32)


def mri_with_region_gains(seed: int, seg: np.ndarray, gains, et_noise: float = 0.0, zero_channel: Optional[int] = None, sigma: float = 3.0,
                          brain: bool = True) -> np.ndarray:
    """Four float32 volumes ``[4, d0, d1, d2]`` (T1, T1ce, T2, FLAIR) on the grid of ``seg`` with integer values below 2^24 (the
    sequence-findings path: region means in a known ratio to the normal brain's).  Every channel is the same kind of smooth
    field, 1000..1150, zero outside an ellipsoidal 'brain' (``brain``); ``gains`` holds rows ``[label, g_t1, g_t1ce, g_t2,
    g_flair]`` and the voxels of ``label`` are multiplied by the row's gain of each channel; T1ce inside the enhancing labels
    (3 and 4) is further multiplied by ``1 + et_noise * U(-1, 1)`` per voxel; ``zero_channel`` names a channel left all zero."""
    from scipy.ndimage import gaussian_filter

    rs = np.random.RandomState(seed)
    shape = seg.shape
    vols = np.empty((4,) + shape, dtype=np.float64)
    for c in range(4):
        smooth = gaussian_filter(rs.standard_normal(shape).astype(np.float32), sigma=sigma, mode="nearest")
        smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min() + 1e-12)
        vols[c] = 1000.0 + 150.0 * smooth
    if brain:
        g = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
        inside = sum(((g[k] - (shape[k] - 1) / 2.0) / (0.47 * shape[k])) ** 2 for k in range(3)) <= 1.0
        vols *= inside[None]
    for row in gains:
        where = seg == int(row[0])
        for c in range(4):
            vols[c][where] *= float(row[1 + c])
    et = (seg == 3) | (seg == 4)
    vols[1][et] *= 1.0 + float(et_noise) * rs.uniform(-1.0, 1.0, int(et.sum()))
    if zero_channel is not None:
        vols[int(zero_channel)] = 0.0
    return np.rint(vols).astype(np.float32)


def mri_for_quality(seed: int, seg: np.ndarray, levels=None, brain_axes: Optional[float] = 0.47, radial_gain: float = 0.0, plateau=(), ghost=(),
                    dropout=(), spikes=(), edge_noise=None, zero_channel: Optional[int] = None, sigma: float = 3.0) -> np.ndarray:
    """Four float32 volumes ``[4, d0, d1, d2]`` (T1, T1ce, T2, FLAIR) on the grid of ``seg`` with integer values below 2^15 (the
    quality-control path: every artefact the reference's step 5 looks for can be switched on by itself).  Channel ``c`` is a
    smooth field ``levels[c] = [base, amplitude]`` (default 1000, 150), zero outside a centred ellipsoidal 'brain' whose
    semi-axes are ``brain_axes`` times the shape (None: no skull strip), then in this order:
    ``radial_gain``  every channel times ``1 + radial_gain * r``, r = 0 at the centre and 1 on the ellipsoid (a bias field);
    ``plateau``      rows ``[channel, fraction]``: the lowest ``fraction`` of the channel's positive voxels take its smallest
                     positive value (a tie at the minimum: the 5th / 10th percentile then IS the minimum);
    ``dropout``      rows ``[channel, lo, hi]``: the box set to zero (missing data);
    ``spikes``       rows ``[channel, p_high, high, p_low, low]``: a share of the voxels inside the ellipsoid set to ``high`` / ``low``;
    ``edge_noise``   ``[p, value]``: T1 plus ``value`` on a share ``p`` of the voxels within two steps of the tumour surface;
    ``ghost``        rows ``[channel, level, kind]``: noise on the zero voxels outside the ellipsoid, ``"exp"`` = 1 + an exponential
                     of mean ``level`` (coefficient of variation near 1), ``"flat"`` = ``level`` .. ``1.1 level`` uniform;
    ``zero_channel`` names a channel left all zero."""
    from scipy.ndimage import binary_dilation, binary_erosion, gaussian_filter

    rs = np.random.RandomState(seed)
    shape = seg.shape
    levels = [[1000.0, 150.0]] * 4 if levels is None else levels
    vols = np.empty((4,) + shape, dtype=np.float64)
    for c in range(4):
        smooth = gaussian_filter(rs.standard_normal(shape).astype(np.float32), sigma=sigma, mode="nearest")
        smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min() + 1e-12)
        vols[c] = float(levels[c][0]) + float(levels[c][1]) * smooth
    g = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    if brain_axes is None:
        r = np.sqrt(sum(((g[k] - (shape[k] - 1) / 2.0) / (0.5 * shape[k])) ** 2 for k in range(3)))
        inside = np.ones(shape, dtype=bool)
    else:
        r = np.sqrt(sum(((g[k] - (shape[k] - 1) / 2.0) / (float(brain_axes) * shape[k])) ** 2 for k in range(3)))
        inside = r <= 1.0
        vols *= inside[None]
    vols *= (1.0 + float(radial_gain) * r)[None]
    vols = np.rint(vols)
    for c, fraction in plateau:
        v = vols[int(c)]
        pos = v[v > 0]
        v[(v > 0) & (v <= np.percentile(pos, 100.0 * float(fraction)))] = pos.min()
    for c, lo, hi in dropout:
        vols[int(c)][tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))] = 0.0
    for c, p_high, high, p_low, low in spikes:
        u = rs.random_sample(shape)
        vols[int(c)][inside & (u < float(p_high))] = float(high)
        vols[int(c)][inside & (u > 1.0 - float(p_low))] = float(low)
    if edge_noise is not None and seg.any():
        wt = seg > 0
        near = binary_dilation(wt, iterations=2) & ~binary_erosion(wt, iterations=3)
        vols[0][near & (rs.random_sample(shape) < float(edge_noise[0]))] += float(edge_noise[1])
    for c, level, kind in ghost:
        outside = ~inside & (vols[int(c)] == 0)
        n = int(outside.sum())
        noise = 1.0 + rs.exponential(float(level), n) if kind == "exp" else float(level) * (1.0 + 0.1 * rs.random_sample(n))
        vols[int(c)][outside] = np.minimum(np.rint(noise), 30000.0)
    if zero_channel is not None:
        vols[int(zero_channel)] = 0.0
    assert vols.max() < 2 ** 15 and vols.min() >= 0
    return vols.astype(np.float32)


def mri_for_mass_effect(seed: int, seg: np.ndarray, brain_axes: float = 0.47, cuts=(), dark=(), noise: float = 0.0, peri_scale: float = 1.0,
                        zero: bool = False, sigma: float = 3.0) -> np.ndarray:
    """One float32 T1 volume ``[d0, d1, d2]`` on the grid of ``seg`` with integer values below 2^15 (the mass-effect path: the
    hemispheric asymmetry of the brain mask, the sides of the CSF-like voxels and the intensity spread around the tumour can be
    steered one by one).  A smooth field 1000..1150 plus white noise of standard deviation ``noise``, zero outside a centred
    ellipsoidal 'brain' whose semi-axes are ``brain_axes`` times the shape, then in this order:
    ``peri_scale``  within ten dilations of the tumour (the tumour excluded) the deviation from 1075 is multiplied by it (below
                    1: the sulci around the tumour are effaced);
    ``dark``        rows ``[lo, hi, factor]``: the box multiplied by ``factor`` (CSF-like signal: with enough of it the 5th and
                    15th percentile fall inside these boxes, and their sizes decide the left / right CSF volumes);
    ``cuts``        rows ``[lo, hi]``: the box set to zero (tissue missing on one side: the two halves of the brain mask lose
                    their symmetry about the middle of its extent);
    ``zero``        all zero (no brain)."""
    from scipy.ndimage import binary_dilation, gaussian_filter

    rs = np.random.RandomState(seed)
    shape = seg.shape
    smooth = gaussian_filter(rs.standard_normal(shape).astype(np.float32), sigma=sigma, mode="nearest")
    smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min() + 1e-12)
    t1 = 1000.0 + 150.0 * smooth.astype(np.float64) + float(noise) * rs.standard_normal(shape)
    g = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    inside = sum(((g[k] - (shape[k] - 1) / 2.0) / (float(brain_axes) * shape[k])) ** 2 for k in range(3)) <= 1.0
    if peri_scale != 1.0 and seg.any():
        wt = seg > 0
        zone = binary_dilation(wt, iterations=10) & ~wt
        t1[zone] = 1075.0 + float(peri_scale) * (t1[zone] - 1075.0)
    t1 = np.maximum(t1, 1.0) * inside
    for lo, hi, factor in dark:
        t1[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))] *= float(factor)
    for lo, hi in cuts:
        t1[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))] = 0.0
    if zero:
        t1[...] = 0.0
    t1 = np.rint(t1)
    assert t1.max() < 2 ** 15 and t1.min() >= 0
    return t1.astype(np.float32)


def painted_mask(shape, parts) -> np.ndarray:
    """Boolean mask ``[d0, d1, d2]``, the union of ``["box", lo, hi]`` (hi exclusive) and ``["obox", lo, hi]`` parts, clipped to the
    volume.  An ``obox`` is the box without its twelve edges: what an erosion and a dilation with the 6-neighbour cross leave of a
    box, so a union of them passes such an opening unchanged, and two of them can touch across an edge or a corner only."""
    mask = np.zeros(tuple(shape), dtype=bool)
    for kind, lo, hi in parts:
        lo = [max(int(v), 0) for v in lo]
        hi = [min(int(v), s) for v, s in zip(hi, shape)]
        box = np.ones([max(b - a, 0) for a, b in zip(lo, hi)], dtype=bool)
        if kind == "obox":
            ends = [np.isin(np.arange(n), (0, n - 1)).astype(int) for n in box.shape]  # 1 on the two end planes of an axis
            box &= (ends[0][:, None, None] + ends[1][None, :, None] + ends[2][None, None, :]) < 2
        elif kind != "box":
            raise ValueError(f"painted_mask: unknown part {kind!r}")
        mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= box
    return mask


def mri_for_normal_structures(seed: int, seg: np.ndarray, ventricles=(), brain_axes: float = 0.47, outside: float = 60.0, contrast: float = 0.0,
                              pv_gain: float = 0.0, voids: Optional[str] = None, enhancement: float = 1.0, cuts=(), zero: bool = False,
                              sigma: float = 3.0) -> np.ndarray:
    """Four float32 volumes ``[4, d0, d1, d2]`` (T1, T1ce, T2, FLAIR) on the grid of ``seg`` with integer values below 2^15 (the
    normal-structures path: the size, side and neighbourhood of the ventricles, the deep / cortical T1 contrast, the
    periventricular FLAIR signal, the flow voids and the enhancement around the tumour can be steered one by one).  T1 is a smooth
    field 1000..1150 and T2 is 1.5 times the same field, so no voxel of the background is dark on T1 and bright on T2 at once;
    T1ce and FLAIR are fields of their own.  Inside a centred ellipsoidal 'brain' whose semi-axes are ``brain_axes`` times the
    shape, in this order:
    ``contrast``     T1 and T2 times ``1 + contrast * (1 - r)``, r = 0 at the centre and 1 on the ellipsoid (bright deep tissue);
    ``ventricles``   parts of ``painted_mask``: CSF-like signal there (T1 300, T2 3000, FLAIR 200);
    ``pv_gain``      FLAIR times ``1 + pv_gain`` within ten dilations of the painted ventricles, themselves excluded;
    ``voids``        the darkest T1 voxels of the brain's inferior third ``[:, :, :d2 // 3]`` outside the ventricles: ``"tie"`` = the
                     lowest 6 % all take one value (nothing lies below their 5th percentile), ``"step"`` = the lowest 3 % take
                     150 and the next 4 % one value (3 % lie below), ``"ramp"`` = the lowest 5.5 % take distinct values;
    ``enhancement``  T1ce times it within ten dilations of the tumour, the tumour excluded.
    Outside the ellipsoid every channel is ``outside`` (more than 5 % of the positive voxels, all tied: the brain mask ``t1 > P5``
    is the ellipsoid); ``cuts`` are rows ``[lo, hi]`` of boxes set to ``outside`` too (no brain there); ``zero`` = all zero."""
    from scipy.ndimage import binary_dilation, gaussian_filter

    rs = np.random.RandomState(seed)
    shape = seg.shape
    fields = []
    for _ in range(3):
        smooth = gaussian_filter(rs.standard_normal(shape).astype(np.float32), sigma=sigma, mode="nearest").astype(np.float64)
        fields.append(1000.0 + 150.0 * (smooth - smooth.min()) / (smooth.max() - smooth.min() + 1e-12))
    g = np.ogrid[0:shape[0], 0:shape[1], 0:shape[2]]
    r = np.sqrt(sum(((g[k] - (shape[k] - 1) / 2.0) / (float(brain_axes) * shape[k])) ** 2 for k in range(3)))
    inside = r <= 1.0
    base = fields[0] * (1.0 + float(contrast) * (1.0 - np.minimum(r, 1.0)))
    t1, t1ce, t2, flair = np.rint(base), np.rint(fields[1]), np.rint(1.5 * base), np.rint(fields[2])
    vent = painted_mask(shape, ventricles) & inside
    t1[vent], t2[vent], flair[vent] = 300.0, 3000.0, 200.0
    if pv_gain and vent.any():
        zone = binary_dilation(vent, iterations=10) & ~vent
        flair[zone] = np.rint(flair[zone] * (1.0 + float(pv_gain)))
    if voids is not None:
        region = inside & ~vent
        region[:, :, shape[2] // 3:] = False
        idx = np.flatnonzero(region.ravel())
        idx = idx[np.argsort(t1.ravel()[idx], kind="stable")]
        flat = t1.reshape(-1)
        if voids == "tie":
            flat[idx[:int(0.06 * idx.size)]] = 850.0
        elif voids == "step":
            flat[idx[:int(0.07 * idx.size)]] = 850.0
            flat[idx[:int(0.03 * idx.size)]] = 150.0
        elif voids == "ramp":
            k = int(0.055 * idx.size)
            assert k <= 650  # (below the darkest background value)
            flat[idx[:k]] = 200.0 + np.arange(k)
        else:
            raise ValueError(f"mri_for_normal_structures: unknown voids {voids!r}")
    if enhancement != 1.0 and seg.any():
        wt = seg > 0
        zone = binary_dilation(wt, iterations=10) & ~wt
        t1ce[zone] = np.rint(t1ce[zone] * float(enhancement))
    vols = np.stack([t1, t1ce, t2, flair])
    vols[:, ~inside] = float(outside)
    for lo, hi in cuts:
        vols[(slice(None),) + tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))] = float(outside)
    if zero:
        vols[...] = 0.0
    assert vols.max() < 2 ** 15 and vols.min() >= 0
    return vols.astype(np.float32)
