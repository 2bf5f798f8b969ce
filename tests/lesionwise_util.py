"""CPU oracle of lesion-wise scoring (csrc/lesionwise.hip, brats_amd.evaluate.lesionwise_*), shared by test_lesionwise_cpu.py and
test_gpu_lesionwise.py: the definition restated with scipy.ndimage on whole masks - label, binary_dilation with the 18-neighbourhood,
one ``np.isin`` per lesion - independent of the tables the product derives the same numbers from, and the scene builders.  The BraTS
challenges' own scoring program is not part of the reference tree: what is pinned here is this text, not parity with that program."""
import numpy as np
from scipy import ndimage

import surface_distance_util as su

REGIONS = su.REGIONS
S26 = ndimage.generate_binary_structure(3, 3)
S18 = ndimage.generate_binary_structure(3, 2)
RTOL = su.RTOL      # the fp64 distance map's bound (surface_distance_util.py); every integer is exact
INTEGER_KEYS = ("num_lesions", "num_counted", "num_tp", "num_fn", "num_fp")
ROW_INTEGERS = ("gt_voxels", "gt_components", "pred_voxels", "intersection")


def structure(neighbours):
    return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[neighbours])


def morph(mask, dilate, neighbours, iterations):
    f = ndimage.binary_dilation if dilate else ndimage.binary_erosion
    return f(np.asarray(mask) != 0, structure=structure(neighbours), iterations=iterations, border_value=0).astype(np.uint8)


def pair_table(a, n_a, b, n_b):
    t = np.zeros((n_a + 1, n_b + 1), dtype=np.int64)
    np.add.at(t, (np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)), 1)
    return t


def lesion_distances(p_l, lesion, spacing):
    """(D(P_L -> L), D(L -> P_L)) between the surfaces of the two masks, each taken alone on the whole volume"""
    sa, sb = su.surface(p_l), su.surface(lesion)
    return su.directed(sa, sb, spacing), su.directed(sb, sa, spacing)


def region_lesionwise(P, G, spacing, dilation=3, min_volume_mm3=50.0, penalty_mm=374.0, with_parts=False):
    """the issue's steps 1-8 for one pair of binary masks"""
    P, G = np.asarray(P).astype(bool), np.asarray(G).astype(bool)
    pcc, n_pred = ndimage.label(P, S26)
    gcc, n_gt = ndimage.label(G, S26)
    GD = ndimage.binary_dilation(G, S18, iterations=dilation, border_value=0)
    gdcc, n_les = ndimage.label(GD, S26)
    voxel = float(np.prod(np.asarray(spacing, dtype=np.float64)))
    rows, used = [], set()
    for L in range(1, n_les + 1):
        lesion = G & (gdcc == L)
        comps = sorted(int(c) for c in np.unique(pcc[gdcc == L]) if c != 0)
        used.update(comps)
        gt_voxels = int(lesion.sum())
        row = {"lesion": L, "gt_voxels": gt_voxels, "gt_components": len([c for c in np.unique(gcc[lesion]) if c != 0]), "pred_components": comps,
               "counted": bool(gt_voxels * voxel > min_volume_mm3)}
        if comps:
            p_l = np.isin(pcc, comps)
            inter = int((p_l & lesion).sum())
            d_ab, d_ba = lesion_distances(p_l, lesion, spacing)
            row.update(pred_voxels=int(p_l.sum()), intersection=inter, dice=2 * inter / (int(p_l.sum()) + gt_voxels),
                       hd95=float(np.percentile(np.hstack((d_ab, d_ba)), 95)))
        else:
            row.update(pred_voxels=0, intersection=0, dice=0.0, hd95=float(penalty_mm))
        rows.append(row)
    fp = [{"id": c, "voxels": int((pcc == c).sum())} for c in range(1, n_pred + 1) if c not in used]
    counted = [r for r in rows if r["counted"]]
    n = len(counted) + len(fp)
    out = {"lesionwise_dice": sum(r["dice"] for r in counted) / n if n else 1.0,
           "lesionwise_hd95": (sum(r["hd95"] for r in counted) + penalty_mm * len(fp)) / n if n else 0.0,
           "num_lesions": len(rows), "num_counted": len(counted), "num_tp": len([r for r in counted if r["pred_components"]]),
           "num_fn": len([r for r in counted if not r["pred_components"]]), "num_fp": len(fp), "fp_components": fp, "lesions": rows,
           "dilation": int(dilation), "min_volume_mm3": float(min_volume_mm3), "penalty_mm": float(penalty_mm)}
    if with_parts:
        return out, {"pcc": pcc.astype(np.int32), "n_pred": n_pred, "gcc": gcc.astype(np.int32), "n_gt": n_gt, "gdcc": gdcc.astype(np.int32), "n_les": n_les}
    return out


def case_lesionwise(pred, gt, spacing, regions=REGIONS, **kw):
    return {name: region_lesionwise(su.region_mask(pred, labels), su.region_mask(gt, labels), spacing, **kw) for name, labels in regions.items()}


def tables_of(P, G, dilation=3):
    """the three joint histograms brats_amd.evaluate.lesionwise_from_tables takes, from scipy's labellings"""
    _, p = region_lesionwise(P, G, (1, 1, 1), dilation=dilation, with_parts=True)
    gg = pair_table(p["gcc"], p["n_gt"], p["gdcc"], p["n_les"])
    pd = pair_table(p["pcc"], p["n_pred"], p["gdcc"], p["n_les"])
    lesion_map = np.where(p["gcc"] > 0, p["gdcc"], 0)
    pl = pair_table(p["pcc"], p["n_pred"], lesion_map, p["n_les"])
    return gg, pd, pl, p


def distance_callback(P, G, spacing, parts):
    def distances(L, comps):
        return lesion_distances(np.isin(parts["pcc"], comps), (np.asarray(G) != 0) & (parts["gdcc"] == L), spacing)
    return distances


def same(got, want, what=""):
    """every integer and list exact, dice the host expression on the row's integers, hd95 and both aggregates within RTOL; returns the
    largest relative difference seen"""
    worst = 0.0
    for k in INTEGER_KEYS + ("dilation",):
        assert got[k] == want[k] and isinstance(got[k], int), (what, k, got[k], want[k])
    for k in ("min_volume_mm3", "penalty_mm"):
        assert got[k] == want[k], (what, k)
    assert got["fp_components"] == want["fp_components"], (what, got["fp_components"], want["fp_components"])
    assert len(got["lesions"]) == len(want["lesions"]), what
    for g, w in zip(got["lesions"], want["lesions"]):
        for k in ROW_INTEGERS + ("lesion",):
            assert g[k] == w[k] and isinstance(g[k], int), (what, w["lesion"], k, g[k], w[k])
        assert g["pred_components"] == w["pred_components"] and g["counted"] is w["counted"], (what, w["lesion"])
        assert g["dice"] == (2 * g["intersection"] / (g["pred_voxels"] + g["gt_voxels"]) if g["pred_components"] else 0.0), (what, w["lesion"])
        assert g["dice"] == w["dice"], (what, w["lesion"])
        d, ok = su.close(g["hd95"], w["hd95"], RTOL)
        assert ok, (what, w["lesion"], g["hd95"], w["hd95"], d)
        worst = max(worst, d)
    for k in ("lesionwise_dice", "lesionwise_hd95"):
        d, ok = su.close(got[k], want[k], RTOL)
        assert ok, (what, k, got[k], want[k], d)
        worst = max(worst, d)
    return worst


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def ball(shape, centre, radius):
    g = np.ogrid[tuple(slice(0, s) for s in shape)]
    return sum((g[k] - centre[k]) ** 2 for k in range(3)) <= radius * radius


SCENE_SHAPE = (24, 40, 72)


def scene():
    """(prediction, ground truth) as binary uint8 masks: a merge by dilation (ball + block), a component shared by two lesions (the
    bridge), a lesion met only inside its dilation (27 voxels, below 50 mm3 at unit spacing), a missed lesion, a false positive"""
    G = np.zeros(SCENE_SHAPE, dtype=bool)
    G |= ball(SCENE_SHAPE, (12, 12, 12), 5)
    G[11:13, 11:13, 21:23] = True
    G |= ball(SCENE_SHAPE, (12, 28, 40), 4)
    G[3:6, 3:6, 59:62] = True
    G[17:21, 33:37, 63:67] = True
    P = np.zeros(SCENE_SHAPE, dtype=bool)
    P |= ball(SCENE_SHAPE, (12, 13, 13), 5)
    P[12, 12:29, 24:26] = False
    P[12, 18:25, 13] = True
    P[12, 24, 13:37] = True
    P[12, 24:29, 36] = True
    P[2:4, 2:4, 58:60] = True
    P[20:23, 4:7, 30:33] = True
    P[12, 28, 47:49] = True
    return P.astype(np.uint8), G.astype(np.uint8)


def scene_labels():
    """the scene as two label maps whose WT, TC and ET are all the scene's masks (every foreground voxel has label 3)"""
    P, G = scene()
    return (P * 3).astype(np.uint8), (G * 3).astype(np.uint8)


def noise_pair(seed, shape):
    """two smooth three-label maps from independent seeded noise with a shared component: blobs that overlap in part, so that some
    lesions are hit, some missed, and some predicted components hit nothing"""
    rs = np.random.RandomState(seed)
    base = ndimage.gaussian_filter(rs.standard_normal(shape), 2.0, mode="constant")
    maps = []
    for k in range(2):
        f = base + 0.9 * ndimage.gaussian_filter(np.random.RandomState(seed + 1 + k).standard_normal(shape), 2.0, mode="constant")
        q = np.quantile(f, (0.90, 0.94, 0.97))
        seg = np.zeros(shape, dtype=np.uint8)
        seg[f > q[0]] = 2
        seg[f > q[1]] = 1
        seg[f > q[2]] = 3
        maps.append(seg)
    return maps[0], maps[1]


def blob_case(shape, seed=7, lesions=4, specks=300):
    """full-size synthetic pair: a few ball lesions (label 2 shell, 1 inside, 3 core) that the prediction shifts or misses, and a few
    hundred one- to three-voxel specks in the prediction"""
    rs = np.random.RandomState(seed)
    pred, gt = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    scale = min(shape) / 155.0
    for i in range(lesions):
        r = int(round((6 + 5 * i) * scale)) + 2
        c = [int(rs.randint(r + 4, s - r - 4)) for s in shape]
        for seg, shift, keep in ((gt, 0, True), (pred, 2, i != 1)):     # the prediction misses the second lesion
            if not keep:
                continue
            cc = [v + shift for v in c]
            for lab, rr in ((2, r), (1, max(r - 2, 1)), (3, max(r - 4, 1))):
                seg[ball(shape, cc, rr)] = lab
    idx = tuple(rs.randint(1, s - 2, specks) for s in shape)
    pred[idx] = 2
    long = rs.random_sample(specks) < 0.5
    pred[idx[0][long], idx[1][long], idx[2][long] + 1] = 3
    return pred, gt
