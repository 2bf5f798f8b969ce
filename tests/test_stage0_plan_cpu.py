"""The shared stage 0 of the sliding window, checked without a device through its dry-run entry point mi355_stage0_plan (the
geometry code a real mi355_sw_predict call runs).

* The plan of the geometries the bench and an uncropped BraTS volume produce.
* The plan is SUFFICIENT: a tiny torch-CPU encoder stage 0 (two 3x3x3 convs + LeakyReLU, random weights) is evaluated once over
  the whole padded volume and over the slabs the plan lists, the per-tile features are assembled exactly as the plan says (a voxel
  within r of a flagged face from that face's slab, first flagged face first; every other voxel from the whole-volume result), and
  compared with the per-tile computation on every voxel, mirrored passes included.  Both sides are convolutions of the same
  27 * Cin products per output and differ in summation order only; they run in fp64 with weights scaled to outputs of order 1,
  so the 1e-5 bound is met with ten orders of magnitude to spare by a right plan and missed by O(1) by a wrong one.
"""
import pytest
import torch
import torch.nn.functional as F


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def test_bench_geometry(ops):
    p = ops.stage0_plan((139, 172, 138), (128, 128, 128), 0.5, (), 2)
    assert p["shared"] and p["n_tiles"] == 8 and p["n_mirrors"] == 1 and len(p["samples"]) == 8
    assert p["padded"] == (139, 172, 138) and p["volume"] == (140, 176, 144) and p["slab_thickness"] == (4, 8, 8)
    origins = sorted(s["origin"] for s in p["samples"])
    assert origins == sorted((z, y, x) for z in (0, 11) for y in (0, 44) for x in (0, 10))
    for s in p["samples"]:
        assert sum(s["face"]) == 3
        for a in range(3):  # the face away from the volume's border, one per axis
            assert s["face"][2 * a:2 * a + 2] == ((0, 1) if s["origin"][a] == 0 else (1, 0))
        for f, (org, shape) in s["slabs"].items():
            a = f // 2
            assert shape == tuple(p["slab_thickness"][k] if k == a else 128 for k in range(3))
            assert org == tuple(s["origin"][k] + ((128 - shape[k]) if (k == a and f & 1) else 0) for k in range(3))


@pytest.mark.parametrize("step_size", [0.0, -0.5, 1.5])
def test_step_size_outside_0_1_is_refused(ops, amd, step_size):
    """make_geom checks the step before compute_steps divides by it: every dry run answers with an error, for a good patch and a bad one."""
    for patch in ((128, 128, 128), (128, 0, 128)):
        for plan in (ops.stage0_plan, ops.stage0_merge_plan, ops.skip_share_plan, ops.stage0_view_plan, ops.level1_share_plan):
            with pytest.raises(amd._lib.Mi355Error):
                plan((139, 172, 138), patch, step_size=step_size)


def test_uncropped_volume(ops):
    p = ops.stage0_plan((155, 240, 240), (128, 128, 128), 0.5, (), 2)
    assert p["shared"] and p["n_tiles"] == 18 and p["volume"] == (156, 240, 240)
    for s in p["samples"]:
        for a in (1, 2):
            middle = 0 < s["origin"][a] < 240 - 128
            assert (s["face"][2 * a] == 1 and s["face"][2 * a + 1] == 1) == middle
    assert sum(1 for s in p["samples"] if s["origin"][1] == 56) == 6 and sum(1 for s in p["samples"] if s["origin"][2] == 56) == 6


def test_mirrored_origins(ops):
    p = ops.stage0_plan((139, 172, 138), (128, 128, 128), 0.5, (0, 1, 2), 2)
    assert p["n_mirrors"] == 8 and len(p["samples"]) == 64
    plain = {s["tile"]: s["origin"] for s in p["samples"] if s["mirror"] == ()}
    for s in p["samples"]:
        want = tuple(p["padded"][a] - 128 - plain[s["tile"]][a] if a in s["mirror"] else plain[s["tile"]][a] for a in range(3))
        assert s["origin"] == want


@pytest.mark.parametrize("volume, r", [((128, 128, 128), 2), ((100, 90, 128), 2), ((139, 172, 138), 0)])
def test_not_shared(ops, volume, r):
    p = ops.stage0_plan(volume, (128, 128, 128), 0.5, (), r)
    assert not p["shared"] and p["samples"] == []


def _enc0(x, ws):
    for w, b in ws:
        x = F.leaky_relu(F.conv3d(x, w, b, padding=1), 0.01)
    return x


def _box(t, org, shape):
    return t[:, :, org[0]:org[0] + shape[0], org[1]:org[1] + shape[1], org[2]:org[2] + shape[2]]


def _assembly_equals_per_tile(ops, patch, volume, step, axes):
    r = 2
    p = ops.stage0_plan(volume, patch, step, axes, r)
    assert p["shared"]
    g = torch.Generator().manual_seed(5)
    f64 = dict(generator=g, dtype=torch.float64)
    ws = [(torch.randn(8, 4, 3, 3, 3, **f64) / (27 * 4) ** 0.5, torch.randn(8, **f64) * 0.5),
          (torch.randn(8, 8, 3, 3, 3, **f64) / (27 * 8) ** 0.5, torch.randn(8, **f64) * 0.5)]
    vol = torch.randn(1, 4, *volume, **f64)
    Zp, Ve = p["padded"], p["volume"]
    lo = [(Zp[a] - volume[a]) // 2 for a in range(3)]
    padded = torch.zeros(1, 4, *Zp, dtype=torch.float64)
    _box(padded, lo, volume).copy_(vol)
    whole = {}
    worst = 0.0
    for s in p["samples"]:
        m = s["mirror"]
        volm = torch.flip(padded, [2 + a for a in m]) if m else padded
        if m not in whole:
            ext = torch.zeros(1, 4, *Ve, dtype=torch.float64)
            _box(ext, (0, 0, 0), Zp).copy_(volm)
            h = F.leaky_relu(F.conv3d(ext, *ws[0], padding=1), 0.01)
            mask = torch.zeros(1, 1, *Ve, dtype=torch.float64)
            _box(mask, (0, 0, 0), Zp).fill_(1.0)
            whole[m] = _enc0(h * mask, ws[1:])
        got = _box(whole[m], s["origin"], patch).clone()
        for f in sorted(s["slabs"], reverse=True):  # the first flagged face wins: write it last
            org, shape = s["slabs"][f]
            out = _enc0(_box(volm, org, shape), ws)
            a, hi = f // 2, f & 1
            src = [slice(None)] * 5
            dst = [slice(None)] * 5
            src[2 + a] = slice(shape[a] - r, shape[a]) if hi else slice(0, r)
            dst[2 + a] = slice(patch[a] - r, patch[a]) if hi else slice(0, r)
            got[tuple(dst)] = out[tuple(src)]
        want = _enc0(_box(volm, s["origin"], patch), ws)
        worst = max(worst, float((got - want).abs().max()))
    print(f"stage-0 assembly vs per tile, patch {patch} on {volume} step {step} mirrors {axes}: max abs diff {worst:.2e} over {len(p['samples'])} samples")
    assert worst <= 1e-5
    return p


@pytest.mark.parametrize("volume, axes", [((41, 57, 43), (0, 1, 2)), ((20, 40, 30), (0, 2)), ((40, 33, 70), ())])
def test_assembly_equals_per_tile(ops, volume, axes):
    _assembly_equals_per_tile(ops, (32, 32, 32), volume, 0.5, axes)


# Off the cube and off step 0.5.  A patch of three different extents and two of its permutations, so that every axis takes the
# smallest and the largest extent once; each volume with a different odd excess (or an odd deficit: one tile, padded) per axis, one
# axis with a middle tile.  Then 32^3 at the steps at which a voxel lies in up to 4 tiles per axis (0.25), at a step no binary
# fraction holds (0.3), and at steps with little or no nominal overlap (0.75, 1.0).
NONCUBIC = [((32, 48, 64), (41, 45, 139), 0.5, (), (2, 1, 4)), ((64, 32, 48), (77, 55, 43), 0.5, (0, 2), (2, 3, 1)),
            ((48, 64, 32), (43, 75, 67), 0.5, (1,), (1, 2, 4))]
STEPPED = [((32, 32, 32), (41, 57, 43), 0.25, (), (3, 5, 3)), ((32, 32, 32), (37, 33, 70), 0.25, (0, 2), (2, 2, 6)),
           ((32, 32, 32), (41, 57, 43), 0.3, (1,), (2, 4, 3)), ((32, 32, 32), (37, 33, 70), 0.3, (), (2, 2, 5)),
           ((32, 32, 32), (41, 57, 43), 0.75, (), (2, 3, 2)), ((32, 32, 32), (37, 33, 70), 0.75, (), (2, 2, 3)),
           ((32, 32, 32), (41, 57, 43), 1.0, (), (2, 2, 2)), ((32, 32, 32), (37, 33, 70), 1.0, (2,), (2, 2, 3))]


@pytest.mark.parametrize("patch, volume, step, axes, tiles", NONCUBIC + STEPPED)
def test_assembly_equals_per_tile_geometries(ops, patch, volume, step, axes, tiles):
    p = _assembly_equals_per_tile(ops, patch, volume, step, axes)
    for a in range(3):
        assert len({s["origin"][a] for s in p["samples"] if s["mirror"] == ()}) == tiles[a]
    assert p["n_tiles"] == tiles[0] * tiles[1] * tiles[2]
    if max(tiles) >= 3:   # a middle tile: both faces of one axis inside the volume
        assert any(s["face"][2 * a] and s["face"][2 * a + 1] for s in p["samples"] for a in range(3))


def test_rightly_refused_geometries(ops):
    """The plan refuses where there is nothing to share or no room for a slab: (30, 48, 60) under the patch (32, 48, 64) is one
    tile after padding; a patch (32, 48, 4) is thinner along x than the x slab of 8 (one 4 x 8 x 8 conv tile >= 2 r)."""
    one = ops.stage0_plan((30, 48, 60), (32, 48, 64), 0.5, (0, 2), 2)
    assert not one["shared"] and one["n_tiles"] == 1 and one["padded"] == (32, 48, 64) and one["samples"] == []
    thin = ops.stage0_plan((41, 45, 9), (32, 48, 4), 0.5, (), 2)
    assert thin["n_tiles"] > 1 and thin["slab_thickness"] == (4, 8, 8) and not thin["shared"]
    assert ops.stage0_plan((41, 45, 19), (32, 48, 8), 0.5, (), 2)["shared"]
