"""The shared level 1 (csrc/sw_share_plan.hip "shared level 1"), checked without a device through the dry run
mi355_level1_share_plan - the geometry and the decision a forward would run on.

* The plan of the bench geometry and of small geometries: merged axes, regions, shell depths, slab thickness, voxel counts.
* The plan is SUFFICIENT, EXACTLY: an int64 chain with small integer weights - stem, a second stage-0 block, a stride-2 block, a
  stride-1 block (ReLU behind each), then the skip half (no bias, no activation).  Encoder level 1 and the skip half are evaluated
  over the regions - whose level-0 input is the whole-volume stage-0 result with stage-0 shells at their faces on per-origin axes,
  zeros restored outside the padded volume between the layers - and over the level-1 slabs, each cut from the tile's own level-0
  features; each tile's two level-1 tensors are assembled as the plan says - the region's values, then the shells d1 / dS deep
  from the slabs, z before y before x - and must EQUAL the tile computed on its own, on every voxel of every sample."""
import inspect

import pytest
import torch
import torch.nn.functional as F

BENCH = ((139, 172, 138), (128, 128, 128))
P32 = (32, 32, 32)


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def test_bench_geometry(ops):
    p = ops.level1_share_plan(*BENCH)
    assert p["possible"] and p["on"]
    assert (p["r0"], p["k1"], p["d1"], p["dS"]) == (2, 2, 3, 4)
    assert p["merged"] == (False, True, True) and p["region"] == (128, 176, 144) and p["slab_thickness"] == (0, 8, 8)
    assert [(r["origin"], r["faces"]) for r in p["regions"]] == [((0, 0, 0), (0, 1, 0, 0, 0, 0)), ((11, 0, 0), (1, 0, 0, 0, 0, 0))]
    assert [d // 2 for d in p["region"]] == [64, 88, 72]
    assert sorted({s["origin1"] for s in p["samples"]}) == [(0, y, x) for y in (0, 22) for x in (0, 5)]
    assert all(s["region"] == (s["origin"][0] == 11) for s in p["samples"])
    assert p["n_slabs"] == (0, 8, 8)
    assert (p["region_voxels"], p["slab_voxels"], p["tile_voxels"]) == (811008, 524288, 2097152)
    for s in p["samples"]:   # one slab per face inside the region: the 16 outermost level-0 layers of the tile
        z, y, x = s["origin"]
        assert set(s["slabs"]) == {3 if y == 0 else 2, 5 if x == 0 else 4}
        for f, (off, shape) in s["slabs"].items():
            a = f >> 1
            assert shape == tuple(16 if c == a else 128 for c in range(3))
            assert off == tuple(112 if c == a and f & 1 else 0 for c in range(3))
    assert not ops.level1_share_plan(*BENCH, mode=0)["on"]
    # the default rule: patch / 2 >= 8 slab thicknesses; half the bench patch does not pass it
    small = ops.level1_share_plan((100, 100, 100), (64, 64, 64))
    assert small["possible"] and not small["on"]


def test_what_the_decision_refuses(ops):
    for kw in ({"dtype": "f16"}, {"norm": "instance"}, {"nonlin_first": True}, {"skip_is_enc1": False}, {"dec1_blocks": 1}, {"num_pool": 1},
               {"enc0_blocks": 0}):
        assert not ops.level1_share_plan(*BENCH, mode=2, **kw)["on"], kw


def test_no_merged_axis(ops):
    """(41, 57, 43), patch 32^3: steps (0, 9) x (0, 12, 25) x (0, 11): an odd origin or an odd extent on every axis."""
    for mode in (1, 2):
        p = ops.level1_share_plan((41, 57, 43), P32, mode=mode, num_pool=2)
        assert not p["possible"] and not p["on"] and p["regions"] == [] and p["samples"] == []


def test_one_tile(ops):
    for mode in (1, 2):
        p = ops.level1_share_plan((32, 32, 32), P32, mode=mode, num_pool=2)
        assert not p["possible"] and not p["on"]


def test_three_tiles_along_y(ops):
    """(41, 56, 44): z per-origin (0, 9); y merged, three tiles (0, 12, 24), the middle one with two faces inside the region; x
    merged (0, 12)."""
    p = ops.level1_share_plan((41, 56, 44), P32, mode=2, num_pool=2)
    assert p["possible"] and p["merged"] == (False, True, True) and p["region"] == (32, 56, 48) and p["slab_thickness"] == (0, 8, 8)
    assert [(r["origin"], r["faces"]) for r in p["regions"]] == [((0, 0, 0), (0, 1, 0, 0, 0, 0)), ((9, 0, 0), (1, 0, 0, 0, 0, 0))]
    middle = [s for s in p["samples"] if s["origin"][1] == 12]
    assert len(middle) == 4 and all({2, 3} <= set(s["slabs"]) and s["origin1"][1] == 6 for s in middle)
    assert p["n_slabs"] == (0, 16, 12)


def test_eight_mirrors(ops):
    """(40, 56, 44) with 8 mirrors: every axis merged, one region per mirror."""
    p = ops.level1_share_plan((40, 56, 44), P32, mirror_axes=(0, 1, 2), mode=2, num_pool=2)
    assert p["possible"] and p["merged"] == (True, True, True) and p["n_mirrors"] == 8
    assert [r["mirror"] for r in p["regions"]] == [(), (2,), (1,), (1, 2), (0,), (0, 2), (0, 1), (0, 1, 2)]
    assert all(r["origin"] == (0, 0, 0) and r["faces"] == (0,) * 6 for r in p["regions"])
    assert all(p["regions"][s["region"]]["mirror"] == s["mirror"] for s in p["samples"])


def test_plan_takes_no_batch_or_rank(ops, amd):
    assert not {"batch_tiles", "batch_samples", "rank", "world"} & set(inspect.signature(ops.level1_share_plan).parameters)
    assert len(amd._lib.load().mi355_level1_share_plan.argtypes) == 13
    assert ops.level1_share_plan(*BENCH, mirror_axes=(0, 1, 2)) == ops.level1_share_plan(*BENCH, mirror_axes=(0, 1, 2))


@pytest.mark.parametrize("volume, patch, axes", [BENCH + ((),), BENCH + ((0, 1, 2),), ((100, 100, 100), (64, 64, 64), ()), ((41, 57, 43), P32, ()),
                                                 ((32, 32, 32), P32, ()), ((41, 56, 44), P32, ()), ((40, 56, 44), P32, (0, 1, 2)), ((37, 33, 68), P32, (2,))])
def test_stage0_part_is_the_other_dry_runs(ops, volume, patch, axes):
    """A window decides once (sw_share_plan): the stage-0 fields this dry run reports are those mi355_skip_share_plan reports for the
    same network description and mi355_stage0_merge_plan for the r and skip half that one decided, in every mode; and the shared
    level 1 is on only on top of the shared stage 0 and the shared skip half."""
    for kw in ({}, {"dtype": "f16"}, {"norm": "instance"}, {"nonlin_first": True}, {"enc0_blocks": 0}, {"enc0_blocks": 1}):
        s = ops.skip_share_plan(volume, patch, mirror_axes=axes, **kw)
        m = ops.stage0_merge_plan(volume, patch, mirror_axes=axes, r=s["r"], skip_half=s["skip_shared"])
        for mode in (0, 1, 2):
            p = ops.level1_share_plan(volume, patch, mirror_axes=axes, mode=mode, num_pool=2, **kw)
            assert (p["volume"], p["stage0_slab_thickness"], p["r0"], p["n_tiles"], p["n_mirrors"]) == \
                   (s["volume"], s["slab_thickness"], s["r"], s["n_tiles"], s["n_mirrors"]), (kw, mode)
            assert (p["padded"], p["volume"], p["stage0_slab_thickness"], p["r0"], p["n_tiles"], p["n_mirrors"]) == \
                   (m["padded"], m["volume"], m["slab_thickness"], m["r"], m["n_tiles"], m["n_mirrors"]), (kw, mode)
            assert not p["on"] or (s["skip_shared"] and s["stage0_shared"] and m["shared"]), (kw, mode)


# ------------------------------------------------------------------ the exact model
def _box(t, org, shape):
    return t[:, :, org[0]:org[0] + shape[0], org[1]:org[1] + shape[1], org[2]:org[2] + shape[2]]


def _weights():
    g = torch.Generator().manual_seed(21)
    iw = lambda *s: torch.randint(-2, 3, s, generator=g)  # noqa: E731
    enc0 = [(iw(4, 2, 3, 3, 3), iw(4) + 3), (iw(4, 4, 3, 3, 3), iw(4) - 1)]
    enc1 = [(iw(4, 4, 3, 3, 3), iw(4) + 2), (iw(4, 4, 3, 3, 3), iw(4) + 1)]
    return enc0, enc1, iw(4, 4, 3, 3, 3)


def _masked(x, keep):
    if keep is None:
        return x
    m = torch.zeros(1, 1, *x.shape[2:], dtype=torch.int64)
    _box(m, (0, 0, 0), keep).fill_(1)
    return x * m


def _enc0(x, W, keep=None):
    """stage 0 over a box; keep: its part inside the padded volume, zeros restored outside it behind every layer"""
    for w, b in W[0]:
        x = _masked(F.relu(F.conv3d(x, w, b, padding=1)), keep)
    return x


def _level1(x, W, keep=None):
    """(enc[1]'s output, the skip half) of a box of level-0 features; keep as above, at level 1"""
    for i, (w, b) in enumerate(W[1]):
        x = _masked(F.relu(F.conv3d(x, w, b, stride=2 if i == 0 else 1, padding=1)), keep)
    return x, F.conv3d(x, W[2], None, padding=1)


def _put_shell(dst, src, a, side, depth):
    """the shell of face (a, side) of dst <- the same layers of src, whose extent along a may be smaller (a slab)"""
    d, s = [slice(None)] * 5, [slice(None)] * 5
    n, t = dst.shape[2 + a], src.shape[2 + a]
    d[2 + a] = slice(n - depth, n) if side else slice(0, depth)
    s[2 + a] = slice(t - depth, t) if side else slice(0, depth)
    dst[tuple(d)] = src[tuple(s)]


def _assembly_equals_per_tile_exactly(ops, patch, volume, step, axes, shrink=(0, 0)):
    """shrink: layers taken off the shell depths (d1, dS); then nothing is asserted of the tensors, and which of the two differed
    on some sample is returned next to the plan"""
    p = ops.level1_share_plan(volume, patch, step, mirror_axes=axes, mode=2, num_pool=2)
    assert p["possible"]
    W = _weights()
    vol = torch.randint(-3, 4, (1, 2) + tuple(volume), generator=torch.Generator().manual_seed(22))
    Zp, Ve, R, t0, t1 = p["padded"], p["volume"], p["region"], p["stage0_slab_thickness"], p["slab_thickness"]
    half = tuple(d // 2 for d in patch)
    lo = [(Zp[a] - volume[a]) // 2 for a in range(3)]
    padded = torch.zeros(1, 2, *Zp, dtype=torch.int64)
    _box(padded, lo, volume).copy_(vol)
    ext, whole, region = {}, {}, {}

    def pass_of(m):   # the extended volume of the mirrored pass, and stage 0 over it (zero outside the padded volume)
        if m not in ext:
            e = torch.zeros(1, 2, *Ve, dtype=torch.int64)
            _box(e, (0, 0, 0), Zp).copy_(torch.flip(padded, [2 + a for a in m]) if m else padded)
            ext[m], whole[m] = e, _enc0(e, W, Zp)
        return ext[m]

    for i, rg in enumerate(p["regions"]):
        e, o = pass_of(rg["mirror"]), rg["origin"]
        x0 = _box(whole[rg["mirror"]], o, R).clone()
        for f in (5, 4, 3, 2, 1, 0):   # the region is a "tile" of the shared stage 0: shells r0 deep, the first in z, y, x wins
            if not rg["faces"][f]:
                continue
            a, side = f >> 1, f & 1
            assert not p["merged"][a]
            so = list(o)
            so[a] += (R[a] - t0[a]) if side else 0
            shape = tuple(t0[c] if c == a else R[c] for c in range(3))
            keep = tuple(min(shape[c], Zp[c] - so[c]) for c in range(3))
            _put_shell(x0, _enc0(_box(e, so, shape), W, keep), a, side, p["r0"])
        keep1 = tuple(Zp[c] // 2 if p["merged"][c] else R[c] // 2 for c in range(3))
        region[i] = _level1(x0, W, keep1)
    worst, differs = 0, [False, False]
    for s in p["samples"]:
        m, org = s["mirror"], s["origin"]
        t0_own = _enc0(_box(pass_of(m), org, patch), W)   # the tile on its own: zero padding at all six faces
        want = _level1(t0_own, W)
        got = [_box(v, s["origin1"], half).clone() for v in region[s["region"]]]
        for f in (5, 4, 3, 2, 1, 0):
            if f not in s["slabs"]:
                continue
            a, side = f >> 1, f & 1
            off, shape = s["slabs"][f]
            assert p["merged"][a] and shape[a] == 2 * t1[a]
            src = _level1(_box(t0_own, off, shape), W)   # zero padding at the cut, the tile's own features everywhere else
            for i, depth in enumerate((p["d1"] - shrink[0], p["dS"] - shrink[1])):
                _put_shell(got[i], src[i], a, side, depth)
        for i, name in enumerate(("enc[1]'s output", "the skip half")):
            differs[i] = differs[i] or not torch.equal(got[i], want[i])
            assert any(shrink) or not differs[i], f"{name} of tile {s['tile']} mirror {m}: {int((got[i] != want[i]).sum())} elements differ"
            worst = max(worst, int(want[i].abs().max()))
    assert 0 < worst < 2 ** 62
    return (p, differs) if any(shrink) else p


@pytest.mark.parametrize("volume, axes", [((41, 56, 44), ()), ((40, 56, 44), (0, 1, 2)), ((37, 33, 68), (2,))])
def test_assembly_equals_per_tile_exactly(ops, volume, axes):
    """The third case: z and y per-origin with odd origins (regions with stage-0 shells on two axes and the edge between them), x
    merged with four tiles (0, 12, 24, 36)."""
    _assembly_equals_per_tile_exactly(ops, P32, volume, 0.5, axes)


# Off the cube and off step 0.5.  The shared level 1 needs an axis on which every origin and the padded extent are even, so each
# volume is the neighbour of an all-odd one - (41, 45, 139), (77, 55, 43), (43, 75, 67), (41, 57, 43), (37, 33, 70), for which the
# plan rightly answers "not possible" (test_rightly_refused_geometries) - that is even on ONE axis: the others keep their odd
# excess or deficit and stay per-origin.  merged: the axis the plan must merge; tiles: tile origins per axis.
NONCUBIC = [((32, 48, 64), (41, 45, 128), 0.5, (), 2, (2, 1, 3)), ((64, 32, 48), (77, 56, 43), 0.5, (0, 2), 1, (2, 3, 1)),
            ((48, 64, 32), (43, 75, 68), 0.5, (1,), 2, (1, 2, 4))]
STEPPED = [(P32, (41, 56, 43), 0.25, (), 1, (3, 4, 3)), (P32, (37, 34, 70), 0.25, (0,), 1, (2, 2, 6)),
           (P32, (41, 56, 43), 0.3, (2,), 1, (2, 4, 3)), (P32, (37, 34, 70), 0.3, (), 1, (2, 2, 5)),
           (P32, (41, 57, 44), 0.75, (), 2, (2, 3, 2)), (P32, (37, 34, 70), 0.75, (), 1, (2, 2, 3)),
           (P32, (41, 57, 44), 1.0, (), 2, (2, 2, 2)), (P32, (37, 34, 70), 1.0, (1,), 1, (2, 2, 3))]


@pytest.mark.parametrize("patch, volume, step, axes, merged, tiles", NONCUBIC + STEPPED)
def test_assembly_equals_per_tile_exactly_geometries(ops, patch, volume, step, axes, merged, tiles):
    p = _assembly_equals_per_tile_exactly(ops, patch, volume, step, axes)
    assert p["merged"] == tuple(a == merged for a in range(3))
    assert p["region"] == tuple(p["volume"][a] if a == merged else patch[a] for a in range(3))
    assert p["n_tiles"] == tiles[0] * tiles[1] * tiles[2] and p["n_mirrors"] == 2 ** len(axes)
    # one region per (mirror, origin tuple on the per-origin axes)
    assert len(p["regions"]) == p["n_mirrors"] * p["n_tiles"] // tiles[merged]
    for s in p["samples"]:
        assert s["origin1"] == tuple(s["origin"][a] // 2 if a == merged else 0 for a in range(3))
        assert set(s["slabs"]) == {2 * merged + side for side in (0, 1) if s["faces"][2 * merged + side]}
    if tiles[merged] >= 3:   # a middle tile: two level-1 slabs
        assert any(len(s["slabs"]) == 2 for s in p["samples"])


def test_rightly_refused_geometries(ops):
    """A stride-2 conv commutes with even shifts only: where every axis has an odd origin or an odd padded extent no axis merges,
    at any step and for any patch - the all-odd neighbours of the geometries above.  And a patch (32, 48, 24) on (41, 45, 48) has
    even x origins (0, 12, 24) but half its x extent, 12, has no room for the two level-1 slabs of thickness 8 a middle tile needs."""
    for patch, volume, step, axes in [((32, 48, 64), (41, 45, 139), 0.5, ()), ((64, 32, 48), (77, 55, 43), 0.5, (0, 2)),
                                      ((48, 64, 32), (43, 75, 67), 0.5, (1,)), (P32, (41, 57, 43), 0.25, ()), (P32, (37, 33, 70), 0.3, ()),
                                      (P32, (41, 57, 43), 0.75, ()), (P32, (37, 33, 70), 1.0, ())]:
        for mode in (1, 2):
            p = ops.level1_share_plan(volume, patch, step, mirror_axes=axes, mode=mode, num_pool=2)
            assert p["n_tiles"] > 1 and not p["possible"] and not p["on"] and p["regions"] == [] and p["samples"] == [], (patch, volume, step)
    assert sorted({s["origin"][2] for s in ops.stage0_plan((41, 45, 48), (32, 48, 24), 0.5, (), 2)["samples"]}) == [0, 12, 24]
    p = ops.level1_share_plan((41, 45, 48), (32, 48, 24), 0.5, mode=2, num_pool=2)
    assert not p["possible"] and not p["on"]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("patch, volume, step, axes, merged, tiles", NONCUBIC + STEPPED[:2])
def test_shallower_shells_are_not_enough_geometries(ops, which, patch, volume, step, axes, merged, tiles):
    """The depths d1 and dS are tight off the cube and at step 0.25 too: one layer less of either and that tensor differs on some tile."""
    shrink = (1, 0) if which == 0 else (0, 1)
    _, differs = _assembly_equals_per_tile_exactly(ops, patch, volume, step, axes, shrink)
    assert differs[which] and not differs[1 - which]


@pytest.mark.parametrize("which, by", [("d1", -1), ("dS", -1)])
def test_shallower_shells_are_not_enough(ops, which, by):
    """The depths are tight: one layer less and some tile differs (so the exact test above is not vacuous)."""
    volume = (41, 56, 44)
    p = ops.level1_share_plan(volume, P32, mode=2, num_pool=2)
    W = _weights()
    vol = torch.randint(-3, 4, (1, 2) + volume, generator=torch.Generator().manual_seed(22))
    depth = dict(d1=p["d1"], dS=p["dS"])
    depth[which] += by
    e = torch.zeros(1, 2, *p["volume"], dtype=torch.int64)
    _box(e, (0, 0, 0), volume).copy_(vol)
    whole = _enc0(e, W, p["padded"])
    differs = False
    for s in p["samples"]:
        if s["origin"][0] != 0:   # (the tiles of the region at z = 0, whose one face inside the volume is the high z face)
            continue
        rg = p["regions"][s["region"]]
        x0 = _box(whole, rg["origin"], p["region"]).clone()
        t0, R = p["stage0_slab_thickness"], p["region"]
        so = (R[0] - t0[0], 0, 0)
        shape = (t0[0], R[1], R[2])
        _put_shell(x0, _enc0(_box(e, so, shape), W, tuple(min(shape[c], p["padded"][c] - so[c]) for c in range(3))), 0, 1, p["r0"])
        reg = _level1(x0, W, (R[0] // 2, p["padded"][1] // 2, p["padded"][2] // 2))
        t0_own = _enc0(_box(e, s["origin"], P32), W)
        want = _level1(t0_own, W)
        got = [_box(v, s["origin1"], (16, 16, 16)).clone() for v in reg]
        for f in (5, 4, 3, 2):
            if f in s["slabs"]:
                src = _level1(_box(t0_own, *s["slabs"][f]), W)
                for i, k in enumerate(("d1", "dS")):
                    _put_shell(got[i], src[i], f >> 1, f & 1, depth[k])
        i = 0 if which == "d1" else 1
        differs = differs or not torch.equal(got[i], want[i])
    assert differs
