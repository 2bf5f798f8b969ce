"""The merged stage-0 slabs (MI355_MERGE_SLABS, csrc/sw_share_plan.hip "merged slabs"), checked without a device through the dry run
mi355_stage0_merge_plan - the geometry code a real call runs.

* The plan of the bench geometry and of the small geometries the GPU tests use: keys, boxes, voxel totals and, per sample, the
  slab index and the tile's origin inside the slab.
* The plan is SUFFICIENT, EXACTLY: a torch-CPU chain with small integer weights (two 3x3x3 convs with bias and a LeakyReLU of slope
  1/2, then a third conv without bias or activation - the skip half S), so that every sum is an exact fp64 number whatever its
  order.  It is evaluated once over the whole extended volume, over the per-tile z-slabs and over the merged y- and x-slabs, with
  zeros restored outside the padded volume between the layers; each tile's skip tensor (shell r) and S (shell r + 1) are assembled
  exactly as the plan says - z shell first, then y, then x - and must EQUAL the tile computed on its own, on every voxel."""
import pytest
import torch
import torch.nn.functional as F

BENCH = ((139, 172, 138), (128, 128, 128))


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def test_bench_geometry(ops):
    p = ops.stage0_merge_plan(*BENCH, 0.5, (), 2, True)
    assert p["shared"] and (p["r"], p["rs"]) == (2, 3) and p["n_tiles"] == 8 and p["n_mirrors"] == 1
    assert p["volume"] == (140, 176, 144) and p["slab_thickness"] == (8, 8, 8)
    assert p["slab_shape"] == ((8, 128, 128), (140, 8, 128), (140, 176, 8))
    assert p["n_slabs"] == (8, 4, 2)
    assert p["voxels"] == (1048576, 573440, 394240) and sum(p["voxels"]) == 2016256
    assert p["voxels_per_tile"] == 3145728
    # every launch group stays above the 1024 tile units (4 x 8 x 8 voxels) of the F(2x2x2,3x3x3) kernel
    assert [v // 256 for v in p["voxels"]] == [4096, 2240, 1540]
    assert [(k["side"], k["origin"]) for k in p["slabs"][1]] == [(0, (0, 44, 0)), (0, (0, 44, 10)), (1, (0, 120, 0)), (1, (0, 120, 10))]
    assert [(k["side"], k["origin"]) for k in p["slabs"][2]] == [(0, (0, 0, 10)), (1, (0, 0, 120))]
    for s in p["samples"]:
        z, y, x = s["origin"]
        assert s["slab"][0:2] == ((-1, 0) if z == 0 else (0, -1))
        assert s["slab"][2:4] == ((-1, 2 + (x > 0)) if y == 0 else (0 + (x > 0), -1))
        assert s["slab"][4:6] == ((-1, 1) if x == 0 else (0, -1))
        for f, off in s["offset"].items():
            assert off == ((z, 0, 0) if f >> 1 == 1 else (z, y, 0))


def _check_plan(p, patch):
    """What the gather relies on, for any geometry: a sample's face indexes a slab of its own pass and side whose box holds the
    tile's part at the offset the plan gives."""
    t, Ve = p["slab_thickness"], p["volume"]
    assert p["slab_shape"][1] == (Ve[0], t[1], patch[2]) and p["slab_shape"][2] == (Ve[0], Ve[1], t[2])
    for a in (1, 2):
        keys = [(k["mirror"], k["side"], k["origin"]) for k in p["slabs"][a]]
        assert len(set(keys)) == len(keys) == p["n_slabs"][a]
        used = set()
        for s in p["samples"]:
            for side in (0, 1):
                f = 2 * a + side
                interior = s["origin"][a] + patch[a] < p["padded"][a] if side else s["origin"][a] > 0
                assert (s["slab"][f] >= 0) == interior
                if not interior:
                    continue
                k = p["slabs"][a][s["slab"][f]]
                used.add(s["slab"][f])
                assert k["mirror"] == s["mirror"] and k["side"] == side
                part = list(s["origin"])
                part[a] += (patch[a] - t[a]) if side else 0      # the tile's part of the slab, in the pass
                assert tuple(part[c] - k["origin"][c] for c in range(3)) == s["offset"][f]
                for c in range(3):
                    ext = t[c] if c == a else patch[c]
                    assert 0 <= s["offset"][f][c] and s["offset"][f][c] + ext <= p["slab_shape"][a][c]
        assert used == set(range(len(keys)))


def test_odd_geometry(ops):
    """(41, 57, 43), patch 32^3: steps (0, 9) x (0, 12, 25) x (0, 11), odd offsets, a middle tile with two interior y faces."""
    patch = (32, 32, 32)
    p = ops.stage0_merge_plan((41, 57, 43), patch, 0.5, (), 2, True)
    assert sorted({s["origin"] for s in p["samples"]}) == sorted((z, y, x) for z in (0, 9) for y in (0, 12, 25) for x in (0, 11))
    assert p["volume"] == (44, 64, 48) and p["n_slabs"] == (12, 8, 2)
    assert sorted((k["side"], k["origin"][1]) for k in p["slabs"][1]) == sorted([(0, 12), (0, 25), (1, 24), (1, 36)] * 2)
    middle = [s for s in p["samples"] if s["origin"][1] == 12]
    assert len(middle) == 4 and all(s["slab"][2] >= 0 and s["slab"][3] >= 0 for s in middle)
    _check_plan(p, patch)


def test_eight_mirrors(ops):
    patch = (32, 32, 32)
    p = ops.stage0_merge_plan((40, 56, 44), patch, 0.5, (0, 1, 2), 2, True)
    one = ops.stage0_merge_plan((40, 56, 44), patch, 0.5, (), 2, True)
    assert p["n_mirrors"] == 8 and len(p["samples"]) == 8 * len(one["samples"])
    assert p["n_slabs"][1] == 8 * one["n_slabs"][1] and p["n_slabs"][2] == 8 * one["n_slabs"][2]
    _check_plan(p, patch)
    # sorted by key, the mirror first
    for a in (1, 2):
        order = [k["mirror"] for k in p["slabs"][a]]
        assert [order[i] for i in range(0, len(order), len(order) // 8)] == [(), (2,), (1,), (1, 2), (0,), (0, 2), (0, 1), (0, 1, 2)]


@pytest.mark.parametrize("volume", [(32, 32, 32), (20, 30, 32)])
def test_no_keys(ops, volume):
    """One tile, and one tile per axis after padding: nothing is shared, no keys."""
    p = ops.stage0_merge_plan(volume, (32, 32, 32), 0.5, (), 2, True)
    assert not p["shared"] and p["n_slabs"] == (0, 0, 0) and p["slabs"] == {1: [], 2: []} and p["samples"] == []


def test_one_tile_along_an_axis(ops):
    """(20, 40, 30): tiles along y only - y keys, no x key, no z-slab."""
    p = ops.stage0_merge_plan((20, 40, 30), (32, 32, 32), 0.5, (), 2, True)
    assert p["shared"] and p["n_slabs"][0] == 0 and p["n_slabs"][1] > 0 and p["n_slabs"][2] == 0
    _check_plan(p, (32, 32, 32))


def test_plan_takes_no_batch_or_rank(ops, amd):
    """The key set is a function of the network and the geometry of all tiles: the entry point has no batch, rank or world argument,
    and repeated calls agree."""
    import inspect
    assert not {"batch_tiles", "rank", "world"} & set(inspect.signature(ops.stage0_merge_plan).parameters)
    assert len(amd._lib.load().mi355_stage0_merge_plan.argtypes) == 13
    assert ops.stage0_merge_plan(*BENCH, 0.5, (0, 1, 2)) == ops.stage0_merge_plan(*BENCH, 0.5, (0, 1, 2))


# ------------------------------------------------------------------ the exact model
def _box(t, org, shape):
    return t[:, :, org[0]:org[0] + shape[0], org[1]:org[1] + shape[1], org[2]:org[2] + shape[2]]


def _weights():
    g = torch.Generator().manual_seed(11)
    iw = lambda *s: torch.randint(-2, 3, s, generator=g).double()
    return [(iw(4, 2, 3, 3, 3), iw(4) + 3.0), (iw(4, 4, 3, 3, 3), iw(4) - 1.0)], iw(4, 4, 3, 3, 3)


def _chain(x, enc, wskip, keep=None):
    """(skip tensor, S) of a box; keep: the part of the box inside the padded volume, zeros restored outside it between layers."""
    mask = None
    if keep is not None:
        mask = torch.zeros(1, 1, *x.shape[2:], dtype=torch.float64)
        _box(mask, (0, 0, 0), keep).fill_(1.0)
    for w, b in enc:
        x = F.leaky_relu(F.conv3d(x, w, b, padding=1), 0.5)
        if mask is not None:
            x = x * mask
    return x, F.conv3d(x, wskip, None, padding=1)


def _put_shell(dst, src, a, side, depth, patch, t):
    """dst [.., P] <- the shell of face (a, side) from src, a tile-shaped cut of the slab whose extent along a is t[a]."""
    d, s = [slice(None)] * 5, [slice(None)] * 5
    d[2 + a] = slice(patch[a] - depth, patch[a]) if side else slice(0, depth)
    s[2 + a] = slice(t[a] - depth, t[a]) if side else slice(0, depth)
    dst[tuple(d)] = src[tuple(s)]


def _assembly_equals_per_tile_exactly(ops, patch, volume, step, axes):
    p = ops.stage0_merge_plan(volume, patch, step, axes, 2, True)
    assert p["shared"]
    enc, wskip = _weights()
    g = torch.Generator().manual_seed(12)
    vol = torch.randint(-3, 4, (1, 2) + tuple(volume), generator=g).double()
    Zp, Ve, t, r, rs = p["padded"], p["volume"], p["slab_thickness"], p["r"], p["rs"]
    lo = [(Zp[a] - volume[a]) // 2 for a in range(3)]
    padded = torch.zeros(1, 2, *Zp, dtype=torch.float64)
    _box(padded, lo, volume).copy_(vol)
    ext, whole, merged = {}, {}, {}

    def pass_of(m):   # the extended volume of the mirrored pass: the flipped padded volume at 0, zeros behind it
        if m not in ext:
            e = torch.zeros(1, 2, *Ve, dtype=torch.float64)
            _box(e, (0, 0, 0), Zp).copy_(torch.flip(padded, [2 + a for a in m]) if m else padded)
            ext[m] = e
            whole[m] = _chain(e, enc, wskip, Zp)
        return ext[m]

    for a in (1, 2):   # every key, whatever tile asks
        for i, k in enumerate(p["slabs"][a]):
            shape = p["slab_shape"][a]
            keep = tuple(min(shape[c], Zp[c] - k["origin"][c]) for c in range(3))
            merged[a, i] = _chain(_box(pass_of(k["mirror"]), k["origin"], shape), enc, wskip, keep)
    for s in p["samples"]:
        m, org = s["mirror"], s["origin"]
        e = pass_of(m)
        want = _chain(_box(e, org, patch), enc, wskip)   # the tile on its own: zero padding at all six faces
        got = [_box(whole[m][i], org, patch).clone() for i in range(2)]
        for f in (5, 4, 3, 2, 1, 0):   # the first shell in the order z, y, x wins: write it last
            if s["slab"][f] < 0:
                continue
            a, side = f >> 1, f & 1
            if a == 0:   # per-tile z-slab: the tile's own y and x padding
                o = list(org)
                o[0] += (patch[0] - t[0]) if side else 0
                src = _chain(_box(e, o, (t[0], patch[1], patch[2])), enc, wskip)
            else:
                cut = tuple(t[c] if c == a else patch[c] for c in range(3))
                src = [_box(v, s["offset"][f], cut) for v in merged[a, s["slab"][f]]]
            for i, depth in enumerate((r, rs)):
                _put_shell(got[i], src[i], a, side, depth, patch, t)
        for i, name in enumerate(("skip tensor", "S")):
            assert torch.equal(got[i], want[i]), f"{name} of tile {s['tile']} mirror {m}: {int((got[i] != want[i]).sum())} elements differ"
    return p


@pytest.mark.parametrize("volume, axes", [((41, 57, 43), ()), ((40, 56, 44), (0, 1, 2)), ((20, 40, 30), (1,)), ((37, 33, 70), (0, 2))])
def test_assembly_equals_per_tile_exactly(ops, volume, axes):
    _assembly_equals_per_tile_exactly(ops, (32, 32, 32), volume, 0.5, axes)


# Off the cube and off step 0.5 (the cases of tests/test_stage0_plan_cpu.py): three different extents in three orders, volumes with
# a different odd excess or deficit per axis, a middle tile on one axis and a single tile on another; 32^3 at steps 0.25 (tiles i
# and i + 2 overlap: a y key is shared by tiles of several x AND z origins), 0.3, 0.75 and 1.0.
NONCUBIC = [((32, 48, 64), (41, 45, 139), 0.5, (), (2, 1, 4)), ((64, 32, 48), (77, 55, 43), 0.5, (0, 2), (2, 3, 1)),
            ((48, 64, 32), (43, 75, 67), 0.5, (1,), (1, 2, 4))]
STEPPED = [((32, 32, 32), (41, 57, 43), 0.25, (), (3, 5, 3)), ((32, 32, 32), (37, 33, 70), 0.25, (0, 2), (2, 2, 6)),
           ((32, 32, 32), (41, 57, 43), 0.3, (1,), (2, 4, 3)), ((32, 32, 32), (37, 33, 70), 0.3, (), (2, 2, 5)),
           ((32, 32, 32), (41, 57, 43), 0.75, (), (2, 3, 2)), ((32, 32, 32), (37, 33, 70), 0.75, (), (2, 2, 3)),
           ((32, 32, 32), (41, 57, 43), 1.0, (), (2, 2, 2)), ((32, 32, 32), (37, 33, 70), 1.0, (2,), (2, 2, 3))]


@pytest.mark.parametrize("patch, volume, step, axes, tiles", NONCUBIC + STEPPED)
def test_assembly_equals_per_tile_exactly_geometries(ops, patch, volume, step, axes, tiles):
    p = _assembly_equals_per_tile_exactly(ops, patch, volume, step, axes)
    _check_plan(p, patch)
    assert p["n_tiles"] == tiles[0] * tiles[1] * tiles[2] and p["n_mirrors"] == 2 ** len(axes)
    for a in range(3):
        assert len({s["origin"][a] for s in p["samples"] if s["mirror"] == ()}) == tiles[a]
        if tiles[a] == 1:   # one tile along an axis: no face of it inside the volume, no slab
            assert p["n_slabs"][a] == 0
    # a y key is (mirror, side, y of the slab, x origin): tiles that differ in z alone share it
    if tiles[1] > 1:
        assert p["n_slabs"][1] == p["n_mirrors"] * 2 * (tiles[1] - 1) * tiles[2]


def test_rightly_refused_geometries(ops):
    """With the skip half the slab chain is r + 1 = 3 layers deep and a z slab 8 thick (two conv tiles of 4 >= 6): a patch
    (6, 48, 64) has no room for it and is refused, while without the skip half (thickness 4) it is shared; and (30, 48, 60) under
    (32, 48, 64) is one tile after padding, with nothing to share."""
    thin = ops.stage0_merge_plan((11, 45, 75), (6, 48, 64), 0.5, (), 2, True)
    assert thin["n_tiles"] > 1 and thin["slab_thickness"][0] == 8 and not thin["shared"] and thin["n_slabs"] == (0, 0, 0)
    assert ops.stage0_merge_plan((11, 45, 75), (6, 48, 64), 0.5, (), 2, False)["shared"]
    one = ops.stage0_merge_plan((30, 48, 60), (32, 48, 64), 0.5, (1,), 2, True)
    assert one["n_tiles"] == 1 and not one["shared"] and one["samples"] == []
