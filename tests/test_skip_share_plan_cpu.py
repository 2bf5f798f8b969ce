"""The shared skip half of the last decoder stage's concat conv (csrc/sw_share_plan.hip "shared skip half"), checked without a device through
its dry-run entry point mi355_skip_share_plan - the decision code a real mi355_sw_predict call runs.

The decision may depend on the network and on the geometry of all tiles only: every rank, lane and batch must compute a tile the
same way (the invariant of the shared stage 0)."""
import itertools

import pytest

BENCH = dict(volume=(139, 172, 138), patch=(128, 128, 128))


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def test_model_a_bench_geometry(ops):
    p = ops.skip_share_plan(**BENCH)
    assert p["stage0_shared"] and p["skip_shared"]
    assert p["n_tiles"] == 8 and p["n_mirrors"] == 1 and p["volume"] == (140, 176, 144)
    # r = 2 stage-0 blocks: the skip is taken 2 layers deep, S one more; the slab chain has 3 layers, 2 * 3 = 6 -> (8, 8, 8)
    assert p["r"] == 2 and p["skip_shell"] == 3 and p["slab_thickness"] == (8, 8, 8)
    # the stage-0 dry run alone still reports the 2-layer chain
    assert ops.stage0_plan(BENCH["volume"], BENCH["patch"], 0.5, (), 2)["slab_thickness"] == (4, 8, 8)


def test_shell_depth_follows_r(ops):
    for r, slab in ((1, (4, 8, 8)), (2, (8, 8, 8)), (3, (8, 8, 8)), (4, (12, 16, 16))):
        p = ops.skip_share_plan(enc0_blocks=r, **BENCH)
        assert p["skip_shared"] and p["r"] == r and p["skip_shell"] == r + 1 and p["slab_thickness"] == slab, (r, p)


@pytest.mark.parametrize("why, kw", [
    ("fp16", dict(dtype="f16")),
    ("InstanceNorm", dict(norm="instance")),
    ("GroupNorm", dict(norm="group")),
    ("BatchNorm behind the nonlinearity", dict(nonlin_first=True)),
    ("stride 2", dict(stride=2)),
    ("another skip", dict(skip_is_enc0=False)),
    ("fused head on that block", dict(head_ncls=3)),
    ("no stage-0 blocks", dict(enc0_blocks=0)),
    ("half not a multiple of 16 channels", dict(c_up=24)),
])
def test_off_by_network(ops, why, kw):
    p = ops.skip_share_plan(**BENCH, **kw)
    assert not p["skip_shared"] and p["skip_shell"] == 0, why
    # the stage-0 slabs keep today's thickness when the skip half is not shared
    if p["stage0_shared"]:
        assert p["slab_thickness"] == (4, 8, 8)


def test_off_by_geometry(ops):
    # one tile: nothing is shared
    p = ops.skip_share_plan((128, 128, 128), (128, 128, 128))
    assert not p["stage0_shared"] and not p["skip_shared"] and p["n_tiles"] == 1
    # a patch thinner than the slab of the deeper chain: stage 0 is still shared (its slab is 4 thick), the skip half is not
    thin = ops.skip_share_plan((6, 300, 300), (4, 256, 256))
    assert thin["stage0_shared"] and not thin["skip_shared"] and thin["slab_thickness"] == (4, 8, 8)
    thick = ops.skip_share_plan((12, 300, 300), (8, 256, 256))
    assert thick["skip_shared"] and thick["slab_thickness"] == (8, 8, 8)
    # one sample of a 32^3 patch does not go to conv3_f32_wino3_kernel<0, false> (128 tiles), one of 64^3 does
    assert not ops.skip_share_plan((41, 57, 43), (32, 32, 32))["skip_shared"]
    assert ops.skip_share_plan((81, 77, 90), (64, 64, 64))["skip_shared"]
    assert ops.conv3d_plan("f32", (1, 64, 64, 64), 32, 32)["kernel"] == "conv3_f32_wino3_kernel<0, false>"
    assert ops.conv3d_plan("f32", (1, 32, 32, 32), 32, 32)["kernel"] != "conv3_f32_wino3_kernel<0, false>"


def test_independent_of_batch_rank_and_world(ops):
    for geom in (BENCH, dict(volume=(81, 77, 90), patch=(64, 64, 64)), dict(volume=(41, 57, 43), patch=(32, 32, 32))):
        for mirrors in ((), (0, 1, 2)):
            base = ops.skip_share_plan(mirror_axes=mirrors, **geom)
            for bt, (rank, world) in itertools.product((0, 1, 2, 16), ((0, 1), (0, 2), (1, 2), (2, 3), (7, 8))):
                assert ops.skip_share_plan(mirror_axes=mirrors, batch_tiles=bt, rank=rank, world=world, **geom) == base
