"""The stage-0 views (MI355_STAGE0_VIEWS, csrc/sw_share_plan.hip "stage-0 views"), checked without a device: the dry-run entry point
mi355_stage0_view_plan - the decision and descriptor code a real mi355_sw_predict call runs - and, in numpy, the rule the readers
implement: a voxel comes from the tile tensor iff it lies within the shell depth of a face whose bit is set, from the view otherwise.
That rule must be SUFFICIENT: with the tile tensor poisoned everywhere else, the assembled tile equals the full gather's."""
import numpy as np
import pytest

import plumbing_util as pu

BENCH = dict(volume=(139, 172, 138), patch=(128, 128, 128))


@pytest.fixture(scope="module")
def ops(amd):
    return amd.ops


def test_bench_geometry_views_both_tensors(ops):
    p = ops.stage0_view_plan(**BENCH)
    assert p["enc0_viewed"] and p["half_viewed"]
    assert p["depth"] == (2, 3) and p["n_tiles"] == 8 and p["n_mirrors"] == 1 and p["volume"] == (140, 176, 144)
    assert len(p["samples"]) == 8
    # every tile has one interior face per axis: 128^3 - 126^3 and 128^3 - 125^3 voxels
    assert all(s["shell_voxels"] == (96776, 144027) for s in p["samples"])
    assert all(sum(s["faces"][2 * a:2 * a + 2]) == 1 for s in p["samples"] for a in range(3))
    origins = [(z, y, x) for z in (0, 11) for y in (0, 44) for x in (0, 10)]
    assert [s["offset"] for s in p["samples"]] == [(z * 176 + y) * 144 + x for z, y, x in origins]
    # the face bits are the interior faces: a tile at origin 0 has its high face inside the volume, the other its low face
    for s, o in zip(p["samples"], origins):
        assert s["faces"] == tuple(f for a in range(3) for f in ((0, 1) if o[a] == 0 else (1, 0)))


@pytest.mark.parametrize("axes", [(), (0,), (0, 1, 2)])
def test_mirrored_origins_match_stage0_plan(ops, axes):
    volume, patch = (100, 80, 72), (64, 64, 64)
    v = ops.stage0_view_plan(volume, patch, mirror_axes=axes)
    s0 = ops.stage0_plan(volume, patch, 0.5, axes, 2)
    ve = v["volume"]
    assert v["half_viewed"] and len(v["samples"]) == len(s0["samples"]) == v["n_tiles"] * v["n_mirrors"]
    for i, (a, b) in enumerate(zip(v["samples"], s0["samples"])):
        m = i % v["n_mirrors"]   # samples are tile-major; the mirror's index is its whole-volume result
        o = b["origin"]
        assert a["offset"] == ((m * ve[0] + o[0]) * ve[1] + o[1]) * ve[2] + o[2]
        assert a["faces"] == b["face"]
        assert all(o[k] >= 0 and o[k] + patch[k] <= ve[k] for k in range(3))
    # (100, 80, 72) has tiles with two interior z faces
    assert any(s["faces"][0] and s["faces"][1] for s in v["samples"])


def test_no_view_without_sharing(ops):
    one = ops.stage0_view_plan((128, 128, 128), (128, 128, 128))
    assert not one["enc0_viewed"] and not one["half_viewed"] and one["samples"] == []
    for kw in (dict(norm="instance"), dict(dtype="f16"), dict(head_ncls=3), dict(skip_is_enc0=False)):
        p = ops.stage0_view_plan(**BENCH, **kw)
        assert not p["enc0_viewed"] and not p["half_viewed"], kw


def test_the_batch_decides_the_level0_view_only(ops):
    """One sample of 64^3 is too small a launch for the stride-2 LDS-DMA kernel: the level-0 features keep the full gather, S is
    viewed all the same (its reader does not depend on the batch)."""
    small = ops.stage0_view_plan((100, 80, 72), (64, 64, 64), batch_samples=1)
    assert small["half_viewed"] and not small["enc0_viewed"]
    conv = ops.conv3d_plan("f32", (1, 64, 64, 64), 32, 64, stride=2)
    assert "s2dma" not in conv["kernel"]
    full = ops.stage0_view_plan(**BENCH, batch_samples=8)
    assert full["enc0_viewed"] and "s2dma" in ops.conv3d_plan("f32", (8, 128, 128, 128), 32, 64, stride=2)["kernel"]


def shell_mask(P, depth, faces):
    """the readers' rule: within `depth` of a face whose flag is set"""
    m = np.zeros(P, bool)
    for a in range(3):
        idx = [slice(None)] * 3
        if faces[2 * a]:
            idx[a] = slice(0, depth)
            m[tuple(idx)] = True
        if faces[2 * a + 1]:
            idx[a] = slice(P[a] - depth, P[a])
            m[tuple(idx)] = True
    return m


def view_read(wv, sample, P):
    """the tile read in place from the whole-volume tensor, as the kernels address it: origin offset + (z * sz + y * sy + x) voxels"""
    Ve = wv.shape[1:4]
    flat = wv.reshape(-1, wv.shape[-1])
    o = sample["origin"]
    off = ((sample["wv"] * Ve[0] + o[0]) * Ve[1] + o[1]) * Ve[2] + o[2]
    sy, sz = Ve[2], Ve[1] * Ve[2]
    z, y, x = np.meshgrid(*(np.arange(p) for p in P), indexing="ij")
    return flat[off + z * sz + y * sy + x]


def test_shells_are_sufficient():
    """plumbing_util's hand-built samples: no face, each face alone, a corner, all six (two interior faces on every axis).  Inside the
    shells the assembled tile is the gather's own output by construction; what this checks is the other half: every voxel OUTSIDE
    the shells, read in place from the whole-volume tensor, is what the full gather would have copied there."""
    P, t, r = pu.S0_P, pu.S0_T, pu.S0_R
    wv, slabs = pu.s0_tensors(P, t, pu.S0_VE, pu.S0_C, 930)
    samples = pu.s0_samples()
    ref = pu.s0_gather_ref(wv, slabs, samples, P, t, r)
    assert any(all(f < 0 for f in s["slab"]) for s in samples) and any(s["slab"][0] >= 0 and s["slab"][1] >= 0 for s in samples)
    for i, sm in enumerate(samples):
        m = shell_mask(P, r, [f >= 0 for f in sm["slab"]])
        dense = np.where(m[..., None], ref[i], np.float32(np.nan))   # what a shell-only gather leaves: poison outside the shells
        tile = np.where(m[..., None], dense, view_read(wv, sm, P))
        assert tile.tobytes() == ref[i].tobytes(), i


@pytest.mark.parametrize("volume, patch", [((100, 64, 72), (64, 64, 64)), ((100, 80, 72), (64, 64, 64)), ((139, 172, 138), (128, 128, 128))])
def test_shell_counts_are_the_size_of_the_readers_mask(ops, volume, patch):
    """What the dry run reports as written by the gather is the size of the mask the readers apply, for both depths: samples with no
    interior face on an axis (one tile along y in the first volume), with one, and with two (the middle z tiles of the first two)."""
    p = ops.stage0_view_plan(volume, patch)
    assert p["half_viewed"] and p["depth"] == (2, 3)
    per_axis = {sum(s["faces"][2 * a:2 * a + 2]) for s in p["samples"] for a in range(3)}
    assert per_axis == ({0, 1, 2} if volume[1] == 64 else {1, 2} if volume[0] == 100 else {1})
    for s in p["samples"]:
        assert s["shell_voxels"] == tuple(int(shell_mask(patch, d, s["faces"]).sum()) for d in p["depth"]), s
