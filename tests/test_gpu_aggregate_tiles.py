"""-m gpu: logits_aggregate_tiles_kernel (csrc/aggregate.hip) - the tiles of one forward aggregated in ONE launch - against the
sequence of per-tile launches it replaces (mi355_logits_aggregate, pinned by test_gpu_plumbing.py).

Every gate is BIT EQUALITY (np.array_equal on agg and cnt): a voxel receives the terms of the tiles that cover it in list order,
starting from the value it held, which is what the launches per tile do.

Patch 8 x 8 x 16 in a padded grid 12 x 8 x 24, tiles at (0,0,0), (4,0,0), (0,0,8), (4,0,8): voxels covered by 1, 2 and 4 tiles.  agg /
cnt start from a sentinel pattern (no zeros), so an uncovered voxel that is written, or a covered one that is not read first, shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PATCH = (8, 8, 16)
PADDED = (12, 8, 24)
TILES = [(0, 0, 0), (4, 0, 0), (0, 0, 8), (4, 0, 8)]
THREE = [(0, 0, 0), (4, 0, 0), (4, 0, 8)]     # leaves z < 4, x >= 16 uncovered
MIRRORS = {1: [0], 8: [0, 4, 2, 6, 1, 5, 3, 7]}   # the production orders (bit0 z, bit1 y, bit2 x)
PV = int(np.prod(PATCH))


def _sentinel(shape, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, shape).astype(np.float32)


def _case(gpu, n_tiles, nm, ncls, seed, gauss):
    rng = np.random.default_rng(seed)
    lg = rng.uniform(-6, 6, (n_tiles * nm, ncls, PV)).astype(np.float32)
    g = rng.uniform(0.05, 1.0, PATCH).astype(np.float32) if gauss else None
    agg, cnt = _sentinel((ncls,) + PADDED, seed + 1), _sentinel(PADDED, seed + 2)
    to = lambda a: None if a is None else torch.from_numpy(a).to(gpu)
    return to(lg), to(g), agg, cnt


def _both(amd, gpu, lg, g, agg, cnt, origins, mirrors, nonlin, with_cnt=True):
    """(agg, cnt) after one launch for all tiles, and after one launch per tile in the same order."""
    out = []
    for one_launch in (True, False):
        a, c = torch.from_numpy(agg).to(gpu), torch.from_numpy(cnt).to(gpu)
        cc = c if with_cnt else None
        if one_launch:
            amd.ops.logits_aggregate_tiles_(lg, mirrors, PATCH, nonlin, a, cc, origins, g)
        else:
            for i, o in enumerate(origins):
                amd.ops.logits_aggregate_(lg, mirrors, PATCH, nonlin, a, cc, o, g, i * len(mirrors))
        out.append((a.cpu().numpy(), c.cpu().numpy()))
    return out


def _covered(origins):
    m = np.zeros(PADDED, bool)
    for o in origins:
        m[tuple(slice(k, k + p) for k, p in zip(o, PATCH))] = True
    return m


@pytest.mark.parametrize("gauss", [True, False])
@pytest.mark.parametrize("nonlin,ncls", [("sigmoid", 3), ("softmax", 3), ("identity", 3), ("sigmoid", 1), ("softmax", 1), ("identity", 1)])
@pytest.mark.parametrize("nm", [1, 8])
def test_tiles_equal_the_sequence(amd, gpu, nm, nonlin, ncls, gauss):
    """Four tiles; 1 and 8 mirrors, 3 classes and 1, the three nonlinearities, with and without the weight map."""
    lg, g, agg, cnt = _case(gpu, len(TILES), nm, ncls, 100 + nm + ncls, gauss)
    (a1, c1), (a2, c2) = _both(amd, gpu, lg, g, agg, cnt, TILES, MIRRORS[nm], nonlin)
    assert np.array_equal(a1, a2) and np.array_equal(c1, c2)
    assert not np.array_equal(a1, agg) and not np.array_equal(c1, cnt)


@pytest.mark.parametrize("nm", [1, 8])
def test_uncovered_voxels_keep_their_values(amd, gpu, nm):
    """Three tiles whose bounding box holds voxels none of them covers: those keep the sentinel, bit for bit."""
    lg, g, agg, cnt = _case(gpu, len(THREE), nm, 3, 200 + nm, True)
    (a1, c1), (a2, c2) = _both(amd, gpu, lg, g, agg, cnt, THREE, MIRRORS[nm], "softmax")
    assert np.array_equal(a1, a2) and np.array_equal(c1, c2)
    free = ~_covered(THREE)
    assert free.any() and free[:4, :, 16:].all()
    assert np.array_equal(a1[:, free], agg[:, free]) and np.array_equal(c1[free], cnt[free])
    assert (c1[~free] != cnt[~free]).all()


def test_cnt_null(amd, gpu):
    """cnt = NULL: agg as the sequence gives it, the normaliser untouched."""
    lg, g, agg, cnt = _case(gpu, len(TILES), 8, 3, 300, True)
    (a1, c1), (a2, c2) = _both(amd, gpu, lg, g, agg, cnt, TILES, MIRRORS[8], "sigmoid", with_cnt=False)
    assert np.array_equal(a1, a2)
    assert np.array_equal(c1, cnt) and np.array_equal(c2, cnt)


def test_permuted_order_equals_the_permuted_sequence(amd, gpu):
    """The list order is the summation order: a permuted list equals the permuted sequence of launches (the logits permuted with it)."""
    nm = 8
    lg, g, agg, cnt = _case(gpu, len(TILES), nm, 3, 400, True)
    perm = [2, 0, 3, 1]
    origins = [TILES[p] for p in perm]
    lgp = lg.reshape(len(TILES), nm, 3, PV)[perm].reshape(lg.shape).contiguous()
    (a1, c1), (a2, c2) = _both(amd, gpu, lgp, g, agg, cnt, origins, MIRRORS[nm], "softmax")
    assert np.array_equal(a1, a2) and np.array_equal(c1, c2)


def test_sixty_five_tiles_run_in_chunks(amd, gpu):
    """65 tiles (the four origins in turn): the 65th runs in a second launch behind the first 64, in order."""
    origins = [TILES[i % 4] for i in range(65)]
    lg, g, agg, cnt = _case(gpu, 65, 1, 3, 500, True)
    (a1, c1), (a2, c2) = _both(amd, gpu, lg, g, agg, cnt, origins, MIRRORS[1], "sigmoid")
    assert np.array_equal(a1, a2) and np.array_equal(c1, c2)


def test_a_tile_outside_the_grid_is_refused(amd, gpu):
    lg, g, agg, cnt = _case(gpu, 2, 1, 3, 600, False)
    a, c = torch.from_numpy(agg).to(gpu), torch.from_numpy(cnt).to(gpu)
    with pytest.raises(ValueError, match="leaves the padded grid"):
        amd.ops.logits_aggregate_tiles_(lg, [0], PATCH, "identity", a, c, [(0, 0, 0), (5, 0, 8)])
    assert np.array_equal(a.cpu().numpy(), agg)
