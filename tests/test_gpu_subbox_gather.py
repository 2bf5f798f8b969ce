"""-m gpu: MI355_SUBBOX_GATHER - the dense gather of SUB-BOXES (the 2 t1 outermost level-0 layers of a tile, from which the shared
level 1 computes a level-1 slab) launched over the boxes that are written (stage0_gather_box_kernel) instead of over every row of the
whole volume - against the launch it replaces, bit for bit.

Through mi355_stage0_gather_boxes, by_box = 1 against 0 (the kernel as it was), on two tiles of 16 x 24 x 32 voxels in a
20 x 32 x 40 volume, 32 channels, slabs 8 thick, r = 2.  Sources and precedence are per voxel - the first shell that holds it, z
before y before x, else the whole volume -, so the comparison is equality of bytes; the destination is NaN before the launch and
sits between NaN guard bands, so a voxel that must not be written shows, and one that is not written although it must does too
(the reference wrote it).  The shells-only form of the same entry (one launch form) writes exactly the shells of sub-boxes.
  * x0: sub-boxes 8 wide at x = 0 of their tiles, the far x face a cut; tile B with shells on all three axes;
  * xfar: sub-boxes 12 wide at the far x face (96 quads per row: a workgroup's rows are no whole pass of its lanes, and the last
    workgroup is ragged); tile A with shells on all three axes;
  * y: sub-boxes 8 rows thick along y, whole rows of x (256 quads per row)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, VE, THICK, R, C = (16, 24, 32), (20, 32, 40), (8, 8, 8), 2, 32
A, B = (0, 0, 0), (4, 8, 8)   # the tiles' origins: A touches the volume's low faces, B its high z face
GUARD = 8192
SPANS = [(0, 0, 0)] * 3

# name: (box extent, [sample: tile origin, offset of the box in the tile, slab indices (z lo, z hi, y lo, y hi, x lo, x hi) or -1])
CASES = {
    "x0": ((16, 24, 8), [(A, (0, 0, 0), [-1, 1, -1, 0, -1, -1]), (B, (0, 0, 0), [0, -1, 2, -1, 1, -1])]),
    "xfar": ((16, 24, 12), [(A, (0, 0, 20), [-1, 2, -1, 1, -1, 0]), (B, (0, 0, 20), [1, -1, 0, -1, -1, -1])]),
    "y": ((16, 8, 32), [(A, (0, 16, 0), [-1, 0, -1, 2, -1, 1]), (B, (0, 0, 0), [2, -1, 1, -1, 0, -1])]),
}


@pytest.fixture(scope="module")
def tensors(gpu):
    """whole volume and three slabs per axis (tile-sized across their axis), shared by every case and left unchanged"""
    rng = np.random.default_rng(17)
    dev = lambda shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(gpu)  # noqa: E731
    slabs = [dev((3,) + tuple(THICK[k] if k == a else T[k] for k in range(3)) + (C,)) for a in range(3)]
    return {"wv": dev((1,) + VE + (C,)), "slabs": slabs}


def _samples(case):
    P, boxes = CASES[case]
    return P, [dict(wv=0, origin=tuple(o + s for o, s in zip(org, sub)), sub=sub, slab=slab) for org, sub, slab in boxes]


def _poisoned(gpu, n, P, ch):
    size = n * int(np.prod(P)) * ch
    buf = torch.full((size + 2 * GUARD,), float("nan"), dtype=torch.float32, device=gpu)
    return buf, buf[GUARD:GUARD + size].view((n,) + tuple(P) + (ch,))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", sorted(CASES))
def test_box_launch_equals_the_row_launch(amd, gpu, tensors, case):
    P, samples = _samples(case)
    got = {}
    for by_box in (False, True):
        buf, out = _poisoned(gpu, len(samples), P, C)
        amd.ops.stage0_gather_merged(tensors["wv"], tensors["slabs"], samples, P, R, SPANS, False, out, tile=T, by_box=by_box)
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), "a guard band was written"
        got[by_box] = out
    assert torch.isfinite(got[False]).all()   # (the row form wrote every voxel of the boxes)
    assert torch.equal(_bits(got[True]), _bits(got[False]))
    # and the values are the sources': a voxel in no shell is the whole volume's, one in the first shell of the order its slab's
    for i, sm in enumerate(samples):
        o = sm["origin"]
        inner = tuple(slice(R if sm["slab"][2 * a] >= 0 else 0, P[a] - (R if sm["slab"][2 * a + 1] >= 0 else 0)) for a in range(3))
        vol = tensors["wv"][0, o[0]:o[0] + P[0], o[1]:o[1] + P[1], o[2]:o[2] + P[2]]
        assert torch.equal(got[True][i][inner], vol[inner]), (case, i)
        f = next(f for f in range(6) if sm["slab"][f] >= 0)   # the winning face: the whole of its shell comes from its slab
        a, side = f >> 1, f & 1
        dst = [slice(None)] * 3
        dst[a] = slice(P[a] - R, P[a]) if side else slice(0, R)
        src = [slice(sm["sub"][k], sm["sub"][k] + P[k]) for k in range(3)]
        src[a] = slice(THICK[a] - R, THICK[a]) if side else slice(0, R)
        assert torch.equal(got[True][i][tuple(dst)], tensors["slabs"][a][sm["slab"][f]][tuple(src)]), (case, i, f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_shells_of_sub_boxes(amd, gpu, tensors, case):
    """The shells-only form on sub-boxes: written are exactly the voxels within r of a face with a slab, with the dense gather's values."""
    P, samples = _samples(case)
    _, dense = _poisoned(gpu, len(samples), P, C)
    amd.ops.stage0_gather_merged(tensors["wv"], tensors["slabs"], samples, P, R, SPANS, False, dense, tile=T, by_box=True)
    buf, out = _poisoned(gpu, len(samples), P, C)
    amd.ops.stage0_gather_merged(tensors["wv"], tensors["slabs"], samples, P, R, SPANS, True, out, tile=T)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), "a guard band was written"
    for i, sm in enumerate(samples):
        shell = np.zeros(P, bool)
        for f in range(6):
            if sm["slab"][f] >= 0:
                idx = [slice(None)] * 3
                idx[f >> 1] = slice(P[f >> 1] - R, P[f >> 1]) if f & 1 else slice(0, R)
                shell[tuple(idx)] = True
        m = torch.from_numpy(shell).to(gpu)
        assert torch.isnan(out[i][~m]).all() and torch.equal(out[i][m], dense[i][m]), (case, i)
