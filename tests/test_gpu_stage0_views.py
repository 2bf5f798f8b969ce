"""-m gpu: the stage-0 views (MI355_STAGE0_VIEWS, csrc/sw_share_plan.hip "stage-0 views"): the two readers of the gathered tile tensors take
every voxel outside the shells in place from the whole-volume tensor, and the gather writes the shells alone.

Views change where bytes are read, never which kernel runs nor in which order anything is summed, so EVERY comparison here is bit
equality (torch.equal / np.array_equal):
  * single ops - the stride-2 LDS-DMA conv and the addend epilogue of the F(2x2x2,3x3x3) conv, each fed a dense tensor that is NaN
    outside the shells and differs from the volume inside them, against the same kernel without a view on the input assembled on the
    host; the shell-only gather against the full gather, with a sentinel wherever it must not write; a view that leaves its tensor;
  * sliding window - the switch on against off, one child process per setting (the switch is read once per process), patch 64^3."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import plumbing_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2 = "conv3_f32_s2dma_kernel<%d>"
S2_VIEW = "conv3_f32_s2dma_kernel_view<%d>"
WINO3_ADD = "conv3_f32_wino3_kernel<3, false>"
NONE, ALL = (0,) * 6, (1,) * 6
FACE_SETS = [NONE] + [tuple(int(f == k) for f in range(6)) for k in range(6)] + [ALL]
ORIGINS = [(3, 5, 7), (0, 8, 0)]


def shell_mask(P, depth, faces):
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


def view_case(rs, vol, P, depth, face_pair):
    """Two samples cut from vol [1, Ve, C] at ORIGINS -> (dense: NaN outside the shells, fresh values inside; assembled: what the
    reader must see; the view's sample list)."""
    C = vol.shape[-1]
    dense = np.full((2,) + tuple(P) + (C,), np.nan, np.float32)
    assembled = np.empty_like(dense)
    samples = []
    for i, (o, faces) in enumerate(zip(ORIGINS, face_pair)):
        m = shell_mask(P, depth, faces)
        fresh = rs.standard_normal(tuple(P) + (C,)).astype(np.float32)
        dense[i][m] = fresh[m]
        assembled[i] = np.where(m[..., None], fresh, vol[0, o[0]:o[0] + P[0], o[1]:o[1] + P[1], o[2]:o[2] + P[2]])
        samples.append(dict(wv=0, origin=o, faces=faces))
    return dense, assembled, samples


@pytest.mark.parametrize("txl, P, Ve", [(5, (16, 16, 64), (20, 24, 72)), (4, (16, 16, 32), (20, 24, 40))])
def test_s2dma_reads_through_a_view(amd, gpu, txl, P, Ve):
    """32 -> 64, N = 2, shells 2 deep: they reach the first and last brick layer of every axis, and the wide x brick holds shell and
    view pieces in one 64-lane range.  Sample 1 carries another face set than sample 0 (the view words are per sample)."""
    rs = np.random.RandomState(40 + txl)
    vol = rs.standard_normal((1,) + Ve + (32,)).astype(np.float32)
    wt = (rs.standard_normal((64, 32, 3, 3, 3)) / np.sqrt(32 * 27)).astype(np.float32)
    b = (0.1 * rs.standard_normal(64)).astype(np.float32)
    src = torch.from_numpy(vol).to(gpu)
    for k, faces in enumerate(FACE_SETS):
        dense, assembled, samples = view_case(rs, vol, P, 2, (faces, FACE_SETS[(k + 3) % len(FACE_SETS)]))
        want = amd.ops.conv3d_s2dma_view_ndhwc(torch.from_numpy(assembled).to(gpu), wt, b, act=1)
        assert amd.ops.last_conv_kernel() == S2 % txl
        got = amd.ops.conv3d_s2dma_view_ndhwc(torch.from_numpy(dense).to(gpu), wt, b, view=(src, samples, 2), act=1)
        assert amd.ops.last_conv_kernel() == S2_VIEW % txl
        assert torch.isfinite(want).all() and torch.equal(got, want), faces


def test_addend_reads_through_a_view(amd, gpu):
    """N = 2, 8 x 16 x 16, 32 -> 32 inside a 12 x 24 x 24 S volume, shells 3 deep: low shell z < 3 and high shell z >= 5 both in D = 8."""
    rs = np.random.RandomState(50)
    P, Ve = (8, 16, 16), (12, 24, 24)
    vol = rs.standard_normal((1,) + Ve + (32,)).astype(np.float32)
    x = torch.from_numpy(rs.standard_normal((2,) + P + (32,)).astype(np.float32)).to(gpu)
    wt = (rs.standard_normal((32, 32, 3, 3, 3)) / np.sqrt(32 * 27)).astype(np.float32)
    b = (0.1 * rs.standard_normal(32)).astype(np.float32)
    src = torch.from_numpy(vol).to(gpu)
    for k, faces in enumerate(FACE_SETS):   # (both origins fit: 3 + 8 <= 12, 8 + 16 <= 24, 7 + 16 <= 24)
        dense, assembled, samples = view_case(rs, vol, P, 3, (faces, FACE_SETS[(k + 3) % len(FACE_SETS)]))
        want = amd.ops.conv3d_wino3_view_ndhwc(x, wt, b, torch.from_numpy(assembled).to(gpu), act=1)
        assert amd.ops.last_conv_kernel() == WINO3_ADD
        got = amd.ops.conv3d_wino3_view_ndhwc(x, wt, b, torch.from_numpy(dense).to(gpu), view=(src, samples, 3), act=1)
        assert amd.ops.last_conv_kernel() == WINO3_ADD
        assert torch.isfinite(want).all() and torch.equal(got, want), faces


@pytest.mark.parametrize("wide", [False, True])
def test_shell_only_gather(amd, gpu, wide):
    """Every voxel it must write equals the full gather's, every other keeps a sentinel.  plumbing_util's samples: no face, each
    single face, a corner, all six, slab indices other than 0; wide: 1088 quads per row."""
    if wide:
        w = pu.S0_WIDE
        P, t, r = w["P"], w["t"], w["r"]
        wv, slabs = pu.s0_tensors(P, t, w["Ve"], w["C"], 941, n_wv=1, n_slab=2)
        samples = [dict(wv=0, origin=(1, 3, 8), slab=[-1, -1, -1, -1, 1, 0]), dict(wv=0, origin=(2, 6, 0), slab=[1, -1, -1, 0, -1, 1]),
                   dict(wv=0, origin=(0, 0, 5), slab=[-1] * 6)]
    else:
        P, t, r = pu.S0_P, pu.S0_T, pu.S0_R
        wv, slabs = pu.s0_tensors(P, t, pu.S0_VE, pu.S0_C, 940)
        samples = pu.s0_samples()
    d_wv, d_slabs = torch.from_numpy(wv).to(gpu), [torch.from_numpy(s).to(gpu) for s in slabs]
    full = amd.ops.stage0_gather(d_wv, d_slabs, samples, P, r).cpu().numpy()
    assert full.tobytes() == pu.s0_gather_ref(wv, slabs, samples, P, t, r).tobytes()
    sentinel = np.float32(-7.25)
    out = torch.full(full.shape, float(sentinel), dtype=torch.float32, device=gpu)
    got = amd.ops.stage0_gather(d_wv, d_slabs, samples, P, r, shells_only=True, out=out).cpu().numpy()
    for i, sm in enumerate(samples):
        m = shell_mask(P, r, [f >= 0 for f in sm["slab"]])
        assert got[i][m].tobytes() == full[i][m].tobytes(), i
        assert (got[i][~m] == sentinel).all(), i


def test_a_view_that_leaves_its_tensor_is_refused(amd, gpu):
    rs = np.random.RandomState(60)
    src = torch.from_numpy(rs.standard_normal((1, 20, 24, 72, 32)).astype(np.float32)).to(gpu)
    x = torch.zeros((1, 16, 16, 64, 32), device=gpu)
    wt = np.zeros((64, 32, 3, 3, 3), np.float32)
    for origin in ((5, 0, 0), (0, 9, 0), (0, 0, 9), (-1, 0, 0)):
        with pytest.raises(amd._lib.Mi355Error, match="leaves its tensor"):
            amd.ops.conv3d_s2dma_view_ndhwc(x, wt, None, view=(src, [dict(wv=0, origin=origin, faces=NONE)], 2))
    with pytest.raises(amd._lib.Mi355Error, match="whole-volume index"):
        amd.ops.conv3d_s2dma_view_ndhwc(x, wt, None, view=(src, [dict(wv=1, origin=(0, 0, 0), faces=NONE)], 2))
    a = torch.zeros((1, 8, 16, 16, 32), device=gpu)
    s = torch.zeros((1, 12, 24, 24, 32), device=gpu)
    with pytest.raises(amd._lib.Mi355Error, match="leaves its tensor"):
        amd.ops.conv3d_wino3_view_ndhwc(a, np.zeros((32, 32, 3, 3, 3), np.float32), None, a, view=(s, [dict(wv=0, origin=(5, 0, 0), faces=ALL)], 3))


def test_a_view_beyond_the_32_bit_offsets_is_refused(amd, gpu):
    """The readers form a piece's element offset from its tile's corner in 32 bits: at most 8 rows-of-planes of the source, so a
    source plane of 2^23 voxels x 32 channels is one too large.  The source is only allocated (8 GiB, never written or read: the
    call is refused before anything is launched); the sample itself lies inside it."""
    a = torch.zeros((1, 8, 16, 16, 32), device=gpu)
    s = torch.empty((1, 8, 4096, 2048, 32), dtype=torch.float32, device=gpu)
    with pytest.raises(amd._lib.Mi355Error, match="exceeds the 32-bit offsets"):
        amd.ops.conv3d_wino3_view_ndhwc(a, np.zeros((32, 32, 3, 3, 3), np.float32), None, a, view=(s, [dict(wv=0, origin=(0, 0, 0), faces=ALL)], 3))
    del s


# ------------------------------------------------------------------ sliding window
PATCH = (64, 64, 64)
# as tests/test_gpu_skip_sharing.py: faces has tiles with two interior z faces, odd a zero-extended volume (81, 77, 90) -> (84, 80,
# 96), mirror the 8-way mirrors, ranks deals the tiles over world = 2
CASES = {"faces": ((100, 80, 72), False, 1), "odd": ((81, 77, 90), False, 1), "mirror": ((72, 80, 72), True, 1), "ranks": ((81, 77, 90), False, 2)}

CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
from brats_amd import predictor
path, cases = sys.argv[1], eval(sys.argv[2])
patch = (64, 64, 64)
out = {}
sd, meta = brats_amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
net = brats_amd.UNet(sd, norm="batch")
for name, (shape, mirror, world) in sorted(cases.items()):
    vol = np.random.RandomState(70 + len(name)).standard_normal((4,) + tuple(shape)).astype(np.float32)
    net.profile(True)
    if world == 1:
        out[name] = predictor.predict_folds([net], vol, patch, 0.5, mirror, (0, 1, 2), True, "sigmoid").cpu().numpy()
    else:
        parts = [predictor.predict_tile_sharded(net, vol, r, world, patch, 0.5, mirror) for r in range(world)]
        agg = parts[0][0].clone()
        for r in range(1, world):
            agg += parts[r][0]
        out[name] = predictor.finish_sharded(agg, parts[0][1], vol.shape[1:], patch).cpu().numpy()
    prof = net.read_profile()
    net.profile(False)
    out[name + "_kernels"] = np.array([e["name"] for e in prof])
    out[name + "_bytes"] = np.array([e["bytes"] for e in prof])
np.savez(path, **out)
"""


@pytest.fixture(scope="module")
def runs(amd, gpu):
    """(views, share skip conv) -> results.  The two settings with the skip half not shared run one case."""
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for views, share in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
            cases = CASES if share == "1" else {"faces": CASES["faces"]}
            path = os.path.join(td, f"v{views}s{share}.npz")
            res = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, repr(cases)],
                                 env=dict(os.environ, MI355_STAGE0_VIEWS=views, MI355_SHARE_SKIP_CONV=share), capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
            with np.load(path) as z:
                outs[(views, share)] = {k: z[k] for k in z.files}
    return outs


@pytest.mark.parametrize("name", sorted(CASES))
def test_views_on_equals_off(runs, name):
    on, off = runs[("1", "1")], runs[("0", "1")]
    assert np.isfinite(on[name]).all() and np.array_equal(on[name], off[name])


def test_views_without_the_shared_skip_half(runs):
    """The concat conv then reads the level-0 features whole, as in1: nothing is viewed and nothing changes."""
    on, off = runs[("1", "0")], runs[("0", "0")]
    assert np.array_equal(on["faces"], off["faces"])
    assert [str(k) for k in on["faces_kernels"]] == [str(k) for k in off["faces_kernels"]]
    assert not [k for k in on["faces_kernels"] if "_view" in str(k)]
    g = [str(k) for k in on["faces_kernels"]].index("stage0_gather_kernel")
    assert float(on["faces_bytes"][g]) == float(off["faces_bytes"][g])


@pytest.mark.parametrize("name", sorted(CASES))
def test_profile_shows_the_views(amd, runs, name):
    on, off = runs[("1", "1")], runs[("0", "1")]
    shape, mirror, world = CASES[name]
    k_on, k_off = [str(k) for k in on[name + "_kernels"]], [str(k) for k in off[name + "_kernels"]]
    b_on, b_off = float(on[name + "_bytes"][k_on.index("stage0_gather_kernel")]), float(off[name + "_bytes"][k_off.index("stage0_gather_kernel")])
    print(f"stage-0 views {name}: gather bytes {b_off:.3e} -> {b_on:.3e}")
    assert b_on < b_off          # S is viewed whenever the skip half is shared
    assert not [k for k in k_off if "_view" in k]
    # the level-0 features: viewed iff the planner sends a forward of this many samples to the stride-2 LDS-DMA kernel
    axes = (0, 1, 2) if mirror else ()
    geom = amd.ops.stage0_view_plan(shape, PATCH, 0.5, axes)
    tiles_here = -(-geom["n_tiles"] // world)
    per_forward = min(tiles_here, max(1, 16 // geom["n_mirrors"])) * geom["n_mirrors"]
    plan = amd.ops.stage0_view_plan(shape, PATCH, 0.5, axes, batch_samples=per_forward)
    viewed = [k for k in k_on if k.startswith("conv3_f32_s2dma_kernel_view<")]
    if plan["enc0_viewed"]:
        assert viewed == [S2_VIEW % 5], k_on
        full = 2.0 * 4.0 * geom["n_tiles"] * geom["n_mirrors"] * 64 ** 3 * (32 + 32)
        shells = 2.0 * 4.0 * 32 * sum(s["shell_voxels"][0] + s["shell_voxels"][1] for s in geom["samples"])
        assert b_off == full and b_on == shells, (b_off, full, b_on, shells)
    else:   # the fallback: the full gather for that tensor, the plain kernel, the same result (test_views_on_equals_off)
        assert not viewed, k_on
