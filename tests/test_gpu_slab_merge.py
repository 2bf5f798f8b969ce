"""-m gpu: the merged stage-0 slabs (MI355_MERGE_SLABS, csrc/sw_share_plan.hip "merged slabs").

* The gather in its general form (mi355_stage0_gather_merged, and its shells-only form) against a numpy model on CODED tensors:
  every element's value names its source tensor and its flat index there, all below 2^24, so the result is exact and a wrong
  slab, offset or precedence shows as another code.  Geometry: patch 16^3, slabs 8 thick, r = 2 for the first tensor (C = 4) and
  r2 = 3 for the second (C2 = 8), volume (24, 32, 24) with tiles at (0, 8) x (0, 8, 16) x (0, 8) - the plan of that volume, two
  mirrors -, per-tile z-slabs, y-slabs that span z, x-slabs that span z and y.  Guard bands around both outputs.
* The network with the switch on against off (5e-5 on probabilities: the suite's bound for another summation order), both against
  the CPU oracle (1e-3, Dice >= 0.999), and three-rank tile-sharded against unsharded (2e-6, one tile per forward on both sides,
  as in test_gpu_stage0_sharing.py).  The switch is read once per process: one child process per setting, once per module.
  The bench-geometry shapes are run by test_gpu_stage0_sharing.py::test_bench_geometry, which takes the default path."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import tiler_ref, unet_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------ gather
P, T, R, R2, C, C2 = (16, 16, 16), (8, 8, 8), 2, 3, 4, 8
VE = (24, 32, 24)
GUARD = 4096
SENTINEL = -7.0


def _coded(shape, source):
    n = int(np.prod(shape))
    assert n < 1 << 21
    return (np.arange(n, dtype=np.float32) + np.float32(source << 21)).reshape(shape)


def _case(amd):
    p = amd.ops.stage0_merge_plan(VE, P, 0.5, (0,), 2, True)
    assert p["volume"] == VE and p["slab_thickness"] == T and (p["r"], p["rs"]) == (R, R2) and p["n_mirrors"] == 2
    assert sorted({s["origin"] for s in p["samples"]}) == sorted((z, y, x) for z in (0, 8) for y in (0, 8, 16) for x in (0, 8))
    samples = []
    nz = 0
    for i, s in enumerate(p["samples"]):
        slab = list(s["slab"])
        for f in (0, 1):   # the per-tile z-slabs, numbered as a forward numbers them
            if slab[f] >= 0:
                slab[f] = nz
                nz += 1
        samples.append({"wv": i % 2, "origin": s["origin"], "slab": slab, "offset": s["offset"]})
    shapes = [(nz, T[0], P[1], P[2]), (p["n_slabs"][1], VE[0], T[1], P[2]), (p["n_slabs"][2], VE[0], VE[1], T[2])]
    assert nz == 24 and p["n_slabs"][1] == 16 and p["n_slabs"][2] == 4
    first = {"wv": _coded((2,) + VE + (C,), 0), "slabs": [_coded(sh + (C,), 1 + a) for a, sh in enumerate(shapes)]}
    second = {"wv": _coded((2,) + VE + (C2,), 4), "slabs": [_coded(sh + (C2,), 5 + a) for a, sh in enumerate(shapes)]}
    return samples, first, second


def _model(samples, t, depth, before=None):
    """The gather of one tensor in numpy; before: the output's previous content - then only the shell voxels are written."""
    ch = t["wv"].shape[-1]
    out = np.empty((len(samples),) + P + (ch,), np.float32)
    for n, s in enumerate(samples):
        o = s["origin"]
        full = t["wv"][s["wv"], o[0]:o[0] + P[0], o[1]:o[1] + P[1], o[2]:o[2] + P[2]].copy()
        shell = np.zeros(P, bool)
        for f in (5, 4, 3, 2, 1, 0):   # z before y before x: the winner is written last
            if s["slab"][f] < 0:
                continue
            a, side = f >> 1, f & 1
            off = s["offset"].get(f, (0, 0, 0))
            dst, src = [slice(None)] * 3, [slice(off[k], off[k] + P[k]) for k in range(3)]
            dst[a] = slice(P[a] - depth, P[a]) if side else slice(0, depth)
            src[a] = slice(off[a] + T[a] - depth, off[a] + T[a]) if side else slice(off[a], off[a] + depth)
            full[tuple(dst)] = t["slabs"][a][s["slab"][f]][tuple(src)]
            shell[tuple(dst)] = True
        out[n] = full if before is None else np.where(shell[..., None], full, before[n])
    return out


SPANS = [(0, 0, 0), (1, 0, 0), (1, 1, 0)]


@pytest.mark.parametrize("shells_only", [False, True])
def test_gather_merged_on_coded_tensors(amd, gpu, shells_only):
    samples, first, second = _case(amd)
    dev = lambda a: torch.from_numpy(a).to(gpu)
    n = len(samples)
    bufs, outs = [], []
    for ch in (C, C2):
        size = n * int(np.prod(P)) * ch
        b = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=gpu)
        bufs.append(b)
        outs.append(b[GUARD:GUARD + size].view((n,) + P + (ch,)))
    before = [o.cpu().numpy() for o in outs]
    got = amd.ops.stage0_gather_merged(dev(first["wv"]), [dev(s) for s in first["slabs"]], samples, P, R, SPANS, shells_only, outs[0],
                                       {"wv": dev(second["wv"]), "slabs": [dev(s) for s in second["slabs"]], "r": R2, "out": outs[1]})
    for i, (t, depth) in enumerate(((first, R), (second, R2))):
        want = _model(samples, t, depth, before[i] if shells_only else None)
        assert np.array_equal(got[i].cpu().numpy(), want), f"tensor {i}, shells_only {shells_only}"
        flat = bufs[i].cpu().numpy()
        assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), f"tensor {i}: a guard band was written"
    if shells_only:   # every sample here has interior faces, and none is all shell
        assert all((got[0][k] != SENTINEL).any() and (got[0][k] == SENTINEL).any() for k in range(n))


def test_gather_merged_equals_the_dense_entry_point(amd, gpu):
    """With no spanning axis the general form is mi355_stage0_gather: same samples, per-tile slabs on all three axes."""
    rng = np.random.default_rng(3)
    wv = torch.from_numpy(rng.standard_normal((1,) + VE + (C,)).astype(np.float32)).to(gpu)
    samples = [{"wv": 0, "origin": (8, 8, 0), "slab": [0, -1, 0, 1, -1, 0]}, {"wv": 0, "origin": (0, 16, 8), "slab": [-1, 1, 2, -1, 1, -1]}]
    counts = (2, 3, 2)
    slabs = [torch.from_numpy(rng.standard_normal((counts[a],) + tuple(T[k] if k == a else P[k] for k in range(3)) + (C,)).astype(np.float32)).to(gpu)
             for a in range(3)]
    want = amd.ops.stage0_gather(wv, slabs, samples, P, R)
    got, _ = amd.ops.stage0_gather_merged(wv, slabs, samples, P, R, [(0, 0, 0)] * 3)
    assert torch.equal(got, want)


def test_gather_merged_refuses_a_wrong_slab_shape(amd, gpu):
    samples, first, _ = _case(amd)
    dev = lambda a: torch.from_numpy(a).to(gpu)
    slabs = [dev(s) for s in first["slabs"]]
    with pytest.raises(ValueError, match="shape"):   # y-slabs that span z, declared as tile-sized
        amd.ops.stage0_gather_merged(dev(first["wv"]), slabs, samples, P, R, [(0, 0, 0), (0, 0, 0), (1, 1, 0)])
    with pytest.raises(amd._lib.Mi355Error, match="extent"):   # a slab cannot span its own axis
        amd.ops.stage0_gather_merged(dev(first["wv"]), slabs, samples, P, R, [(0, 0, 0), (1, 1, 0), (1, 1, 0)])


# ------------------------------------------------------------------ network
PATCH = (32, 32, 32)
# (41, 57, 43): odd offsets, a middle tile with two interior y faces; (40, 56, 44): 8 mirrors; (32, 32, 32): one tile, no keys
CASES = {"odd": ((41, 57, 43), False), "mirror": ((40, 56, 44), True), "single": ((32, 32, 32), False)}

CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
import brats_amd
from brats_amd import predictor
path, cases = sys.argv[1], eval(sys.argv[2])
patch = (32, 32, 32)
out = {}
sd, meta = brats_amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
net = brats_amd.UNet(sd, norm="batch")
for i, (name, (shape, mirror)) in enumerate(sorted(cases.items())):
    vol = np.random.RandomState(60 + i).standard_normal((4,) + tuple(shape)).astype(np.float32)
    net.profile(True)
    out[name] = predictor.predict_folds([net], vol, patch, 0.5, mirror, (0, 1, 2), True, "sigmoid").cpu().numpy()
    out[name + "_kernels"] = np.array(sorted(e["name"] for e in net.read_profile()))
    net.profile(False)
    parts = [predictor.predict_tile_sharded(net, vol, r, 3, patch, 0.5, False, batch_tiles=1) for r in range(3)]
    agg = parts[0][0].clone()
    for r in (1, 2):
        agg += parts[r][0]
    out[name + "_sharded"] = predictor.finish_sharded(agg, parts[0][1], vol.shape[1:], patch).cpu().numpy()
    out[name + "_whole"] = predictor.predict_folds([net], vol, patch, 0.5, False, (0, 1, 2), True, "sigmoid", batch_tiles=1).cpu().numpy()
np.savez(path, **out)
"""


@pytest.fixture(scope="module")
def runs(amd, gpu):
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for flag in ("1", "0"):
            path = os.path.join(td, f"m{flag}.npz")
            res = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, repr(CASES)], env=dict(os.environ, MI355_MERGE_SLABS=flag),
                                 capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
            with np.load(path) as z:
                outs[flag] = {k: z[k] for k in z.files}
    return outs["1"], outs["0"]


@pytest.fixture(scope="module")
def oracle(amd):
    sd, meta = amd.synthetic.make_model("A", seed=21, num_pool=2, max_feat=128)
    fn = tiler_ref.make_net_fn(sd, unet_ref.default_cfg("batch"))
    refs = {}
    for i, (name, (shape, mirror)) in enumerate(sorted(CASES.items())):
        vol = np.random.RandomState(60 + i).standard_normal((4,) + shape).astype(np.float32)
        refs[name] = tiler_ref.predict_3d_tiled(fn, vol, PATCH, 3, 0.5, mirror, (0, 1, 2), True, "sigmoid")
    return refs


@pytest.mark.parametrize("name", sorted(CASES))
def test_merged_matches_per_tile_and_oracle(runs, oracle, name):
    on, off = runs
    merged = "extract_tiles_kernel merged-slabs"   # the profile entry of the merged slabs' input gather
    assert (merged in list(on[name + "_kernels"])) == (name != "single"), list(on[name + "_kernels"])
    assert merged not in list(off[name + "_kernels"])
    d = float(np.abs(on[name] - off[name]).max())
    e_on, e_off = (float(np.abs(x[name] - oracle[name]).max()) for x in (on, off))
    print(f"merged slabs {name}: on vs off {d:.2e}, on vs oracle {e_on:.2e}, off vs oracle {e_off:.2e}")
    assert d <= 5e-5
    for got, err in ((on[name], e_on), (off[name], e_off)):
        assert err <= 1e-3
        dice = tiler_ref.brats_region_dice(tiler_ref.regions_to_labels(got), tiler_ref.regions_to_labels(oracle[name]))
        assert dice["mean"] >= 0.999


def test_tile_sharded_matches_unsharded(runs):
    """Every rank computes all merged slabs in launches of the same size, whatever tiles it holds: three ranks against the unsharded
    call within 2e-6, one tile per forward on both sides (see test_gpu_stage0_sharing.py for why)."""
    for run, sw in zip(runs, ("on", "off")):
        for name in sorted(CASES):
            d = float(np.abs(run[name + "_sharded"] - run[name + "_whole"]).max())
            print(f"merged slabs {sw} {name}: 3 ranks vs unsharded {d:.2e}")
            assert d <= 2e-6, (sw, name)
