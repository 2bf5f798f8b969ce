"""The batched radix select (``mi355_masked_percentiles_multi``): per volume of a batch, bit for bit what the single-volume call
returns, and ``np.percentile`` exactly."""
import functools
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 8192                                          # PCT_CHUNK: voxels per workgroup
SIZES = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
INF = np.inf
#: name -> (volume kind, percentiles, require, forbid, lo, hi): nq from 1 to 8, every predicate different
SPECS = {
    "A": ("negatives", (50,), 0, 0, -INF, INF),
    "B": ("dups", (0, 10, 25, 50, 75, 90, 100, 33.3), 1, 0, -INF, INF),
    "C": ("const", (5, 95), 0, 2, 0.0, INF),
    "D": ("zeros", (0, 50, 100), 4, 1, -INF, INF),
    "E": ("bits", (1, 25, 75, 99, 50), 0, 0, -1e30, 1e30),
    "F": ("negatives", (1, 2, 3, 4, 5, 6, 7), 2, 4, -50.0, 80.0),
    "G": ("dups", (15, 85, 40, 60, 20, 30), 0, 0, 0.0, 4.5),
    "H": ("bits", (0, 100, 10, 90), 8, 0, 0.0, INF),
}
BATCHES = ("A", "B", "E", "BC", "AD", "DEF", "GHC", "GHCB", "EFGH", "ABEA")   # 1, 2, 3 and 4 volumes; the last holds one volume twice


@pytest.fixture(scope="module")
def pct(amd):
    return importlib.import_module("brats_amd.percentile")


@functools.lru_cache(maxsize=None)
def host_volumes(n):
    rng = np.random.RandomState(1000 + n % 997)
    vols = {"const": np.full(n, 3.5, dtype=np.float32),
            "zeros": np.where(rng.rand(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32),
            "negatives": (rng.standard_normal(n) * 100).astype(np.float32),
            "dups": rng.randint(0, 6, size=n).astype(np.float32),            # several ranks share a group in every pass
            "bits": rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)}
    flags = rng.randint(0, 256, size=n).astype(np.uint8)
    for a in list(vols.values()) + [flags]:
        a.setflags(write=False)
    return vols, flags


@functools.lru_cache(maxsize=None)
def device_volumes(n):
    vols, flags = host_volumes(n)
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in vols.items()}, torch.from_numpy(np.array(flags)).cuda()


def selected(x, flags, require, forbid, lo, hi):
    """(the values that take part, the NaN among the flag-selected voxels) as numpy selects them"""
    f = np.zeros(x.shape, dtype=np.uint8) if flags is None else flags
    by_flags = ((f & require) == require) & ((f & forbid) == 0)
    with np.errstate(invalid="ignore"):
        inside = by_flags & (x.astype(np.float64) > lo) & (x.astype(np.float64) < hi)
    return x[inside], int(np.isnan(x[by_flags]).sum())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_batch(pct, n, names, with_flags):
    host, host_flags = host_volumes(n)
    dev, dev_flags = device_volumes(n)
    flags = dev_flags if with_flags else None
    requests = [(dev[SPECS[k][0]],) + SPECS[k][1:] for k in names]
    got = pct.masked_order_stats_multi(requests, flags)
    assert len(got) == len(names)
    for k, (count, nans, below, above) in zip(names, got):
        kind, qs, require, forbid, lo, hi = SPECS[k]
        alone = pct.masked_order_stats(dev[kind], qs, flags, require, forbid, lo, hi)
        assert (count, nans) == alone[:2], (n, names, k)
        assert np.array_equal(bits(below), bits(alone[2]), equal_nan=False) and np.array_equal(bits(above), bits(alone[3])), (n, names, k)
        values, want_nans = selected(host[kind], host_flags if with_flags else None, require, forbid, lo, hi)
        assert count == values.size and nans == want_nans, (n, names, k)
        if count:
            want = np.percentile(values.astype(np.float64), qs)
            assert np.array_equal(pct.percentile_from_order_stats(count, qs, below, above), want), (n, names, k)
        else:
            assert np.isnan(below).all() and np.isnan(above).all()
    return got


@pytest.mark.parametrize("with_flags", [True, False], ids=["flags", "no_flags"])
@pytest.mark.parametrize("n", SIZES)
def test_every_volume_of_a_batch_equals_the_single_call_and_numpy(pct, gpu, n, with_flags):
    for names in BATCHES:
        check_batch(pct, n, names, with_flags)
    # without flags a request that requires a bit selects nothing and its neighbours go on
    if not with_flags:
        got = check_batch(pct, n, "BA", False)
        assert got[0][0] == 0 and got[1][0] == n


@pytest.mark.parametrize("n", (CHUNK + 1, 2 * CHUNK + 5))
def test_a_volume_that_selects_nothing_drops_out_alone(pct, gpu, n):
    dev, flags = device_volumes(n)
    empty = (dev["negatives"], (10, 90), 0, 0, 1e37, INF)       # no value that large
    a, b = (dev["negatives"],) + SPECS["F"][1:], (dev["dups"],) + SPECS["B"][1:]
    for where in range(3):
        requests = [a, b]
        requests.insert(where, empty)
        info = {}
        got = pct.masked_order_stats_multi(requests, flags, info)
        assert info["launches"] == 4
        count, nans, below, above = got.pop(where)
        assert count == 0 and nans == 0 and np.isnan(below).all() and np.isnan(above).all() and below.shape == (2,)
        for (x, qs, require, forbid, lo, hi), g in zip((a, b), got):
            alone = pct.masked_order_stats(x, qs, flags, require, forbid, lo, hi)
            assert g[:2] == alone[:2] and g[0] > 0 and np.array_equal(bits(g[2]), bits(alone[2])) and np.array_equal(bits(g[3]), bits(alone[3]))
        values = pct.masked_percentiles_multi(requests, flags)
        assert values[where][0] == 0 and np.isnan(values[where][1]).all()
    # nothing selected anywhere: one pass, then done
    got = pct.masked_order_stats_multi([empty, empty], flags, info)
    assert [g[0] for g in got] == [0, 0] and info["launches"] == 1


def test_two_calls_are_bit_equal(pct, gpu):
    n = 2 * CHUNK + 5
    dev, flags = device_volumes(n)
    requests = [(dev[SPECS[k][0]],) + SPECS[k][1:] for k in "EFGH"]
    first, second = pct.masked_order_stats_multi(requests, flags), pct.masked_order_stats_multi(requests, flags)
    for f, s in zip(first, second):
        assert f[:2] == s[:2] and np.array_equal(bits(f[2]), bits(s[2])) and np.array_equal(bits(f[3]), bits(s[3]))


def test_nan_voxels_are_counted_aside_and_the_wrapper_raises(pct, gpu):
    n = 2 * CHUNK + 5
    host, host_flags = host_volumes(n)
    dev, flags = device_volumes(n)
    requests = [(dev["negatives"], 50), (dev["bits"], (25, 75), 8, 0, -1e30, 1e30)]
    got = pct.masked_order_stats_multi(requests, flags)
    want_nans = int(np.isnan(host["bits"][(host_flags & 8) == 8]).sum())
    assert want_nans > 0 and got[1][1] == want_nans and got[0][1] == 0       # lo / hi do not hide a NaN: it is counted aside
    with pytest.raises(ValueError, match=f"{want_nans} of the voxels the flags select are NaN"):
        pct.masked_percentiles_multi(requests, flags)
    with pytest.raises(ValueError, match=f"{want_nans} of the voxels the flags select are NaN"):
        pct.masked_percentiles(dev["bits"], (25, 75), flags, 8, 0, -1e30, 1e30)
    assert pct.masked_percentiles_multi(requests[:1], flags)[0][0] == n


def _key24(x):
    b = bits(x).astype(np.uint32)
    b = np.where(b == 0x80000000, 0, b).astype(np.uint32)
    key = np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)
    return key >> 8


def test_four_volumes_of_sixteen_live_groups_each(pct, gpu):
    """The most a pass can count: 4 volumes x 16 prefixes x 256 bins (64 KiB and 4 side counters).  Whether that is one launch or
    a pass split by volume depends on the LDS the device grants a workgroup; the results do not."""
    n = 2 * CHUNK + 5
    qs = (2, 14, 27, 40, 53, 66, 79, 92)
    rng = np.random.RandomState(77)
    host = [(np.where(rng.rand(n) < 0.5, -1.0, 1.0) * np.exp2(rng.uniform(-60, 60, size=n))).astype(np.float32) for _ in range(4)]
    for x in host:  # the sixteen order statistics differ in their first three digits: sixteen live groups in the last pass
        s = np.sort(x)
        v = (n - 1) * np.true_divide(np.asarray(qs, dtype=np.float64), 100)
        ranks = np.concatenate([np.floor(v).astype(np.int64), np.floor(v).astype(np.int64) + 1])
        assert len(set(_key24(s[ranks]).tolist())) == 16
    dev = [torch.from_numpy(x).cuda() for x in host]
    info = {}
    got = pct.masked_order_stats_multi([(x, qs) for x in dev], None, info)
    launches = info["launches"]
    assert 4 <= launches <= 4 + 3 * 3, launches     # pass 0 always fits; a split pass is at most one launch per volume
    for x, h, (count, nans, below, above) in zip(dev, host, got):
        alone = pct.masked_order_stats(x, qs)
        assert (count, nans) == alone[:2] == (n, 0)
        assert np.array_equal(bits(below), bits(alone[2])) and np.array_equal(bits(above), bits(alone[3]))
        assert np.array_equal(pct.percentile_from_order_stats(count, qs, below, above), np.percentile(h.astype(np.float64), qs))


@pytest.mark.parametrize("requests,match", [
    (lambda x, y: [], "nvol = 0"),
    (lambda x, y: [(x, 50)] * 5, "nvol = 5"),
    (lambda x, y: [(x, 50), (x, ())], "volume 1: nq = 0"),
    (lambda x, y: [(x, tuple(range(9)))], "volume 0: nq = 9"),
    (lambda x, y: [(x, 50), (x, (10, 100.5))], "volume 1: percentile 1 is 100.5"),
    (lambda x, y: [(x, -1)], "volume 0: percentile 0 is -1"),
    (lambda x, y: [(x, 50, 0, 0, float("nan"), 1.0)], "volume 0: a bound .* is NaN"),
    (lambda x, y: [(x, 50), (x, 50), (x, 50, 3, 1)], "volume 2: require 3, forbid 1"),
    (lambda x, y: [(x, 50), (y, 50)], "differ in length"),
], ids=["no_volume", "five_volumes", "nq_0", "nq_9", "percentile_above_100", "percentile_below_0", "nan_bound", "require_and_forbid", "lengths"])
def test_refusals_name_the_argument(amd, pct, gpu, requests, match):
    x, y = torch.ones(100, dtype=torch.float32, device=gpu), torch.ones(101, dtype=torch.float32, device=gpu)
    with pytest.raises(amd._lib.Mi355Error, match=match):     # every one a host-side check that returns before any launch
        pct.masked_order_stats_multi(requests(x, y))
    with pytest.raises(amd._lib.Mi355Error, match=match):
        pct.masked_percentiles_multi(requests(x, y))
