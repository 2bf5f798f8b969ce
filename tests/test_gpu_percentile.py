"""Exact masked order statistics on the MI355X (csrc/percentile.hip): the two order statistics that bracket a
percentile equal np.sort's as float32 bits, the percentile equals np.percentile of the float64 copy with ==, the selection
equals a numpy mask, two calls are bit-equal, and everything the entry point refuses is refused before it writes."""
import ctypes as C

import numpy as np
import pytest
import torch

import sequence_findings_util as su

pytestmark = pytest.mark.gpu

QS8 = (0, 5, 10, 25, 50, 85, 99, 100)      # eight percentiles in one call
SINGLES = (20, 33.3, 100)                  # one per call
LENGTHS = (1, 2, 63, 64, 65, 257, 4099, 48 * 56 * 40, 97 * 61 * 53)
INF = float("inf")


@pytest.fixture(scope="module")
def pct(amd):
    return su.module("percentile")


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def brats_like(rs, n):
    """integer intensities with an exact-zero background (selected with lo = 0)"""
    return (rs.randint(1, 4000, n) * (rs.random_sample(n) < 0.6)).astype(np.float32)


def constant(rs, n):
    return np.full(n, 1234.5, dtype=np.float32)


def low_byte(rs, n):
    """two values that differ only in the lowest byte of the key"""
    return _bits(0x447A0000 + rs.randint(0, 2, n).astype(np.uint32))


def top_byte(rs, n):
    """values that differ only in the top byte of the key, both signs (bit 23 is clear: every pattern is finite)"""
    tops = np.array([0x00, 0x3F, 0x40, 0x7F, 0x80, 0xBF, 0xC0, 0xFF], dtype=np.uint32)
    return _bits((tops[rs.randint(0, 8, n)] << 24) | 0x123456)


def random_bits(rs, n):
    """uniform random finite bit patterns: every digit is live; negatives, denormals, +-inf and both zeros among them"""
    u = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    u[(u & 0x7F800000) == 0x7F800000] &= np.uint32(0xFF7FFFFF)  # no NaN (and no inf but the two put in below)
    if n >= 64:
        u[3:11] = [0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x80000000, 0x00000000]
        u[40:44] = [0x80000000, 0x00000000, 0x80000000, 0x00000001]
    return _bits(u)


CONTENTS = {"brats_like": (brats_like, 0.0), "constant": (constant, -INF), "low_byte": (low_byte, -INF), "top_byte": (top_byte, -INF),
            "random_bits": (random_bits, -INF)}


def _select(x, flags=None, require=0, forbid=0, lo=-INF, hi=INF):
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = (lo < x64) & (x64 < hi)
    if flags is not None:
        keep &= ((flags & require) == require) & ((flags & forbid) == 0)
    return x[keep]


def _check(pct, gpu, x, what, flags=None, singles=SINGLES, qs=QS8, **sel):
    selected = _select(x, flags, **sel)
    dx, dflags = _dev(x, gpu), None if flags is None else _dev(flags, gpu)
    count, nans, below, above = pct.masked_order_stats(dx, qs, dflags, **sel)
    assert (count, nans) == (selected.size, 0), what
    if selected.size == 0:
        assert np.isnan(below).all() and np.isnan(above).all(), what
        got_count, got = pct.masked_percentiles(dx, qs, dflags, **sel)
        assert got_count == 0 and np.isnan(got).all(), what
        return
    want_below, want_above, want = su.order_stats(selected, qs)
    assert below.dtype == np.float32 and su.same_floats(below, want_below), (what, below, want_below)
    assert su.same_floats(above, want_above), (what, above, want_above)
    got_count, got = pct.masked_percentiles(dx, qs, dflags, **sel)
    assert got_count == selected.size and got.dtype == np.float64 and np.all(got == want), (what, got, want)
    for q in singles:
        one_count, one = pct.masked_percentiles(dx, q, dflags, **sel)
        assert one_count == selected.size and one.shape == (1,) and one[0] == np.percentile(selected.astype(np.float64), q), (what, q)


@pytest.mark.parametrize("content", list(CONTENTS))
def test_order_statistics_and_percentiles_equal_numpy(pct, gpu, content):
    make, lo = CONTENTS[content]
    rs = np.random.RandomState(17)
    for n in LENGTHS:
        _check(pct, gpu, make(rs, n), (content, n), lo=lo)


def test_brats_sized_volume(pct, gpu):
    x = brats_like(np.random.RandomState(18), 240 * 240 * 155).reshape(240, 240, 155)
    _check(pct, gpu, x, "240x240x155", singles=(20,), lo=0.0)


def test_a_run_of_ties_straddles_the_rank(pct, gpu):
    rs = np.random.RandomState(19)
    n = 30011
    x = np.concatenate([rs.randint(1, 500, 10000), np.full(10000, 500), rs.randint(501, 4000, n - 20000)]).astype(np.float32)
    rs.shuffle(x)
    qs = [100 * r / (n - 1) for r in (9998.5, 9999.5, 10000.5, 15000.25, 19998.5, 19999.5, 20000.5)] + [50]  # ranks at both ends of the run and inside
    _check(pct, gpu, x, "ties", qs=qs, singles=(qs[1], qs[5]))


def test_selection_equals_a_numpy_mask(pct, gpu):
    rs = np.random.RandomState(20)
    shape = (37, 41, 150)
    x = brats_like(rs, int(np.prod(shape))).reshape(shape)
    flags = rs.randint(0, 256, shape).astype(np.uint8)
    flags[..., :40] &= 0xFE  # a required bit absent from whole chunks
    _check(pct, gpu, x, "require / forbid", flags, require=0x05, forbid=0x12)
    _check(pct, gpu, x, "require / forbid, lo = 0", flags, require=0x05, forbid=0x12, lo=0.0)
    _check(pct, gpu, x, "finite bounds", flags, require=0x80, lo=100.0, hi=3000.0)
    _check(pct, gpu, x, "finite bounds, no flags", lo=99.5, hi=100.5)   # one value passes
    _check(pct, gpu, x, "forbid only", flags, forbid=0xF0, hi=2000.0)
    _check(pct, gpu, x, "empty: bounds", flags, lo=5000.0)
    _check(pct, gpu, x, "empty: flags", flags & 0x7F, require=0x80)
    _check(pct, gpu, np.zeros(70, np.float32), "empty: an all-zero volume above 0", lo=0.0)


def test_nan_voxels_are_counted_and_the_wrapper_raises(pct, gpu):
    rs = np.random.RandomState(21)
    n = 20000
    x = brats_like(rs, n)
    flags = rs.randint(0, 4, n).astype(np.uint8)
    x[rs.choice(n, 300, replace=False)] = np.nan
    x[5] = _bits(0xFFC00001)  # a negative NaN with a payload
    selected = _select(x, flags, require=0x01, lo=0.0)
    want_nans = int(np.isnan(x[(flags & 0x01) != 0]).sum())
    assert want_nans > 50
    count, nans, below, above = pct.masked_order_stats(_dev(x, gpu), QS8, _dev(flags, gpu), require=0x01, lo=0.0)
    assert (count, nans) == (selected.size, want_nans)  # the NaN the flags select, whatever the bounds
    want_below, want_above, _ = su.order_stats(selected, QS8)
    assert su.same_floats(below, want_below) and su.same_floats(above, want_above)
    with pytest.raises(ValueError, match="NaN"):
        pct.masked_percentiles(_dev(x, gpu), 50, _dev(flags, gpu), require=0x01, lo=0.0)
    clean = np.where(np.isnan(x), np.float32(7), x)
    assert pct.masked_order_stats(_dev(clean, gpu), 50)[1] == 0


def test_two_calls_are_bit_equal_and_scratch_is_reused(pct, gpu):
    rs = np.random.RandomState(22)
    big, small = _dev(random_bits(rs, 97 * 61 * 53), gpu), _dev(brats_like(rs, 257), gpu)
    flags = _dev(rs.randint(0, 256, 97 * 61 * 53).astype(np.uint8), gpu)
    first = pct.masked_order_stats(big, QS8, flags, forbid=0x03)
    first_small = pct.masked_order_stats(small, QS8, lo=0.0)  # a small call after a large one, same stream and scratch
    again = pct.masked_order_stats(big, QS8, flags, forbid=0x03)
    again_small = pct.masked_order_stats(small, QS8, lo=0.0)
    for a, b in ((first, again), (first_small, again_small)):
        assert a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    want_below, want_above, _ = su.order_stats(_select(small.cpu().numpy(), lo=0.0), QS8)
    assert su.same_floats(first_small[2], want_below) and su.same_floats(first_small[3], want_above)


def _raw(amd, gpu, x, q=(50.0,), n=None, nq=None, flags=None, require=0, forbid=0, lo=-INF, hi=INF):
    lib = amd._lib.load()
    qa = np.asarray(q, dtype=np.float64)
    count = (C.c_int64 * 2)(-7, -7)
    below, above = np.full(16, -7, np.float32), np.full(16, -7, np.float32)
    rc = lib.mi355_masked_percentiles(x.data_ptr(), x.numel() if n is None else n, None if flags is None else flags.data_ptr(), require, forbid, lo, hi,
                                      qa.ctypes.data_as(C.POINTER(C.c_double)), qa.size if nq is None else nq, count, amd._lib.fptr(below),
                                      amd._lib.fptr(above), torch.cuda.current_stream(gpu).cuda_stream)
    untouched = list(count) == [-7, -7] and bool((below == -7).all() and (above == -7).all())
    return rc, lib.mi355_last_error().decode(), untouched


@pytest.mark.parametrize("kwargs,match", [
    (dict(nq=0), "percentiles"), (dict(q=tuple(range(9))), "percentiles"),
    (dict(q=(50.0, -0.5)), "percentile 1"), (dict(q=(100.5,)), "percentile 0"), (dict(q=(float("nan"),)), "percentile 0"),
    (dict(n=0), "n = 0"), (dict(n=2 ** 31), "n = 2147483648"),
    (dict(lo=float("nan")), "NaN"), (dict(hi=float("nan")), "NaN"),
    (dict(require=0x06, forbid=0x04), "share no bit"), (dict(require=256), "require 256"), (dict(forbid=-1), "forbid -1"),
])
def test_refusals_write_nothing(amd, gpu, kwargs, match):
    x = torch.arange(70, dtype=torch.float32, device=gpu)
    flags = torch.full((70,), 0xFF, dtype=torch.uint8, device=gpu)
    rc, message, untouched = _raw(amd, gpu, x, flags=flags, **kwargs)
    assert rc == -1 and match in message, (rc, message)
    assert untouched, "a refused call wrote to its outputs"


def test_an_empty_selection_leaves_the_outputs_and_succeeds(amd, gpu):
    x = torch.arange(70, dtype=torch.float32, device=gpu)
    lib = amd._lib.load()
    qa = np.asarray([50.0], dtype=np.float64)
    count = (C.c_int64 * 2)(-7, -7)
    below, above = np.full(1, -7, np.float32), np.full(1, -7, np.float32)
    rc = lib.mi355_masked_percentiles(x.data_ptr(), 70, None, 0, 0, 100.0, INF, qa.ctypes.data_as(C.POINTER(C.c_double)), 1, count,
                                      amd._lib.fptr(below), amd._lib.fptr(above), torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0 and list(count) == [0, 0] and below[0] == -7 and above[0] == -7


def _intensity_stats(data, mask):  # utils.get_intensity_stats, utils.py:27-51
    if mask.sum() == 0:
        return {'mean': None, 'std': None, 'min': None, 'max': None, 'median': None, 'q25': None, 'q75': None, 'voxel_count': 0}
    values = data[mask > 0]
    return {'mean': float(np.mean(values)), 'std': float(np.std(values)), 'min': float(np.min(values)), 'max': float(np.max(values)),
            'median': float(np.median(values)), 'q25': float(np.percentile(values, 25)), 'q75': float(np.percentile(values, 75)),
            'voxel_count': int(mask.sum())}


def test_intensity_stats_equal_the_numpy_restatement(pct, gpu):
    rs = np.random.RandomState(23)
    shape = (20, 30, 90)
    x = brats_like(rs, int(np.prod(shape))).reshape(shape)
    flags = rs.randint(0, 128, shape).astype(np.uint8)
    for bit in (0, 3, 7):  # (bit 7 is set nowhere: the empty region)
        got = pct.intensity_stats(_dev(x, gpu), _dev(flags, gpu), bit)
        want = _intensity_stats(x.astype(np.float64), (flags >> bit) & 1)
        assert list(got) == list(want)
        for k in want:
            if k == 'std' and want[k] is not None:
                assert abs(got[k] - want[k]) <= su.RTOL_STD * want[k], (bit, k, got[k], want[k])
            else:
                assert type(got[k]) is type(want[k]) and got[k] == want[k], (bit, k, got[k], want[k])
