"""The split-bf16 weight pack of the fp32 stride-2 LDS-DMA kernel (pack_conv_weights_s2split, conv3d.hip) through the host-only
entry mi355_conv_s2_split_pack: no device.

Layout under test (ops.conv_s2_split_pack returns [cout/64][cin_pad/8][dz][piece: hi, mid, lo][4608] bf16 bit patterns):
  group 0 of a dz plane = tap dz*9 alone:              offset nf*256 + lane*4 + e,                     e = 0..3
  group g = 1..4 = taps dz*9 + 2g-1 and dz*9 + 2g:     offset 512 + (g-1)*1024 + nf*512 + lane*8 + e,  e = 0..7, tap 2g-1 + (e>>2)
  cout = (block*2 + nf)*32 + (lane & 31), cin = chunk*8 + (lane >> 5)*4 + (e & 3); channels at or beyond cin are zero.

* every stored piece is a finite bf16 and hi + mid + lo equals the fp32 weight EXACTLY: random weights over 40 binades, +-0, values
  with 24 significant bits, the zero padding of cin_pad;
* a weight tensor that encodes its own indices sits where the layout says."""
import numpy as np
import pytest


def _where(cout, cin_pad):
    """(block, chunk, dz, offset) -> (cout, cin, tap) of every element of a piece, as index arrays of shape [nblk, nchunks, 3, 4608]"""
    nblk, nch = cout // 64, cin_pad // 8
    co = np.zeros((nblk, nch, 3, 4608), np.int64)
    ci, tap = np.zeros_like(co), np.zeros_like(co)
    for b in range(nblk):
        for ch in range(nch):
            for dz in range(3):
                for g in range(5):
                    for nf in range(2):
                        for lane in range(64):
                            for e in range(8 if g else 4):
                                o = 512 + (g - 1) * 1024 + nf * 512 + lane * 8 + e if g else nf * 256 + lane * 4 + e
                                co[b, ch, dz, o] = (b * 2 + nf) * 32 + (lane & 31)
                                ci[b, ch, dz, o] = ch * 8 + (lane >> 5) * 4 + (e & 3)
                                tap[b, ch, dz, o] = dz * 9 + (2 * g - 1 + (e >> 2) if g else 0)
    return co, ci, tap


def _bf16_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _check(amd, wt, cin_pad):
    cout, cin = wt.shape[:2]
    pack = amd.ops.conv_s2_split_pack(wt, cin_pad)
    assert pack.dtype == np.uint16 and pack.shape == (cout // 64, cin_pad // 8, 3, 3, 4608)
    assert ((pack & 0x7f80) != 0x7f80).all()   # finite bf16 values
    co, ci, tap = _where(cout, cin_pad)
    # every (cout, cin, tap) of the padded tensor is stored exactly once
    ids = (co * cin_pad + ci) * 27 + tap
    assert np.array_equal(np.sort(ids.ravel()), np.arange(cout * cin_pad * 27))
    padded = np.zeros((cout, cin_pad, 27), np.float32)
    padded[:, :cin] = wt.reshape(cout, cin, 27)
    want = padded[co, ci, tap].astype(np.float64)
    pieces = _bf16_to_f64(pack)
    got = pieces[:, :, :, 0] + pieces[:, :, :, 1] + pieces[:, :, :, 2]   # (exact in fp64: three 8-bit pieces inside 24 bits)
    assert np.array_equal(got, want)
    # the pieces shrink: |mid| <= 2^-7 |hi|, |lo| <= 2^-7 |mid| (the kernel drops mid x lo and lo x lo on that ground)
    assert (np.abs(pieces[:, :, :, 1]) <= np.abs(pieces[:, :, :, 0]) * 2.0 ** -7).all()
    assert (np.abs(pieces[:, :, :, 2]) <= np.abs(pieces[:, :, :, 0]) * 2.0 ** -15).all()
    # zeros keep nothing, and the padding channels hold zero bits (+0: nothing a NaN-free product could turn into a NaN)
    assert (pack[np.broadcast_to((ci >= cin)[:, :, :, None, :], pack.shape)] == 0).all()
    return pack


def test_random_weights_over_40_binades_recombine_exactly(amd):
    rs = np.random.RandomState(3)
    wt = (rs.standard_normal((128, 16, 3, 3, 3)) * 2.0 ** rs.randint(-20, 20, size=(128, 16, 3, 3, 3))).astype(np.float32)
    _check(amd, wt, 16)


def test_signed_zeros_full_mantissas_and_channel_padding(amd):
    rs = np.random.RandomState(4)
    wt = rs.standard_normal((64, 5, 3, 3, 3)).astype(np.float32)
    # 24 significant bits: an odd 24-bit integer scaled by a power of two
    full = ((rs.randint(1 << 23, 1 << 24, size=wt.shape) | 1) * 2.0 ** rs.randint(-30, 6, size=wt.shape)).astype(np.float32)
    full *= rs.choice([-1.0, 1.0], size=wt.shape).astype(np.float32)
    wt = np.where(rs.rand(*wt.shape) < 0.5, full, wt).astype(np.float32)
    wt[rs.rand(*wt.shape) < 0.1] = 0.0
    wt[rs.rand(*wt.shape) < 0.1] = -0.0
    pack = _check(amd, wt, 8)   # cin 5 padded to 8
    assert pack.any()


def test_an_index_encoding_tensor_sits_where_the_layout_says(amd):
    cout, cin = 128, 24
    co, ci, tap = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(27), indexing="ij")
    wt = (co * 1024 + ci * 32 + tap + 1).astype(np.float32).reshape(cout, cin, 3, 3, 3)   # < 2^17: exact in fp32, spread over hi and mid
    pack = _check(amd, wt, 24)
    pieces = _bf16_to_f64(pack)
    code = (pieces[:, :, :, 0] + pieces[:, :, :, 1] + pieces[:, :, :, 2]).astype(np.int64) - 1
    # spot positions spelt out by hand: block 1, chunk 2, dz 1
    assert code[1, 2, 1, 0] == (64 * 1024) + (16 * 32) + 9                      # group 0, nf 0, lane 0, e 0: cout 64, cin 16, tap 9
    assert code[1, 2, 1, 256 + 33 * 4 + 2] == (97 * 1024) + (22 * 32) + 9       # group 0, nf 1, lane 33, e 2: cout 64 + 32 + 1, cin 16 + 4 + 2
    assert code[1, 2, 1, 512 + 2 * 1024 + 512 + 40 * 8 + 5] == ((96 + 8) * 1024) + (21 * 32) + 9 + 6   # group 3, nf 1, lane 40, e 5: tap 5 + 1


def test_a_bad_shape_is_refused(amd):
    with pytest.raises(amd._lib.Mi355Error, match="mi355_conv_s2_split_pack: bad argument"):
        amd.ops.conv_s2_split_pack(np.zeros((32, 8, 3, 3, 3), np.float32))   # cout not a multiple of 64
