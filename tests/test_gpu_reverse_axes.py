"""-m gpu: ``mi355_reverse_axes`` / ``volume_ops.reverse_axes`` (csrc/resident_case.hip), the hand-off of a case in file order
[C, Z, Y, X] to the (x, y, z) volumes the evaluator and the feature steps take.  The kernel moves bits, so every comparison is an
equality of bits with ``np.ascontiguousarray(a.transpose(0, 3, 2, 1))``: random 32-bit patterns (NaN payloads, infinities and
denormals among them) for float32, random bytes for uint8.

Shapes: 1 x 1 x 1; dimensions below the tile (64 for 4-byte elements, 128 for bytes) and not divisible by 4; 130 = one tile of
bytes and two voxels, three tiles of words, on either transposed axis; 65 and 67 = one word tile and 1 or 3; a middle axis of 1;
and the 155 x 240 x 240 volume of a BraTS case."""
import importlib
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 7, 9), (3, 5, 130), (130, 5, 3), (67, 2, 3), (33, 34, 35), (65, 1, 64), (64, 3, 65)]
GUARD = 64   # elements behind the output that must stay as they were
FILL = 0xA5


def _vo():
    return importlib.import_module("brats_amd.volume_ops")


def _random(rs, shape, dtype):
    if dtype == np.float32:
        return rs.randint(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return rs.randint(0, 256, size=shape, dtype=np.uint16).astype(np.uint8)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _want(a):
    return np.ascontiguousarray(_bits(a).transpose(0, 3, 2, 1))


def _raw_call(amd, src, dst, channels, d0, d1, d2, elem_bytes):
    """The C entry point on two device tensors (or addresses), on the current stream; returns (rc, message)"""
    lib = amd._lib.load()
    ptr = [t.data_ptr() if torch.is_tensor(t) else t for t in (src, dst)]
    rc = lib.mi355_reverse_axes(ptr[0], ptr[1], channels, d0, d1, d2, elem_bytes, torch.cuda.current_stream().cuda_stream)
    return rc, (lib.mi355_last_error() or b"").decode()


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["float32", "uint8"])
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_reversal_is_bit_exact_behind_an_offset_and_inside_its_output(amd, gpu, shape, channels, dtype):
    """The source starts one element into a larger buffer (a pointer aligned to the element only); the output lies in a buffer
    prefilled with 0xA5 bytes whose elements behind the output's end must not change."""
    rs = np.random.RandomState(sum(shape) * 7 + channels + (dtype == np.uint8))
    a = _random(rs, (channels,) + shape, dtype)
    n = a.size
    tdtype = torch.float32 if dtype == np.float32 else torch.uint8
    big = torch.empty(n + 1, dtype=tdtype, device=gpu)
    big.view(torch.uint8)[:] = 0
    src = big[1:]
    src.copy_(torch.from_numpy(a.reshape(-1)).to(gpu))
    assert src.data_ptr() == big.data_ptr() + a.itemsize
    out = torch.empty(n + GUARD, dtype=tdtype, device=gpu)
    out.view(torch.uint8)[:] = FILL
    rc, msg = _raw_call(amd, src, out, channels, *shape, a.itemsize)
    assert rc == 0, msg
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:n]).reshape((channels,) + shape[::-1]), _want(a))
    assert np.all(got[n:].view(np.uint8) == FILL)
    # the wrapper: 4-D and 3-D, and twice is the identity
    vo = _vo()
    t = src.view((channels,) + shape)
    once = vo.reverse_axes(t)
    assert once.shape == (channels,) + shape[::-1] and once.dtype == tdtype and once.is_contiguous()
    assert np.array_equal(_bits(once.cpu().numpy()), _want(a))
    assert np.array_equal(_bits(vo.reverse_axes(once).cpu().numpy()), _bits(a))
    one = vo.reverse_axes(t[0])
    assert one.shape == shape[::-1]
    assert np.array_equal(_bits(one.cpu().numpy()), _want(a)[0])


@pytest.mark.parametrize("dtype,channels", [(np.float32, 4), (np.uint8, 1)], ids=["modalities", "label_map"])
def test_a_whole_case(amd, gpu, dtype, channels):
    """155 x 240 x 240 (Z, Y, X): the four float32 modalities in one launch, and the label map"""
    rs = np.random.RandomState(5)
    a = _random(rs, (channels, 155, 240, 240), dtype)
    got = _vo().reverse_axes(torch.from_numpy(a).to(gpu))
    assert got.shape == (channels, 240, 240, 155)
    assert np.array_equal(_bits(got.cpu().numpy()), _want(a))
    back = _vo().reverse_axes(got)
    assert np.array_equal(_bits(back.cpu().numpy()), _bits(a))


def test_refusals_write_nothing(amd, gpu):
    src = torch.arange(4 * 6 * 5 * 3, dtype=torch.float32, device=gpu)
    out = torch.empty(src.numel() + GUARD, dtype=torch.float32, device=gpu)
    out.view(torch.uint8)[:] = FILL
    ok = (src, out, 4, 6, 5, 3, 4)
    cases = [
        ("null pointer", (0,) + ok[1:]),
        ("null pointer", (src, 0) + ok[2:]),
        ("bad shape", (src, out, 0, 6, 5, 3, 4)),
        ("bad shape", (src, out, 4, 0, 5, 3, 4)),
        ("bad shape", (src, out, 4, 6, -1, 3, 4)),
        ("bad shape", (src, out, 4, 6, 5, 0, 4)),
        ("bytes per element", (src, out, 4, 6, 5, 3, 2)),
        ("bytes per element", (src, out, 4, 6, 5, 3, 8)),
        ("bytes per element", (src, out, 4, 6, 5, 3, 0)),
        ("2\\^31 elements or more", (src, out, 1, 2048, 1024, 1024, 1)),
        ("2\\^31 elements or more", (src, out, 2, 65536, 65536, 65536, 4)),
        ("2\\^31 elements or more", (src, out, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1)),
        ("overlap", (src, src, 4, 6, 5, 3, 4)),
        ("overlap", (out[:src.numel()], out[src.numel() - 1:], 4, 6, 5, 3, 4)),
        ("overlap", (out[1:], out, 4, 6, 5, 3, 4)),
        ("not aligned to 4 bytes", (src.data_ptr() + 1, out, 1, 6, 5, 3, 4)),
    ]
    for pattern, args in cases:
        rc, msg = _raw_call(amd, *args)
        assert rc == -1 and re.search(pattern, msg), (pattern, rc, msg)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy().view(np.uint8) == FILL)
    assert np.array_equal(src.cpu().numpy(), np.arange(4 * 6 * 5 * 3, dtype=np.float32))
    # two buffers that touch but do not overlap are served
    both = torch.empty(2 * src.numel(), dtype=torch.float32, device=gpu)
    both[:src.numel()] = src
    rc, msg = _raw_call(amd, both[:src.numel()], both[src.numel():], 4, 6, 5, 3, 4)
    assert rc == 0, msg
    assert np.array_equal(both[src.numel():].cpu().numpy().reshape(4, 3, 5, 6), src.cpu().numpy().reshape(4, 6, 5, 3).transpose(0, 3, 2, 1))
    vo = _vo()
    with pytest.raises(ValueError, match="uint8 or float32"):
        vo.reverse_axes(torch.zeros((2, 3, 4), dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError, match="uint8 or float32"):
        vo.reverse_axes(torch.zeros((3, 4), dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match="uint8 or float32"):
        vo.reverse_axes(torch.zeros((2, 3, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="contiguous"):
        vo.reverse_axes(torch.zeros((2, 3, 4), dtype=torch.uint8, device=gpu).permute(2, 1, 0))
