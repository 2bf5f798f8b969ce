"""-m gpu: who owns device memory that is not scratch (csrc/common.h, DeviceAllocs).  A network handle owns its weights and its
Gaussian map, a single-op entry point owns its buffers and weights for the length of the call, and ``ops.live_allocations()``
counts what all owners of the process hold.  Every test takes its baseline when it starts (other tests' networks may be alive) and
asserts that count and bytes return to it EXACTLY: after a handle is closed, after a create that was refused part-way, after a
single-op call that ran or was refused.  Nothing here launches more than one tiny kernel; the refusals are validated refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sd(amd, **kw):
    return amd.synthetic.make_state_dict(num_pool=1, seed=11, **kw)


def _conv_weight_elements(sd):
    return sum(int(v.size) for k, v in sd.items() if k.endswith(".weight") and v.ndim == 5)


@pytest.mark.parametrize("in_ch", [4, 5])   # 4 -> 32: the first conv is the stem kernel's; 5 channels: the generic path
@pytest.mark.parametrize("norm,nonlin_first", [("batch", False), ("batch", True), ("instance", False)])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_balanced_lifetime(amd, gpu, dtype, norm, nonlin_first, in_ch):
    """Bytes: every weight element of every conv, transposed conv and head is on the device at least once in the network's element
    type (fp32 keeps several packs of a conv, both types pad channels), so bytes >= elements x element size."""
    base = amd.ops.live_allocations()
    sd = _sd(amd, norm=norm, base=32, in_ch=in_ch)
    net = amd.UNet(sd, norm=norm, nonlin_first=nonlin_first, dtype=dtype)
    count, nbytes = amd.ops.live_allocations()
    assert count > base[0]
    assert nbytes - base[1] >= _conv_weight_elements(sd) * (4 if dtype == "f32" else 2)
    net.close()
    assert amd.ops.live_allocations() == base


def _wrong_head(amd):
    sd = _sd(amd, norm="batch", base=32)
    sd["seg_outputs.0.weight"] = np.ascontiguousarray(sd["seg_outputs.0.weight"][:, :16])
    return sd


REFUSED = {
    # name: (state dict, UNet arguments, what the library says)
    "f16_cout_24_after_its_affine": (lambda amd: _sd(amd, norm="instance", base=24), dict(norm="instance", dtype="f16"), "cout % 32 == 0 (got 24)"),
    "f32_cin_pad_30_instance": (lambda amd: _sd(amd, norm="instance", base=30), dict(norm="instance", dtype="f32"), "bad cin_pad 30 for cin 30"),
    "f32_cin_pad_30_batch_nonlin_first": (lambda amd: _sd(amd, norm="batch", base=30), dict(norm="batch", nonlin_first=True, dtype="f32"),
                                          "bad cin_pad 30 for cin 30"),
    "head_cin_16_after_everything": (_wrong_head, dict(norm="batch", dtype="f32"), "head: cin 16 classes 3, expected 32 / 3"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_create_returns_to_baseline(amd, gpu, name):
    """A create the library refuses part-way leaves nothing on the device.  By inspection the first three leaked before the handle
    owned its allocations: the layer's affine (gamma / beta, or the BatchNorm scale / shift with nonlin_first) was uploaded into a
    local layer that nobody freed when the conv uploader then refused the layer - in the second and third also after layer 0 had
    been uploaded whole.  The fourth is refused at the very end, after every conv and transposed conv."""
    make_sd, kw, message = REFUSED[name]
    base = amd.ops.live_allocations()
    with pytest.raises(amd._lib.Mi355Error) as e:
        amd.UNet(make_sd(amd), **kw)
    assert "mi355_unet_create failed" in str(e.value) and message in str(e.value), str(e.value)
    assert amd.ops.live_allocations() == base


def _x(shape, dtype, seed=5):
    import torch
    x = torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32)).cuda()
    return x.half() if dtype == "f16" else x


def _w(shape, seed=6):
    return (np.random.RandomState(seed).standard_normal(shape) * 0.1).astype(np.float32)


SINGLE_OPS = {
    # the smallest legal shape of each entry point: volume 1 x 4 x 8 x 32 for the convs, 1 x 2 x 4 x 16 for the transposed convs
    "conv_f32_s1": lambda ops: ops.conv3d_ndhwc(_x((1, 4, 8, 32, 8), "f32"), _w((32, 8, 3, 3, 3)), _w((32,)), stride=1),
    "conv_f32_s2": lambda ops: ops.conv3d_ndhwc(_x((1, 4, 8, 32, 8), "f32"), _w((32, 8, 3, 3, 3)), _w((32,)), stride=2),
    "conv_f16": lambda ops: ops.conv3d_ndhwc(_x((1, 4, 8, 32, 16), "f16"), _w((32, 16, 3, 3, 3)), _w((32,))),
    "stem_f32": lambda ops: ops.conv3d_ndhwc(_x((1, 4, 8, 32, 4), "f32"), _w((32, 4, 3, 3, 3)), _w((32,))),
    "stem_f16": lambda ops: ops.conv3d_ndhwc(_x((1, 4, 8, 32, 4), "f16"), _w((32, 4, 3, 3, 3)), None),
    "tconv_f32": lambda ops: ops.tconv3d_ndhwc(_x((1, 2, 4, 16, 8), "f32"), _w((8, 32, 2, 2, 2))),
    "tconv_f16": lambda ops: ops.tconv3d_ndhwc(_x((1, 2, 4, 16, 16), "f16"), _w((16, 32, 2, 2, 2))),
    "head_logits": lambda ops: ops.head_logits(_x((1, 4 * 8 * 32, 32), "f32"), _w((3, 32)), _w((3,))),
}


@pytest.mark.parametrize("name", sorted(SINGLE_OPS))
def test_single_op_call_returns_to_baseline(amd, gpu, name):
    import torch
    base = amd.ops.live_allocations()
    y = SINGLE_OPS[name](amd.ops)
    assert bool(torch.isfinite(y.float()).all()), "the call stored nothing"   # (the wrappers hand the library an all-NaN output)
    assert amd.ops.live_allocations() == base


def test_refused_single_op_call_returns_to_baseline(amd, gpu):
    """The fp16 conv with 12 input channels is refused after its guarded output buffer was allocated."""
    base = amd.ops.live_allocations()
    with pytest.raises(amd._lib.Mi355Error) as e:
        amd.ops.conv3d_ndhwc(_x((1, 4, 8, 32, 12), "f16"), _w((32, 12, 3, 3, 3)), _w((32,)))
    assert "fp16 conv needs cin % 8 == 0" in str(e.value), str(e.value)
    assert amd.ops.live_allocations() == base


def test_gaussian_map_is_replaced_not_added(amd, gpu):
    """Sliding windows with different patch sizes on one handle (volume 16^3): the handle holds one map at a time, and none once it
    is closed.  Patch 8^3: 27 tiles, the first map.  Patch 16^3: one tile, which is not weighted - the map stays as it is.  Patch
    8 x 8 x 16: 9 tiles, the map is replaced (ensure_gaussian releases the old one)."""
    base = amd.ops.live_allocations()
    net = amd.UNet(_sd(amd, norm="batch", base=32), norm="batch")
    with_net = amd.ops.live_allocations()
    vol = np.random.RandomState(3).standard_normal((4, 16, 16, 16)).astype(np.float32)
    for patch, map_voxels in (((8, 8, 8), 512), ((16, 16, 16), 512), ((8, 8, 16), 1024)):
        probs = amd.predict_folds([net], vol, patch, 0.5, False, (0, 1, 2), True, "sigmoid", lanes=1)
        assert tuple(probs.shape) == (3, 16, 16, 16) and bool(probs.isfinite().all())
        count, nbytes = amd.ops.live_allocations()
        assert count == with_net[0] + 1, "the handle holds one map beside its weights"
        assert nbytes == with_net[1] + 4 * map_voxels
    net.close()
    assert amd.ops.live_allocations() == base
