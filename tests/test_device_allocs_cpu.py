"""not gpu: device memory that is not scratch has one owner per handle or call (csrc/common.h, DeviceAllocs), and
``ops.live_allocations()`` counts what all owners hold.  Without a device they hold nothing, whatever is asked of the library: a
refused create, and the conv planner's stand-in weights, which never touch an owner.

The checks run in a process of their own with every device hidden: the counters are process-wide, and on a machine with a GPU the
suite's process holds networks of other tests."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import brats_amd
from brats_amd import _lib, ops, synthetic

assert ops.live_allocations() == (0, 0), ops.live_allocations()      # a fresh process

sd = synthetic.make_state_dict(norm="instance", num_pool=1, base=32)
for dtype in ("f32", "f16"):
    try:
        brats_amd.UNet(sd, norm="instance", dtype=dtype)
    except _lib.Mi355Error as e:
        assert "failed (-3)" in str(e) and "no HIP device" in str(e), e      # MI355_ERR_NO_DEVICE, the library's own message
    else:
        raise AssertionError("mi355_unet_create succeeded without a device")
    assert ops.live_allocations() == (0, 0), ops.live_allocations()

# the dry-run planner: stand-in weights, no owner, no device
p32 = ops.conv3d_plan("f32", (2, 32, 32, 32), 32, 32)
p16 = ops.conv3d_plan("f16", (2, 32, 32, 32), 32, 64, stats=True)
assert p32["rc"] == 0 and p32["kernel"].startswith("conv3_f32_"), p32
assert p16["rc"] == 0 and p16["kernel"].startswith("conv3_f16_"), p16
assert ops.live_allocations() == (0, 0), ops.live_allocations()
print("ok")
"""


def test_nothing_is_held_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    res = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), res.stdout + res.stderr


def test_the_aid_is_bound_and_declared(amd):
    api = open(os.path.join(ROOT, "include", "mi355_nnunet.h"), encoding="utf-8").read()
    assert "int mi355_live_allocations(int64_t *count, int64_t *bytes);" in api
    assert "mi355_live_allocations" in amd._lib.EXPORTS
    count, nbytes = amd.ops.live_allocations()   # host code: needs no device
    assert count >= 0 and nbytes >= 0 and (count == 0) == (nbytes == 0)
