"""What "fp16 parity" means for one conv or transposed-conv launch of the fp16 storage path, and the defects it is for.

include/mi355_nnunet.h promises of every fp16 kernel: fp32 accumulation, bias and LeakyReLU applied to the fp32 value, ONE
rounding (to nearest even) of the result to fp16.  A kernel that keeps the promise returns, element for element, the fp16
number nearest to the exact result, except where the fp32 sum lands on the other side of a rounding boundary than the exact
sum does - a fp32 sum is off by ~1e-7 relative and fp16 boundaries are 2^-11 relative apart, so that happens to well under
1 % of the outputs.  The gate is therefore a RATE of bit mismatches against RNE16(fp64 reference), calibrated by the rate
an independent fp32 implementation (torch on the CPU) has on the same operands, plus a one-ulp cap on every element.

Numpy only.  float64 -> float16 goes through numpy's astype, which rounds once (torch's CPU conversion of a double goes
through float32 and can round twice)."""
import numpy as np

FLOOR = 2.0 ** -16      # error scale for outputs near zero: fp32 summation noise (~1e-6 absolute) is several fp16 ulps there
CAP_FLOOR = 0.005       # smallest mismatch cap: at small K the natural rate is ~0.06 %, a handful of elements moves it
CAP_FACTOR = 4.0        # room for another summation order than the reference's (MFMA block accumulation, fp32 split-K)
WORST = 1.0             # never off by more than one fp16 ulp
MUTANT_FACTOR = 3.0     # a defective kernel (MUTANTS) must miss the cap by this factor


def ulp16(v):
    """spacing of fp16 at |v| (fp64 in, fp64 out): 2^(floor(log2 |v|) - 10) for |v| >= 2^-14, 2^-24 below (subnormals, 0).
    Read off the exponent field of the fp64 number, so it is the binade of the reference, not of its rounded value."""
    expo = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) & np.uint64(0x7FF0000000000000)
    return (np.maximum(expo, np.uint64((1023 - 14) << 52)) - np.uint64(10 << 52)).view(np.float64)


_CHUNK = 1 << 20  # elements per pass: the temporaries of a pass stay in cache (the largest outputs of the suite have 7e7 elements)


def _ratio(got16, ref):
    return np.abs(got16.astype(np.float64) - ref) / np.maximum(ulp16(ref), FLOOR)


def _scan(got16, ref64, full):
    """one chunked pass over a kernel output and its reference: (differing elements, worst, bias sum, bias count, size)"""
    got16 = np.ascontiguousarray(got16).reshape(-1)
    ref64 = np.ascontiguousarray(ref64, dtype=np.float64).reshape(-1)
    differing, worst, bias_sum, bias_n = 0, np.float64(0.0), 0.0, 0
    for lo in range(0, got16.size, _CHUNK):
        g16, ref = got16[lo:lo + _CHUNK], ref64[lo:lo + _CHUNK]
        gb, wb = g16.view(np.uint16), ref.astype(np.float16).view(np.uint16)
        at = np.flatnonzero((gb != wb) & (((gb | wb) & 0x7FFF) != 0))
        differing += at.size
        if not full:
            continue
        # an element equal to RNE16(ref) is within half a spacing of ref's binade: the maximum is among the differing
        # elements as soon as one of them reaches 0.5 (or is NaN); otherwise look at every element of the chunk
        w = np.max(_ratio(g16[at], ref[at])) if at.size else np.float64(0.0)
        if not (w >= 0.5 or np.isnan(w)):
            w = np.max(_ratio(g16, ref))
        worst = np.maximum(worst, w)  # (np.max and np.maximum keep a NaN)
        big = np.abs(ref) >= 2.0 ** -6
        bias_sum += float(np.sum((np.abs(g16.astype(np.float32)) - np.abs(ref)) / ulp16(ref) * big))
        bias_n += int(np.count_nonzero(big))
    return differing, float(worst), bias_sum, bias_n, got16.size


def rounding_report(got16, ref64):
    """(mismatch, worst, bias) of a kernel's fp16 output against the fp64 reference.
      mismatch  share of elements whose fp16 bits differ from RNE16(ref64) (+0 and -0 are equal)
      worst     max |got - ref64| / max(ulp16(ref64), 2^-16)
      bias      mean (|got| - |ref64|) / ulp16(ref64) over |ref64| >= 2^-6: ~ -0.5 under truncation, ~ 0 otherwise"""
    assert np.asarray(got16).dtype == np.float16, np.asarray(got16).dtype
    assert np.shape(got16) == np.shape(ref64), (np.shape(got16), np.shape(ref64))
    differing, worst, bias_sum, bias_n, size = _scan(got16, ref64, True)
    return differing / max(1, size), worst, bias_sum / bias_n if bias_n else 0.0


def natural_rate(ref32, ref64):
    """mismatch of an independent fp32-accumulate implementation (torch CPU float32 on the same operands) rounded once"""
    ref32 = np.asarray(ref32)
    assert ref32.dtype == np.float32, ref32.dtype
    assert ref32.shape == np.shape(ref64), (ref32.shape, np.shape(ref64))
    differing, _, _, _, size = _scan(ref32.astype(np.float16), ref64, False)
    return differing / max(1, size)


def _cap(natural):
    return max(CAP_FLOOR, CAP_FACTOR * natural)


def gate(ref32, ref64):
    """(cap on mismatch, cap on worst) for a kernel output with these references"""
    return _cap(natural_rate(ref32, ref64)), WORST


def check(label, got16, ref32, ref64):
    """print the ROUNDING line of one kernel output and return (mismatch, cap, worst, worst cap) for the caller's asserts"""
    mismatch, worst, bias = rounding_report(got16, ref64)
    natural = natural_rate(ref32, ref64)
    print(f"ROUNDING {label} mismatch={mismatch:.3e} natural={natural:.3e} worst={worst:.3f} bias={bias:+.3f}")
    return mismatch, _cap(natural), worst, WORST


# ---------------------------------------------------------------------------------------------------------------------
# The defects the gate is for, as functions of (operands, bias, act, slope) evaluated with torch on the CPU.  Each returns
# the np.float16 array a kernel with that defect would store (NCDHW).
class Operands:
    """one conv3d (padding 1) or conv_transpose3d (kernel 2, stride 2) on fp16-rounded operands; x NCDHW, w as torch has it"""

    def __init__(self, kind, x, w, stride=1):
        assert kind in ("conv", "tconv")
        assert np.array_equal(np.asarray(x, np.float64), np.asarray(x).astype(np.float16).astype(np.float64)), "x is not fp16-rounded"
        assert np.array_equal(np.asarray(w, np.float64), np.asarray(w).astype(np.float16).astype(np.float64)), "w is not fp16-rounded"
        self.kind, self.stride = kind, stride
        self.x, self.w = np.asarray(x, np.float64), np.asarray(w, np.float64)

    @property
    def cin(self):
        return self.x.shape[1]

    def linear(self, dtype, channels=slice(None)):
        """the op without bias on input channels `channels`, accumulated in `dtype` (torch tensor)"""
        import torch
        import torch.nn.functional as F
        x = torch.from_numpy(np.ascontiguousarray(self.x[:, channels])).to(dtype)
        if self.kind == "conv":
            return F.conv3d(x, torch.from_numpy(np.ascontiguousarray(self.w[:, channels])).to(dtype), None, stride=self.stride, padding=1)
        return F.conv_transpose3d(x, torch.from_numpy(np.ascontiguousarray(self.w[channels])).to(dtype), None, stride=2)


def _bias_act(t, bias, act, slope):
    import torch
    if bias is not None:
        t = t + torch.from_numpy(np.asarray(bias)).to(t.dtype)[None, :, None, None, None]
    return torch.maximum(t, t * slope) if act else t  # (the kernels' max(x, slope x); slope in [0, 1])


def _h(t):
    """round a torch tensor to fp16 once, back in its own dtype"""
    import torch
    return torch.from_numpy(t.numpy().astype(np.float16)).to(t.dtype)


def reference(operands, bias, act, slope, dtype="float64"):
    """the promised op: accumulate, bias, LeakyReLU in `dtype` ('float64': the reference; 'float32': torch's own fp32
    implementation, for natural_rate).  numpy array of that dtype, NCDHW, not rounded to fp16"""
    import torch
    return _bias_act(operands.linear(getattr(torch, dtype)), bias, act, slope).numpy()


def truncate(operands, bias, act, slope):
    """right in fp32, but the result is truncated (rounded toward zero) to fp16 instead of round-to-nearest-even"""
    v = reference(operands, bias, act, slope, "float32")
    r = v.astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float16)


def round_before_bias_act(operands, bias, act, slope):
    """the conv sum is rounded to fp16 before bias and LeakyReLU are applied (in fp32), then rounded again"""
    import torch
    return _bias_act(_h(operands.linear(torch.float32)), bias, act, slope).numpy().astype(np.float16)


def act_in_f16(operands, bias, act, slope):
    """conv + bias rounded to fp16, then LeakyReLU in fp16: fp16 slope, product rounded to fp16"""
    import torch
    pre = _h(_bias_act(operands.linear(torch.float32), bias, 0, slope))
    if act:
        pre = torch.maximum(pre, _h(pre * float(np.float16(slope))))
    return pre.numpy().astype(np.float16)


def f16_partial(operands, bias, act, slope):
    """the first half of the input channels is accumulated to an fp16 partial (split-K or chunk partials kept in fp16)"""
    import torch
    half = operands.cin // 2
    t = _h(operands.linear(torch.float32, slice(0, half))) + operands.linear(torch.float32, slice(half, None))
    return _bias_act(t, bias, act, slope).numpy().astype(np.float16)


MUTANTS = {"truncate": truncate, "round_before_bias_act": round_before_bias_act, "act_in_f16": act_in_f16, "f16_partial": f16_partial}


def mutants_that_apply(bias, act):
    """truncate and f16_partial always; round_before_bias_act needs something applied after the rounding (without bias and
    activation the second rounding changes nothing); act_in_f16 needs an activation"""
    names = ["truncate", "f16_partial"]
    if bias is not None or act:
        names.append("round_before_bias_act")
    if act:
        names.append("act_in_f16")
    return names
