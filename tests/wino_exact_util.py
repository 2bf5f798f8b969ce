"""Exact-integer operands, an integer emulation of both Winograd transform domains and the table of GPU cases of the fp32 Winograd
conv kernels (plain numpy: no GPU import).  tests/test_wino_exact_cpu.py checks all of it without a device,
tests/test_gpu_wino_exact.py runs the table.

Why integers are exact.  conv3_f32_wino3_kernel is F(2x2x2, 3x3x3), conv3_f32_wino2_kernel F(2x2, 3x3) over (z, y) with x walked
directly.  B^T and A^T hold only 0 and +-1; G holds 1 and +-1/2.  For integer weights U = G w G^T is therefore a multiple of 1/8
(3-D form) or 1/4 (2-D form), for integer inputs V = B^T d B is an integer, and every product, every partial sum over the input
channels and every partial sum of the output transform is a multiple of that unit.  While all of them, counted in units, stay
below 2^24, fp32 holds each exactly and no order of addition rounds: the output must EQUAL the integer conv.

`emulate` computes exactly those scaled quantities in integers (8 U and V, or 4 U and V), the per-component sums over cin and
the output transform, and next to the result
  * the BOUND: the same pipeline on absolute values (|B^T|, |G|, |A^T|, |x|, |w|, |bias|, |addend|) - by the triangle inequality
    no partial sum of the real pipeline, in whatever order, exceeds the largest value of this one.  It is asserted < 2^24 HERE,
    for every set of operands (checked_case is the only way the GPU module gets operands);
  * the widest V, U and product V * U in significant bits (the bit length of the odd part): what an implementation has to carry.

Operand classes (`operands`), each written so that one kind of defect moves some output by at least 1/2:
  dense    conv_rows_util.int_operands: x in [-4, 4], w in {-1, 0, 1} thinned to 16 channels' worth, integer bias;
  taps     output channel o reads ONE (tap, input channel) with a gain in +-{1, 2, 3}; all 27 taps and every input channel are
           read by some o; x is 12-bit.  The output is a shifted, scaled copy of one input channel, so a wrong halo plane, a
           swapped channel pair, quad or chunk and a wrong tile origin each show, and `describe_tap_failure` names the tap, the
           channel, the tile and the 2x2x2 block of the first wrong output;
  wide_x   wide x, one unit weight per output channel;   wide_w   wide w, x in {-1, 0, 1};   mid   x of about 11 bits times w of
           about 8 bits, one weight per output channel.  Widths: a single weight w at a tap puts 8 |w| s into the bound per unit of
           |V| <= 8 max|x| (3-D; 4 |w| s and 4 max|x| in the 2-D form), s = the product over the transformed axes of (2 for an
           outer tap, 1 for the centre tap).  With bits(x) + bits(w) + log2 s = 17 (3-D) or 19 (2-D) the bound is at most
           2^23 + 8 |bias| whatever the data: the widest budget that guarantees it (one more bit reaches 2^24 on the worst draw).  Input channel c belongs to tap class c % 4 (c % 3 in the 2-D form: log2 s = 0..3 or 0..2) and is read through taps
           of that class only, so both widths follow the class: the centre taps carry 17- (19-) bit operands.  The emulation
           must then report more than 16 significant bits for V (wide_x), U (wide_w) and the product (mid): an implementation
           that carries two bf16 pieces' worth of an operand cannot pass;
  norm     (conv3_f32_wino3_kernel<2, true>) dense, plus a producer norm: in_scale a power of two (1, 2, 4) per (n, c), in_shift a
           non-zero integer, LeakyReLU at 0.5.  The normalised brick holds half-integers: the unit halves (1/16) and the bound
           is asserted in it.  The shift is non-zero so that "padding follows the norm" is exact: a shift applied to an
           out-of-volume piece moves border outputs by whole numbers;
  head     dense, plus integer head weights in {-2 .. 2} and an integer head bias: the logits are exact too.
LeakyReLU at 0.5 everywhere: it halves negative outputs exactly.

These classes pin the present exact-fmaf product form.  A change of product form that legitimately cannot meet a class must
restate that class in the same change, as tests/test_gpu_s2_split.py does for the stride-2 kernel - not delete it."""
import itertools
import zlib
from collections import namedtuple

import numpy as np

import conv_rows_util as U

LIMIT = 2 ** 24
SLOPE = U.INT_SLOPE
CLASSES = ("dense", "taps", "wide_x", "wide_w", "mid", "norm", "head")
BITS_CLASSES = ("wide_x", "wide_w", "mid")
TAPS = list(itertools.product(range(3), repeat=3))  # (dz, dy, dx), tap index dz * 9 + dy * 3 + dx

# B^T, 2 G and A^T of F(2, 3) as the kernels apply them (conv3d_wino3.hip: xi = 0..3 are d0 - d2, d1 + d2, d2 - d1, d1 - d3;
# out0 = p0 + p1 + p2, out1 = p1 - p2 - p3)
G2 = np.array([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], np.int64)
TILE = {3: (4, 8, 8), 2: (4, 4, 32)}       # output tile of the kernel of each form
U_SCALE = {3: 8, 2: 4}                     # U is a multiple of 1 / U_SCALE
WIDTH_BUDGET = {3: 17, 2: 19}              # bits(x) + bits(w) + log2 s of the bits classes (module docstring)

Operands = namedtuple("Operands", "cls form x wt bias scale shift head_w head_b addend")
Emulation = namedtuple("Emulation", "result bound v_bits u_bits product_bits")


# ------------------------------------------------------------------ the transforms, on any dtype
def _bt(a, axis, absolute=False):
    """B^T along `axis` of a zero-padded array (even length L + 2): windows of 4 at stride 2 -> L / 2 blocks on `axis`, the four
    components on a new last axis"""
    n = (a.shape[axis] - 2) // 2
    d = [a[(slice(None),) * axis + (slice(k, k + 2 * n, 2),)] for k in range(4)]
    if absolute:
        comps = [d[0] + d[2], d[1] + d[2], d[2] + d[1], d[1] + d[3]]
    else:
        comps = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    return np.stack(comps, axis=-1)


def _at(m, axis, absolute=False):
    """A^T along `axis` (length 4 -> 2)"""
    p = [m[(slice(None),) * axis + (k,)] for k in range(4)]
    if absolute:
        outs = [p[0] + p[1] + p[2], p[1] + p[2] + p[3]]
    else:
        outs = [p[0] + p[1] + p[2], p[1] - p[2] - p[3]]
    return np.stack(outs, axis=axis)


def input_transform(xs, form, absolute=False, outside=None):
    """V of one sample.  xs: [D, H, W, C] (D, H - and W in the 3-D form - even); `outside`: what the out-of-volume voxels hold per
    channel, instead of zeros.  3-D: [64, blocks, C], component fz * 16 + fy * 4 + fx, blocks (zb, yb, xb) row-major.  2-D:
    [16, blocks, 3 * C], component fz * 4 + fy, blocks (zb, yb, x), the last axis dx-major"""
    d, h, w, c = xs.shape
    xp = np.zeros((d + 2, h + 2, w + 2, c), xs.dtype)
    if outside is not None:
        xp[:] = outside
    xp[1:-1, 1:-1, 1:-1] = xs
    v = _bt(_bt(xp, 0, absolute), 1, absolute)          # [zb, yb, W + 2, C, fz, fy]
    if form == 3:
        v = _bt(v, 2, absolute)                         # [zb, yb, xb, C, fz, fy, fx]
        return np.ascontiguousarray(v.transpose(4, 5, 6, 0, 1, 2, 3)).reshape(64, -1, c)
    v = np.stack([v[:, :, dx:dx + w] for dx in range(3)], axis=3)   # [zb, yb, W, dx, C, fz, fy]
    return np.ascontiguousarray(v.transpose(5, 6, 0, 1, 2, 3, 4)).reshape(16, -1, 3 * c)


def weight_transform(wt, form, absolute=False):
    """U_SCALE[form] * U as integers: [64, Cin, Cout] (3-D) or [16, 3 * Cin, Cout] (2-D, dx-major)"""
    g = np.abs(G2) if absolute else G2
    w = np.abs(wt) if absolute else wt
    cout, cin = w.shape[:2]
    if form == 3:
        return np.ascontiguousarray(np.einsum("az,by,cx,oizyx->abcio", g, g, g, w)).reshape(64, cin, cout)
    return np.ascontiguousarray(np.einsum("az,by,oizyx->abxio", g, g, w)).reshape(16, 3 * cin, cout)


def output_transform(m, form, vol, absolute=False):
    """per-component sums [components, blocks, Cout] of one sample -> [D, H, W, Cout] (still scaled by U_SCALE), axis by axis"""
    d, h, w = vol
    cout = m.shape[-1]
    if form == 3:
        m = m.reshape(4, 4, 4, d // 2, h // 2, w // 2, cout)
        y = _at(_at(_at(m, 0, absolute), 1, absolute), 2, absolute)           # [oz, oy, ox, zb, yb, xb, Cout]
        return y.transpose(3, 0, 4, 1, 5, 2, 6).reshape(d, h, w, cout)
    m = m.reshape(4, 4, d // 2, h // 2, w, cout)
    y = _at(_at(m, 0, absolute), 1, absolute)                                 # [oz, oy, zb, yb, x, Cout]
    return y.transpose(2, 0, 3, 1, 4, 5).reshape(d, h, w, cout)


def _even(x, form):
    """the volume padded with zeros to even sizes on the transformed axes (the kernels' tiles do the same past a ragged edge)"""
    n, d, h, w, c = x.shape
    pd, ph, pw = d % 2, h % 2, (w % 2 if form == 3 else 0)
    if pd or ph or pw:
        x = np.pad(x, ((0, 0), (0, pd), (0, ph), (0, pw), (0, 0)))
    return x


def sig_bits(a):
    """the widest element of an integer array in significant bits: the bit length of its odd part"""
    a = np.abs(np.asarray(a, np.int64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 0
    return int((a // (a & -a)).max()).bit_length()


# ------------------------------------------------------------------ the integer emulation
def emulate(form, x, wt, bias, addend=None, unit=1, product_bits=False):
    """The transform-domain pipeline of `form` (3: F(2x2x2, 3x3x3), 2: F(2x2, 3x3) over z, y) in integers.
    x: int64 [N, D, H, W, Cin], in units of 1 / unit (unit = 2: the half-integers of a normalised brick, doubled); wt: int64
    [Cout, Cin, 3, 3, 3]; bias, addend (or None): integers in real units.
    Returns Emulation: result = unit * (bias + conv + addend) as int64 [N, D, H, W, Cout], before the activation; bound = the
    largest partial sum of the all-absolute-values pipeline, in units of 1 / (U_SCALE * unit) - ASSERTED < 2^24 here; the
    widest V, U and (product_bits=True: sparse weights only) V * U in significant bits."""
    x = np.asarray(x, np.int64)
    wt = np.asarray(wt, np.int64)
    n, d, h, w, cin = x.shape
    cout = wt.shape[0]
    k = U_SCALE[form]
    xe = _even(x, form).astype(np.float64)  # float64 holds every quantity below exactly (asserted: < 2^52)
    vol = xe.shape[1:4]
    u = weight_transform(wt, form)
    uf, uaf = u.astype(np.float64), weight_transform(wt, form, absolute=True).astype(np.float64)
    b = k * unit * np.asarray(bias, np.int64)
    res = np.empty((n, d, h, w, cout), np.int64)
    bound, v_bits, p_bits = 0, 0, 0
    nz = np.argwhere(np.any(u != 0, axis=0)) if product_bits else None   # (row of U, cout) pairs with a weight
    for i in range(n):
        v = input_transform(xe[i], form)
        va = input_transform(np.abs(xe[i]), form, absolute=True)
        ma = np.matmul(va, uaf)
        assert ma.max() < 2.0 ** 52
        out = np.rint(output_transform(np.matmul(v, uf), form, vol)[:d, :h, :w]).astype(np.int64) + b
        outa = np.rint(output_transform(ma, form, vol, absolute=True)[:d, :h, :w]).astype(np.int64) + np.abs(b)
        if addend is not None:
            out = out + k * unit * np.asarray(addend[i], np.int64)
            outa = outa + k * unit * np.abs(np.asarray(addend[i], np.int64))
        assert not (out % k).any(), "the output transform must leave whole numbers"
        res[i] = out // k
        bound = max(bound, int(outa.max()), int(va.max()))
        vi = v.astype(np.int64)
        v_bits = max(v_bits, sig_bits(vi))
        if product_bits:
            assert len(nz) <= 12 * cout, "product_bits is for sparse weights"
            for r, o in nz:
                p_bits = max(p_bits, sig_bits(vi[:, :, r] * u[:, r, o][:, None]))
    assert bound < LIMIT, f"the all-absolute-values bound {bound} reaches 2^24: these operands are not exact in fp32"
    return Emulation(res, bound, v_bits, sig_bits(u), p_bits)


def emulate_f32(ops, rs, defect=None):
    """The same pipeline in fp32 arithmetic, as a kernel may order it: the producer norm (if any), U and V in float32, the sum
    over cin accumulated sequentially in float32 in a SHUFFLED channel order per sample, the output transform axis by axis in
    float32.  Returns float64 [N, D, H, W, Cout]: bias + conv + addend, before the activation.  `defect` (what the classes must
    see, tests/test_wino_exact_cpu.py): "drop_tap" - the weights of tap (0, 1, 2) are lost; "swap_pair" - the channel pairs
    of quad 1 change places in V only; "trunc_v16" - V keeps 16 significant bits; "shift_outside" - the producer norm is
    applied to the out-of-volume pieces too (padding in front of the norm)."""
    form = ops.form
    x = np.asarray(ops.x, np.float32)
    wt = np.asarray(ops.wt, np.int64)
    n, d, h, w, cin = x.shape
    assert d % 2 == 0 and h % 2 == 0 and w % 2 == 0
    if defect == "drop_tap":
        wt = wt.copy()
        wt[:, :, 0, 1, 2] = 0
    uf = (weight_transform(wt, form).astype(np.float64) / U_SCALE[form]).astype(np.float32)
    assert np.array_equal(uf.astype(np.float64) * U_SCALE[form], weight_transform(wt, form))
    res = np.empty((n, d, h, w, wt.shape[0]), np.float64)
    for i in range(n):
        xs, outside = x[i], None
        if ops.scale is not None:
            norm = lambda t: np.maximum(t * ops.scale[i] + ops.shift[i], np.float32(SLOPE) * (t * ops.scale[i] + ops.shift[i]))  # noqa: E731
            xs = norm(xs)
            if defect == "shift_outside":
                outside = norm(np.zeros(cin, np.float32))
        assert xs.dtype == np.float32
        v = input_transform(xs, form, outside=outside)
        assert v.dtype == np.float32
        if defect == "swap_pair":
            v = v.reshape(v.shape[0], v.shape[1], -1, cin).copy()
            v[..., [4, 5, 6, 7]] = v[..., [6, 7, 4, 5]]
            v = v.reshape(v.shape[0], v.shape[1], -1)
        if defect == "trunc_v16":
            mant, ex = np.frexp(v.astype(np.float64))
            v = np.ldexp(np.trunc(mant * 65536.0) / 65536.0, ex).astype(np.float32)
        m = np.zeros((v.shape[0], v.shape[1], wt.shape[0]), np.float32)
        for c in rs.permutation(v.shape[2]):
            m += v[:, :, c, None] * uf[:, c, None, :]
        out = output_transform(m, form, (d, h, w)) + np.asarray(ops.bias, np.float32)
        if ops.addend is not None:
            out = out + np.asarray(ops.addend[i], np.float32)
        assert out.dtype == np.float32
        res[i] = out.astype(np.float64)
    return res


# ------------------------------------------------------------------ operands
def _rs(*key):
    return np.random.RandomState(zlib.crc32(" ".join(str(k) for k in key).encode()) % (2 ** 31))


def tap_class(form, tap):
    """log2 of s (module docstring): the number of transformed axes on which the tap is an outer one"""
    dz, dy, dx = TAPS[tap]
    return int(dz != 1) + int(dy != 1) + (int(dx != 1) if form == 3 else 0)


def _wide(rs, bits, size):
    """random integers of exactly `bits` significant bits: top bit and bit 0 set, random sign"""
    mag = rs.randint(0, 1 << (bits - 1), size=size).astype(np.int64) | (1 << (bits - 1)) | 1
    return mag * rs.choice(np.array([-1, 1], np.int64), size=size)


def _one_weight_per_cout(form, cin, cout):
    """(channel, tap) of every output channel of the bits classes: o reads channel o % cin through a tap of that channel's class"""
    ncls = 4 if form == 3 else 3
    by_class = [[t for t in range(27) if tap_class(form, t) == k] for k in range(ncls)]
    ch = np.arange(cout) % cin
    tap = np.array([by_class[c % ncls][(o // cin) % len(by_class[c % ncls])] for o, c in enumerate(ch)])
    return ch, tap


def _split_bits(total):
    """(bits of x, bits of w) of class `mid` for a budget of `total` bits"""
    xb = (total + 3) // 2
    return xb, total - xb


def operands(cls, form, shape, cin, cout, key, head=0, addend=False):
    """Operands of class `cls` for the kernel of `form`, deterministic per `key`.  shape = (N, D, H, W)"""
    assert cls in CLASSES, cls
    rs = _rs(key, cls, form)
    n, d, h, w = shape
    xs, ws = (n, d, h, w, cin), (cout, cin, 3, 3, 3)
    scale = shift = head_w = head_b = add = None
    if cls in ("dense", "norm", "head"):
        shim = namedtuple("Shim", "name shape cin cout")(f"{key} {cls} {form}", tuple(shape), cin, cout)
        x, wt, b = U.int_operands(shim)
    elif cls == "taps":
        assert cout >= 27 and cout >= cin, "taps needs an output channel per tap and per input channel"
        x = rs.randint(-4095, 4096, size=xs).astype(np.int64)
        o = np.arange(cout)
        wt = np.zeros(ws, np.int64)
        gain = rs.randint(1, 4, size=cout) * rs.choice(np.array([-1, 1]), size=cout)
        wt.reshape(cout, cin, 27)[o, o % cin, o % 27] = gain
        b = rs.randint(-8, 9, size=cout).astype(np.int64)
    else:
        ncls = 4 if form == 3 else 3
        budget = WIDTH_BUDGET[form] - np.arange(cin) % ncls          # per input channel
        ch, tap = _one_weight_per_cout(form, cin, cout)
        wt = np.zeros(ws, np.int64)
        wflat = wt.reshape(cout, cin, 27)
        x = np.empty(xs, np.int64)
        for c in range(cin):
            xb = {"wide_x": budget[c], "wide_w": 0, "mid": _split_bits(budget[c])[0]}[cls]
            x[..., c] = rs.randint(-1, 2, size=xs[:4]) if xb == 0 else rs.randint(-(1 << xb) + 1, 1 << xb, size=xs[:4])
        for o in range(cout):
            wb = {"wide_x": 1, "wide_w": budget[ch[o]], "mid": _split_bits(budget[ch[o]])[1]}[cls]
            wflat[o, ch[o], tap[o]] = _wide(rs, wb, 1)[0] if wb > 1 else rs.choice(np.array([-1, 1]))
        b = rs.randint(-8, 9, size=cout).astype(np.int64)
    if cls == "norm":
        scale = rs.choice(np.array([1.0, 2.0, 4.0], np.float32), size=(n, cin))
        shift = (rs.randint(1, 4, size=(n, cin)) * rs.choice(np.array([-1, 1]), size=(n, cin))).astype(np.float32)
    if head:
        head_w = rs.randint(-2, 3, size=(head, cout)).astype(np.int64)
        head_b = rs.randint(-4, 5, size=head).astype(np.int64)
    if addend:
        add = rs.randint(-8, 9, size=(n, d, h, w, cout)).astype(np.int64)
    return Operands(cls, form, x, wt, b, scale, shift, head_w, head_b, add)


def staged(ops):
    """(the brick the conv multiplies, in units of 1 / unit, int64; unit): x itself, or 2 * LeakyReLU(x * scale + shift, 0.5)"""
    if ops.scale is None:
        return ops.x, 1
    pre = ops.x * ops.scale.astype(np.int64)[:, None, None, None, :] + ops.shift.astype(np.int64)[:, None, None, None, :]
    return np.where(pre >= 0, 2 * pre, pre), 2


Expected = namedtuple("Expected", "unit pre y_scaled logits2 emu")


def expected(ops, product_bits=False):
    """The integer reference of a set of operands, its emulation compared and the bound asserted.
    pre: unit * (bias + conv + addend), int64, from conv_rows_util.int_conv; y_scaled = 2 * unit * LeakyReLU(., 0.5), what
    2 * unit * the kernel's output must equal; logits2 = 2 * unit * the head's logits (or None)."""
    xu, unit = staged(ops)
    pre = U.int_conv(xu, ops.wt, unit * ops.bias, 1)
    if ops.addend is not None:
        pre = pre + unit * ops.addend
    emu = emulate(ops.form, xu, ops.wt, ops.bias, addend=ops.addend, unit=unit, product_bits=product_bits)
    assert np.array_equal(emu.result, pre), "the transform-domain emulation differs from the integer conv"
    y = np.where(pre >= 0, 2 * pre, pre)
    logits2 = None
    if ops.head_w is not None:
        logits2 = np.einsum("ndhwc,kc->nkdhw", y, ops.head_w) + 2 * unit * ops.head_b[None, :, None, None, None]
        worst = np.einsum("ndhwc,kc->nkdhw", np.abs(y), np.abs(ops.head_w)).max() + 2 * unit * np.abs(ops.head_b).max()
        assert worst < LIMIT, "the head's partial sums leave fp32's integers"
    return Expected(unit, pre, y, logits2, emu)


def assert_bits(cls, emu):
    """the condition of a bits class: what it is about is wider than two bf16 pieces (16 significant bits)"""
    got = {"wide_x": emu.v_bits, "wide_w": emu.u_bits, "mid": emu.product_bits}[cls]
    assert got > 16, f"{cls}: the widest {'V' if cls == 'wide_x' else 'U' if cls == 'wide_w' else 'product'} has only {got} significant bits"
    return got


def describe_tap_failure(ops, y_scaled, got_scaled):
    """for class `taps`: which tap, channel, tile and 2x2x2 block the first wrong output belongs to"""
    bad = np.argwhere(got_scaled != y_scaled)
    if bad.size == 0:
        return ""
    n, z, y, x, o = (int(v) for v in bad[0])
    cin = ops.wt.shape[1]
    dz, dy, dx = TAPS[o % 27]
    tz, ty, tx = TILE[ops.form]
    return (f"{len(bad)} outputs differ, first at (n, z, y, x, cout) = {(n, z, y, x, o)}: {got_scaled[n, z, y, x, o]} instead of "
            f"{y_scaled[n, z, y, x, o]} (in units of 1/2): cout {o} reads tap (dz, dy, dx) = {(dz, dy, dx)} of input channel {o % cin} "
            f"(chunk {o % cin // 16}, quad {o % cin % 16 // 4}, pair {o % cin % 4 // 2}) with gain {int(ops.wt[o, o % cin, dz, dy, dx])}; "
            f"tile (z, y, x) = {(z // tz, y // ty, x // tx)} of sample {n}, 2x2x2 block {(z % tz // 2, y % ty // 2, x % tx // 2)} of it, "
            f"output {(z % 2, y % 2, x % 2)} of the block")


# ------------------------------------------------------------------ the persistent grid (conv_plan.h persistent_grid_x, the kernels' tile ranges)
def persistent_grid_x(workgroups, gy, tiles):
    """grid.x of a persistent kernel: `workgroups` on the chip shared by the gy cout blocks, a multiple of 8, no more than the
    tiles need"""
    gx = workgroups // gy
    gx = 8 if gx < 8 else gx // 8 * 8
    return min(gx, (tiles + 7) // 8 * 8)


def workgroup_tiles(gx, tiles):
    """the tile ids each of the gx workgroups of a cout block walks: XCD group b & 7 owns one contiguous range of tile ids (the
    first tiles % 8 ranges are one longer), its workgroups stride through it"""
    q8, r8 = divmod(tiles, 8)
    out = []
    for b in range(gx):
        xcd, li = b & 7, b >> 3
        nl = (gx - xcd + 7) >> 3
        lo = xcd * q8 + min(xcd, r8)
        hi = lo + q8 + (1 if xcd < r8 else 0)
        out.append(list(range(lo + li, hi, nl)))
    return out


# ------------------------------------------------------------------ the GPU cases
# entry: "wino3" = the forced single-op entry mi355_conv3d_wino3_ndhwc, "fused" = mi355_conv3d_fused_ndhwc (through the planner);
# shape = (N, D, H, W); grid = (grid.x, grid.y) the case counts on; classes: the operand classes it runs;
# reaches: what the launch must contain, asserted on the CPU from the grid - "few" (fewer than 8 tiles: workgroups that return at
# once), "r8" (a tile count that is no multiple of 8), "second" (a workgroup walks a second tile), "sample" (a workgroup's
# consecutive tiles lie in different samples), "ragged" (the volume is no whole number of tiles)
Case = namedtuple("Case", "name entry form shape c0 c1 cout stats norm head addend kernel grid classes reaches")

W3, W2 = "conv3_f32_wino3_kernel<%s>", "conv3_f32_wino2_kernel<%d>"
BOTH = ("dense", "taps")


def _forced(name, shape, c0, c1, cout, grid, reaches, classes=BOTH):
    return [Case(name, "wino3", 3, shape, c0, c1, cout, False, False, 0, False, W3 % "0, false", grid, classes, reaches),
            Case(name + "_addend", "wino3", 3, shape, c0, c1, cout, False, False, 0, True, W3 % "3, false", grid,
                 tuple(k for k in classes if k not in BITS_CLASSES), reaches)]


def _planned(name, form, shape, c0, c1, cout, kernel, grid, reaches, classes=BOTH, stats=False, norm=False, head=0):
    return Case(name, "fused", form, shape, c0, c1, cout, stats, norm, head, False, kernel, grid, classes, reaches)


GPU_CASES = [
    # ---- conv3_f32_wino3_kernel<0, false> / <3, false> through the forced entry
    # one tile: every halo piece from the zero page, seven of the eight XCD ranges empty
    *_forced("w3_one_tile", (1, 4, 8, 8), 16, 0, 32, (8, 1), ("few", "r8")),
    # 12 tiles on 16 workgroups: r8 = 4; also where the bits classes run
    *_forced("w3_r8", (3, 4, 16, 16), 16, 0, 32, (16, 1), ("r8",), BOTH + BITS_CLASSES),
    # 96 tiles on 64 workgroups: second tiles, tile ranges that cross a sample
    *_forced("w3_second_tile", (3, 8, 32, 32), 16, 0, 128, (64, 4), ("second", "sample")),
    # concat 32 + 16: three chunks, the last one from the second tensor; two cout blocks
    *_forced("w3_concat", (2, 8, 16, 16), 32, 16, 64, (16, 2), ()),
    # ---- conv3_f32_wino3_kernel through the planner
    _planned("w3_stats", 3, (3, 4, 16, 16), 128, 0, 256, W3 % "2, false", (16, 8), ("r8",), stats=True),
    _planned("w3_stats_second_tile", 3, (12, 4, 16, 16), 128, 0, 256, W3 % "2, false", (32, 8), ("second", "sample"), stats=True),
    _planned("w3_norm", 3, (3, 4, 16, 16), 128, 0, 256, W3 % "2, true", (16, 8), ("r8",), ("norm",), stats=True, norm=True),
    _planned("w3_norm_second_tile", 3, (12, 4, 16, 16), 128, 0, 256, W3 % "2, true", (32, 8), ("second", "sample"), ("norm",), stats=True, norm=True),
    _planned("w3_deep", 3, (10, 8, 8, 24), 128, 0, 128, W3 % "0, false", (64, 4), ("r8",)),
    _planned("w3_head", 3, (16, 16, 32, 32), 16, 0, 32, W3 % "1, false", (256, 1), ("second", "sample"), ("head",), head=3),
    # ---- conv3_f32_wino2_kernel through the planner: ragged in z, y and x
    _planned("w2_second_tile", 2, (16, 6, 7, 40), 16, 0, 128, W2 % 0, (64, 4), ("second", "sample", "ragged"), BOTH + BITS_CLASSES),
    _planned("w2_stats", 2, (16, 6, 7, 40), 16, 0, 128, W2 % 2, (64, 4), ("second", "sample", "ragged"), stats=True),
    _planned("w2_cout320", 2, (7, 5, 6, 33), 32, 0, 320, W2 % 0, (24, 10), ("second", "sample", "ragged")),
    _planned("w2_head", 2, (64, 6, 7, 40), 16, 0, 32, W2 % 1, (256, 1), ("second", "sample", "ragged"), ("head",), head=3),
    _planned("w2_concat", 2, (16, 5, 5, 33), 16, 16, 128, W2 % 0, (64, 4), ("second", "sample", "ragged")),
]
assert len({c.name for c in GPU_CASES}) == len(GPU_CASES)

#: every instantiation of the two kernels: each must be the kernel of some case
INSTANTIATIONS = [W3 % "0, false", W3 % "1, false", W3 % "2, false", W3 % "2, true", W3 % "3, false", W2 % 0, W2 % 1, W2 % 2]

RUNS = [(c, cls) for c in GPU_CASES for cls in c.classes]


def case_tiles(c):
    tz, ty, tx = TILE[c.form]
    n, d, h, w = c.shape
    return n * -(-d // tz) * -(-h // ty) * -(-w // tx)


def case_operands(c, cls):
    return operands(cls, c.form, c.shape, c.c0 + c.c1, c.cout, c.name, head=c.head, addend=c.addend)


def checked_case(c, cls):
    """(operands, Expected) of a GPU run: the reference computed, the emulation equal to it, the bound asserted - and for a bits
    class its condition.  The GPU module takes its operands from here only"""
    ops = case_operands(c, cls)
    exp = expected(ops, product_bits=cls in BITS_CLASSES)
    if cls in BITS_CLASSES:
        assert_bits(cls, exp.emu)
    return ops, exp
