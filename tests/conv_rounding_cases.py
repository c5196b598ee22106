"""Operands at which the store of every MFMA conv kernel ROUNDS, and what it has to store, bit for bit.

The bit-exact conv tests elsewhere draw x in [-2, 2], w in [-1, 1] and bias in [-3, 3]: their sums stay below 256, where bf16
holds every integer, so the fp32 -> bf16 / e4m3 conversion of the epilogues never rounds there -- they pin layout, swizzle and
fragment maps.  This module widens the integers: x in [-15, 15] and w in [-7, 7] (bf16 AND e4m3 hold both ranges exactly), the
bias in multiples of 1/4 up to 64, every second channel a whole number (ties at magnitudes >= 256 need integer sums), the
addend of the data gradient / the residual conv in bf16 values (integers up to 255, halves below 128).  Every product and every
partial sum in any order is then an exact fp32 value as long as 4 * mag < 2^24 (two fractional bits), so the accumulator is
KNOWN and the stored value must be THE round-to-nearest-even of it: `stored_bf16(exact(...))`, compared with np.array_equal.

    exact         float64 accumulator v and mag = sum |x w| + |b| + |addend| of a forward conv (bias, relu), a data gradient
                  (+ addend, mask > 0 select) or a residual 1x1 conv (relu(conv + b) + residual)
    stored_bf16   ONE rounding (oracle.fcn_oracle.round_bf16);  stored_e4m3: one rounding after the power-of-two scale,
                  saturating at +-448 (round_e4m3);  pool2x2: the maximum of the STORED values
    route_bytes   the routed pool's header rule on the stored relu'd map (first maximum among stored values)
    truncated_bf16, half_away_bf16, accumulator_route_bytes: the WRONG rules, for the sensitivity checks of
                  tests/test_conv_rounding_cases_cpu.py -- no GPU test uses them

The case table gives, per tile configuration, the smallest map the configuration tiles exactly, and four rows and columns more
where it takes partial tiles; two images so that a tile walk crosses an image; 64, 128 and (once per generation) 512 input
channels; 128 output channels so that configuration 1 applies.  Which configuration the library picks is asked of
xv_conv2d_choose_cfg by the GPU test, not restated here.  The 1x1 shapes are those of conv1x1_cases.build_cases.
No torch at module level: numpy and the oracle's roundings are imported when called."""
import collections

X_MAX, W_MAX = 15, 7
B_MAX = 64                          # |bias| <= 64 in multiples of 1/4 (the route case: ROUTE_B_MAX)
ROUTE_B_MAX = 65536
ADD_INT_MAX = 255                   # the addend: an integer up to 255 ...
ADD_HALVES = 255                    # ... or this many halves at the most: up to 127.5
DY_MAX_1X1 = 31                     # the 1x1 data gradient's dy (bf16 only: not tied to what e4m3 holds)

Case = collections.namedtuple('Case', 'name kind k n h w cin cout f8_in b_max x_max')
Case.__new__.__defaults__ = (X_MAX,)
Operands = collections.namedtuple('Operands', 'x w b addend mask')   # float32: [n,h,w,cin], HWIO, [cout], [n,h,w,cout] twice

# the smallest map each 3x3 tile configuration tiles exactly; `partial`: it also takes maps it does not tile
TILES = collections.OrderedDict([
    (1, (8, 16, True)), (14, (16, 16, True)), (15, (8, 32, True)), (16, (16, 32, True)),      # generation 1
    (17, (16, 32, True)), (22, (24, 16, True)),                                                # generation 2
    (24, (16, 32, True)), (26, (16, 32, True)),                                                # generation 4 (EDGE forms)
    (27, (24, 16, False)), (28, (32, 16, False)),                                              # generation 5
])
GENERATION = {1: 1, 14: 1, 15: 1, 16: 1, 17: 2, 22: 2, 18: 3, 23: 3, 24: 4, 26: 4, 27: 5, 28: 5}


def _fwd3_cases():
    exact_maps, partial_maps = [], []
    for th, tw, partial in TILES.values():
        if (th, tw) not in exact_maps:
            exact_maps.append((th, tw))
        if partial and (th + 4, tw + 4) not in partial_maps:
            partial_maps.append((th + 4, tw + 4))
    cases = []
    for h, w in exact_maps:
        for cin in (64, 128):
            cases.append(Case('fwd3-%dx%d-c%d' % (h, w, cin), 'fwd', 3, 2, h, w, cin, 128, (h, w) == (16, 32), B_MAX))
    for h, w in partial_maps:
        cases.append(Case('fwd3-%dx%d-c64' % (h, w), 'fwd', 3, 3, h, w, 64, 128, False, B_MAX))
    # e4m3 operands on partial tiles (128-channel chunks: configurations 14 - 16 and 24)
    cases.append(Case('fwd3-20x36-c128', 'fwd', 3, 2, 20, 36, 128, 128, True, B_MAX))
    # the longest sum, once per generation: 16x32 (1, 14 - 17, 24, 26), 24x16 (22, 27: the chunk-group summation that
    # xv_conv2d_fwd_split splits), 32x16 (28)
    for h, w, f8 in ((16, 32, True), (24, 16, False), (32, 16, False)):
        cases.append(Case('fwd3-%dx%d-c512' % (h, w), 'fwd', 3, 2, h, w, 512, 128, f8, B_MAX))
    return cases


FWD3 = _fwd3_cases()
SPLIT_CASE = 'fwd3-24x16-c512'
STREAMK_CASE = 'fwd3-16x32-c512'
STATS_CASE = 'fwd3-16x32-c64'

# the data gradient: maps the chooser sends to 26, 27, a first-generation tile and generation 2 (the GPU test asserts the pick)
DGRAD3 = [
    Case('dgrad3-16x32', 'dgrad', 3, 2, 16, 32, 128, 64, False, 0),
    Case('dgrad3-24x16', 'dgrad', 3, 2, 24, 16, 64, 128, False, 0),
    Case('dgrad3-8x16', 'dgrad', 3, 3, 8, 16, 64, 64, False, 0),
    Case('dgrad3-20x36', 'dgrad', 3, 2, 20, 36, 64, 64, False, 0),
]
DGRAD3_PICK = {'dgrad3-16x32': (26,), 'dgrad3-24x16': (27,), 'dgrad3-8x16': (1, 14, 15, 16), 'dgrad3-20x36': (17, 22)}

# the routed pool: the pooled map tiles in 16x32 too (the data gradient behind the pool runs at that size); the bias is
# widened so that a window's accumulators sit close together at a magnitude where bf16 steps by 2 and more
ROUTE = Case('route-32x64', 'route', 3, 2, 32, 64, 64, 128, False, ROUTE_B_MAX)
ROUTE_C2 = 64                       # output channels of the layer behind the pool

# 1x1: rows of conv1x1_cases.ROWS -- the three flat-GEMM forms and a first-generation fallback.  The e4m3 inputs run on the
# row with the longest sum (512 channels): a quarter of a shorter one is so small that bf16 holds most of the values.
ROWS_1X1 = (('g128', 'one_partial'), ('wide', 'noremap_tail'), ('n64', 'one_partial'), ('gen1', 'k128'))
ROW_1X1_F8 = ('wide', 'noremap_tail')
ROWS_1X1_DGRAD = ROWS_1X1[:3]       # configurations 18, 18 and 23


def cases_1x1(cus):
    """{row: Case} from conv1x1_cases.build_cases(cus): K reduction channels onto C output channels."""
    import conv1x1_cases as cc
    built = {(c.form, c.prop): c for c in cc.build_cases(cus)}
    out = collections.OrderedDict()
    for row in ROWS_1X1:
        c = built[row]
        out[row] = Case('k1-%s-%s' % row, 'k1', 1, c.n, c.h, c.w, c.k, c.c, row == ROW_1X1_F8, B_MAX)
    return out


def cases_1x1_dgrad(cus):
    """{row: Case} of the 1x1 data gradients on the same shapes: dy of K channels onto dx of C.  There is no bias in quarters
    here and sums over 128 to 512 channels of [-15, 15] stay so small that fewer than half of them round, so dy is widened to
    [-31, 31] (bf16 holds it; no e4m3 map takes part)."""
    out = collections.OrderedDict()
    for row, c in cases_1x1(cus).items():
        if row in ROWS_1X1_DGRAD:
            out[row] = c._replace(name='k1d-%s-%s' % row, kind='dgrad', f8_in=False, b_max=0, x_max=DY_MAX_1X1)
    return out


def case_id(c):
    return c.name


def seed(case):
    """The seed of a case's draw: a function of its name, so that the CPU conditions hold for the operands the GPU test uses."""
    import zlib
    return zlib.crc32(case.name.encode()) % 2 ** 31


def in_scales(case):
    """The input scale exponents an e4m3-input case runs at (a power-of-two scale keeps every sum exact)."""
    return (0, -2) if case.f8_in else ()


def fwd3_case(name):
    """The 3x3 forward case of that name."""
    return [c for c in FWD3 if c.name == name][0]


# the mask values the select has to tell apart: > 0 keeps; zero of either sign, and anything negative, clears
SPECIAL_MASK = (0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0)
SPECIAL_KEEPS = (False, False, True, False, True, False)
MASK_VALUES = (-1.0, 0.0, 0.5, 1.0, 1.5)


def draw(case, seed):
    """x in [-15, 15] (the 1x1 data gradient: [-x_max, x_max]), w in [-7, 7] (HWIO), bias in multiples of 1/4 up to b_max with every second channel whole, the addend
    from integers up to 255 and halves below 128, the mask map from MASK_VALUES with SPECIAL_MASK in the first channels of
    the first pixel and in the last channels of the last pixel.  For an e4m3 input map the same x is the STORED integer: with
    an input scale_exp of e the real input is x 2^e (`exact(..., in_scale_exp=e)`)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    shape = (case.n, case.h, case.w)
    x = rng.integers(-case.x_max, case.x_max + 1, shape + (case.cin,)).astype(np.float32)
    w = rng.integers(-W_MAX, W_MAX + 1, (case.k, case.k, case.cin, case.cout)).astype(np.float32)
    b = (rng.integers(-4 * case.b_max, 4 * case.b_max + 1, case.cout) / 4.0).astype(np.float32)
    b[::2] = rng.integers(-case.b_max, case.b_max + 1, b[::2].shape)
    ints = rng.integers(-ADD_INT_MAX, ADD_INT_MAX + 1, shape + (case.cout,))
    halves = rng.integers(-ADD_HALVES, ADD_HALVES + 1, shape + (case.cout,)) / 2.0
    addend = np.where(rng.integers(0, 2, shape + (case.cout,)) == 1, ints, halves).astype(np.float32)
    mask = rng.choice(np.asarray(MASK_VALUES, dtype=np.float32), size=shape + (case.cout,))
    mask[0, 0, 0, :6] = SPECIAL_MASK
    mask[-1, -1, -1, -6:] = SPECIAL_MASK
    return Operands(x, w, b, addend, mask)


def conv_sums(x, w):
    """(sum x w, sum |x w|) of the 'same' convolution in float64: x [n,h,w,cin], w HWIO [k,k,cin,cout], k odd."""
    import numpy as np
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n, h, wd, cin = x.shape
    k, p = w.shape[0], w.shape[0] // 2
    xp = np.zeros((n, h + 2 * p, wd + 2 * p, cin))
    xp[:, p:p + h, p:p + wd] = x
    v = np.zeros((n * h * wd, w.shape[3]))
    mag = np.zeros_like(v)
    for ty in range(k):
        for tx in range(k):
            patch = xp[:, ty:ty + h, tx:tx + wd].reshape(-1, cin)
            v += patch @ w[ty, tx]
            mag += np.abs(patch) @ np.abs(w[ty, tx])
    return v.reshape(n, h, wd, -1), mag.reshape(n, h, wd, -1)


def exact(sums, b=None, relu=False, addend=None, mask=None, residual=None, in_scale_exp=0):
    """(v, mag) in float64 from `sums = conv_sums(x, w)` (left unchanged):
        forward        v = conv + b, then relu
        data gradient  v = conv (+ addend), then where(mask > 0, v, 0)
        residual 1x1   v = relu(conv + b) + residual
    mag = sum |x w| + |b| + |addend| (+ |residual|).  in_scale_exp: the power-of-two scale of an e4m3 input map."""
    import numpy as np
    v, mag = sums[0] * 2.0 ** in_scale_exp, sums[1] * 2.0 ** in_scale_exp
    if b is not None:
        v = v + np.asarray(b, dtype=np.float64)
        mag = mag + np.abs(np.asarray(b, dtype=np.float64))
    if relu:
        v = np.maximum(v, 0.0)
    for a in (addend, residual):
        if a is not None:
            v = v + np.asarray(a, dtype=np.float64)
            mag = mag + np.abs(np.asarray(a, dtype=np.float64))
    if mask is not None:
        v = np.where(np.asarray(mask, dtype=np.float64) > 0, v, 0.0)
    return v, mag


def stored_bf16(v):
    """ONE round-to-nearest-even of the exact accumulator to bf16, as float32."""
    import numpy as np
    from oracle.fcn_oracle import round_bf16
    v32 = np.asarray(v).astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v), 'the accumulator is not an fp32 value'
    return round_bf16(v32)


def stored_e4m3(v, scale_exp):
    """ONE round-to-nearest-even of v 2^-scale_exp to e4m3, saturating at +-448; returned in real units (float32)."""
    import numpy as np
    from oracle.fcn_oracle import round_e4m3
    return round_e4m3(np.asarray(v, dtype=np.float64), scale_exp)


def pool2x2(stored):
    """The 2x2 / 2 maximum of the STORED map [n,h,w,c]."""
    return windows(stored).max(-1)


def windows(a):
    """[n,h,w,c] -> [n,h/2,w/2,c,4]: the pooling windows in MaxPoolGrad's order (row 0 columns 0, 1, row 1 columns 0, 1)."""
    n, h, w, c = a.shape
    return a.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


def route_bytes(stored):
    """The routed pool's rule on the STORED relu'd map: 0 where the window's maximum is not positive, else 0x80 >> the first
    position of the maximum (numpy's argmax is the first)."""
    import numpy as np
    win = windows(stored)
    return np.where(win.max(-1) > 0, 0x80 >> win.argmax(-1), 0).astype(np.uint8)


def e4m3_scales(v):
    """(in-range, saturating) output scale exponents for the accumulators v: the smallest exponent at which fewer than 1 % of
    the outputs lie beyond +-448 (a finer grid than the one max |v| asks for, so more values sit on ties), and two below it.
    Taken from the accumulators WITHOUT relu and used for both forms of a case."""
    import numpy as np
    a = np.abs(np.asarray(v, dtype=np.float64))
    top = float(np.quantile(a, 0.995))
    e = int(np.ceil(np.log2(max(top, 1.0) / 448.0)))
    while (a > 448.0 * 2.0 ** e).mean() >= 0.01:
        e += 1
    return e, e - 2


# ---- what the comparison is sensitive to (CPU checks only) -------------------------------------------------------------

def _bits(v):
    import numpy as np
    return np.asarray(v).astype(np.float32).view(np.uint32)


def truncated_bf16(v):
    """The WRONG store: the upper 16 bits of the fp32 value."""
    import numpy as np
    return (_bits(v) & np.uint32(0xffff0000)).view(np.float32)


def half_away_bf16(v):
    """The WRONG store: round half away from zero (add 0x8000 to the bits, truncate)."""
    import numpy as np
    return ((_bits(v) + np.uint32(0x8000)) & np.uint32(0xffff0000)).view(np.float32)


def bf16_tie_classes(v):
    """(rounds, tie_down, tie_up) boolean maps of the accumulators v: changed by the bf16 rounding; exact ties whose even
    neighbour is the one nearer zero / farther from zero."""
    import numpy as np
    bits = _bits(v)
    low = bits & np.uint32(0xffff)
    tie = low == 0x8000
    odd = (bits >> np.uint32(16)) & np.uint32(1)
    return low != 0, tie & (odd == 0), tie & (odd == 1)


def e4m3_classes(v, scale_exp):
    """(rounds, tie, saturates) of the e4m3 store at `scale_exp`: `rounds` = the stored value differs from v."""
    import numpy as np
    a = np.abs(np.asarray(v, dtype=np.float64)) * 2.0 ** -scale_exp
    sat = a > 448.0
    with np.errstate(divide='ignore'):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    step = 2.0 ** (np.maximum(e, -6.0) - 3.0)
    frac = a / step - np.floor(a / step)
    return stored_e4m3(v, scale_exp) != np.asarray(v, dtype=np.float32), (frac == 0.5) & ~sat, sat


def accumulator_route_bytes(v):
    """The WRONG route rule: the first maximum among the relu'd ACCUMULATORS."""
    import numpy as np
    return route_bytes(np.maximum(np.asarray(v, dtype=np.float64), 0.0))


def route_split_windows(v):
    """Windows in which two DIFFERENT accumulators store as the SAME maximal positive bf16 value: boolean [n,h/2,w/2,c]."""
    import numpy as np
    s = windows(stored_bf16(np.maximum(v, 0.0)))
    a = windows(np.maximum(v, 0.0))
    top = s.max(-1, keepdims=True)
    at_top = (s == top) & (top > 0)
    amax = np.where(at_top, a, -np.inf).max(-1)
    amin = np.where(at_top, a, np.inf).min(-1)
    return (at_top.sum(-1) >= 2) & (amax != amin)


# ---- weights for the packers (fp32 values that are NOT bf16 / e4m3 values) ----------------------------------------------

PACK_CLASSES = ('exact', 'below_half', 'tie_even', 'tie_odd', 'above_half')
BF16_MAX = float.fromhex('0x1.fep127')


def packer_weights(shape, seed):
    """(w float32 of `shape`, class index per element): w = t + f ulp(t), t a random bf16 value of either sign over twelve
    binades (2^-8 .. 2^4), f in {0, +-1/4, +-1/2, +-3/4} taken AWAY from zero so that ulp(t) is the spacing on that side; then
    +-0 and the largest finite bf16 plus a quarter ulp planted at the front.  No fp32 subnormals."""
    import numpy as np
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    mant = rng.integers(128, 256, size).astype(np.float64)                 # 8 significant bits
    expo = rng.integers(-8, 4, size)                                       # twelve binades
    sign = rng.choice(np.array([-1.0, 1.0]), size)
    quarters = rng.integers(0, 4, size)                                    # f = quarters / 4 of an ulp, away from zero
    ulp = 2.0 ** (expo - 7.0)
    w = sign * (mant + quarters / 4.0) * ulp
    cls = np.select([quarters == 0, quarters == 1, (quarters == 2) & (mant % 2 == 0), quarters == 2], [0, 1, 2, 3], 4)
    w[:2] = (0.0, -0.0)
    cls[:2] = 0
    w[2:4] = (BF16_MAX + 2.0 ** 118, -BF16_MAX - 2.0 ** 118)              # ulp = 2^120: a quarter above the largest finite
    cls[2:4] = 1
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w)
    return w32.reshape(shape), cls.reshape(shape)


def packer_weights_e4m3(shape, scale_exp, seed):
    """fp32 weights around the e4m3 grid of `scale_exp`: q = (m + f) 2^(e - 3) 2^scale_exp with m in 8 .. 15, e over the
    normal binades 2^-6 .. 2^8 and below them (subnormal step 2^-9), f in quarters; so ties of both parities occur, and
    whatever exceeds 448 after scaling (m + f > 14 at e = 8; a sixteenth of the weights is put at m = 15 there) saturates.  Returns (w, class, saturates)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    mant = rng.integers(8, 16, size).astype(np.float64)
    expo = rng.integers(-6, 9, size)
    sign = rng.choice(np.array([-1.0, 1.0]), size)
    quarters = rng.integers(0, 4, size)
    sub = rng.integers(0, 8, size) == 0                                    # an eighth of them on the subnormal grid
    mant = np.where(sub, rng.integers(0, 8, size), mant)
    expo = np.where(sub, -6, expo)
    big = rng.integers(0, 16, size) == 0                                   # a sixteenth at 480 .. 510: beyond 448
    mant = np.where(big, 15.0, mant)
    expo = np.where(big, 8, expo)
    a = (mant + quarters / 4.0) * 2.0 ** (expo - 3.0)
    w = sign * a * 2.0 ** scale_exp
    cls = np.select([quarters == 0, quarters == 1, (quarters == 2) & (mant % 2 == 0), quarters == 2], [0, 1, 2, 3], 4)
    w[:2] = (0.0, -0.0)
    cls[:2] = 0
    a[:2] = 0
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w)
    return w32.reshape(shape), cls.reshape(shape), (a > 448.0).reshape(shape)


def one_hot_map(n, h, w, cin, k):
    """A bf16-exact input that reads a packed weight image back through the conv: value 1.0 in channel c at ONE pixel, the
    pixels three apart and one inside the border for k = 3 (a 16x32 map holds 50), any pixel for k = 1.  With zero bias and no
    relu y[pixel - tap offset, co] = w[tap, c, co]: every weight appears once, with no second rounding.
    Returns (x, [(image, row, column) of channel c])."""
    import numpy as np
    if k == 3:
        pix = [(y, x) for y in range(1, h - 1, 3) for x in range(1, w - 1, 3)]
    else:
        pix = [(y, x) for y in range(h) for x in range(w)]
    assert n * len(pix) >= cin, 'the maps hold %d pixels for %d channels' % (n * len(pix), cin)
    x = np.zeros((n, h, w, cin), dtype=np.float32)
    where = []
    for c in range(cin):
        img, (py, px) = c // len(pix), pix[c % len(pix)]
        x[img, py, px, c] = 1.0
        where.append((img, py, px))
    return x, where


def read_back(y, where, k):
    """The weights [k,k,cin,cout] a one-hot run of `one_hot_map` shows in its output y [n,h,w,cout]."""
    import numpy as np
    p = k // 2
    out = np.zeros((k, k, len(where), y.shape[-1]), dtype=y.dtype)
    for c, (img, py, px) in enumerate(where):
        for ty in range(k):
            for tx in range(k):
                out[ty, tx, c] = y[img, py - (ty - p), px - (tx - p)]
    return out


def dgrad_forward_weights(w_eff):
    """The FORWARD kernel [k,k,cin,cout] whose data-gradient convolution has the HWIO weights w_eff [k,k,cout,cin]:
    point-reflected taps, channels swapped."""
    import numpy as np
    return np.ascontiguousarray(w_eff[::-1, ::-1].transpose(0, 1, 3, 2))
