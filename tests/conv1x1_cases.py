"""Shapes that put a 1x1 conv onto each flat-GEMM kernel of csrc/conv1x1_gemm.hip, and the float64 references of its epilogue.

A padded NHWC map is a dense [Mp = n (h + 2) (w + 2)][channels] matrix and a 1x1 conv a GEMM over ALL its rows, K reduction
channels onto C output channels, with the stores predicated to the interior.  Three kernels, each with its own copy of the
epilogue (bias, relu, + addend, mask > 0 select, in that order):
  g128   conv1x1_gemm_kernel            128 rows x 128 channels per workgroup    tile configuration 18
  wide   conv1x1_gemm_wide_kernel<0>    256 rows x 128 channels, three stages    tile configuration 18
  n64    conv1x1_n64_kernel<false>      64 rows x 64 channels                    tile configuration 23
Which one runs follows from the channel counts (pick_cfg, conv_mfma.hip) and, between g128 and wide, from the device's CU
count (xv_launch_conv1x1_gemm), so a shape that is `g128` on 256 CUs is `wide` on a partition.  This module restates those
rules (`geometry`) and builds the case list FROM the CU count (`build_cases`): the cheapest shape of a fixed search grid that
has the properties of each row of `ROWS`, so that every case lands in the form it names wherever the suite runs.  `gen1` holds
two shapes the chooser keeps on the first-generation tiles (fewer than 256 / 128 reduction channels), whose shared epilogue
serves as the control.  tests/test_conv1x1_cases_cpu.py holds the builder to that without a GPU;
tests/test_conv1x1_epilogue_gpu.py runs the cases.

On 256 CUs the largest map is 2048 rows x 1024 channels of bf16 (4 MB) and the largest reference 4158 x 512 x 512 products
(2.2 GFLOP); on 304 CUs a fifth more.  From 32 CUs down no launch of 16 workgroups stays on the 128-row form (it makes 8 of
the wide form's, a quarter of a round), so the row g128/remap_tail does not exist there (`unreachable`).
No torch at module level: the references import numpy and the oracle's bf16 rounding when called."""
import collections

ROWS_PER_TILE = collections.OrderedDict([('g128', 128), ('wide', 256), ('n64', 64)])

# (form, property) in the order of the table of DESIGN.md; what each property asks for is in `claims`
ROWS = (
    ('g128', 'one_partial'),        # one workgroup, its only row tile partial but for the last 16-row block: no remap, 4 K steps
    ('g128', 'tiles_noremap'),      # several row tiles x three channel tiles, images > 1, 8 K steps, partial tail
    ('g128', 'remap_tail'),         # the XCD remap with at least two workgroups per XCD, images > 1, partial tail
    ('wide', 'noremap_tail'),       # 8 K steps (the three stages wrap twice), images > 1, partial tail
    ('wide', 'remap_tail'),         # the XCD remap, images > 1, partial tail
    ('wide', 'remap_whole'),        # the XCD remap, Mp a multiple of 256
    ('n64', 'one_partial'),         # one workgroup of fewer than 64 rows, 2 K steps
    ('n64', 'tiles_tail'),          # several tiles, images > 1, 8 K steps, partial tail
    ('n64', 'whole'),               # Mp a multiple of 64
    ('gen1', 'k64'),                # 64 reduction channels: configuration 14 / 15
    ('gen1', 'k128'),               # 128 reduction channels onto 256: configuration 1
)
FORMS = ('g128', 'wide', 'n64', 'gen1')

Case = collections.namedtuple('Case', 'form prop n h w k c')         # k reduction channels, c output channels
Geometry = collections.namedtuple('Geometry', 'cfg form mp rows m_tiles n_tiles nblk remap whole ksteps')

# integer operands of the exact tests: |x| <= 2, |w| <= 1, |bias| <= 3, |residual| <= 9 (the data gradient: |addend| <= 3, no bias)
X_MAX, W_MAX, B_MAX, R_MAX = 2, 1, 3, 9

# the search grid of build_cases
_N, _H, _W = range(1, 5), range(4, 34), range(4, 53)
_K = (256, 512)
_C18 = (128, 256, 384, 512, 1024)


def _cdiv(a, b):
    return -(-a // b)


def padded_rows(n, h, w):
    return n * (h + 2) * (w + 2)


def gen1_cfg(h, w, k, c):
    """pick_cfg's last two lines for a 1x1 conv that neither flat-GEMM form takes: the 8x16 tile with 128 output channels
    (configuration 1) where it covers the map within 1.1 x the better of the 16x16 (14) and 8x32 (15) tiles."""
    def covered(th, tw):
        return _cdiv(h, th) * th * _cdiv(w, tw) * tw
    c14, c15 = covered(16, 16), covered(8, 32)
    if c % 128 == 0 and k >= 128 and covered(8, 16) <= 1.1 * min(c14, c15):
        return 1
    return 15 if c15 < c14 else 14


def geometry(cus, n, h, w, k, c):
    """What runs a bf16 1x1 conv of K = k onto C = c channels with a full-resolution output on `cus` compute units."""
    assert k % 64 == 0 and c % 64 == 0
    mp = padded_rows(n, h, w)
    if c % 128 == 0 and k >= 256:
        n_tiles = c // 128
        wide_blocks = _cdiv(mp, 256) * n_tiles
        form = 'wide' if 4 * wide_blocks >= cus else 'g128'         # at least a quarter of a round of 256-row workgroups
        cfg = 18
    elif c == 64 and k >= 128:
        form, cfg, n_tiles = 'n64', 23, 1
    else:
        return Geometry(gen1_cfg(h, w, k, c), 'gen1', mp, None, None, None, None, False, None, k // 64)
    rows = ROWS_PER_TILE[form]
    m_tiles = _cdiv(mp, rows)
    nblk = m_tiles * n_tiles
    remap = form != 'n64' and nblk % 8 == 0                         # the narrow form has no remap
    return Geometry(cfg, form, mp, rows, m_tiles, n_tiles, nblk, remap, mp % rows == 0, k // 64)


def claims(case, cus):
    """Why `case` does NOT have the properties its row names on `cus` compute units, as a list of strings (empty: it has)."""
    g = geometry(cus, case.n, case.h, case.w, case.k, case.c)
    bad = []

    def need(cond, what):
        if not cond:
            bad.append('%s (%s)' % (what, g,))
    need(g.form == case.form, 'the form')
    if bad:
        return bad
    p = case.prop
    if case.form == 'gen1':
        need(g.cfg == {'k64': 14, 'k128': 1}.get(p), 'the first-generation tile')
        need(case.k == {'k64': 64, 'k128': 128}.get(p), 'the reduction channels')
        return bad
    if (case.form, p) not in ROWS:
        return ['unknown row %s/%s' % (case.form, p)]
    if p == 'one_partial':
        need(g.nblk == 1 and not g.whole and not g.remap, 'one workgroup, partial')
        need(g.mp > g.rows - 16, 'rows in every 16-row block of the tile, the last one partial')
        need(g.ksteps == (2 if case.form == 'n64' else 4), 'the fewest K steps the form is chosen for')
    if p in ('tiles_noremap', 'noremap_tail', 'tiles_tail'):
        need(not g.remap and not g.whole and g.m_tiles >= 2 and case.n > 1, 'several row tiles over several images, partial tail, no remap')
        need(g.ksteps == 8, '8 K steps')
    if p == 'tiles_noremap':
        need(g.n_tiles == 3, 'three channel tiles')
    if p in ('remap_tail', 'remap_whole'):
        need(g.remap and g.nblk >= 16 and g.m_tiles >= 2 and g.n_tiles >= 2, 'the remap with two workgroups per XCD or more')
    if p == 'remap_tail':
        need(not g.whole and case.n > 1, 'partial tail, several images')
    if p in ('remap_whole', 'whole'):
        need(g.whole and g.m_tiles >= 2 and case.n > 1, 'whole row tiles, several, over several images')
    if not bad:
        # the last padded row and a pixel more are border: a tail of a few rows would store nothing
        need(interior_rows(case, (g.m_tiles - 1) * g.rows, g.mp) >= 16, 'at least 16 interior pixels in the last row tile')
    return bad


def interior_rows(case, m0, m1):
    """How many of the padded rows m0 .. m1 - 1 are interior pixels -- the kernels' own store predicate."""
    wp, hp = case.w + 2, case.h + 2
    return sum(1 for m in range(m0, m1) if 1 <= m % wp <= case.w and 1 <= (m // wp) % hp <= case.h)


def map_elems(c):
    return padded_rows(c.n, c.h, c.w) * max(c.k, c.c)


def _cost(c):
    """Orders the candidates of a row: the maps first, then the reference's products, then a fixed order of the fields."""
    mp = padded_rows(c.n, c.h, c.w)
    return (mp * (c.k + c.c), mp * c.k * c.c, c.n, c.h, c.w)


def unreachable(cus):
    """Rows no shape can have on `cus` compute units.  The remap of the 128-row form needs 16 workgroups = m_tiles x n_tiles;
    the wide form then makes ceil(m_tiles / 2) x n_tiles >= 8, and is taken as soon as 4 x 8 >= cus."""
    return (('g128', 'remap_tail'),) if cus <= 32 else ()


def build_cases(cus):
    """One case per row of ROWS (but the unreachable ones) on a device of `cus` compute units: the cheapest shape of the grid
    with the row's properties."""
    cases = []
    for form, prop in ROWS:
        if (form, prop) in unreachable(cus):
            continue
        if form == 'gen1':
            cases.append(Case(form, prop, 2, 10, 14, 64, 128) if prop == 'k64' else Case(form, prop, 2, 10, 14, 128, 256))
            continue
        ks = (128, 256, 512) if form == 'n64' else _K
        cs = (64,) if form == 'n64' else _C18
        best = None
        for k in ks:
            for c in cs:
                for n in _N:
                    for h in _H:
                        for w in _W:
                            cand = Case(form, prop, n, h, w, k, c)
                            if best is not None and _cost(cand) >= _cost(best):
                                continue
                            if not claims(cand, cus):
                                best = cand
        if best is None:
            raise ValueError('no %s/%s shape on %d CUs' % (form, prop, cus))
        cases.append(best)
    return cases


def case_id(c):
    return '%s-%s' % (c.form, c.prop)


def max_abs_sum(c):
    """Bound on every intermediate of the exact tests: K products of |x| <= 2 and |w| <= 1, the bias and the residual."""
    return X_MAX * W_MAX * c.k + B_MAX + R_MAX


# the mask values the select has to tell apart: > 0 keeps; zero of either sign, and anything negative, clears
TINY = 2.0 ** -126                  # the smallest positive normal bf16 (and float32)
SPECIAL_MASK = (0.0, -0.0, TINY, -TINY, 3.0, -3.0)
SPECIAL_KEEPS = (False, False, True, False, True, False)


MASK_VALUES = (-1.0, 0.0, 0.5, 1.0, 1.5)

Operands = collections.namedtuple('Operands', 'x w b addend mask')       # float32: [n,h,w,K], [K,C], [C], [n,h,w,C], [n,h,w,C]


def mask_map(rng, shape):
    """Values from MASK_VALUES, with SPECIAL_MASK in the first channels of the first pixel and in the last channels of the LAST
    interior pixel of the last image (the one a short tail tile stores)."""
    import numpy as np
    m = rng.choice(np.asarray(MASK_VALUES, dtype=np.float32), size=shape)
    m[0, 0, 0, :6] = SPECIAL_MASK
    m[-1, -1, -1, -6:] = SPECIAL_MASK
    return m


def draw_integers(case, seed, addend_max=R_MAX):
    """x in [-2, 2], w in [-1, 1], bias in [-3, 3], addend in [-addend_max, addend_max], all integers: every partial sum is an
    integer below max_abs_sum(case) < 2^24, so fp32 accumulation is exact in any order and the one rounding is the store's."""
    import numpy as np
    rng = np.random.default_rng(seed)
    shape = (case.n, case.h, case.w)
    return Operands(rng.integers(-X_MAX, X_MAX + 1, shape + (case.k,)).astype(np.float32),
                    rng.integers(-W_MAX, W_MAX + 1, (case.k, case.c)).astype(np.float32),
                    rng.integers(-B_MAX, B_MAX + 1, case.c).astype(np.float32),
                    rng.integers(-addend_max, addend_max + 1, shape + (case.c,)).astype(np.float32),
                    mask_map(rng, shape + (case.c,)))


def draw_reals(case, seed):
    """x and the addend from N(0, 1) and the weights from N(0, 1) K^-1/2, rounded to bf16; the bias from N(0, 1) in float32."""
    import numpy as np
    from oracle.fcn_oracle import round_bf16
    rng = np.random.default_rng(seed)
    shape = (case.n, case.h, case.w)
    return Operands(round_bf16(rng.standard_normal(shape + (case.k,)).astype(np.float32)),
                    round_bf16((rng.standard_normal((case.k, case.c)) * case.k ** -0.5).astype(np.float32)),
                    rng.standard_normal(case.c).astype(np.float32),
                    round_bf16(rng.standard_normal(shape + (case.c,)).astype(np.float32)),
                    mask_map(rng, shape + (case.c,)))


def reference(x, w, b=None, relu=False, addend=None, mask=None, rounded=True):
    """The epilogue in float64, a function of the dense operands only: x [..., K], w [K, C], b [C], addend / mask [..., C].
        v = sum_k x w + b;  v = max(v, 0) if relu;  v += addend if given;  v = where(mask > 0, v, 0) if given
    then ONE round-to-nearest-even to bf16 (returned as float32), or v itself with rounded=False."""
    return epilogue(linear(x, w), b, relu, addend, mask, rounded)


def linear(x, w):
    """sum_k x w in float64 (the part of `reference` that costs: a test that needs several epilogues of one case shares it)."""
    import numpy as np
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    return (x.reshape(-1, x.shape[-1]) @ w).reshape(x.shape[:-1] + (w.shape[1],))


def epilogue(v, b=None, relu=False, addend=None, mask=None, rounded=True):
    """`reference` from the float64 sums `v` on (v is left unchanged)."""
    import numpy as np
    if b is not None:
        v = v + np.asarray(b, dtype=np.float64)
    if relu:
        v = np.maximum(v, 0.0)
    if addend is not None:
        v = v + np.asarray(addend, dtype=np.float64)
    if mask is not None:
        v = np.where(np.asarray(mask, dtype=np.float64) > 0, v, 0.0)
    if not rounded:
        return v
    from oracle.fcn_oracle import round_bf16
    return round_bf16(v)


def magnitude(x, w, b=None, addend=None):
    """sum_k |x w| + |b| + |addend| per output element, float64: what the rounding errors of the sum scale with."""
    import numpy as np
    x = np.abs(np.asarray(x, dtype=np.float64))
    w = np.abs(np.asarray(w, dtype=np.float64))
    a = (x.reshape(-1, x.shape[-1]) @ w).reshape(x.shape[:-1] + (w.shape[1],))
    if b is not None:
        a = a + np.abs(np.asarray(b, dtype=np.float64))
    if addend is not None:
        a = a + np.abs(np.asarray(addend, dtype=np.float64))
    return a


def tolerance(ref, mag, k):
    """Per element, for bf16 operands, fp32 accumulation in any order and one bf16 store:
        2^-8 |ref| + (K + 3) 2^-24 mag
    Products of two bf16 values are exact in fp32, so only additions round: K - 1 in the sum, then the bias, (the relu is
    exact,) the addend -- at most K + 1 roundings of 2^-24 relative to a partial sum that |.| <= mag bounds, K + 3 with the
    second-order terms (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4, K u << 1): the value v the
    kernel holds is within d = (K + 1) 2^-24 mag of ref.  The store rounds v once to bf16 (8 significant bits): half an ulp is
    2^-9 .. 2^-8 of |v|, 2^-8 at the bottom of a binade, and 2^-8 |v| <= 2^-8 |ref| + 2^-8 d.  Together
    2^-8 |ref| + (1 + 2^-8) d, which the bound covers up to K = 511; at K = 512, the longest sum here, it is short by
    0.004 x 2^-24 mag of that worst case (all K + 1 roundings erring fully and in one direction).  Derived, not tuned; the
    first term is attained (a float32 evaluation on the CPU reaches 0.98 of the bound, tests/test_conv1x1_cases_cpu.py)."""
    import numpy as np
    return 2.0 ** -8 * np.abs(ref) + (k + 3) * 2.0 ** -24 * mag
