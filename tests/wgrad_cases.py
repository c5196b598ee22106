"""Shapes at which the split-K filter-gradient kernels of csrc/conv_wgrad.hip walk SEVERAL pixel tiles per workgroup.

A launch of conv_wgrad_kernel<3> (version 1), conv_wgrad_dma_kernel<3> (2), conv_wgrad_lw_kernel (3) or conv_wgrad_kernel<1>
(the generic 1x1 form) cuts its `ptiles` pixel tiles of 8x32 pixels into `splits` ranges of `per = ceil(ptiles / splits)`
tiles; `splits` follows from the device's CU count (`wgrad_splits()`), so a shape that reaches `per = 2` on 256 CUs sits at
`per = 1` or `per = 4` on a partition.  This module restates the split rule (`regime`), the tile decode (`walk`) and builds the
case list FROM the CU count, so that every case lands in the regime it names wherever the suite runs.
tests/test_wgrad_cases_cpu.py holds the builder to that without a GPU; tests/test_conv_wgrad_tiles_gpu.py runs the cases.

What a case costs: every workgroup of the launch walks `per` tiles of 256 pixels against a 64 x 64 block and nine (one) taps,
so the reference is per x mult x cus x 18.9 (2.1) MFLOP whatever the channel counts -- 4.8 GFLOP per unit of `per` for versions
2 and 3 on 256 CUs, three times that for version 1.  The channel counts decide the size of the MAPS: the builder takes the
channel pair with the most 64 x 64 blocks that still leaves the number of splits the regime needs, so few tiles are needed."""
import collections

TH, TW = 8, 32                      # the pixel tile of every kernel here

# kinds of launch: (k, versions that share the split rule)
KINDS = collections.OrderedDict([
    ('v23', (3, (2, 3))),           # one 8-wave workgroup per CU
    ('v1', (3, (1,))),              # ~3 four-wave workgroups per CU
    ('1x1', (1, (3,))),             # generic 1x1 kernel, ~3 per CU: the version switch does not reach it
])

# (cin, cout) by falling number of 64 x 64 blocks.  The 1x1 list holds only pairs that wgrad1_gi() rejects, so that the generic
# kernel runs with a workspace too (the flat-GEMM form has its own tests).
CHANNELS_3X3 = [(512, 512), (256, 512), (256, 256), (192, 192), (128, 256), (128, 128), (64, 128), (64, 64)]
CHANNELS_1X1 = [(576, 576), (448, 448), (320, 320), (192, 192), (512, 64), (128, 64), (64, 64)]
UNEQUAL = [(320, 448), (192, 256), (128, 192)]      # cin != cout, 35 / 12 / 6 blocks; all rejected by wgrad1_gi() as well

# Padded elements of the larger of a case's two maps (n (h + 2) (w + 2) max(cin, cout)): 7.9 M is the largest on 256 CUs
# (version 1, reduce_16: 48 tiles of 512 channels) and 9.5 M the largest on 304; half as much again on top of the 256-CU figure
# keeps every map under 24 MB of bf16 on any partition.
MAX_MAP_ELEMS = 12 * 1000 * 1000
# exact integer sums: |x| <= 2, |dy| <= 1, so |sum| <= 2 n h w, and the prefill adds 2 at the most
MAX_PIXELS = (2 ** 24 - 2) // 2

Case = collections.namedtuple('Case', 'name kind k variants n h w cin cout')


def wgrad1_gi(cin, cout):
    """Channel pairs the flat-GEMM 1x1 form takes (non-zero) -- restated from conv_wgrad.hip."""
    if cin % 256 == 0 and cout % 128 == 0:
        return 4
    if cin % 128 == 0 and cout % 256 == 0:
        return 2
    return 0


def _cdiv(a, b):
    return -(-a // b)


def base_splits(cus, variant, k, cin, cout):
    """wgrad_splits() before its cap at the number of tiles."""
    pairs = (cin // 64) * (cout // 64)
    mult = 1 if (variant >= 2 and k == 3) else 3
    return max(1, _cdiv(mult * cus, pairs))


def tiles_of(n, h, w):
    return _cdiv(w, TW), _cdiv(h, TH), _cdiv(w, TW) * _cdiv(h, TH) * n


def regime(cus, variant, k, n, h, w, cin, cout):
    """(splits, per, tiles_in_last_nonempty_split, empty_splits) of one launch: wgrad_splits() and the kernels'
    per = ceil(ptiles / splits), t_begin = split * per, t_end = min(t_begin + per, ptiles)."""
    ptiles = tiles_of(n, h, w)[2]
    splits = max(1, min(base_splits(cus, variant, k, cin, cout), ptiles))
    per = _cdiv(ptiles, splits)
    counts = [max(0, min(s * per + per, ptiles) - s * per) for s in range(splits)]
    nonempty = [c for c in counts if c > 0]
    assert sum(counts) == ptiles and counts[:len(nonempty)] == nonempty      # empty ranges come last
    return splits, per, nonempty[-1], splits - len(nonempty)


def walk(cus, variant, k, n, h, w, cin, cout):
    """Per split the tiles it walks, each as (image, ty, tx, edge): the kernels' decode t -> (n, ty, tx); `edge` is their
    clamped-offset path (the tile reaches past the bottom or the right of the image)."""
    tiles_x, tiles_y, ptiles = tiles_of(n, h, w)
    splits, per, _, _ = regime(cus, variant, k, n, h, w, cin, cout)
    out = []
    for s in range(splits):
        row = []
        for t in range(s * per, min(s * per + per, ptiles)):
            tx, r = t % tiles_x, t // tiles_x
            ty, img = r % tiles_y, r // tiles_y
            row.append((img, ty, tx, ty * TH + TH > h or tx * TW + TW > w))
        out.append(row)
    return out


def map_elems(c):
    return c.n * (c.h + 2) * (c.w + 2) * max(c.cin, c.cout)


def _channels(cus, kind, lo, hi=None, prefer=None):
    """The channel pair with the most blocks whose split count (before the cap) is in [lo, hi]; `prefer` narrows further
    where some pair meets it."""
    k, variants = KINDS[kind]
    ok = [(ci, co) for ci, co in (CHANNELS_3X3 if k == 3 else CHANNELS_1X1)
          if lo <= base_splits(cus, variants[0], k, ci, co) <= (hi if hi is not None else 1 << 30)]
    if not ok:
        raise ValueError('no channel pair gives %s..%s splits on %d CUs (%s)' % (lo, hi, cus, kind))
    best = [c for c in ok if prefer is not None and prefer(base_splits(cus, variants[0], k, *c))]
    return (best or ok)[0]


def long_walk_ok(cus, variant, k, n, h, w, cin, cout):
    """The `long_walk_edges` regime, checked by walking it: per >= 5, ragged height and width, at least two images whose tile
    count is no multiple of per, a split that crosses an image boundary, and across the splits an edge tile first, in the
    middle and last within a split, as well as a split that begins and one that ends on an inner tile."""
    tiles_x, tiles_y, _ = tiles_of(n, h, w)
    splits, per, _, _ = regime(cus, variant, k, n, h, w, cin, cout)
    if per < 5 or h % TH == 0 or w % TW == 0 or n < 2 or (tiles_x * tiles_y) % per == 0 or splits < 2:
        return False
    rows = [r for r in walk(cus, variant, k, n, h, w, cin, cout) if r]
    return (any(r[0][0] != r[-1][0] for r in rows)
            and any(r[0][3] for r in rows) and any(r[-1][3] for r in rows)
            and any(t[3] for r in rows for t in r[1:-1])
            and any(not r[0][3] for r in rows) and any(not r[-1][3] for r in rows))


def _long_walk(cus, kind):
    k, variants = KINDS[kind]
    cin, cout = _channels(cus, kind, 4)
    best = None
    for tiles_y in (2, 3):
        for tiles_x in (2, 3):
            h, w = tiles_y * TH - 3, tiles_x * TW - 24
            for n in range(2, 6 * base_splits(cus, variants[0], k, cin, cout) + 2):
                if regime(cus, variants[0], k, n, h, w, cin, cout)[1] > 7:
                    break
                if long_walk_ok(cus, variants[0], k, n, h, w, cin, cout):
                    cand = (n * tiles_y * tiles_x, n, h, w)
                    best = cand if best is None or cand < best else best
                    break
    if best is None:
        raise ValueError('no long_walk_edges shape on %d CUs (%s)' % (cus, kind))
    return best[1], best[2], best[3], (cin, cout)


def build_cases(cus):
    """Every regime for every kind of launch on a device of `cus` compute units."""
    cases = []
    for kind, (k, variants) in KINDS.items():
        def base(c):
            return base_splits(cus, variants[0], k, *c)

        def add(name, n, h, w, c):
            cases.append(Case(name, kind, k, variants, n, h, w, c[0], c[1]))

        c = _channels(cus, kind, 4)                 # 4 splits: the fewest with a full, a short and an empty range at per = 2
        s = base(c)
        add('two_full', 1, 2 * TH, s * TW, c)                               # 2 s tiles: 2, 2, .., 2
        add('short_and_empty', 2 * s - 3, TH, TW, c)                        # 2 s - 3 tiles, one image each: 2, .., 2, 1, 0
        add('three_odd', 1, 3 * TH, (s - 1) * TW, c)                        # 3 (s - 1) tiles: 3, .., 3, 0
        add('long_walk_edges', *_long_walk(cus, kind))
        c = [u for u in UNEQUAL if base(u) >= 2][0]
        add('pairs_unequal', 2, TH, base(c) * TW - 8, c)                    # 2 s tiles, the last of a row reaches past it
        c = _channels(cus, kind, 16, prefer=lambda b: b % 16 != 0)          # lanes of slab_reduce_kernel<16> with 1 and 2 slabs
        add('reduce_16', 2, TH, base(c) * TW, c)
        c = _channels(cus, kind, 2, 15)
        add('reduce_1', 1, TH, (2 * base(c) - 1) * TW, c)                   # 2 s - 1 tiles: 2, .., 2, 1 and no empty range
    return cases


def claims(case, cus):
    """Why `case` is NOT in the regime its name claims on `cus` compute units, as a list of strings (empty: it is)."""
    bad = []

    def need(cond, what):
        if not cond:
            bad.append(what)
    ptiles = tiles_of(case.n, case.h, case.w)[2]
    need(case.cin % 64 == 0 and case.cout % 64 == 0, 'channel counts in whole 64-blocks')
    if case.k == 1:
        need(wgrad1_gi(case.cin, case.cout) == 0, 'a channel pair the flat-GEMM 1x1 form rejects')
    for v in case.variants:
        args = (cus, v, case.k, case.n, case.h, case.w, case.cin, case.cout)
        splits, per, last, empty = regime(*args)
        where = '%s: splits %d per %d last %d empty %d, %d tiles' % (v, splits, per, last, empty, ptiles)
        need(per >= 2 and splits >= 2, 'several tiles per split, several splits (' + where + ')')
        if case.name == 'two_full':
            need(per == 2 and last == 2 and empty == 0, 'per = 2, every split full (' + where + ')')
        elif case.name == 'short_and_empty':
            need(per == 2 and ptiles == 2 * splits - 3 and last == 1 and empty == 1, 'per = 2, 2 s - 3 tiles (' + where + ')')
        elif case.name == 'three_odd':
            need(per == 3 and last == 3 and empty == 1, 'per = 3, full splits, then an empty one (' + where + ')')
        elif case.name == 'long_walk_edges':
            need(long_walk_ok(*args), 'per >= 5 over ragged images, across an image boundary (' + where + ')')
        elif case.name == 'pairs_unequal':
            need(case.cin != case.cout and case.cin > 64 and case.cout > 64, 'several blocks of both channel counts, unequal')
        elif case.name == 'reduce_16':
            need(splits >= 16, 'slab_reduce_kernel<16> (' + where + ')')
        elif case.name == 'reduce_1':
            need(splits < 16, 'slab_reduce_kernel<1> (' + where + ')')
        else:
            bad.append('unknown regime ' + case.name)
    return bad


REGIMES = ('two_full', 'short_and_empty', 'three_odd', 'long_walk_edges', 'pairs_unequal', 'reduce_16', 'reduce_1')


def case_id(c):
    return '%s-%s' % (c.name, c.kind)
