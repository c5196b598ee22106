"""The split-K filter-gradient kernels (csrc/conv_wgrad.hip: versions 1, 2, 3 of the 3x3 kernel and the generic 1x1 kernel) where
a workgroup walks SEVERAL pixel tiles: both LDS buffers, the hand-over between tiles, a short last range, an empty range, an
image boundary inside a range, edge tiles anywhere in a range, unequal channel blocks and both slab reductions.  The shapes
come from tests/wgrad_cases.py, built from the live CU count; the first test fails if one of them is not where it claims to be.

References restate the sum in float64 on the CPU, one matrix product per tap, and call no kernel.
(a) integers: every partial sum is an integer far below 2^24, so any order of summation gives the same bits -- array_equal.
(b) bf16-rounded floats: every product of two bf16 values is exact in fp32, only the additions round, and for ANY order of the
    K = n h w terms |got - ref| <= g A per element, A = sum |x| |dy| of that element, g = K u / (1 - K u), u = 2^-24 (Higham,
    Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4).  Nothing in the bound is measured.
`xv_bias_grad` (the stand-alone bias gradient) is held to exact integer sums at every thread mapping at the end of the file.

Slowest case on an MI355X (256 CUs), references included: 0.21 s (three_odd-v1, 1x24x352, 512 -> 512: two float64 references
of 40 GFLOP); the 71 tests of the file take 16 s, half of it the first test's start-up."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as wc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of fp32

CASE_KEYS = [(name, kind) for kind in wc.KINDS for name in wc.REGIMES]
case_param = pytest.mark.parametrize('key', CASE_KEYS, ids=['%s-%s' % k for k in CASE_KEYS])


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture
def set_variant(ops):
    """Selects the 3x3 kernel version (a process-wide switch); the default is back whatever the test does."""
    from modular_semantic_segmentation_amd import _lib

    def select(v):
        assert _lib.lib().xv_set_wgrad_variant(v) == 0
    yield select
    _lib.lib().xv_set_wgrad_variant(0)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _cases(cus):
    return {(c.name, c.kind): c for c in wc.build_cases(cus)}


def _case(key):
    return _cases(_cus())[key]


def _tap_sums(x, dy, k):
    """float64 [k][k][cin][cout]: sum over n, y, x of X[n, y + ky - p, x + kx - p, ci] dY[n, y, x, co], zero outside the image."""
    n, h, w, cin = x.shape
    p = (k - 1) // 2
    xp = F.pad(x.double(), (0, 0, p, p, p, p))
    d = dy.double().reshape(-1, dy.shape[-1])
    out = torch.empty((k, k, cin, dy.shape[-1]), dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            out[ky, kx] = xp[:, ky:ky + h, kx:kx + w].reshape(-1, cin).T @ d
    return out


def _forms(ops, c, xa, dya, set_variant, dw0, db0):
    """Runs every version of the case in both forms on prefilled dw / db; yields (label, dw, db)."""
    nws = ops.conv2d_bwd_filter_workspace_bytes(xa, c.cout, c.k) // 4
    for v in c.variants:
        set_variant(v)
        dw = torch.full((c.k, c.k, c.cin, c.cout), dw0, device='cuda')
        db = torch.full((c.cout,), db0, device='cuda')
        ops.conv2d_bwd_filter(xa, dya, dw, db, c.k)
        yield 'version %d, atomics' % v, dw, db
        # a slab element that no workgroup writes stays NaN and poisons its sum: the empty range has to write zeros
        ws = torch.full((nws,), float('nan'), device='cuda')
        dw = torch.full((c.k, c.k, c.cin, c.cout), dw0, device='cuda')
        db = torch.full((c.cout,), db0, device='cuda')
        ops.conv2d_bwd_filter(xa, dya, dw, db, c.k, workspace=ws)
        yield 'version %d, slabs' % v, dw, db
        ws.fill_(float('nan'))
        dw = torch.full((c.k, c.k, c.cin, c.cout), dw0, device='cuda')
        ops.conv2d_bwd_filter(xa, dya, dw, None, c.k, workspace=ws)
        yield 'version %d, slabs, no bias gradient' % v, dw, None


def test_every_case_is_in_the_regime_it_names(ops):
    """With the LIVE CU count: splits, tiles per split, the short and the empty range of every case; and the library's own
    count of compute units against the one the cases were built from (the workspace query is the version-1 split count times
    one slab and its bias row)."""
    cus = _cus()
    bad = []
    for c in wc.build_cases(cus):
        ptiles = wc.tiles_of(c.n, c.h, c.w)[2]
        where = ['v%d splits %d per %d last %d empty %d' % ((v,) + wc.regime(cus, v, c.k, c.n, c.h, c.w, c.cin, c.cout))
                 for v in c.variants]
        print('%-22s %dx%dx%d %d->%d k%d  %d tiles: %s' % (wc.case_id(c), c.n, c.h, c.w, c.cin, c.cout, c.k, ptiles, ', '.join(where)))
        bad += ['%s on %d CUs: not %s' % (wc.case_id(c), cus, b) for b in wc.claims(c, cus)]
        want = min(wc.base_splits(cus, 1, c.k, c.cin, c.cout), ptiles) * (c.k * c.k * c.cin * c.cout + c.cout) * 4
        got = ops.conv2d_bwd_filter_workspace_bytes(ops.Act(c.n, c.h, c.w, c.cin), c.cout, c.k)
        if got != want:
            bad.append('%s: workspace query %d, %d by the restated rule on %d CUs' % (wc.case_id(c), got, want, cus))
        if wc.map_elems(c) > wc.MAX_MAP_ELEMS or c.n * c.h * c.w > wc.MAX_PIXELS:
            bad.append('%s: map of %d elements' % (wc.case_id(c), wc.map_elems(c)))
    assert sorted((c.name, c.kind) for c in wc.build_cases(cus)) == sorted(CASE_KEYS)
    assert not bad, '\n'.join(bad)


@case_param
def test_filter_and_bias_gradient_exact_on_integers(ops, set_variant, key):
    c = _case(key)
    g = torch.Generator().manual_seed(1000 + CASE_KEYS.index(key))
    x = torch.randint(-2, 3, (c.n, c.h, c.w, c.cin), generator=g).float()
    dy = torch.randint(-1, 2, (c.n, c.h, c.w, c.cout), generator=g).float()
    ref = _tap_sums(x, dy, c.k).numpy()
    bias_ref = dy.double().sum((0, 1, 2)).numpy()
    assert np.abs(ref).max() < 2 ** 23 and ref.any()
    xa, dya = ops.Act.from_dense(x.cuda()), ops.Act.from_dense(dy.cuda())
    for label, dw, db in _forms(ops, c, xa, dya, set_variant, 1.0, 2.0):
        got = dw.cpu().numpy().astype(np.float64)
        wrong = got != ref + 1
        assert not wrong.any(), '%s: %d of %d elements differ, first at %s' % (label, wrong.sum(), wrong.size,
                                                                              tuple(np.argwhere(wrong)[0]))
        assert np.array_equal(got, ref + 1), label
        if db is not None:
            assert np.array_equal(db.cpu().numpy().astype(np.float64), bias_ref + 2), label


@case_param
def test_filter_gradient_of_floats_within_the_summation_bound_and_reproducible(ops, set_variant, key):
    c = _case(key)
    g = torch.Generator().manual_seed(2000 + CASE_KEYS.index(key))
    x = torch.randn((c.n, c.h, c.w, c.cin), generator=g).relu_().bfloat16()
    dy = (torch.randn((c.n, c.h, c.w, c.cout), generator=g) * 1e-2).bfloat16()
    # x >= 0: with dy = p - m (p, m >= 0) the reference is X'p - X'm and the sum of absolute terms X'p + X'm
    xf, dyf = x.float(), dy.float()
    sp, sm = _tap_sums(xf, dyf.clamp(min=0), c.k), _tap_sums(xf, (-dyf).clamp(min=0), c.k)
    ref, A = sp - sm, sp + sm
    bias_ref, bias_A = dyf.double().sum((0, 1, 2)), dyf.double().abs().sum((0, 1, 2))
    K = c.n * c.h * c.w
    gamma = K * U / (1 - K * U)
    xa, dya = ops.Act.from_dense(x.cuda()), ops.Act.from_dense(dy.cuda())
    assert torch.equal(xa.interior().cpu(), x) and torch.equal(dya.interior().cpu(), dy)
    for label, dw, db in _forms(ops, c, xa, dya, set_variant, 0.0, 0.0):
        err = (dw.cpu().double() - ref).abs()
        assert bool(torch.isfinite(err).all()), label
        over = err > gamma * A
        print('%s %s: largest |got - ref| / (g A) = %.3g' % (key, label, float((err / (gamma * A).clamp(min=1e-300)).max())))
        assert not bool(over.any()), '%s: %d elements beyond g A, g = %.3g' % (label, int(over.sum()), gamma)
        if db is not None:
            assert bool(((db.cpu().double() - bias_ref).abs() <= gamma * bias_A).all()), label
    # the slab form adds in a fixed order: the same bits from run to run, with several tiles per range too
    nws = ops.conv2d_bwd_filter_workspace_bytes(xa, c.cout, c.k) // 4
    for v in c.variants:
        set_variant(v)
        outs = []
        for _ in range(2):
            ws = torch.full((nws,), float('nan'), device='cuda')
            dw, db = torch.zeros((c.k, c.k, c.cin, c.cout), device='cuda'), torch.zeros(c.cout, device='cuda')
            ops.conv2d_bwd_filter(xa, dya, dw, db, c.k, workspace=ws)
            outs.append((dw, db))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'version %d' % v


@case_param
def test_workspace_contract(ops, set_variant, key):
    """The queried size is an upper bound over the versions: each takes it.  k k cin cout floats hold no slab with its bias
    row: each version refuses them with XV_EWORKSPACE and leaves dw and db alone."""
    from modular_semantic_segmentation_amd import _lib
    c = _case(key)
    g = torch.Generator().manual_seed(3000 + CASE_KEYS.index(key))
    xa = ops.Act.from_dense(torch.randint(-2, 3, (c.n, c.h, c.w, c.cin), generator=g).float().cuda())
    dya = ops.Act.from_dense(torch.randint(-1, 2, (c.n, c.h, c.w, c.cout), generator=g).float().cuda())
    nws = ops.conv2d_bwd_filter_workspace_bytes(xa, c.cout, c.k) // 4
    elems = c.k * c.k * c.cin * c.cout
    assert nws >= 2 * (elems + c.cout)
    for v in (1, 2, 3):
        set_variant(v)
        for with_bias in (True, False):
            dw = torch.full((c.k, c.k, c.cin, c.cout), 1.0, device='cuda')
            db = torch.full((c.cout,), 2.0, device='cuda')
            ops.conv2d_bwd_filter(xa, dya, dw, db if with_bias else None, c.k,
                                  workspace=torch.full((nws,), float('nan'), device='cuda'))
            assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), v
            dw.fill_(1.0), db.fill_(2.0)
            with pytest.raises(_lib.XvError, match='XV_EWORKSPACE'):
                ops.conv2d_bwd_filter(xa, dya, dw, db if with_bias else None, c.k,
                                      workspace=torch.full((elems,), float('nan'), device='cuda'))
            torch.cuda.synchronize()
            assert torch.equal(dw, torch.full_like(dw, 1.0)) and torch.equal(db, torch.full_like(db, 2.0)), v


# ---- xv_bias_grad: thread -> (8-channel group tid % (C / 8), row lane tid / (C / 8)), rstep = 256 / (C / 8) rows per workgroup
# and pass, at most 1024 workgroups.  Per C: a one-pixel map, a small ragged one, and the smallest map whose padded rows
# n (h + 2) (w + 2) exceed 1024 rstep (the grid-stride loop past the capped grid; C = 2048: 34 x 34).
BIAS_SHAPES = {
    8: [(1, 1, 1), (2, 5, 7), (5, 479, 107)],          # rstep 256: 5 * 481 * 109 = 262 145 rows
    64: [(1, 1, 1), (2, 5, 7), (9, 9, 329)],           # rstep 32: 9 * 11 * 331 = 32 769 rows
    512: [(1, 1, 1), (2, 5, 7), (1, 15, 239)],         # rstep 4: 17 * 241 = 4 097 rows
    2048: [(1, 1, 1), (2, 5, 7), (1, 34, 34)],         # rstep 1 (no LDS reduction step): 36 * 36 = 1 296 rows
}


@pytest.mark.parametrize('C', sorted(BIAS_SHAPES))
def test_bias_grad_exact_on_integers_at_every_thread_mapping(ops, C):
    for i, (n, h, w) in enumerate(BIAS_SHAPES[C]):
        rows, rstep = n * (h + 2) * (w + 2), 256 // (C // 8)
        assert i < 2 or rows > 1024 * rstep
        g = torch.Generator().manual_seed(C + i)
        dy = torch.randint(-3, 4, (n, h, w, C), generator=g).float()
        ref = dy.double().sum((0, 1, 2)).numpy()
        assert 3 * n * h * w < 2 ** 24 - 2
        db = torch.full((C,), 2.0, device='cuda')
        ops.bias_grad(ops.Act.from_dense(dy.cuda()), db)
        assert np.array_equal(db.cpu().numpy().astype(np.float64), ref + 2), (n, h, w)


@pytest.mark.parametrize('c,dtype', [(24, 'bf16'), (4096, 'bf16'), (64, 'fp8')], ids=['C24', 'C4096', 'fp8'])
def test_bias_grad_refuses_what_its_thread_mapping_cannot_take(ops, c, dtype):
    """C = 24 is a multiple of 8 whose 3 channel groups do not divide the 256 threads; C = 4096 needs more than 256 groups; an
    fp8 map would be read as bf16."""
    from modular_semantic_segmentation_amd import _lib
    a = ops.Act(1, 4, 4, c, dtype=dtype)
    db = torch.full((c,), 2.0, device='cuda')
    with pytest.raises(_lib.XvError):
        ops.bias_grad(a, db)
    torch.cuda.synchronize()
    assert torch.equal(db, torch.full_like(db, 2.0))
