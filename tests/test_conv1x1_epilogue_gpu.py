"""The epilogues of the three flat-GEMM 1x1 kernels (csrc/conv1x1_gemm.hip: conv1x1_gemm_kernel, conv1x1_gemm_wide_kernel<0>,
conv1x1_n64_kernel<false>; tile configurations 18 and 23) on the two paths that hand them an addend and a mask:
xv_conv2d_fwd_residual (the closing conv of a ResNet block: relu BEFORE the residual) and xv_conv2d_bwd_data with k = 1
(addend = the shortcut's gradient, mask = relu_ref > 0, applied last).  Each kernel carries its own copy of
bias -> relu -> + addend -> mask select on packed bf16 pairs; the first-generation tiles' shared epilogue runs as the control.

The shapes come from tests/conv1x1_cases.py, built from the live CU count (between the 128-row and the 256-row form the launcher
decides by it); every test first asserts that the case is in the form it names and that xv_conv2d_choose_cfg -- the library's
own pick -- names its configuration, so none can pass on a fallback.  References are float64 on the CPU and call no kernel.
(a), (b) integers: every partial sum is an integer below 2^24, exact in fp32 in any order, so the one rounding is the store's:
    np.array_equal.  Outputs start as NaN in the interior: an element no workgroup stores fails, a border one written fails.
(c) bf16-rounded normal operands against the unrounded reference within conv1x1_cases.tolerance (derived there).
    Largest error / bound measured on an MI355X (256 CUs), residual / data gradient: g128 0.974 / 0.967, wide 0.966 / 0.965,
    n64 0.917 / 0.925, gen1 0.977 / 0.984 -- the bf16 store at the bottom of a binade, which is the bound's first term; a
    float32 evaluation on the CPU gives the same figures to two digits (tests/test_conv1x1_cases_cpu.py).
    The whole file: 27 tests in 6.5 s there, 3 s of it the first test's start-up.
(d) what xv_conv2d_fwd_residual refuses, with the output left alone."""
import functools

import numpy as np
import pytest
import torch

import conv1x1_cases as cc

pytestmark = pytest.mark.gpu

row_param = pytest.mark.parametrize('row', cc.ROWS, ids=['%s-%s' % r for r in cc.ROWS])
REAL_ROWS = [('g128', 'remap_tail'), ('wide', 'noremap_tail'), ('n64', 'tiles_tail'), ('gen1', 'k128')]     # one per form
real_param = pytest.mark.parametrize('row', REAL_ROWS, ids=['%s-%s' % r for r in REAL_ROWS])


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops as _ops
    return _ops


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _cases(cus):
    return {(c.form, c.prop): c for c in cc.build_cases(cus)}


@functools.lru_cache(maxsize=None)
def _integers(cus, row, addend_max):
    """(operands, float64 sums) of a case: drawn and multiplied once, shared by the tests and left unchanged."""
    c = _cases(cus)[row]
    o = cc.draw_integers(c, 100 + cc.ROWS.index(row), addend_max)
    v = cc.linear(o.x, o.w)
    for a in tuple(o) + (v,):
        a.setflags(write=False)
    return o, v


def _case(row):
    """The case of `row` on this device, after the checks every test makes: the restated rule on the live CU count names the
    form, and the library's chooser names the configuration."""
    from modular_semantic_segmentation_amd import _lib
    cus = _cus()
    if row in cc.unreachable(cus):
        pytest.skip('no %s/%s shape exists on %d CUs' % (row + (cus,)))
    c = _cases(cus)[row]
    assert _lib.lib().xv_conv2d_stats_rows() == cus
    assert cc.claims(c, cus) == [], c
    g = cc.geometry(cus, c.n, c.h, c.w, c.k, c.c)
    assert g.form == c.form == row[0]
    bf16 = _lib.CONSTANTS['XV_BF16']
    for flags in (0, 2):            # bit 1: with addend / mask -- no 1x1 rule looks at it
        got = _lib.lib().xv_conv2d_choose_cfg(c.n, c.h, c.w, c.k, c.c, 1, bf16, bf16, flags)
        assert got == g.cfg, 'the library picks configuration %d for %s, the case is meant for %d' % (got, c, g.cfg)
    assert (g.cfg in (18, 23)) == (c.form != 'gen1')
    return c, g


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()           # a copy: the shared operands are read-only


def _fresh(ops, c):
    """An output map whose interior is NaN: every interior element has to be stored, no border element may be."""
    y = ops.Act(c.n, c.h, c.w, c.c)
    y.interior().fill_(float('nan'))
    return y


def _border_is_zero(a):
    t = a.t.float()
    return not (t[:, 0].ne(0).any() or t[:, -1].ne(0).any() or t[:, :, 0].ne(0).any() or t[:, :, -1].ne(0).any())


def _mismatch(got, ref):
    bad = np.argwhere(~(got == ref))
    return '%d of %d differ, first (n,y,x,c) %s: got %s, want %s' % (
        len(bad), ref.size, bad[:4].tolist(), got[tuple(bad[:4].T)].tolist(), ref[tuple(bad[:4].T)].tolist())


def _forward_weights(ops, w):
    return ops.pack_conv_weights(_dev(w[None, None]))                           # HWIO [1, 1, K, C]


def _dgrad_weights(ops, w):
    # the forward conv of this gradient maps C (the channels of dx) onto K (the channels of dy): HWIO [1, 1, C, K]
    return ops.pack_conv_weights_dgrad(_dev(np.ascontiguousarray(w.T)[None, None]))


@row_param
def test_residual_conv_exact_on_integers(ops, row):
    """xv_conv2d_fwd_residual: y = act(x w + b) + residual with residuals of both signs, relu on and off."""
    c, g = _case(row)
    o, v = _integers(_cus(), row, cc.R_MAX)
    assert o.addend.min() < 0 < o.addend.max() and cc.max_abs_sum(c) < 2 ** 24
    xa, wp, bd = ops.Act.from_dense(_dev(o.x)), _forward_weights(ops, o.w), _dev(o.b)
    res = ops.Act.from_dense(_dev(o.addend))
    res_before = res.t.clone()
    for relu in (1, 0):
        ref = cc.epilogue(v, o.b, relu=bool(relu), addend=o.addend)
        if relu:
            # the order is under test: a relu behind the add gives other values on this very case
            swapped = cc.epilogue(np.maximum(v + o.b + o.addend, 0.0))
            assert (swapped != ref).any()
        y = ops.conv1x1_residual(xa, wp, bd, res, relu=relu, y=_fresh(ops, c))
        torch.cuda.synchronize()
        got = y.interior().float().cpu().numpy()
        assert np.array_equal(got, ref), 'relu %d: %s' % (relu, _mismatch(got, ref))
        assert _border_is_zero(y), 'relu %d: the border of y was written' % relu
        assert torch.equal(res.t, res_before), 'relu %d: the residual map changed' % relu


@row_param
def test_data_gradient_exact_on_integers(ops, row):
    """xv_conv2d_bwd_data, k = 1: dx = where(relu_ref > 0, dy w + addend, 0), every combination of addend and relu_ref; the
    mask map carries +-0, +- the smallest normal and +-3 in its first and in its last stored pixel."""
    c, g = _case(row)               # K = channels of dy, C = channels of dx
    o, v = _integers(_cus(), row, 3)
    dy, wd, zb = ops.Act.from_dense(_dev(o.x)), _dgrad_weights(ops, o.w), torch.zeros(c.c, device='cuda')
    add, ref_map = ops.Act.from_dense(_dev(o.addend)), ops.Act.from_dense(_dev(o.mask))
    assert np.array_equal(ref_map.interior().float().cpu().numpy(), o.mask)         # bf16 holds every mask value, the tiny ones too
    assert np.signbit(ref_map.interior()[0, 0, 0, 1].float().item())
    before = (add.t.clone(), ref_map.t.clone())
    for use_add, use_ref in ((True, True), (False, True), (True, False), (False, False)):
        ref = cc.epilogue(v, addend=o.addend if use_add else None, mask=o.mask if use_ref else None)
        dx = ops.conv2d_bwd_data(dy, wd, zb, _fresh(ops, c), 1, relu_ref=ref_map if use_ref else None,
                                 addend=add if use_add else None)
        torch.cuda.synchronize()
        got = dx.interior().float().cpu().numpy()
        assert np.array_equal(got, ref), 'addend %d mask %d: %s' % (use_add, use_ref, _mismatch(got, ref))
        if use_ref:
            for pix in (got[0, 0, 0, :6], got[-1, -1, -1, -6:]):
                assert not pix[[0, 1, 3, 5]].any()
        assert _border_is_zero(dx), 'addend %d mask %d: the border of dx was written' % (use_add, use_ref)
    assert torch.equal(add.t, before[0]) and torch.equal(ref_map.t, before[1])


@real_param
def test_both_entry_points_on_real_operands_within_the_derived_bound(ops, row):
    c, g = _case(row)
    o = cc.draw_reals(c, 40 + REAL_ROWS.index(row))
    v = cc.linear(o.x, o.w)
    xa, add = ops.Act.from_dense(_dev(o.x)), ops.Act.from_dense(_dev(o.addend))
    assert np.array_equal(xa.interior().float().cpu().numpy(), o.x)                  # the operands are bf16 values already
    worst = []
    # the residual conv, relu on
    ref = cc.epilogue(v, o.b, relu=True, addend=o.addend, rounded=False)
    tol = cc.tolerance(ref, cc.magnitude(o.x, o.w, o.b, o.addend), c.k)
    y = ops.conv1x1_residual(xa, _forward_weights(ops, o.w), _dev(o.b), add, relu=True, y=_fresh(ops, c))
    torch.cuda.synchronize()
    worst.append(np.abs(y.interior().float().cpu().numpy().astype(np.float64) - ref) / np.maximum(tol, 1e-300))
    assert _border_is_zero(y)
    # the data gradient with addend and mask
    ref = cc.epilogue(v, addend=o.addend, mask=o.mask, rounded=False)
    tol = cc.tolerance(ref, cc.magnitude(o.x, o.w, None, o.addend), c.k)
    dx = ops.conv2d_bwd_data(xa, _dgrad_weights(ops, o.w), torch.zeros(c.c, device='cuda'), _fresh(ops, c), 1,
                             relu_ref=ops.Act.from_dense(_dev(o.mask)), addend=add)
    torch.cuda.synchronize()
    worst.append(np.abs(dx.interior().float().cpu().numpy().astype(np.float64) - ref) / np.maximum(tol, 1e-300))
    assert _border_is_zero(dx)
    print('%s-%s (%d,%d,%d,%d->%d): largest error / bound: residual %.3f, data gradient %.3f' % (
        row + (c.n, c.h, c.w, c.k, c.c, np.nanmax(worst[0]), np.nanmax(worst[1]))))
    for name, r in zip(('residual', 'data gradient'), worst):
        assert np.isfinite(r).all(), '%s: elements never stored' % name
        assert r.max() <= 1.0, '%s: %d elements beyond the bound, largest ratio %.3f' % (name, int((r > 1).sum()), r.max())


def test_residual_conv_refusals(ops):
    """A residual of another shape is XV_ESHAPE; none at all, or an e4m3 descriptor for any of the three maps (it would be read
    as bf16, past the end of a map of half the bytes), XV_EINVAL.  Nothing is launched: y keeps its bits."""
    from modular_semantic_segmentation_amd import _lib
    c, g = _case(('g128', 'one_partial'))
    o, _ = _integers(_cus(), ('g128', 'one_partial'), cc.R_MAX)
    xa, wp, bd = ops.Act.from_dense(_dev(o.x)), _forward_weights(ops, o.w), _dev(o.b)
    res = ops.Act.from_dense(_dev(o.addend))
    y = ops.Act(c.n, c.h, c.w, c.c)
    y.interior().fill_(7.0)
    kept = y.t.clone()

    class Null(object):
        def xv(self):
            return ops._NULL_ACT
    no_data = ops.Act(c.n, c.h, c.w, c.c)
    no_data._xv.data = None
    other_shapes = [ops.Act(c.n, c.h, c.w, c.c + 64), ops.Act(c.n, c.h + 1, c.w, c.c), ops.Act(c.n, c.h, c.w - 1, c.c),
                    ops.Act(c.n + 1, c.h, c.w, c.c)]
    for r in other_shapes:
        with pytest.raises(_lib.XvError, match='XV_ESHAPE'):
            ops.conv1x1_residual(xa, wp, bd, r, relu=True, y=y)
    for r in (Null(), no_data, ops.Act(c.n, c.h, c.w, c.c, dtype='fp8')):
        with pytest.raises(_lib.XvError, match='XV_EINVAL'):
            ops.conv1x1_residual(xa, wp, bd, r, relu=True, y=y)
    with pytest.raises(_lib.XvError, match='XV_EINVAL'):
        ops.conv1x1_residual(ops.Act(c.n, c.h, c.w, c.k, dtype='fp8'), wp, bd, res, relu=True, y=y)
    y8 = ops.Act(c.n, c.h, c.w, c.c, dtype='fp8')
    with pytest.raises(_lib.XvError, match='XV_EINVAL'):
        ops.conv1x1_residual(xa, wp, bd, res, relu=True, y=y8)
    torch.cuda.synchronize()
    assert torch.equal(y.t, kept) and not y8.t.view(torch.uint8).any()
    # ... and the same arguments with the residual it asks for go through
    ops.conv1x1_residual(xa, wp, bd, res, relu=True, y=y)
    torch.cuda.synchronize()
    assert not torch.equal(y.t, kept)
