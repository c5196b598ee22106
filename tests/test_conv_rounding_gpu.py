"""The fp32 -> bf16 / e4m3 conversion of every conv epilogue, and of the weight packers, against ONE round-to-nearest-even of
an exactly known value -- bit for bit, no tolerance anywhere.

The small-integer tests (test_kernels_gpu.py and its neighbours) never round at the store.  Here the operands are the wide
integers of tests/conv_rounding_cases.py (x in [-15, 15], w in [-7, 7], bias in quarters): every partial sum in any order is
an exact fp32 value, so the accumulator is known and the store must be `stored_bf16` / `stored_e4m3` of it.  More than half of
the outputs round and several per cent are exact ties to either side (tests/test_conv_rounding_cases_cpu.py holds the draws to
that and shows that a truncating and a round-half-away store each fail every case).  Outputs start as NaN in the interior and
zero on the border: an element never stored fails, a border element written fails.  +0 and -0 compare equal (the packed-pair
maximum legitimately turns -0 into +0).

  forward      every tile configuration x relu on / off x full map, full map + fused pool, pooled only x bf16, e4m3 in range,
               e4m3 saturating; bf16 and e4m3 input maps.  Which (configuration, form) pairs the library refuses is the
               explicit table `_takes`; a refusal outside it fails, a launch the table does not expect fails, and the
               number of launches per configuration is asserted (FORMS_*).
  chooser      the same cases with cfg = -1, the split form (xv_conv2d_fwd_split) and the stream-K form (xv_conv2d_fwd_ws)
  data gradient / residual 1x1: the sum plus the addend is rounded ONCE
  routed pool  pooled bits, route bytes by the first maximum among the STORED values, the routed data gradient against the
               unrouted chain and against the reference
  statistics   the y of xv_conv2d_fwd_stats
  packers      fp32 weights that are not bf16 / e4m3 values (every class: exact, below half, tie to even / odd, above half, +-0,
               the largest finite bf16 plus a quarter ulp, beyond +-448 after scaling), read back through the convs with a
               one-hot input -- one packed image per configuration -- and compared with round_bf16 / round_e4m3 of the weights"""
import functools

import numpy as np
import pytest
import torch

import conv_rounding_cases as rc

pytestmark = pytest.mark.gpu

RETIRED = frozenset([0, 19, 20, 21, 25]) | frozenset(range(2, 14))
# launches per configuration on a case it applies to: relu on / off x map forms x output types
FORMS_K3_BF16_IN = {1: 18, 14: 18, 15: 18, 16: 18, 17: 6, 22: 2, 26: 18, 27: 2, 28: 6}
FORMS_K3_F8_IN = {14: 18, 15: 18, 16: 18, 24: 12}          # per input scale; 14 - 16 on 128-channel chunks only
FORMS_K1_BF16_IN = {1: 6, 14: 6, 15: 6, 16: 6, 18: 2, 23: 2}
FORMS_K1_F8_IN = {14: 6, 15: 6, 16: 6}


def _takes(cfg, case, in_f8, out_f8, pool, write_y):
    """The explicit table of what xv_conv2d_fwd_cfg accepts (conv_mfma.hip launch_cfg and the launchers behind it)."""
    k = case.k
    if cfg in RETIRED:
        return False
    if k == 1 and pool:
        return False
    if cfg in (17, 22, 24, 26, 27, 28) and k != 3:          # generations 2, 4, 5: 3x3 only
        return False
    if cfg in (18, 23) and k != 1:                          # generation 3: 1x1 only
        return False
    if cfg in (1, 18) and case.cout % 128:
        return False
    if cfg == 23 and case.cout != 64:
        return False
    if cfg in (18, 22, 23, 27) and pool:                    # no fused pool: odd rows per wave / flat GEMM
        return False
    if cfg in (17, 18, 22, 23, 27, 28) and out_f8:          # bf16 epilogues only
        return False
    if cfg == 27 and (case.h % 24 or case.w % 16):          # generation 5: exact tilings only
        return False
    if cfg == 28 and (case.h % 32 or case.w % 16):
        return False
    if cfg == 24:
        return in_f8 and out_f8                             # e4m3 in and out
    if in_f8:
        return cfg in (14, 15, 16) and case.cin % 128 == 0  # the first-generation e4m3 kernel: 128-channel chunks
    return True


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops as _ops
    return _ops


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()           # a copy: the shared operands are read-only


@functools.lru_cache(maxsize=None)
def _k1_cases(cus):
    return rc.cases_1x1(cus)


@functools.lru_cache(maxsize=None)
def _drawn(case):
    """(operands, conv sums) of a case: drawn and multiplied once, shared by the tests and left unchanged."""
    o = rc.draw(case, rc.seed(case))
    s = rc.conv_sums(o.x, o.w)
    for a in tuple(o) + s:
        a.setflags(write=False)
    return o, s


def _fresh(ops, n, h, w, c, out=None):
    """An output map whose interior is NaN (bf16, or the e4m3 NaN byte); out = None: bf16, else the e4m3 scale exponent."""
    if out is None:
        y = ops.Act(n, h, w, c)
        y.interior().fill_(float('nan'))
    else:
        y = ops.Act(n, h, w, c, dtype='fp8', scale_exp=out)
        y.t.view(torch.uint8)[:, 1:-1, 1:-1] = 0x7f
    return y


def _values(a):
    return a.real().cpu().numpy() if a.dtype == 'fp8' else a.interior().float().cpu().numpy()


def _border_is_zero(a):
    t = a.t.view(torch.uint8) if a.dtype == 'fp8' else a.t.view(torch.int16)
    return not (t[:, 0].any() or t[:, -1].any() or t[:, :, 0].any() or t[:, :, -1].any())


def _mismatch(got, ref):
    bad = np.argwhere(~(got == ref))
    return '%d of %d differ, first (n,y,x,c) %s: got %s, want %s' % (
        len(bad), ref.size, bad[:4].tolist(), got[tuple(bad[:4].T)].tolist(), ref[tuple(bad[:4].T)].tolist())


def _check(a, ref, what):
    got = _values(a)
    assert np.array_equal(got, ref), '%s: %s' % (what, _mismatch(got, ref))
    assert _border_is_zero(a), '%s: the border was written' % (what,)


def _choose(case, in_f8=False, out_f8=False, flags=0):
    from modular_semantic_segmentation_amd import _lib
    bf16, fp8 = _lib.CONSTANTS['XV_BF16'], _lib.CONSTANTS['XV_FP8']
    return _lib.lib().xv_conv2d_choose_cfg(case.n, case.h, case.w, case.cin, case.cout, case.k, fp8 if in_f8 else bf16,
                                           fp8 if out_f8 else bf16, flags)


class _Forward(object):
    """The operands of a forward case on the device and its references per (input scale, relu, output type)."""

    def __init__(self, ops, case):
        self.ops, self.case = ops, case
        self.o, self.s = _drawn(case)
        self.bias = _dev(self.o.b)
        self.inputs = [(None, ops.Act.from_dense(_dev(self.o.x)), ops.pack_conv_weights(_dev(self.o.w)))]
        for e in rc.in_scales(case):
            xa = ops.Act.from_dense(_dev(self.o.x * np.float32(2.0 ** e)), dtype='fp8', scale_exp=e)
            assert np.array_equal(xa.t[:, 1:-1, 1:-1].float().cpu().numpy(), self.o.x)      # the stored integers
            self.inputs.append((e, xa, ops.pack_conv_weights_f8(_dev(self.o.w), scale_exp=0)[0]))
        self.refs = {}

    def ref(self, in_exp, relu, out):
        """(full map, pooled map) as stored: out None = bf16, else the e4m3 scale exponent."""
        key = (in_exp, relu, out)
        if key not in self.refs:
            v, _ = rc.exact(self.s, self.o.b, relu=bool(relu), in_scale_exp=in_exp or 0)
            st = rc.stored_bf16(v) if out is None else rc.stored_e4m3(v, out)
            self.refs[key] = (st, rc.pool2x2(st) if self.case.k == 3 else None)
        return self.refs[key]

    def outs(self, in_exp):
        return (None,) + rc.e4m3_scales(rc.exact(self.s, self.o.b, in_scale_exp=in_exp or 0)[0])

    def run(self, in_exp, xa, wp, relu, form, out, cfg, **kw):
        c, ops = self.case, self.ops
        y = _fresh(ops, c.n, c.h, c.w, c.cout, out) if form != 'pool' else None
        q = _fresh(ops, c.n, c.h // 2, c.w // 2, c.cout, out) if form != 'y' else None
        ops.conv2d_fwd(xa, wp, self.bias, c.k, relu=relu, y=y, pooled=q, write_y=y is not None, cfg=cfg, **kw)
        torch.cuda.synchronize()
        ry, rq = self.ref(in_exp, relu, out)
        what = '%s cfg %d, input %s, relu %d, %s, output %s' % (c.name, cfg, in_exp, relu, form, out)
        if y is not None:
            _check(y, ry, what)
        if q is not None:
            _check(q, rq, what + ' (pooled)')


def _forms(k):
    return ('y', 'y+pool', 'pool') if k == 3 else ('y',)


def _forward_every_configuration(ops, case):
    from modular_semantic_segmentation_amd import _lib
    f = _Forward(ops, case)
    for in_exp, xa, wp in f.inputs:
        ran = {}
        for cfg in range(_lib.lib().xv_conv2d_num_cfgs()):
            for relu in (1, 0):
                for form in _forms(case.k):
                    for out in f.outs(in_exp):
                        takes = _takes(cfg, case, in_exp is not None, out is not None, form != 'y', form != 'pool')
                        try:
                            f.run(in_exp, xa, wp, relu, form, out, cfg)
                        except _lib.XvError:
                            assert not takes, 'cfg %d refuses input %s, relu %d, %s, output %s of %s' % (
                                cfg, in_exp, relu, form, out, case.name)
                            continue
                        assert takes, 'cfg %d runs input %s, relu %d, %s, output %s of %s: not in the table' % (
                            cfg, in_exp, relu, form, out, case.name)
                        ran[cfg] = ran.get(cfg, 0) + 1
        # the table again, as counts: nothing passes by being refused
        if case.k == 3:
            want = dict(FORMS_K3_BF16_IN if in_exp is None else FORMS_K3_F8_IN)
            if case.h % 24 or case.w % 16:
                want.pop(27, None)
            if case.h % 32 or case.w % 16:
                want.pop(28, None)
        else:
            want = dict(FORMS_K1_BF16_IN if in_exp is None else FORMS_K1_F8_IN)
            want.pop(23 if case.cout != 64 else 18, None)
            if case.cout % 128:
                want.pop(1, None)
        if in_exp is not None and case.cin % 128:
            want = {c: m for c, m in want.items() if c == 24}
        assert ran == want, (case.name, in_exp, ran, want)
        for cfg, (th, tw, _) in rc.TILES.items():
            if (th, tw) == (case.h, case.w) and (cfg == 24) == (in_exp is not None) and in_exp in (None, 0):
                assert cfg in ran, 'the case of configuration %d did not run on it' % cfg


@pytest.mark.parametrize('case', rc.FWD3, ids=rc.case_id)
def test_forward_3x3_every_configuration_stores_the_rounded_accumulator(ops, case):
    _forward_every_configuration(ops, case)


@pytest.mark.parametrize('row', rc.ROWS_1X1, ids=['%s-%s' % r for r in rc.ROWS_1X1])
def test_forward_1x1_every_configuration_stores_the_rounded_accumulator(ops, row):
    import conv1x1_cases as cc
    case = _k1_cases(_cus())[row]
    g = cc.geometry(_cus(), case.n, case.h, case.w, case.cin, case.cout)
    assert g.form == row[0] and _choose(case) == g.cfg, (case, g)
    _forward_every_configuration(ops, case)


@pytest.mark.parametrize('case', rc.FWD3, ids=rc.case_id)
def test_forward_3x3_on_the_choosers_pick(ops, case):
    """cfg = -1 on every form; the pick is asserted where the case is meant for one generation.  The 512-channel 24x16 case
    also runs through the split form with its workspace, the 16x32 case through the stream-K form with a zeroed workspace:
    the partial sums in the slabs are exact, so both give the same bits."""
    from modular_semantic_segmentation_amd import _lib
    f = _Forward(ops, case)
    exact16, exact24 = case.h % 16 == 0 and case.w % 32 == 0, case.h % 24 == 0 and case.w % 16 == 0
    pick = _choose(case)
    if exact16:
        assert pick == 26 and _choose(case, flags=1) == 26 and _choose(case, out_f8=True) == 26
    elif exact24:
        assert pick == 27
    else:
        assert rc.GENERATION[pick] in (1, 2), pick
    if case.f8_in and exact16:
        assert _choose(case, in_f8=True, out_f8=True) == 24
    ran = 0
    for in_exp, xa, wp in f.inputs:
        for relu in (1, 0):
            for form in _forms(3):
                for out in f.outs(in_exp):
                    if in_exp is not None and out is None and case.cin % 128:
                        # 64-channel e4m3 chunks exist in generation 4 only, which writes e4m3: refused
                        with pytest.raises(_lib.XvError):
                            f.run(in_exp, xa, wp, relu, form, out, -1)
                        continue
                    f.run(in_exp, xa, wp, relu, form, out, -1)
                    ran += 1
    assert ran == 18 * len(f.inputs) - (0 if case.cin % 128 == 0 else 6 * (len(f.inputs) - 1))
    _, xa, wp = f.inputs[0]
    if case.name == rc.SPLIT_CASE:
        arena = {}
        ws = ops.split_workspace(xa, case.cout, arena)
        assert ws is not None and pick == 27, 'the case is meant for the split form of the 24x16 tile'
        ws.fill_(float('nan'))
        for relu in (1, 0):
            f.run(None, xa, wp, relu, 'y', None, -1, split_ws=ws)
            f.run(None, xa, wp, relu, 'y', None, 27, split_ws=ws)
    if case.name == rc.STREAMK_CASE:
        # 2 images x 1 tile x 2 channel tiles = 4 tiles of 16 chunks for all the CUs: the only round is incomplete, so its
        # 64 (tile, chunk) items are dealt out and every tile is summed from slabs.  The slabs start as NaN patterns
        # (the header, which holds the arrival counters, as zeros): a launch that splits a tile has to write some.
        ws = ops.streamk_workspace('cuda')
        assert _choose(case, flags=1 | 4) == 17, 'with a pooled output and a workspace the 16x32 tile of generation 2 runs'
        for relu in (1, 0):
            for form in _forms(3):
                for cfg in (-1, 17):
                    ws[4096:] = 0xff
                    f.run(None, xa, wp, relu, form, None, cfg, workspace=ws)
                    if cfg == 17 or form != 'y':
                        assert (ws[4096:] != 0xff).any(), 'no tile was split: relu %d, %s, cfg %d' % (relu, form, cfg)
                    assert not ws[:4096].any()


def _dgrad_run(ops, case, want_cfgs):
    o, s = _drawn(case)
    got_cfg = _choose(case, flags=2)
    assert got_cfg in want_cfgs, 'the library picks configuration %d for %s, the case is meant for %s' % (got_cfg, case, want_cfgs)
    dy = ops.Act.from_dense(_dev(o.x))
    wd = ops.pack_conv_weights_dgrad(_dev(rc.dgrad_forward_weights(o.w)))
    zb = torch.zeros(case.cout, device='cuda')
    add, ref_map = ops.Act.from_dense(_dev(o.addend)), ops.Act.from_dense(_dev(o.mask))
    assert np.array_equal(add.interior().float().cpu().numpy(), o.addend)           # the addend is made of bf16 values
    assert np.array_equal(ref_map.interior().float().cpu().numpy() > 0, o.mask > 0)
    assert np.signbit(ref_map.interior()[0, 0, 0, 1].float().item()) and ref_map.interior()[0, 0, 0, 2].float().item() > 0
    before = (add.t.clone(), ref_map.t.clone())
    for use_add, use_ref in ((True, True), (False, True), (True, False), (False, False)):
        v, _ = rc.exact(s, addend=o.addend if use_add else None, mask=o.mask if use_ref else None)
        ref = rc.stored_bf16(v)
        if use_add:
            # the sum plus the addend is rounded once: a kernel that rounds before the add gives other values on this very case
            twice = rc.stored_bf16(rc.stored_bf16(s[0]).astype(np.float64) + o.addend)
            assert (twice != rc.stored_bf16(s[0] + o.addend)).mean() > 0.05
        dx = ops.conv2d_bwd_data(dy, wd, zb, _fresh(ops, case.n, case.h, case.w, case.cout), case.k,
                                 relu_ref=ref_map if use_ref else None, addend=add if use_add else None)
        torch.cuda.synchronize()
        _check(dx, ref, '%s addend %d mask %d' % (case.name, use_add, use_ref))
        if use_ref:
            got = _values(dx)
            for pix in (got[0, 0, 0, :6], got[-1, -1, -1, -6:]):
                assert not pix[[0, 1, 3, 5]].any()
    assert torch.equal(add.t, before[0]) and torch.equal(ref_map.t, before[1])


@pytest.mark.parametrize('case', rc.DGRAD3, ids=rc.case_id)
def test_data_gradient_3x3_rounds_the_sum_plus_addend_once(ops, case):
    _dgrad_run(ops, case, rc.DGRAD3_PICK[case.name])


@pytest.mark.parametrize('row', rc.ROWS_1X1_DGRAD, ids=['%s-%s' % r for r in rc.ROWS_1X1_DGRAD])
def test_data_gradient_1x1_rounds_the_sum_plus_addend_once(ops, row):
    """dy in [-31, 31] here: without a bias in quarters the narrower integers round fewer than half of these short sums."""
    _dgrad_run(ops, rc.cases_1x1_dgrad(_cus())[row], (23,) if row[0] == 'n64' else (18,))


@pytest.mark.parametrize('row', rc.ROWS_1X1, ids=['%s-%s' % r for r in rc.ROWS_1X1])
def test_residual_1x1_rounds_once_after_the_add(ops, row):
    case = _k1_cases(_cus())[row]
    o, s = _drawn(case)
    assert _choose(case, flags=2) == {'g128': 18, 'wide': 18, 'n64': 23, 'gen1': 1}[row[0]]
    xa, wp, bd = ops.Act.from_dense(_dev(o.x)), ops.pack_conv_weights(_dev(o.w)), _dev(o.b)
    res = ops.Act.from_dense(_dev(o.addend))
    for relu in (1, 0):
        v, _ = rc.exact(s, o.b, relu=bool(relu), residual=o.addend)
        y = ops.conv1x1_residual(xa, wp, bd, res, relu=relu, y=_fresh(ops, case.n, case.h, case.w, case.cout))
        torch.cuda.synchronize()
        _check(y, rc.stored_bf16(v), '%s relu %d' % (case.name, relu))
    # a kernel that rounds relu(conv + b) before the add gives other values on this very case
    twice = rc.stored_bf16(rc.stored_bf16(rc.exact(s, o.b, relu=True)[0]).astype(np.float64) + o.addend)
    assert (twice != rc.stored_bf16(rc.exact(s, o.b, relu=True, residual=o.addend)[0])).mean() > 0.05


def test_routed_pool_follows_the_stored_values(ops):
    """xv_conv2d_fwd_route: the pooled bits and the route bytes by the first maximum among the STORED values (in 4.7 % of the
    windows of this case two different accumulators store as the same maximum, in 2.5 % the accumulators name another
    position); xv_conv2d_bwd_data_route with that route: the bits of the unrouted chain xv_conv2d_bwd_data ->
    xv_maxpool2x2_bwd -> xv_relu_bwd on the map stored by xv_conv2d_fwd, and of the reference."""
    case = rc.ROUTE
    o, s = _drawn(case)
    n, h, w, cout, c2 = case.n, case.h, case.w, case.cout, rc.ROUTE_C2
    v, _ = rc.exact(s, o.b, relu=True)
    stored = rc.stored_bf16(v)
    codes = rc.route_bytes(stored)
    assert (rc.accumulator_route_bytes(v) != codes).mean() > 0.01
    xa, wp, bd = ops.Act.from_dense(_dev(o.x)), ops.pack_conv_weights(_dev(o.w)), _dev(o.b)
    q = _fresh(ops, n, h // 2, w // 2, cout)
    route = torch.full((n * (h // 2) * (w // 2) * cout,), 77, dtype=torch.uint8, device='cuda')
    assert ops.conv2d_fwd_route(xa, wp, bd, q, route)
    y, q2 = ops.conv2d_fwd(xa, wp, bd, 3, relu=True, y=_fresh(ops, n, h, w, cout), pooled=_fresh(ops, n, h // 2, w // 2, cout))
    torch.cuda.synchronize()
    _check(y, stored, 'the full map')
    _check(q, rc.pool2x2(stored), 'the routed pool')
    assert torch.equal(q.t, q2.t)
    got = route.view(n, h // 2, w // 2, cout).cpu().numpy()
    assert np.array_equal(got, codes), _mismatch(got, codes)
    # the layer behind the pool: its output gradient g, the data gradient at the pooled size, routed onto the full map
    rng = np.random.default_rng(rc.seed(case) + 1)
    g = rng.integers(-rc.X_MAX, rc.X_MAX + 1, (n, h // 2, w // 2, c2)).astype(np.float32)
    w_eff = rng.integers(-rc.W_MAX, rc.W_MAX + 1, (3, 3, c2, cout)).astype(np.float32)
    sums = rc.conv_sums(g, w_eff)
    assert 4 * sums[1].max() < 2 ** 24
    dpool_ref = rc.stored_bf16(sums[0])
    ga, wd, zero = ops.Act.from_dense(_dev(g)), ops.pack_conv_weights_dgrad(_dev(rc.dgrad_forward_weights(w_eff))), torch.zeros(cout, device='cuda')
    dpool = ops.conv2d_bwd_data(ga, wd, zero, _fresh(ops, n, h // 2, w // 2, cout), 3)
    chain = ops.maxpool2x2_bwd(y, dpool, _fresh(ops, n, h, w, cout))
    chain2 = ops.relu_bwd(chain, y, _fresh(ops, n, h, w, cout))
    dx = _fresh(ops, n, h, w, cout)
    ops.conv2d_bwd_data_route(ga, wd, zero, route, dx)
    torch.cuda.synchronize()
    _check(dpool, dpool_ref, 'the data gradient at the pooled size')
    assert torch.equal(dx.t, chain.t) and torch.equal(dx.t, chain2.t)
    win = np.zeros((n, h // 2, w // 2, cout, 4), dtype=np.float32)
    for pos in range(4):
        win[..., pos] = np.where(codes == (0x80 >> pos), dpool_ref, 0.0)
    ref = win.reshape(n, h // 2, w // 2, cout, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, h, w, cout)
    _check(dx, ref, 'the routed data gradient')


def test_statistics_form_stores_the_rounded_accumulator(ops):
    """The y of xv_conv2d_fwd_stats; the sums are not exact at these magnitudes and are held as
    test_conv_with_batch_statistics_in_its_epilogue holds them: against sums of the STORED values, with its tolerance."""
    from modular_semantic_segmentation_amd import _lib
    case = rc.fwd3_case(rc.STATS_CASE)
    o, s = _drawn(case)
    st = ops.BnState(case.cout, 'cuda')
    z = _fresh(ops, case.n, case.h, case.w, case.cout)
    assert ops.conv2d_fwd_stats(ops.Act.from_dense(_dev(o.x)), ops.pack_conv_weights(_dev(o.w)), _dev(o.b), z, st)
    _lib.check(_lib.lib().xv_bn_sums_from_rows(st.conv_rows.data_ptr(), st.conv_rows_n, 2 * case.cout, st.sums.data_ptr(), None),
               'xv_bn_sums_from_rows')
    torch.cuda.synchronize()
    stored = rc.stored_bf16(rc.exact(s, o.b)[0])
    _check(z, stored, 'the statistics form')
    zs = stored.astype(np.float64)
    want = np.concatenate([zs.sum((0, 1, 2)), (zs * zs).sum((0, 1, 2))])
    np.testing.assert_allclose(st.sums.cpu().numpy(), want, rtol=1e-5, atol=1e-3)


# ---- the weight packers ----------------------------------------------------------------------------------------------------

def _read(ops, xa, packed, k, cout, cfg, out=None):
    y = _fresh(ops, xa.n, xa.h, xa.w, cout, out)
    ops.conv2d_fwd(xa, packed, torch.zeros(cout, device='cuda'), k, relu=False, y=y, cfg=cfg)
    torch.cuda.synchronize()
    return y


def test_bf16_weight_packers_round_to_nearest_even(ops):
    """xv_pack_conv_weights, both outputs of xv_pack_conv_weights_pair, xv_pack_conv_weights_dgrad and one table launch of
    xv_pack_conv_weights_multi on fp32 weights that are not bf16 values.  A one-hot input reads each packed image back with no
    second rounding: image 1 through configuration 14, image 2 through 17, image 3 through 26 (the row permutation inside each
    64-row block along the way), the 1x1 image through 14, 18 and 23; the data-gradient images also through
    xv_conv2d_bwd_data, against the point-reflected, channel-swapped weights."""
    from oracle.fcn_oracle import round_bf16
    layers = [(3, 64, 128, (14, 17, 26)), (1, 64, 128, (14, 18)), (1, 128, 64, (14, 23))]
    W = [rc.packer_weights((k, k, cin, cout), 7)[0] for k, cin, cout, _ in layers]
    Wd = [_dev(w) for w in W]

    def buffers(transposed):
        return [torch.full((ops.packed_weight_elems(k, cout if transposed else cin, cin if transposed else cout),), float('nan'),
                           dtype=torch.bfloat16, device='cuda') for k, cin, cout, _ in layers]
    single = [ops.pack_conv_weights(w) for w in Wd]
    single_d = [ops.pack_conv_weights_dgrad(w) for w in Wd]
    pair, pair_d = buffers(False), buffers(True)
    for w, a, b in zip(Wd, pair, pair_d):
        ops.pack_conv_weights_pair(w, a, b)
    multi, multi_d = buffers(False), buffers(True)
    ops.PackTable(list(zip(Wd, multi, multi_d)), 'cuda').run()
    torch.cuda.synchronize()
    for i, (k, cin, cout, cfgs) in enumerate(layers):
        want = round_bf16(W[i])
        assert (want != W[i]).mean() > 0.6 and np.isfinite(want).all()
        # forward images
        n, h, w = (2, 16, 32) if k == 3 else (1, 8, 16)
        x, where = rc.one_hot_map(n, h, w, cin, k)
        ref = rc.conv_sums(x, want)[0].astype(np.float32)
        assert np.array_equal(rc.read_back(ref, where, k), want)
        xa = ops.Act.from_dense(_dev(x))
        for name, packed in (('xv_pack_conv_weights', single[i]), ('pair', pair[i]), ('multi', multi[i])):
            for cfg in cfgs:
                _check(_read(ops, xa, packed, k, cout, cfg), ref, '%s, layer %s, read through %d' % (name, layers[i][:3], cfg))
        # data-gradient images: a conv of `cout` channels onto `cin`
        n = -(-cout // (50 if k == 3 else h * w))
        x, where = rc.one_hot_map(n, h, w, cout, k)
        w_eff = rc.dgrad_forward_weights(want)
        ref = rc.conv_sums(x, w_eff)[0].astype(np.float32)
        assert np.array_equal(rc.read_back(ref, where, k), w_eff)
        xa = ops.Act.from_dense(_dev(x))
        for name, packed in (('xv_pack_conv_weights_dgrad', single_d[i]), ('pair', pair_d[i]), ('multi', multi_d[i])):
            dx = ops.conv2d_bwd_data(xa, packed, torch.zeros(cin, device='cuda'), _fresh(ops, n, h, w, cin), k)
            torch.cuda.synchronize()
            _check(dx, ref, '%s, layer %s, read through xv_conv2d_bwd_data' % (name, layers[i][:3]))
            for cfg in ((14, 17, 26) if k == 3 else (14,)):
                _check(_read(ops, xa, packed, k, cin, cfg), ref, '%s (dgrad), layer %s, read through %d' % (name, layers[i][:3], cfg))


@pytest.mark.parametrize('scale_exp', [0, -5])
def test_e4m3_weight_packer_rounds_to_nearest_even_and_saturates(ops, scale_exp):
    """xv_pack_conv_weights_f8 on weights at e4m3 ties and beyond +-448 after scaling, read back through an e4m3 conv with a
    one-hot e4m3 input: the 128-channel-chunk image through configurations 14 and 15 onto bf16 maps (every e4m3 value times
    a power of two is a bf16 value), the generation-4 image through 24, which writes e4m3 only: onto an e4m3 map of the
    weights' own scale, which holds every packed value exactly."""
    for k, cin, cout, cfgs in ((3, 128, 64, (14, 15, 24)), (1, 128, 64, (14, 15))):
        wt, cls, sat = rc.packer_weights_e4m3((k, k, cin, cout), scale_exp, 11)
        want = rc.stored_e4m3(wt, scale_exp)
        assert sat.sum() >= (100 if k == 3 else 10) and (want != wt).mean() > 0.6
        packed, e = ops.pack_conv_weights_f8(_dev(wt), scale_exp=scale_exp)
        assert e == scale_exp
        n, h, w = (3, 16, 32) if k == 3 else (1, 8, 16)
        x, where = rc.one_hot_map(n, h, w, cin, k)
        ref = rc.conv_sums(x, want)[0].astype(np.float32)
        assert np.array_equal(rc.read_back(ref, where, k), want)
        xa = ops.Act.from_dense(_dev(x), dtype='fp8', scale_exp=0)
        for cfg in cfgs:
            y = _read(ops, xa, packed, k, cout, cfg, out=scale_exp if cfg == 24 else None)
            _check(y, ref, 'k %d, scale 2^%d, read through %d' % (k, scale_exp, cfg))
