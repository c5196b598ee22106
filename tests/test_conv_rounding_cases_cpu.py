"""tests/conv_rounding_cases.py without a GPU: the drawn operands meet the conditions that make tests/test_conv_rounding_gpu.py
mean something.  They are conditions on the float64 reference alone -- no kernel runs here:
  * 4 mag < 2^24 for every case: every partial sum in any order is an exact fp32 value (two fractional bits);
  * the bf16 store rounds more than half of the outputs, with exact ties to both sides and of both signs, so a truncating and a
    round-half-away store each differ from `stored_bf16` on every case;
  * each e4m3 output scale rounds, ties and saturates as its name says;
  * the route case holds windows in which the first maximum among the ACCUMULATORS is not the first among the STORED values;
  * the packer weights hold every rounding class at least 100 times per packed image.
The measured shares are printed (pytest -s) for DESIGN.md."""
import numpy as np
import pytest
import torch

import conv_rounding_cases as rc

CUS = (256, 304, 64, 80)            # the 1x1 shapes follow the CU count; names (and seeds) do not carry the shape
K1 = [(cus, c) for cus in CUS for c in rc.cases_1x1(cus).values()]
K1D = [(cus, c) for cus in CUS for c in rc.cases_1x1_dgrad(cus).values()]
ALL = [(0, c) for c in rc.FWD3 + rc.DGRAD3] + K1 + K1D


def _id(p):
    return p[1].name + ('@%d' % p[0] if p[0] else '')


def _drawn(case):
    o = rc.draw(case, rc.seed(case))
    return o, rc.conv_sums(o.x, o.w)


def test_reference_is_the_convolution_and_the_roundings_it_claims():
    rng = np.random.default_rng(0)
    x = rng.integers(-15, 16, (2, 5, 7, 8)).astype(np.float32)
    for k in (3, 1):
        w = rng.integers(-7, 8, (k, k, 8, 4)).astype(np.float32)
        want = torch.nn.functional.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2),
                                          torch.from_numpy(w).double().permute(3, 2, 0, 1), padding=k // 2).permute(0, 2, 3, 1).numpy()
        v, mag = rc.conv_sums(x, w)
        assert np.array_equal(v, want) and (mag >= np.abs(v)).all()
    # bf16 keeps 8 significant bits: 256 .. 512 in steps of 2, ties go to the even neighbour
    v = np.array([257.0, 259.0, 258.5, 257.5, -257.0, -259.0, 128.5, 129.5, 129.25, 0.0])
    assert rc.stored_bf16(v).tolist() == [256.0, 260.0, 258.0, 258.0, -256.0, -260.0, 128.0, 130.0, 129.0, 0.0]
    assert rc.truncated_bf16(v).tolist() == [256.0, 258.0, 258.0, 256.0, -256.0, -258.0, 128.0, 129.0, 129.0, 0.0]
    assert rc.half_away_bf16(v).tolist() == [258.0, 260.0, 258.0, 258.0, -258.0, -260.0, 129.0, 130.0, 129.0, 0.0]
    r, down, up = rc.bf16_tie_classes(v)
    assert down.tolist() == [True, False, False, False, True, False, True, False, False, False]
    assert up.tolist() == [False, True, False, False, False, True, False, True, False, False]
    assert r.tolist() == [True, True, True, True, True, True, True, True, True, False]
    # e4m3 keeps 4 significant bits and saturates at 448; the scale is applied first
    v = np.array([17.0, 19.0, 18.5, -17.0, 500.0, -1e6, 448.0, 0.0])
    assert rc.stored_e4m3(v, 0).tolist() == [16.0, 20.0, 18.0, -16.0, 448.0, -448.0, 448.0, 0.0]
    assert rc.stored_e4m3(v * 4, 2).tolist() == [64.0, 80.0, 72.0, -64.0, 1792.0, -1792.0, 1792.0, 0.0]
    r, tie, sat = rc.e4m3_classes(v, 0)
    assert tie.tolist() == [True, True, False, True, False, False, False, False] and sat.tolist() == [False] * 4 + [True, True, False, False]
    # the route rule, and a window where the accumulators name another position than the stored values
    acc = np.array([[[[257.0]], [[258.0]]], [[[3.0]], [[-5.0]]]]).reshape(1, 2, 2, 1)       # stores as 256, 258 | 3, 0
    assert rc.route_bytes(rc.stored_bf16(acc)).ravel().tolist() == [0x40]
    acc = np.array([259.0, 260.0, 3.0, -5.0]).reshape(1, 2, 2, 1)                            # stores as 260, 260
    assert rc.route_bytes(rc.stored_bf16(acc)).ravel().tolist() == [0x80] and rc.accumulator_route_bytes(acc).ravel().tolist() == [0x40]
    assert rc.route_split_windows(acc).ravel().tolist() == [True]
    assert rc.route_bytes(np.array([0.0, -1.0, 0.0, -0.0]).reshape(1, 2, 2, 1)).ravel().tolist() == [0]
    # a mask select that tells +-0 and +-1e-30 apart
    o = rc.draw(rc.DGRAD3[0], 1)
    keep = np.asarray(o.mask[0, 0, 0, :6], dtype=np.float64) > 0
    assert keep.tolist() == list(rc.SPECIAL_KEEPS) and np.signbit(o.mask[0, 0, 0, 1]) and o.mask.min() < 0


def test_case_table_covers_every_tile_configuration():
    names = [c.name for c in rc.FWD3]
    assert len(set(names)) == len(names)
    for cfg, (th, tw, partial) in rc.TILES.items():
        for cin in (64, 128):
            assert 'fwd3-%dx%d-c%d' % (th, tw, cin) in names, cfg
        if partial:
            assert 'fwd3-%dx%d-c64' % (th + 4, tw + 4) in names, cfg
    for c in rc.FWD3:
        assert c.n in (2, 3) and c.cout == 128 and c.h % 2 == 0 and c.w % 2 == 0
        if c.f8_in:
            assert c.cin % 64 == 0
    for name in (rc.SPLIT_CASE, rc.STREAMK_CASE, rc.STATS_CASE):
        assert name in names
    assert rc.fwd3_case(rc.SPLIT_CASE).cin == 512 and {c.h * 1000 + c.w for c in rc.FWD3 if c.cin == 512} == {16032, 24016, 32016}
    assert rc.ROUTE.h % 32 == 0 and rc.ROUTE.w % 64 == 0
    for cus in CUS:
        assert set(rc.cases_1x1(cus)) == set(rc.ROWS_1X1) and set(rc.cases_1x1_dgrad(cus)) == set(rc.ROWS_1X1_DGRAD)
        assert [c.f8_in for c in rc.cases_1x1(cus).values()] == [False, True, False, False]
        assert rc.cases_1x1(cus)[rc.ROW_1X1_F8].cin == 512


@pytest.mark.parametrize('cus_case', ALL, ids=_id)
def test_operands_are_exact_and_the_bf16_store_rounds(cus_case):
    case = cus_case[1]
    o, s = _drawn(case)
    assert np.abs(o.x).max() == case.x_max and np.abs(o.w).max() == rc.W_MAX and np.abs(o.b).max() <= case.b_max
    assert case.x_max == rc.X_MAX or (case.x_max <= 255 and not case.f8_in)     # wider than e4m3 holds: bf16 maps only
    assert np.array_equal(o.b * 4, np.round(o.b * 4)) and np.array_equal(o.b[::2], np.round(o.b[::2]))
    from oracle.fcn_oracle import round_bf16, round_e4m3
    for a in (o.x, o.w, o.addend, o.mask[o.mask >= 0.25]):
        assert np.array_equal(round_bf16(a), a)
    assert (np.array_equal(round_e4m3(o.x), o.x) or not case.f8_in) and np.array_equal(round_e4m3(o.w), o.w)
    assert np.abs(o.addend).max() == 255 and (o.addend != np.round(o.addend)).mean() > 0.2
    if case.kind == 'dgrad':
        forms = [('plain', dict()), ('addend', dict(addend=o.addend))]
    elif case.kind == 'k1':
        forms = [('relu off', dict(b=o.b)), ('relu on', dict(b=o.b, relu=True)), ('residual', dict(b=o.b, relu=True, residual=o.addend))]
    else:
        forms = [('relu off', dict(b=o.b)), ('relu on', dict(b=o.b, relu=True))]
    for in_exp in sorted(set((0,) + rc.in_scales(case)), reverse=True):
        for name, kw in forms:
            v, mag = rc.exact(s, in_scale_exp=in_exp, **kw)
            assert 4 * mag.max() < 2 ** 24 and np.array_equal(v * 4, np.round(v * 4))
            # relu on: over the outputs the relu lets through (a residual on a cleared output is stored unchanged)
            sel = rc.exact(s, o.b, relu=True, in_scale_exp=in_exp)[0] > 0 if kw.get('relu') else np.ones(v.shape, dtype=bool)
            stored = rc.stored_bf16(v)
            rounds, down, up = rc.bf16_tie_classes(v)
            assert np.array_equal(rounds, stored != v)
            trunc = (rc.truncated_bf16(v) != stored)[sel].mean()
            away = (rc.half_away_bf16(v) != stored)[sel].mean()
            print('%s, %s, input 2^%d: max 4 mag %d; rounds %.1f %%, ties down / up %.1f / %.1f %%; truncation differs in %.1f %%, '
                  'half-away in %.1f %%' % (case.name, name, in_exp, 4 * mag.max(), 100 * rounds[sel].mean(), 100 * down[sel].mean(),
                                            100 * up[sel].mean(), 100 * trunc, 100 * away))
            assert rounds[sel].mean() >= 0.5 and down[sel].mean() >= 0.03 and up[sel].mean() >= 0.03
            assert trunc >= 0.25 and away >= 0.03
            ties = (down | up) & sel
            assert (v[ties] > 0).any() and ((v[ties] < 0).any() or bool(kw.get('relu')))


@pytest.mark.parametrize('cus_case', [(0, c) for c in rc.FWD3] + K1, ids=_id)
def test_e4m3_scales_round_tie_and_saturate(cus_case):
    case = cus_case[1]
    o, s = _drawn(case)
    for in_exp in sorted(set((0,) + rc.in_scales(case)), reverse=True):
        e_in, e_sat = rc.e4m3_scales(rc.exact(s, o.b, in_scale_exp=in_exp)[0])
        for relu in (False, True):
            v, _ = rc.exact(s, o.b, relu=relu, in_scale_exp=in_exp)
            sel = v > 0 if relu else np.ones(v.shape, dtype=bool)
            for e, lo, hi in ((e_in, 0.0, 0.01), (e_sat, 0.10, 0.90)):
                rounds, tie, sat = rc.e4m3_classes(v, e)
                print('%s relu %d, input 2^%d, output 2^%d: rounds %.1f %%, ties %.2f %%, saturates %.1f %%' % (
                    case.name, relu, in_exp, e, 100 * rounds[sel].mean(), 100 * tie[sel].mean(), 100 * sat[sel].mean()))
                assert rounds[sel].mean() >= 0.30 and tie[sel].mean() >= 0.01
                assert lo <= sat[sel].mean() < hi if lo else sat[sel].mean() < hi
                # the stored values are bf16 values too: an e4m3 map read back as float32 compares exactly
                from oracle.fcn_oracle import round_bf16
                assert np.array_equal(round_bf16(rc.stored_e4m3(v, e)), rc.stored_e4m3(v, e))


def test_route_case_tells_the_stored_value_rule_from_the_accumulator_rule():
    o, s = _drawn(rc.ROUTE)
    v, mag = rc.exact(s, o.b, relu=True)
    assert 4 * mag.max() < 2 ** 24
    stored = rc.stored_bf16(v)
    split = rc.route_split_windows(v)
    differ = rc.accumulator_route_bytes(v) != rc.route_bytes(stored)
    codes = rc.route_bytes(stored)
    print('%s: %.2f %% of the windows hold two different accumulators that store as the same maximum; the two rules name '
          'different positions in %.2f %%; %.1f %% of the windows have no positive value' % (
              rc.ROUTE.name, 100 * split.mean(), 100 * differ.mean(), 100 * (codes == 0).mean()))
    assert split.mean() >= 0.01
    assert differ.any() and not (differ & ~split).any()
    assert sorted(np.unique(codes).tolist()) == [0, 0x10, 0x20, 0x40, 0x80] and 0.02 < (codes == 0).mean() < 0.98
    # the pooled map is the maximum of the stored values, which is the stored maximum (rounding is monotonic)
    assert np.array_equal(rc.pool2x2(stored), rc.stored_bf16(rc.pool2x2(v)))


@pytest.mark.parametrize('k,cin,cout', [(3, 64, 128), (1, 64, 128), (1, 128, 64)])
def test_packer_weights_hold_every_rounding_class(k, cin, cout):
    w, cls = rc.packer_weights((k, k, cin, cout), 7)
    from oracle.fcn_oracle import round_bf16
    r = round_bf16(w)
    assert np.isfinite(r).all() and np.abs(r).max() == np.float32(rc.BF16_MAX)
    assert np.signbit(w.ravel()[1]) and w.ravel()[0] == 0 and not np.signbit(w.ravel()[0])
    small = np.abs(w[w != 0]).min()
    assert small >= 2.0 ** -9 and np.abs(w.ravel()[4:]).max() < 32          # twelve binades, no fp32 subnormals
    counts = [int((cls == i).sum()) for i in range(5)]
    print('bf16 packer weights %s: %s' % ((k, k, cin, cout), dict(zip(rc.PACK_CLASSES, counts))))
    assert min(counts) >= 100
    assert np.array_equal(r != w, cls != 0)
    trunc, away = rc.truncated_bf16(w), rc.half_away_bf16(w)
    assert np.array_equal(trunc != r, (cls == 3) | (cls == 4)) and np.array_equal(away != r, cls == 2)
    for sign in (-1, 1):
        assert min(int(((cls == i) & (np.sign(w) == sign)).sum()) for i in range(5)) >= 40


@pytest.mark.parametrize('k', [3, 1])
@pytest.mark.parametrize('scale_exp', [0, -5])
def test_e4m3_packer_weights_tie_and_saturate(scale_exp, k):
    w, cls, sat = rc.packer_weights_e4m3((k, k, 128, 64), scale_exp, 11)
    r = rc.stored_e4m3(w, scale_exp)
    counts = [int(((cls == i) & ~sat).sum()) for i in range(5)]
    print('e4m3 packer weights at 2^%d: %s, %d saturate' % (scale_exp, dict(zip(rc.PACK_CLASSES, counts)), int(sat.sum())))
    assert min(counts) >= 100 and sat.sum() >= 100
    assert np.array_equal(np.abs(r[sat]), np.full(int(sat.sum()), 448.0 * 2.0 ** scale_exp, dtype=np.float32))
    assert np.array_equal((r != w) & ~sat, (cls != 0) & ~sat)
    rounds, tie, s2 = rc.e4m3_classes(w, scale_exp)
    assert np.array_equal(s2, sat) and np.array_equal(tie, ((cls == 2) | (cls == 3)) & ~sat)


def test_one_hot_map_reads_every_weight_once():
    for k, n, h, w, cin in ((3, 2, 16, 32, 64), (3, 3, 16, 32, 128), (1, 1, 8, 16, 128)):
        x, where = rc.one_hot_map(n, h, w, cin, k)
        assert x.sum() == cin and (x.sum((0, 1, 2)) == 1).all() and (x.sum(-1) <= 1).all()
        wt, _ = rc.packer_weights((k, k, cin, 64), k)
        from oracle.fcn_oracle import round_bf16
        y = rc.conv_sums(x, round_bf16(wt))[0]
        assert np.array_equal(rc.read_back(y, where, k), round_bf16(wt).astype(np.float64))
        assert np.count_nonzero(y) == np.count_nonzero(wt)
    # the data gradient's weights: conv_transpose of dy by the forward kernel = conv of dy by the reflected, swapped kernel
    rng = np.random.default_rng(3)
    w_eff = rng.integers(-7, 8, (3, 3, 4, 6)).astype(np.float32)            # dy has 4 channels, dx 6
    wf = rc.dgrad_forward_weights(w_eff)                                    # forward HWIO [3,3,6,4]
    dy = rng.integers(-15, 16, (1, 5, 6, 4)).astype(np.float32)
    xin = torch.zeros((1, 6, 5, 6), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xin, torch.from_numpy(wf).double().permute(3, 2, 0, 1), padding=1).backward(
        torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    assert np.array_equal(rc.conv_sums(dy, w_eff)[0], xin.grad.permute(0, 2, 3, 1).numpy())
