"""The confidence maps of csrc/confidence.hip on small maps: xv_confidence_map against the float64 definition
(calibration.confidence_reference), the histogram of the written confidences against the reliability table of
xv_calibration_table (integer for integer), and xv_fused_head_multi_confidence_fwd against xv_fused_head_multi_fwd (labels),
xv_fused_head_multi_calibration_fwd (the table) and the materialised route (E decoder heads, the fusion kernel's score output,
xv_confidence_map).

Bounds.  DELTA = (C + 8) 2^-23 bounds |conf32 - conf64| for scores given exactly (tests/test_calibration_gpu.py derives it); the
margin is a difference of two such quotients: 2 DELTA.  The entropy ln z - (sum e d) / z carries the error of z and of every
term e_k d_k, |d_k| <= spread / T: K DELTA max(1, spread / T), the form of that file's per-pixel NLL bound.  K = 2^-4 was set
from the worst measured ratio err / (DELTA max(1, spread / T)) over all cases of test_map_against_the_reference, 0.019 (the
spread of these scores is about 25, and e_k d_k peaks at 1 / e whatever the spread), doubled for inputs other than these seeds
and rounded up to a power of two; every case prints its ratio before it asserts.  Between the fused
launch and the materialised route the fused scores themselves differ by rounding: DELTA + (E C + 2) 2^-23 spread / T per
pixel, as that file has it between the two routes."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from modular_semantic_segmentation_amd.calibration import Q_ONE, confidence_reference
from test_calibration_gpu import (DEV, H, N, SENTINEL, W, _guard, _materialised, _scores, _tables, delta, random_labels,
                                  random_scores)
from test_calibration_gpu import ops  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

CLASSES = [2, 3, 12, 13, 32]
TEMPS = [0.5, 1.0, 2.5]
SHAPES = {'two_images': (N, H, W), 'one_8x8': (1, 8, 8), 'ppi_999': (1, 1, 999)}     # < one workgroup, > one, no vector width
ALL = ('label', 'confidence', 'entropy', 'margin')
ENTROPY_K = 2.0 ** -4                                   # (worst measured ratio 0.019, doubled, the next power of two)
BITS = 10

_REF = {}


def _case(c, shape):
    """(values on the host, on the device, {T: the float64 reference}) of a case, made once"""
    key = (c, shape)
    if key not in _REF:
        n, h, w = SHAPES[shape]
        values = random_scores(c, 100 + c + 7 * list(SHAPES).index(shape), n=n, h=h, w=w)
        _REF[key] = (values, torch.from_numpy(values).to(DEV), {T: confidence_reference(values, T) for T in TEMPS})
    return _REF[key]


def _q(conf):
    """the fixed-point confidence of a written float32 confidence (the product is exact)"""
    return np.floor(conf.astype(np.float64) * Q_ONE).astype(np.int64)


def _histogram(q, win, labels, c, bits=BITS):
    """the reliability table [NB, 3] of written confidences, binned with the labels"""
    nb = 1 << bits
    valid = (labels >= 0) & (labels < c)
    b = np.minimum(q >> (24 - bits), nb - 1)[valid]
    table = np.zeros((nb, 3), np.int64)
    np.add.at(table[:, 0], b, 1)
    np.add.at(table[:, 1], b, (win == labels)[valid].astype(np.int64))
    np.add.at(table[:, 2], b, q[valid])
    return table


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('c', CLASSES)
def test_map_against_the_reference(ops, c, shape):
    values, dev, ref = _case(c, shape)
    spread = float((values.max(-1) - values.min(-1)).max())
    for T in TEMPS:
        got = {k: v.cpu().numpy() for k, v in ops.confidence_map(dev, T, want=ALL).items()}
        label, conf, entropy, margin = ref[T]
        assert all(got[k].shape == label.shape for k in ALL) and got['label'].dtype == np.int64
        assert np.array_equal(got['label'], label)
        d = delta(c)
        unit = d * max(1.0, spread / T)
        errs = [np.abs(got[k].astype(np.float64) - want).max() for k, want in (('confidence', conf), ('margin', margin),
                                                                                ('entropy', entropy))]
        print('C=%d %s T=%g: |conf| %.3e |margin| %.3e (delta %.3e); entropy err %.3e = %.3f delta max(1, spread / T)' % (
            c, shape, T, errs[0], errs[1], d, errs[2], errs[2] / unit))
        assert errs[0] <= d and errs[1] <= 2 * d and errs[2] <= ENTROPY_K * unit
        assert (got['margin'] >= 0).all() and (got['margin'] <= 1).all() and (got['entropy'] >= 0).all()
        assert (got['confidence'] > 0).all() and (got['confidence'] <= 1).all()


def test_ties_and_a_spread_of_200(ops):
    c = 12
    values = torch.full((1, 4, 8, c), -200.0)
    values[..., 3] = 0.0                                 # confidence 1, margin 1, entropy 0
    values[0, 0, :, 7] = 0.0                             # the first row: classes 3 and 7 tied
    values[0, 1] = 1.5                                   # the second: every class tied
    got = {k: v.cpu().numpy()[0] for k, v in ops.confidence_map(values.to(DEV), 1.0, want=ALL).items()}
    assert (got['label'][[0, 2, 3]] == 3).all() and (got['label'][1] == 0).all()
    assert (got['margin'][:2] == 0).all() and (got['confidence'][0] == 0.5).all() and (got['confidence'][1] == np.float32(1) / np.float32(12)).all()
    assert (got['confidence'][2:] == 1).all() and (got['margin'][2:] == 1).all() and (got['entropy'][2:] == 0).all()
    assert all(np.isfinite(got[k]).all() for k in ALL[1:])
    # ln 12 from z = 12 exactly: one ulp of v_log_f32 at log2 12 < 4 (2^-21) times ln 2, and the product's rounding (2^-23)
    assert np.abs(got['entropy'][1] - np.log(12.0)).max() <= 2.0 ** -21 * np.log(2.0) + 2.0 ** -23


@pytest.mark.parametrize('c', CLASSES)
def test_the_histogram_of_the_confidences_is_the_calibration_table(ops, c):
    values, dev, _ = _case(c, 'two_images')
    labels = random_labels(values, 200 + c)
    labels[0, 0, :3] = (c, 255, -1)                      # three kinds of void
    labels_dev = torch.from_numpy(labels).to(DEV)
    for kind, source in ((0, dev), (1, torch.softmax(dev, -1).contiguous())):
        for T in TEMPS:
            got = ops.confidence_map(source, T, kind=kind)
            want, _ = ops.calibration_table(source, labels_dev, [T], BITS, kind=kind)
            table = _histogram(_q(got['confidence'].cpu().numpy()), got['label'].cpu().numpy(), labels, c)
            assert np.array_equal(table, want[0].cpu().numpy()), (kind, T)
            assert int(table[:, 0].sum()) == int(((labels >= 0) & (labels < c)).sum()) > 1000        # no pixel is set aside


FUSED_CASES = [(e, m, c) for e in (2, 3, 4) for m in (0, 1, 2) for c in (12, 13)]
GEOS = [(N, H // 8, W // 8), (1, 1, 1)]


@pytest.mark.parametrize('experts,mode,c', FUSED_CASES, ids=['E%d-%s-C%d' % (e, 'bdm'[m], c) for e, m, c in FUSED_CASES])
def test_fused_launch(ops, experts, mode, c):
    for geo in GEOS:
        n, hi, wi = geo
        S, bias = _scores(c, geo, 40 + c + experts, experts)
        tables = _tables(c, experts, mode, c + experts)
        values, kind, _ = _materialised(ops, S, bias, geo, c, mode, tables)
        host = values.cpu().numpy()
        labels_h = random_labels(host, 50 + c)
        labels = torch.from_numpy(labels_h).to(DEV)
        logs = np.log(np.float64(np.float32(1e-20)) + host) if kind == 1 else host
        spread = float((logs.max(-1) - logs.min(-1)).max())
        want_label = ops.fused_head_multi(S, bias, n, hi, wi, c, mode, **tables)
        for T in TEMPS:
            got = ops.fused_head_multi_confidence(S, bias, n, hi, wi, c, mode, T, want=ALL, **tables)
            assert all(tuple(got[k].shape) == (n, 8 * hi, 8 * wi) for k in ALL)
            assert torch.equal(got['label'], want_label)                                   # bit for bit
            table, _ = ops.fused_head_multi_calibration(S, bias, n, hi, wi, c, mode, labels, [T], BITS, **tables)
            conf = got['confidence'].cpu().numpy()
            assert np.array_equal(_histogram(_q(conf), got['label'].cpu().numpy(), labels_h, c), table[0].cpu().numpy()), T
            plain = ops.confidence_map(values, T, kind=kind, want=ALL)
            assert torch.equal(plain['label'], want_label)
            err = float(np.abs(conf.astype(np.float64) - plain['confidence'].cpu().numpy()).max())
            bound = delta(c) + (experts * c + 2) * 2.0 ** -23 * spread / T
            print('E=%d mode=%d C=%d %s T=%g: fused against materialised |conf| %.3e (bound %.3e), equal bits: %s' % (
                experts, mode, c, geo, T, err, bound, all(torch.equal(got[k], plain[k]) for k in ALL)))
            # measured: the fused scores of both routes carry the same bits in every mode (the head runs the statements of the
            # decoder heads and the fusion kernels), so all four maps are EQUAL; the bound is what rounding could cost at most
            assert err <= bound and all(torch.equal(got[k], plain[k]) for k in ALL)


def test_the_threshold_voids_below_the_bin_edge(ops):
    c, geo = 12, (N, H // 8, W // 8)
    values, dev, _ = _case(c, 'two_images')
    S, bias = _scores(c, geo, 3, 3)
    tables = _tables(c, 3, 1, 3)
    for run in (lambda **kw: ops.confidence_map(dev, 2.5, **kw),
                lambda **kw: ops.fused_head_multi_confidence(S, bias, *geo, c, 1, 2.5, **dict(tables, **kw))):
        base = run()
        q, label = _q(base['confidence'].cpu().numpy()), base['label'].cpu().numpy()
        seen = set()
        for j in range(17):
            for void in (-1, 255):
                got = run(threshold=j / 16.0, void_label=void)
                assert np.array_equal(got['label'].cpu().numpy(), np.where(q < j << 20, void, label)), (j, void)
                assert torch.equal(got['confidence'], base['confidence'])                  # the threshold moves the label alone
            seen.add(int((q < j << 20).sum()))
        assert len(seen) > 8 and 0 in seen and q.size in seen                             # the thresholds cut the pixels apart


def _raw_calls(ops):
    """(call(entry, **changes) -> return code, the four sentinel buffers) for both entry points on a small case"""
    from modular_semantic_segmentation_amd import _lib
    from modular_semantic_segmentation_amd.ops import _ptr, _ptr_array
    c, geo = 12, (N, H // 8, W // 8)
    n, hi, wi = geo
    values = _case(c, 'two_images')[1]
    S, bias = _scores(c, geo, 3, 3)
    t = _tables(c, 3, 1, 3)
    bufs = {'label_out': _guard((N, H, W), torch.int64), 'conf_out': _guard((N, H, W), torch.float32),
            'entropy_out': _guard((N, H, W), torch.float32), 'margin_out': _guard((N, H, W), torch.float32)}
    outs = dict(dict(temperature=1.0, threshold=0.0, void_label=-1), **{k: _ptr(v) for k, v in bufs.items()})
    good = {'xv_confidence_map': dict(dict(values=_ptr(values), kind=0, n=N, ppi=H * W, num_classes=c), **outs),
            'xv_fused_head_multi_confidence_fwd': dict(dict(
                S=_ptr_array(S), bias=_ptr_array(bias), num_experts=3, n=n, hi=hi, wi=wi, num_classes=c, mode=1, tab=_ptr(t['tab']),
                lognorm=_ptr(t['lognorm']), logprior=_ptr(t['logprior'])), **outs)}
    keep = [values, S, bias, t]

    def call(entry, **change):
        assert keep
        return getattr(_lib.lib(), entry)(*dict(good[entry], **change).values(), ctypes.c_void_p(0))
    return call, bufs, (S, bias, t, values)


@pytest.mark.parametrize('entry', ['xv_confidence_map', 'xv_fused_head_multi_confidence_fwd'])
def test_outputs_not_asked_for_are_not_touched(ops, entry):
    call, bufs, _ = _raw_calls(ops)
    null = ctypes.c_void_p(0)
    assert call(entry) == 0
    full = {k: v.clone() for k, v in bufs.items()}
    assert all(not bool((v == SENTINEL).any()) for k, v in full.items() if k != 'label_out')
    assert bool((full['label_out'] >= 0).all())
    for r in range(1, 4):
        for subset in itertools.combinations(bufs, r):
            for v in bufs.values():
                v.fill_(SENTINEL)
            assert call(entry, **{k: null for k in bufs if k not in subset}) == 0
            for k, v in bufs.items():
                assert torch.equal(v, full[k]) if k in subset else bool((v == SENTINEL).all()), (subset, k)


def test_refusals_leave_the_outputs_untouched(ops):
    call, bufs, (S, bias, t, values) = _raw_calls(ops)
    null = ctypes.c_void_p(0)

    def off(tensor, by):
        return ctypes.c_void_p(tensor.data_ptr() + by)
    shared = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('nan')), dict(temperature=float('inf')),
              dict(threshold=-0.5), dict(threshold=1.5), dict(threshold=float('nan')), dict(threshold=float('inf')),
              dict(num_classes=1), dict(num_classes=33), dict(n=0),
              dict(label_out=null, conf_out=null, entropy_out=null, margin_out=null),
              dict(label_out=off(bufs['label_out'], 4)), dict(conf_out=off(bufs['conf_out'], 2)),
              dict(entropy_out=off(bufs['entropy_out'], 2)), dict(margin_out=off(bufs['margin_out'], 2))]
    only = {'xv_confidence_map': [dict(kind=2), dict(kind=-1), dict(ppi=0), dict(values=null), dict(values=off(values, 2))],
            'xv_fused_head_multi_confidence_fwd': [
                dict(mode=3), dict(mode=-1), dict(hi=0), dict(wi=-1), dict(num_experts=1), dict(num_experts=5), dict(S=None),
                dict(bias=None), dict(tab=null), dict(lognorm=null), dict(logprior=null), dict(mode=0, tab=null),
                dict(mode=0, logprior=null), dict(tab=off(t['tab'], 2))]}
    for e in range(3):
        for name, tensors, offsets in (('S', S, (None, 4)), ('bias', bias, (None, 2))):
            for by in offsets:
                ptrs = [x.data_ptr() for x in tensors]
                ptrs[e] = 0 if by is None else ptrs[e] + by
                only['xv_fused_head_multi_confidence_fwd'].append({name: (ctypes.c_void_p * 3)(*ptrs)})
    for entry, cases in only.items():
        for change in shared + cases:
            assert call(entry, **change) == -1, (entry, change)
    torch.cuda.synchronize()
    assert all(bool((v == SENTINEL).all()) for v in bufs.values())
    for kwargs in (dict(temperature=0.0), dict(threshold=1.5), dict(kind=2), dict(want=()), dict(want=('label', 'label')),
                   dict(want=('variance',))):
        with pytest.raises(ValueError):
            ops.confidence_map(values, **kwargs)
    with pytest.raises(ValueError):
        ops.fused_head_multi_confidence(S, bias, N, H // 8, W // 8, 12, 1, tab=t['tab'])
    with pytest.raises(ValueError):
        ops.fused_head_multi_confidence(S[:1], bias[:1], N, H // 8, W // 8, 12, 2)
    with pytest.raises(TypeError):
        ops.confidence_map(values.double())
    # `out` takes the maps it is given
    mine = torch.empty((N, H, W), dtype=torch.float32, device=DEV)
    got = ops.confidence_map(values, out={'confidence': mine})
    assert got['confidence'] is mine and sorted(got) == ['confidence', 'label']


def test_probabilities_of_exactly_zero_and_one(ops):
    c = 12
    probs = torch.softmax(torch.from_numpy(random_scores(c, 5, n=1, h=8, w=8)), -1)
    probs[0, 0, :] = 0.0
    probs[0, 0, :, 5] = 1.0                              # one class has it all
    probs[0, 1, :] = 0.0
    probs[0, 1, :, 2] = 0.5
    probs[0, 1, :, 9] = 0.5                              # a tie, the rest exactly 0
    for T in TEMPS:
        got = {k: v.cpu().numpy()[0] for k, v in ops.confidence_map(probs.to(DEV), T, kind=1, want=ALL).items()}
        assert all(np.isfinite(got[k]).all() for k in ALL[1:])
        assert np.array_equal(got['label'], probs[0].numpy().argmax(-1))
        assert (got['label'][0] == 5).all() and (got['label'][1] == 2).all() and (got['margin'][1] == 0).all()
        label, conf, entropy, margin = confidence_reference(probs.numpy(), T, kind=1)
        # the bound of tests/test_calibration_gpu.py for probability maps: the float32 rounding of ln(1e-20 + p) moves every
        # exponent by up to 2 |ln 1e-20| 2^-23 / T
        d = delta(c) + c * (2 * 46.06 / T + 1) * 2.0 ** -23
        assert np.abs(got['confidence'] - conf[0]).max() <= d and np.abs(got['margin'] - margin[0]).max() <= 2 * d
