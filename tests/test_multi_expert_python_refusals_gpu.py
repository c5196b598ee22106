"""Which layer refuses what in the seven multi-expert heads of ops.py, and with which exception class: TypeError from the
tensor checks, ValueError from the shape checks in Python, XvError (XV_EINVAL) where an op leaves the decision to the native
check.  The differences between the siblings are recorded, not smoothed: fused_head_multi hands a wrong expert count, an
unknown mode and missing tables to the native check, the counting, agreement and calibration forms refuse them in Python.

One geometry: n, hi, wi = 1, 3, 5, three experts, 5 classes (CP = 8: the padded class axis differs from C).  After each
refusal every output handed in is still full of its sentinel; then one good call per op runs."""
import pytest
import torch

from modular_semantic_segmentation_amd._lib import XvError

DEV = 'cuda:0'
N, HI, WI, C, E = 1, 3, 5, 5, 3
CP = 8
NPIX = N * HI * WI * 64
SENTINEL = -7
V, T, X = ValueError, TypeError, XvError

OPS = ['fused_head_multi', 'fused_head_multi_count', 'fused_head_multi_agreement', 'fused_head_multi_calibration',
       'fused_head_multi_tuple_hist', 'fused_head_multi_lut', 'fused_head_multi_lut_count']
# the exception class per bad input and op, in the order of OPS, as the ops raised them before their checks were gathered into
# shared helpers (None: the op does not take the argument)
EXPECTED = {
    #                       multi count agree calib hist  lut   lut_count
    'unequal_lists':       (V,    V,    V,    V,    V,    V,    V),
    'score_column_short':  (V,    V,    V,    V,    V,    V,    V),
    'score_float64':       (T,    T,    T,    T,    T,    T,    T),
    'bias_one_more':       (V,    V,    V,    V,    V,    V,    V),
    'labels_int64':        (None, T,    T,    T,    None, None, T),
    'labels_row_short':    (None, V,    V,    V,    None, None, V),
    'mode_3':              (X,    V,    V,    V,    None, None, None),
    'tab_wrong_shape':     (V,    V,    V,    V,    None, None, None),
    'bayes_without_tab':   (X,    V,    V,    V,    None, None, None),
    'lut_one_short':       (None, None, None, None, None, V,    V),
    'one_expert':          (X,    V,    V,    V,    V,    V,    V),
    'five_experts':        (X,    V,    V,    V,    V,    V,    V),
}


@pytest.fixture(scope='module')
def data():
    g = torch.Generator().manual_seed(5)
    scores = []
    for _ in range(5):
        s = torch.zeros((N, HI + 2, WI + 2, CP))
        s[:, 1:-1, 1:-1, :C] = torch.randn((N, HI, WI, C), generator=g) * 3.0
        scores.append(s.to(DEV))
    biases = [torch.randn(C, generator=g).to(DEV) for _ in range(5)]
    labels = torch.randint(-1, C, (N, 8 * HI, 8 * WI), generator=g, dtype=torch.int32).to(DEV)
    lut = torch.randint(0, C, (C ** E,), generator=g, dtype=torch.uint8).to(DEV)
    return dict(scores=scores, biases=biases, labels=labels, lut=lut, valid=int((labels >= 0).sum()))


def _tables(op, experts, mode=0, tab_shape=None):
    """the Bayes tables of `op` for `experts` experts (the counting form takes its priors per parameter set: one set)"""
    if op not in OPS[:4] or mode == 2:
        return {}
    tab = torch.zeros(tab_shape or (experts, C, C), device=DEV)
    return dict(tab=tab, logprior=torch.zeros((1, C) if op == 'fused_head_multi_count' else (C,), device=DEV))


def _sentinels(op):
    """the outputs of `op`, full of the sentinel, as keyword arguments"""
    def full(shape, dtype=torch.int64):
        return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
    return {'fused_head_multi': lambda: dict(out=full((N, 8 * HI, 8 * WI))),
            'fused_head_multi_count': lambda: dict(cm=full((1, C, C))),
            'fused_head_multi_agreement': lambda: dict(table=full((C, 1 << E, 2, 3))),
            'fused_head_multi_calibration': lambda: dict(table=full((1, 64, 3)), nll=full((1,), torch.float64)),
            'fused_head_multi_tuple_hist': lambda: dict(hist=full((C ** E,))),
            'fused_head_multi_lut': lambda: dict(out=full((N, 8 * HI, 8 * WI))),
            'fused_head_multi_lut_count': lambda: dict(cm=full((C, C)))}[op]()


def _call(ops, op, a, outs):
    head = (a['scores'], a['biases'], N, HI, WI, C)
    fn = getattr(ops, op)
    if op == 'fused_head_multi':
        return fn(*head, a['mode'], **a['tables'], **outs)
    if op in ('fused_head_multi_count', 'fused_head_multi_agreement'):
        return fn(*head, a['mode'], a['labels'], **a['tables'], **outs)
    if op == 'fused_head_multi_calibration':
        return fn(*head, a['mode'], a['labels'], temperatures=1.0, bin_bits=6, **a['tables'], **outs)
    if op == 'fused_head_multi_tuple_hist':
        return fn(*head, **outs)
    if op == 'fused_head_multi_lut':
        return fn(*head, a['lut'], **outs)
    return fn(*head, a['lut'], a['labels'], **outs)


def _bad_inputs(op, data):
    """name -> the arguments of the good call with one thing wrong"""
    S, b = data['scores'][:E], data['biases'][:E]
    good = dict(scores=S, biases=b, mode=0, labels=data['labels'], lut=data['lut'], tables=_tables(op, E))
    narrow = torch.zeros((N, HI + 2, WI + 1, CP), device=DEV)
    return {
        'unequal_lists': dict(good, biases=b[:2]),
        'score_column_short': dict(good, scores=[S[0], narrow, S[2]]),
        'score_float64': dict(good, scores=[S[0], S[1].double(), S[2]]),
        'bias_one_more': dict(good, biases=[b[0], b[1], torch.zeros(C + 1, device=DEV)]),
        'labels_int64': dict(good, labels=data['labels'].long()),
        'labels_row_short': dict(good, labels=data['labels'][:, 1:].contiguous()),
        'mode_3': dict(good, mode=3),
        'tab_wrong_shape': dict(good, tables=_tables(op, E, tab_shape=(E, C, C - 1))),
        'bayes_without_tab': dict(good, tables={k: v for k, v in good['tables'].items() if k != 'tab'}),
        'lut_one_short': dict(good, lut=data['lut'][:-1].contiguous()),
        # (tables for that many experts: what is refused is the expert count, not a table's shape)
        'one_expert': dict(good, scores=S[:1], biases=b[:1], tables=_tables(op, 1)),
        'five_experts': dict(good, scores=data['scores'], biases=data['biases'], tables=_tables(op, 5)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize('op', OPS)
def test_python_layer_refusals(op, data):
    from modular_semantic_segmentation_amd import ops
    outs = _sentinels(op)
    bad = _bad_inputs(op, data)
    assert set(bad) == set(EXPECTED)
    for name, classes in EXPECTED.items():
        cls = classes[OPS.index(op)]
        if cls is None:
            continue
        with pytest.raises(cls, match='XV_EINVAL' if cls is X else None) as info:
            _call(ops, op, bad[name], outs)
        assert info.type is cls, (op, name, info.type)         # (the class itself, not a subclass of it)
        torch.cuda.synchronize()
        for out_name, t in outs.items():
            assert int((t != SENTINEL).sum()) == 0, (op, name, out_name)   # nothing ran
    # the good call: the mean for the ops with a mode (no tables), every output made by the op
    good = dict(scores=data['scores'][:E], biases=data['biases'][:E], mode=2, labels=data['labels'], lut=data['lut'], tables={})
    if op in ('fused_head_multi', 'fused_head_multi_lut'):
        assert _call(ops, op, good, outs) is outs['out']
        torch.cuda.synchronize()
        assert int(((outs['out'] < 0) | (outs['out'] >= C)).sum()) == 0
        return
    res = _call(ops, op, good, {})
    torch.cuda.synchronize()
    if op == 'fused_head_multi_calibration':
        table, nll = res
        assert tuple(table.shape) == (1, 64, 3) and tuple(nll.shape) == (1,)
        assert int(table[..., 0].sum()) == data['valid']
    else:
        assert int(res.sum()) == (NPIX if op == 'fused_head_multi_tuple_hist' else data['valid'])
