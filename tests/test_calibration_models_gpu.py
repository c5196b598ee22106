"""BaseModel.score_calibration / calibration_search on small models: the fused route (one ops.fused_head_multi_calibration
launch per batch, nothing materialised) against the same model with fused_head=False (the fusion kernel's score output,
ops.calibration_table), against score() -- the table's count and correct columns are the confusion matrix's total and trace --
and, for the experts' own tables, against a single `fcn` model built from the same weights.  Fixtures as
tests/test_agreement_models_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo

U = 64
H, W = 48, 64
C = 12
CHANNELS = {'rgb': 3, 'depth': 1, 'ir': 1}
FIRST_SCALE = {'rgb': 0.02, 'depth': 2e-4, 'ir': 2e-4}                  # conv1_1 against inputs up to 255 / 65 535
TWO, THREE = ('rgb', 'depth'), ('rgb', 'depth', 'ir')
KINDS = ('bayes_fusion', 'dirichlet_fusion', 'average_fusion')
CASES = [(kind, mods) for kind in KINDS for mods in (TWO, THREE)]
IDS = ['%s-e%d' % (k, len(m)) for k, m in CASES]
LEFT_OUT = 0.01
BITS = 10


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _desc(mods):
    return (dict({m: 'float32' for m in mods}, labels='int32'),
            dict({m: (None, None, CHANNELS[m]) for m in mods}, labels=(None, None)), C)


@pytest.fixture(scope='module')
def data():
    """two batches of two images; labels with some void"""
    rng = np.random.default_rng(3)
    d = {m: rng.integers(0, 256 if FIRST_SCALE[m] > 1e-3 else 65536, (4, H, W, CHANNELS[m])).astype(np.float32) for m in THREE}
    d['labels'] = rng.integers(-1, C, (4, H, W)).astype(np.int32)
    return d


@pytest.fixture(scope='module')
def weights(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp('calibration')
    paths = {}
    for i, m in enumerate(THREE):
        w = fo.init_fcn_weights(m, CHANNELS[m], U, C, seed=11 + i, bias_scale=0.02)
        w['%s/conv1_1/kernel' % m] *= FIRST_SCALE[m]
        for k in w:
            if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
                w[k] *= 1.6
        paths[m] = os.path.join(str(tmp), '%s.npz' % m)
        np.savez(paths[m], **w)
    return paths


def _tables(kind, mods):
    rng = np.random.default_rng(5 * C + len(mods))
    if kind == 'bayes_fusion':
        return dict(confusion_matrices={m: rng.integers(1, 50, (C, C)) + 400 * np.eye(C, dtype=np.int64) for m in mods})
    if kind == 'dirichlet_fusion':
        params = {m: rng.uniform(0.5, 2.0, (C, C)) + 4.0 * np.eye(C) for m in mods}
        params['class_counts'] = rng.integers(100, 1000, C).astype(np.float64)
        return dict(dirichlet_params=params, sigma=1.0, delta=1e-2, beta=1e-2)
    return {}


def _model(weights, kind, mods, **config):
    from modular_semantic_segmentation_amd import get_model
    named = dict(modalities=list(mods)) if kind == 'dirichlet_fusion' else dict(prefixes={m: m for m in mods})
    cfg = dict(num_units=U, num_channels={m: CHANNELS[m] for m in mods}, expert_model='fcn', batchsize=2, class_prior='data')
    cfg.update(_tables(kind, mods))
    cfg.update(named)
    cfg.update(config)
    net = get_model(kind)(data_description=_desc(mods), **cfg)
    for m in mods:
        net.import_weights(weights[m], warnings=False)
    return net


def _only(data, mods):
    return {k: v for k, v in data.items() if k in mods or k == 'labels'}


_CACHE = {}


def _scored(weights, data, kind, mods):
    """the model pair of a case and what both routes count, computed once"""
    key = (kind, mods)
    if key not in _CACHE:
        fused, plain = _model(weights, kind, mods), _model(weights, kind, mods, fused_head=False)
        d = _only(data, mods)
        _CACHE[key] = dict(fused=fused, plain=plain, data=d, on=fused.score_calibration(d, bin_bits=BITS),
                           off=plain.score_calibration(d, bin_bits=BITS), cm=fused.score(d)[1])
    return _CACHE[key]


@pytest.mark.parametrize('kind,mods', CASES, ids=IDS)
def test_fused_head_on_against_off_and_against_score(gpu, weights, data, kind, mods, monkeypatch):
    from modular_semantic_segmentation_amd import ops
    k = _scored(weights, data, kind, mods)
    (m_on, t_on), (m_off, t_off), cm = k['on'], k['off'], k['cm']
    assert t_on.shape == (1 << BITS, 3) and t_on.dtype == np.int64
    pixels = int(cm.sum())
    for t in (t_on, t_off):
        assert int(t[:, 0].sum()) == pixels and int(t[:, 1].sum()) == int(np.trace(cm))
    moved = np.abs(t_on[:, 0] - t_off[:, 0]).sum() / 2
    print('%s, %d experts: %d of %d pixels moved bin between the routes; ECE %.5f / %.5f, overconfidence %.4f' % (
        kind, len(mods), moved, pixels, m_on['ECE'], m_off['ECE'], m_on['overconfidence']))
    assert moved <= LEFT_OUT * pixels
    assert abs(m_on['ECE'] - m_off['ECE']) <= 2.0 ** -BITS
    assert m_on['accuracy'] == np.trace(cm) / pixels and m_on['pixels'] == pixels
    # which route ran: the fused one never materialises, the plain one never launches the fused head
    calls = {'head': 0, 'table': 0}
    real = (ops.fused_head_multi_calibration, ops.calibration_table)
    monkeypatch.setattr(ops, 'fused_head_multi_calibration', lambda *a, **kw: calls.__setitem__('head', calls['head'] + 1) or real[0](*a, **kw))
    monkeypatch.setattr(ops, 'calibration_table', lambda *a, **kw: calls.__setitem__('table', calls['table'] + 1) or real[1](*a, **kw))
    k['fused'].score_calibration(k['data'], max_iterations=1)
    assert calls == {'head': 1, 'table': 0}
    k['plain'].score_calibration(k['data'], max_iterations=1)
    assert calls == {'head': 1, 'table': 1}


@pytest.mark.parametrize('kind,mods', [CASES[0], CASES[3], CASES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_search_and_groups(gpu, weights, data, kind, mods):
    k = _scored(weights, data, kind, mods)
    net, d = k['fused'], k['data']
    search = net.calibration_search(d, [0.5, 1.0, 2.0], bin_bits=BITS)
    assert search['temperatures'] == [0.5, 1.0, 2.0] and search['best'] in search['temperatures']
    assert np.array_equal(search['tables'][1], k['on'][1])
    one = dict(search['measures'][1])
    want = dict(k['on'][0])
    assert one.pop('NLL') == pytest.approx(want.pop('NLL'), rel=1e-9)            # (a double sum: the order of the atomics)
    da, db = one.pop('diagram'), want.pop('diagram')
    assert one == want and all(np.array_equal(da[x], db[x], equal_nan=True) for x in da)
    assert search['best'] == search['temperatures'][int(np.argmin([m['NLL'] for m in search['measures']]))]
    per_image = net.score_calibration(d, groups='image', bin_bits=BITS)
    assert sorted(per_image) == [0, 1, 2, 3]
    assert np.array_equal(sum(t for _, t in per_image.values()), k['on'][1])
    plain = k['plain'].score_calibration(d, groups=['a', 'b', 'a', 'b'], bin_bits=BITS)
    assert sorted(plain) == ['a', 'b'] and np.array_equal(plain['a'][1] + plain['b'][1], k['off'][1])


@pytest.mark.parametrize('fused_head', [True, False], ids=['fused', 'materialised'])
def test_experts_equal_single_fcn_models(gpu, weights, data, fused_head):
    from modular_semantic_segmentation_amd import get_model
    mods = THREE
    net = _model(weights, 'dirichlet_fusion', mods, fused_head=fused_head)
    d = _only(data, mods)
    measures, table, experts = net.score_calibration(d, experts=True, bin_bits=BITS)
    assert np.array_equal(table, _scored(weights, data, 'dirichlet_fusion', mods)['on' if fused_head else 'off'][1])
    assert list(experts) == list(mods)
    for m in mods:
        single = get_model('fcn')(m, _desc((m,)), m, num_units=U, batch_normalization=False, batchsize=2)
        single.import_weights(weights[m], warnings=False)
        want_m, want = single.score_calibration(_only(data, (m,)), bin_bits=BITS)
        got_m, got = experts[m]
        assert np.array_equal(got[:, :2], want[:, :2]), m                         # the exact columns
        assert abs(got_m['ECE'] - want_m['ECE']) <= 2.0 ** -BITS, m
        print('%s: q sums %d (from the fusion) and %d (single model)' % (m, int(got[:, 2].sum()), int(want[:, 2].sum())))
        assert int(got[:, 0].sum()) == int((d['labels'] >= 0).sum())


def test_models_without_class_scores_refuse(gpu, weights, data):
    d = _only(data, TWO)
    with pytest.raises(NotImplementedError, match='lookup'):
        _model(weights, 'bayes_fusion', TWO, decision_matrix=True).score_calibration(d)
    from modular_semantic_segmentation_amd import get_model
    cfg = dict(num_units=U, num_channels={m: CHANNELS[m] for m in TWO}, expert_model='fcn', batchsize=2,
               prefixes={m: m for m in TWO})
    variance = get_model('variance_fusion')(data_description=_desc(TWO), dropout_rate=0.5, num_samples=3, **cfg)
    with pytest.raises(NotImplementedError, match='dropout'):
        variance.score_calibration(d)
    ibcc = get_model('ibcc_fusion')(data_description=_desc(TWO), **dict(cfg, **_tables('bayes_fusion', TWO)))
    with pytest.raises(NotImplementedError, match='lookup'):
        ibcc.calibration_search(d, [1.0, 2.0])
