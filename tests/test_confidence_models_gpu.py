"""BaseModel.predict_confidence / fit_temperature on small models (the fixtures of tests/test_calibration_models_gpu.py): the label
is predict()'s, the fused route (one ops.fused_head_multi_confidence launch per batch) against the same model with
fused_head=False within the bound tests/test_confidence_gpu.py holds between the two routes, the histogram of the returned
confidences against score_calibration's table on the same route (integer for integer), the threshold against
calibration.risk_coverage of that table, the stored temperature, a single `fcn`, and the models that refuse."""
import numpy as np
import pytest
import torch

from modular_semantic_segmentation_amd.calibration import Q_ONE, risk_coverage
from test_calibration_models_gpu import BITS, C, CASES, CHANNELS, IDS, TWO, U, _desc, _model, _only, _scored, _tables
from test_calibration_models_gpu import data, gpu, weights  # noqa: F401  (the module-scoped fixtures)

pytestmark = pytest.mark.gpu

MAPS = ('confidence', 'entropy', 'margin')


def _table_of(conf, label, truth):
    """the reliability table [NB, 3] of returned confidences against the ground truth"""
    nb = 1 << BITS
    q = np.floor(conf.astype(np.float64) * Q_ONE).astype(np.int64)
    valid = (truth >= 0) & (truth < C)
    b = np.minimum(q >> (24 - BITS), nb - 1)[valid]
    table = np.zeros((nb, 3), np.int64)
    np.add.at(table[:, 0], b, 1)
    np.add.at(table[:, 1], b, (label == truth)[valid].astype(np.int64))
    np.add.at(table[:, 2], b, q[valid])
    return table


def _spread(net, d):
    """the largest spread of the class scores the materialised route hands to ops.confidence_map"""
    from modular_semantic_segmentation_amd.base_model import iterate_batches
    from modular_semantic_segmentation_amd.basic_fusion_model import run_experts
    worst = 0.0
    for batch in iterate_batches(d, net.config['batchsize']):
        values, kind = net._calibration_values(run_experts(net, batch, net.expert_wants))
        v = values.double()
        v = torch.log(float(np.float32(1e-20)) + v) if kind == 1 else v
        worst = max(worst, float((v.max(-1).values - v.min(-1).values).max()))
    return worst


@pytest.mark.parametrize('kind,mods', CASES, ids=IDS)
def test_fused_head_on_against_off_and_against_the_tables(gpu, weights, data, kind, mods, monkeypatch):
    from modular_semantic_segmentation_amd import ops
    k = _scored(weights, data, kind, mods)
    d, truth, E = k['data'], k['data']['labels'], len(mods)
    on, off = k['fused'].predict_confidence(d, outputs=MAPS), k['plain'].predict_confidence(d, outputs=MAPS)
    assert sorted(on) == sorted(('label',) + MAPS) and on['label'].dtype == np.int64 and on['label'].shape == truth.shape
    assert all(on[m].dtype == np.float32 and on[m].shape == truth.shape for m in MAPS)
    assert np.array_equal(on['label'], k['fused'].predict(d)) and np.array_equal(off['label'], k['plain'].predict(d))
    # the two routes: the bound of tests/test_confidence_gpu.py between the fused launch and the materialised route (T = 1)
    bound = (C + 8) * 2.0 ** -23 + (E * C + 2) * 2.0 ** -23 * _spread(k['plain'], d)
    err = float(np.abs(on['confidence'].astype(np.float64) - off['confidence']).max())
    print('%s, %d experts: fused head on against off |conf| %.3e (bound %.3e)' % (kind, E, err, bound))
    assert np.array_equal(on['label'], off['label']) and err <= bound
    # the histogram of what is returned is the table score_calibration counts on the same route
    assert np.array_equal(_table_of(on['confidence'], on['label'], truth), k['on'][1])
    assert np.array_equal(_table_of(off['confidence'], off['label'], truth), k['off'][1])
    # the threshold: what stays is what risk_coverage reads off the table at that edge
    curve, nb, valid = risk_coverage(k['on'][1]), 1 << BITS, (truth >= 0) & (truth < C)
    for j in (0, 1, nb // 4, nb // 2, nb - 100, nb - 1):
        got = k['fused'].predict_confidence(d, threshold=j / nb, void_label=255)
        kept = (got['label'] != 255) & valid
        assert np.array_equal(got['label'], np.where(on['confidence'] < np.float32(j / nb), 255, on['label']))
        assert kept.sum() / np.float64(valid.sum()) == curve['coverage'][j], j
        if kept.any():
            assert 1.0 - (got['label'] == truth)[kept].sum() / np.float64(kept.sum()) == curve['risk'][j], j
    # which route ran: the fused one never materialises, the plain one never launches the fused head
    calls = {'head': 0, 'map': 0}
    real = (ops.fused_head_multi_confidence, ops.confidence_map)
    monkeypatch.setattr(ops, 'fused_head_multi_confidence', lambda *a, **kw: calls.__setitem__('head', calls['head'] + 1) or real[0](*a, **kw))
    monkeypatch.setattr(ops, 'confidence_map', lambda *a, **kw: calls.__setitem__('map', calls['map'] + 1) or real[1](*a, **kw))
    one = {m: v[:2] for m, v in d.items()}
    k['fused'].predict_confidence(one)
    assert calls == {'head': 1, 'map': 0}
    k['plain'].predict_confidence(one)
    assert calls == {'head': 1, 'map': 1}


def test_the_fitted_temperature_is_the_default(gpu, weights, data):
    k = _scored(weights, data, *CASES[0])
    net, d = k['fused'], k['data']
    try:
        search = net.fit_temperature(d, [0.5, 2.0, 4.0])
        best = net.config['temperature']
        assert best == search['best'] and best in (0.5, 2.0, 4.0) and search['temperatures'] == [0.5, 2.0, 4.0]
        stored, named, one = net.predict_confidence(d), net.predict_confidence(d, temperature=best), net.predict_confidence(d, temperature=1.0)
        assert np.array_equal(stored['confidence'], named['confidence']) and np.array_equal(stored['label'], one['label'])
        assert not np.array_equal(stored['confidence'], one['confidence'])
        assert np.array_equal(_table_of(stored['confidence'], stored['label'], d['labels']), search['tables'][search['temperatures'].index(best)])
        default = net.fit_temperature(d)
        assert len(default['temperatures']) == 9 and default['temperatures'][0] == 0.25 and default['temperatures'][-1] == 4.0
    finally:
        net.config.pop('temperature', None)               # (the model is shared with the other tests)


def test_a_single_fcn(gpu, weights, data):
    from modular_semantic_segmentation_amd import get_model
    m = 'rgb'
    net = get_model('fcn')(m, _desc((m,)), m, num_units=U, batch_normalization=False, batchsize=2)
    net.import_weights(weights[m], warnings=False)
    d = _only(data, (m,))
    got = net.predict_confidence(d, outputs=MAPS)
    assert np.array_equal(got['label'], net.predict(d))
    assert np.array_equal(_table_of(got['confidence'], got['label'], d['labels']), net.score_calibration(d, bin_bits=BITS)[1])
    assert (got['margin'] >= 0).all() and (got['margin'] <= got['confidence']).all() and (got['entropy'] >= 0).all()


def test_models_without_class_scores_refuse(gpu, weights, data):
    d = _only(data, TWO)
    with pytest.raises(NotImplementedError, match='lookup'):
        _model(weights, 'bayes_fusion', TWO, decision_matrix=True).predict_confidence(d)
    from modular_semantic_segmentation_amd import get_model
    cfg = dict(num_units=U, num_channels={m: CHANNELS[m] for m in TWO}, expert_model='fcn', batchsize=2,
               prefixes={m: m for m in TWO})
    variance = get_model('variance_fusion')(data_description=_desc(TWO), dropout_rate=0.5, num_samples=3, **cfg)
    with pytest.raises(NotImplementedError, match='dropout'):
        variance.predict_confidence(d)
    ibcc = get_model('ibcc_fusion')(data_description=_desc(TWO), **dict(cfg, **_tables('bayes_fusion', TWO)))
    with pytest.raises(NotImplementedError, match='lookup'):
        ibcc.predict_confidence(d, outputs=('margin',))
