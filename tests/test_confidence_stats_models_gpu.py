"""The uncertainty benchmarks of the fusion models and of a single `fcn` on small models (the fixtures of
tests/test_calibration_models_gpu.py): the fused route (one ops.fused_head_multi_confidence_stats launch per batch and
temperature) against the same model with fused_head=False (the fusion kernel's score output, ops.confidence_stats), integer
for integer; the public methods against the ROC of those tables; a temperature search against separate passes; the experts' own
tables against a single `fcn` built from the same weights; and the models that refuse."""
import numpy as np
import pytest

from modular_semantic_segmentation_amd import ops
from modular_semantic_segmentation_amd.uncertainty_model import bin_index, confidence_tables_reference, roc_from_histogram
from test_calibration_models_gpu import C, CASES, CHANNELS, IDS, TWO, U, _desc, _model, _only, _scored, _tables
from test_calibration_models_gpu import data, gpu, weights  # noqa: F401  (the module-scoped fixtures)

pytestmark = pytest.mark.gpu

METRICS = ('entropy', 'least_confidence', 'small_margin')


@pytest.mark.parametrize('kind,mods', CASES, ids=IDS)
def test_fused_head_on_against_off(gpu, weights, data, kind, mods, monkeypatch):
    k = _scored(weights, data, kind, mods)
    d, truth = k['data'], k['data']['labels']
    assert k['fused'].uncertainty_metrics == ops.CONFIDENCE_METRICS == METRICS
    on, off = k['fused'].uncertainty_tables(d, experts=True), k['plain'].uncertainty_tables(d, experts=True)
    valid = int(((truth >= 0) & (truth < C)).sum())
    assert on['metrics'] == METRICS and on['hist'].shape == (3, 2, 24 << 5) and on['hist'].dtype == np.int64
    assert (on['hist'].sum((1, 2)) == valid).all() and int(on['counts'].sum()) == valid
    moved = int(np.abs(on['hist'] - off['hist']).sum()) // 2
    print('%s, %d experts: %d of %d x 3 counts differ between the routes; nll %.12g / %.12g' % (
        kind, len(mods), moved, valid, on['nll_sum'].sum(), off['nll_sum'].sum()))
    assert np.array_equal(on['hist'], off['hist']) and np.array_equal(on['counts'], off['counts'])
    assert sorted(on['experts']) == sorted(mods)
    for m in mods:
        assert np.array_equal(on['experts'][m]['hist'], off['experts'][m]['hist']), m
        assert np.array_equal(on['experts'][m]['counts'], on['counts'])
    # the tables are those of the maps predict_confidence returns on the same route
    maps = k['fused'].predict_confidence(d, outputs=('confidence', 'entropy', 'margin'))
    want = confidence_tables_reference(maps, maps['label'], truth, num_classes=C)
    assert np.array_equal(on['hist'], want['hist']) and np.array_equal(on['counts'], want['counts'])
    # the public methods are the ROC of those tables; a data set against itself is a coin
    for i, metric in enumerate(METRICS):
        fpr, tpr, auroc, thresholds = k['fused'].misclassification_detection_score(d, metric)
        ref = roc_from_histogram(on['hist'][i], on['edges'])
        assert auroc == ref[2] and np.array_equal(fpr, ref[0]) and np.array_equal(tpr, ref[1])
        assert k['fused'].out_of_distribution_detection_score(d, metric, d)[2] == 0.5
        counts, edges = k['fused'].value_distribution(d, metric)
        assert np.array_equal(counts, on['hist'][i].sum(0)) and np.array_equal(edges, on['edges'])
    nll, class_counts = k['fused'].nll_score(d)
    # (another pass: the double atomics add the same float terms in another order, 1e-12 relative as tests/test_confidence_stats_gpu.py has it)
    assert np.array_equal(class_counts, on['counts']) and np.allclose(nll, on['nll_sum'] / on['counts'], rtol=1e-12, atol=0)
    # which route ran: the fused one never materialises, the plain one never launches the fused head
    calls = {'head': 0, 'map': 0}
    real = (ops.fused_head_multi_confidence_stats, ops.confidence_stats)
    monkeypatch.setattr(ops, 'fused_head_multi_confidence_stats',
                        lambda *a, **kw: calls.__setitem__('head', calls['head'] + 1) or real[0](*a, **kw))
    monkeypatch.setattr(ops, 'confidence_stats', lambda *a, **kw: calls.__setitem__('map', calls['map'] + 1) or real[1](*a, **kw))
    one = {m: v[:2] for m, v in d.items()}
    k['fused'].uncertainty_tables(one, experts=True)
    assert calls == {'head': 1, 'map': 0}
    k['plain'].uncertainty_tables(one)
    assert calls == {'head': 1, 'map': 1}


def test_out_of_distribution_reads_no_labels(gpu, weights, data):
    k = _scored(weights, data, *CASES[0])
    d = k['data']
    foreign = {m: v[::-1].copy() * 0.25 for m, v in d.items() if m != 'labels'}          # no labels at all
    inside = {m: v for m, v in d.items() if m != 'labels'}
    fpr, tpr, auroc, _ = k['fused'].out_of_distribution_detection_score(inside, 'entropy', foreign)
    assert 0.0 <= auroc <= 1.0 and fpr[-1] == 1.0 and tpr[-1] == 1.0
    t = k['fused'].uncertainty_tables(foreign, fixed_row=1)
    assert int(t['hist'][0][1].sum()) == d['labels'].size and not t['hist'][:, 0].any() and not t['counts'].any()


@pytest.mark.parametrize('kind,mods', [CASES[0], CASES[3], CASES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_temperature_search_is_separate_passes(gpu, weights, data, kind, mods):
    k = _scored(weights, data, kind, mods)
    net, d = k['fused'], k['data']
    search = net.temperature_search(d, [1.0, 0.5])
    assert [s['temperature'] for s in search] == [1.0, 0.5]
    for s in search:
        alone = net.uncertainty_tables(d, temperature=s['temperature'])
        assert np.array_equal(s['tables']['hist'], alone['hist']) and np.array_equal(s['class_counts'], alone['counts'])
        assert np.allclose(s['tables']['nll_sum'], alone['nll_sum'], rtol=1e-12, atol=0)     # (double atomics: the order)
        assert sorted(s['auroc']) == sorted(METRICS)
    assert not np.array_equal(search[0]['tables']['hist'][0], search[1]['tables']['hist'][0])
    # the default temperature: temperature_scaling where it is set, else the fitted one, else 1
    try:
        net.config['temperature'] = 0.5
        assert np.array_equal(net.uncertainty_tables(d)['hist'], search[1]['tables']['hist'])
        net.config['temperature_scaling'] = 1.0
        assert np.array_equal(net.uncertainty_tables(d)['hist'], search[0]['tables']['hist'])
    finally:
        net.config.pop('temperature', None), net.config.pop('temperature_scaling', None)    # (the model is shared)


def test_a_single_fcn_and_the_experts_own_tables(gpu, weights, data, capsys):
    from modular_semantic_segmentation_amd import experiments, get_model
    k = _scored(weights, data, *CASES[0])
    fused = k['fused'].uncertainty_tables(k['data'], experts=True)
    for m in TWO:
        net = get_model('fcn')(m, _desc((m,)), m, num_units=U, batch_normalization=False, batchsize=2)
        net.import_weights(weights[m], warnings=False)
        d = _only(data, (m,))
        assert net.uncertainty_metrics == METRICS
        got = net.uncertainty_tables(d)
        maps = net.predict_confidence(d, outputs=('confidence', 'entropy', 'margin'))
        want = confidence_tables_reference(maps, maps['label'], d['labels'], num_classes=C)
        assert np.array_equal(got['hist'], want['hist']) and np.array_equal(got['counts'], want['counts'])
        moved = int(np.abs(got['hist'] - fused['experts'][m]['hist']).sum()) // 2
        print('%s: %d counts differ between the expert table of the fused head and the single model' % (m, moved))
        assert np.array_equal(got['hist'], fused['experts'][m]['hist'])
        assert net.misclassification_detection_score(d, 'small_margin')[2] == roc_from_histogram(got['hist'][2], got['edges'])[2]
        r = experiments.evaluate_uncertainty(net, d, 'entropy', print_results=False)
        assert r['AUROC'] == roc_from_histogram(got['hist'][0], got['edges'])[2]
        assert sorted(experiments.measure_metrics(net, d, ['entropy'])) == ['class_counts', 'entropy', 'nll']
        with pytest.raises(ValueError, match='experts'):
            net.uncertainty_tables(d, experts=True)
    capsys.readouterr()
    rows = experiments.evaluate_fusion_uncertainty(k['fused'], k['data'], ood_set=k['data'])
    lines = capsys.readouterr().out.splitlines()
    assert list(rows) == list(k['fused'].modalities) + ['fusion'] and len(lines) == 3 and lines[-1].lstrip().startswith('fusion')
    for i, metric in enumerate(METRICS):
        assert rows['fusion']['misclassification'][metric] == roc_from_histogram(fused['hist'][i], fused['edges'])[2]
    # (two passes: the double atomics add in another order)
    assert abs(rows['fusion']['nll'] - fused['nll_sum'].sum() / fused['counts'].sum()) <= 1e-12 * rows['fusion']['nll']
    assert all(0.0 <= rows[m]['out_of_distribution'][metric] <= 1.0 for m in rows for metric in METRICS)


def test_models_without_class_scores_refuse(gpu, weights, data):
    from modular_semantic_segmentation_amd import get_model
    d = _only(data, TWO)
    cfg = dict(num_units=U, num_channels={m: CHANNELS[m] for m in TWO}, expert_model='fcn', batchsize=2,
               prefixes={m: m for m in TWO})
    nets = [_model(weights, 'bayes_fusion', TWO, decision_matrix=True),
            get_model('variance_fusion')(data_description=_desc(TWO), dropout_rate=0.5, num_samples=3, **cfg),
            get_model('uncertainty_mix')(data_description=_desc(TWO), class_prior='uniform', delta=1e-2, beta=1e-2,
                                         dropout_rate=0.5, num_samples=3, modalities=list(TWO),
                                         **{k: v for k, v in cfg.items() if k != 'prefixes'}),
            get_model('ibcc_fusion')(data_description=_desc(TWO), **dict(cfg, **_tables('bayes_fusion', TWO)))]
    for net in nets:
        reason = net._calibration_refusal()
        assert reason
        for call in (lambda: net.uncertainty_tables(d), lambda: net.misclassification_detection_score(d, 'entropy'),
                     lambda: net.out_of_distribution_detection_score(d, 'entropy', d), lambda: net.nll_score(d),
                     lambda: net.value_distribution(d, 'entropy'), lambda: net.temperature_search(d, [1.0])):
            with pytest.raises(NotImplementedError) as info:
                call()
            assert reason in str(info.value)
    from modular_semantic_segmentation_amd.bayesian_fcn import BayesianFCN
    assert BayesianFCN.uncertainty_metrics == ops.UNCERTAINTY_METRICS and int(bin_index(np.float32([1.0]))[0]) == 23 * 32
