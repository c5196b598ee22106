"""The evaluation flows with three and four FCN experts: score_grid of dirichlet_fusion and bayes_fusion and FusionComparison's
score_all / score_all_groups count through ops.fused_head_multi_count (one launch per batch and fusion, no expert output
materialised) and give the integers of the same model with fused_head=False and of score() of a model built per grid point.
Fixtures as tests/test_multi_head_models_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo

U = 64
H, W = 64, 96
CHANNELS = {'rgb': 3, 'depth': 1, 'ir': 1, 'gray': 1}
FIRST_SCALE = {'rgb': 0.02, 'depth': 2e-4, 'ir': 2e-4, 'gray': 0.02}       # conv1_1 against inputs up to 255 / 65 535
THREE, FOUR = ('rgb', 'depth', 'ir'), ('rgb', 'depth', 'ir', 'gray')
KINDS = ('bayes_fusion', 'dirichlet_fusion', 'average_fusion')


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _desc(mods, c):
    return (dict({m: 'float32' for m in mods}, labels='int32'),
            dict({m: (None, None, CHANNELS[m]) for m in mods}, labels=(None, None)), c)


def _data(n, c, seed):
    rng = np.random.default_rng(seed)
    d = {m: rng.integers(0, 256 if FIRST_SCALE[m] > 1e-3 else 65536, (n, H, W, CHANNELS[m])).astype(np.float32) for m in FOUR}
    d['labels'] = rng.integers(-1, c, (n, H, W)).astype(np.int32)
    return d


@pytest.fixture(scope='module')
def weights(gpu, tmp_path_factory):
    """{(modality, classes): npz path} of random weights by seed, scaled so that the experts disagree"""
    tmp = tmp_path_factory.mktemp('multi_count')
    paths = {}
    for c in (12, 5):
        for i, m in enumerate(FOUR):
            w = fo.init_fcn_weights(m, CHANNELS[m], U, c, seed=11 + i, bias_scale=0.02)
            w['%s/conv1_1/kernel' % m] *= FIRST_SCALE[m]
            for k in w:
                if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
                    w[k] *= 1.6
            paths[(m, c)] = os.path.join(str(tmp), '%s_%d.npz' % (m, c))
            np.savez(paths[(m, c)], **w)
    return paths


def _tables(kind, mods, c):
    """confusion matrices / Dirichlet parameters handed in by config"""
    rng = np.random.default_rng(5 * c + len(mods))
    if kind == 'bayes_fusion':
        return dict(confusion_matrices={m: rng.integers(1, 50, (c, c)) + 400 * np.eye(c, dtype=np.int64) for m in mods})
    if kind == 'dirichlet_fusion':
        params = {m: rng.uniform(0.5, 2.0, (c, c)) + 4.0 * np.eye(c) for m in mods}
        params['class_counts'] = rng.integers(100, 1000, c).astype(np.float64)
        return dict(dirichlet_params=params, sigma=1.0, delta=1e-2, beta=1e-2)
    return {}


def _model(weights, kind, mods, c, batchsize=2, tables=None, **config):
    from modular_semantic_segmentation_amd import get_model
    named = dict(modalities=list(mods)) if kind == 'dirichlet_fusion' else dict(prefixes={m: m for m in mods})
    cfg = dict(num_units=U, num_channels={m: CHANNELS[m] for m in mods}, expert_model='fcn', batchsize=batchsize,
               class_prior='data')
    cfg.update(_tables(kind, mods, c) if tables is None else tables)
    cfg.update(named)
    cfg.update(config)
    net = get_model(kind)(data_description=_desc(mods, c), **cfg)
    for m in mods:
        net.import_weights(weights[(m, c)], warnings=False)
    return net


def _only(data, mods, rows=None):
    return {k: (v if rows is None else v[rows]) for k, v in data.items() if k in mods or k == 'labels'}


def _spies(monkeypatch):
    from modular_semantic_segmentation_amd import basic_fusion_model, bayes_mix, dirichlet_mix, fusion_comparison, ops
    calls = {'count': 0, 'experts': 0}
    real_count, real_experts = ops.fused_head_multi_count, basic_fusion_model.run_experts

    def count(*a, **k):
        calls['count'] += 1
        return real_count(*a, **k)

    def experts(*a, **k):
        calls['experts'] += 1
        return real_experts(*a, **k)
    monkeypatch.setattr(ops, 'fused_head_multi_count', count)
    for mod in (basic_fusion_model, bayes_mix, dirichlet_mix, fusion_comparison):
        if hasattr(mod, 'run_experts'):
            monkeypatch.setattr(mod, 'run_experts', experts)
    return calls


GRIDS = {'dirichlet_fusion': {'sigma': [0.5, 1.0], 'class_prior': ['data', 'uniform']},
         'bayes_fusion': {'class_prior': ['data', 'uniform', 0.5]}}
GRID_CASES = [('dirichlet_fusion', THREE, 12, 2), ('dirichlet_fusion', THREE, 5, 3), ('dirichlet_fusion', FOUR, 12, 2),
              ('bayes_fusion', THREE, 12, 2), ('bayes_fusion', THREE, 5, 3)]


@pytest.mark.parametrize('kind,mods,c,n', GRID_CASES, ids=['%s-e%d-c%d' % (k, len(m), c) for k, m, c, n in GRID_CASES])
def test_score_grid_counts_in_one_launch_per_batch(weights, monkeypatch, kind, mods, c, n):
    test = _only(_data(n, c, seed=60 + c), mods)
    fused = _model(weights, kind, mods, c, batchsize=1)
    calls = _spies(monkeypatch)
    got = fused.score_grid(test, GRIDS[kind])
    assert calls == {'count': n, 'experts': 0}                               # one call per batch, no expert materialised
    unfused = _model(weights, kind, mods, c, batchsize=1, fused_head=False).score_grid(test, GRIDS[kind])
    assert calls['count'] == n and calls['experts'] == n
    assert len(got) == len(unfused) == int(np.prod([len(v) for v in GRIDS[kind].values()]))
    for (config, measures, cm), (config_u, measures_u, cm_u) in zip(got, unfused):
        assert np.array_equal(cm, cm_u) and cm.sum() == (test['labels'] >= 0).sum()
        point = {k: config[k] for k in GRIDS[kind]}
        assert point == {k: config_u[k] for k in GRIDS[kind]}
        single = _model(weights, kind, mods, c, batchsize=n, **point).score(test)[1]
        assert np.array_equal(cm, single), point
    if kind == 'dirichlet_fusion':                                           # (sigma moves labels; these priors need not)
        assert any(not np.array_equal(got[0][2], g[2]) for g in got[1:])


def test_bayes_decision_matrix_keeps_the_generic_route(weights, monkeypatch):
    test = _only(_data(2, 12, seed=71), THREE)
    net = _model(weights, 'bayes_fusion', THREE, 12, batchsize=2, decision_matrix=True)
    calls = _spies(monkeypatch)
    net.score_grid(test, GRIDS['bayes_fusion'])
    assert calls == {'count': 0, 'experts': 1}


def test_two_expert_models_keep_their_heads(weights, monkeypatch):
    two = ('rgb', 'depth')
    test = _only(_data(2, 12, seed=72), two)
    calls = _spies(monkeypatch)
    for kind in GRIDS:
        _model(weights, kind, two, 12, batchsize=2).score_grid(test, GRIDS[kind])
    assert calls == {'count': 0, 'experts': 0}


def _comparison(weights, mods, c, batchsize, **config):
    from modular_semantic_segmentation_amd.fusion_comparison import FusionComparison
    cfg = dict(num_units=U, num_channels={m: CHANNELS[m] for m in mods}, expert_model='fcn', batchsize=batchsize,
               class_prior='data', sigma=1.0, delta=1e-2, beta=1e-2, prefixes={m: m for m in mods})
    cfg.update(config)
    net = FusionComparison(data_description=_desc(mods, c), **cfg)
    for m in mods:
        net.import_weights(weights[(m, c)], warnings=False)
    return net


def test_comparison_with_three_experts(weights, monkeypatch):
    c, n = 12, 3
    fit, test = _only(_data(2, c, seed=80), THREE), _only(_data(n, c, seed=81), THREE)
    net = _comparison(weights, THREE, c, batchsize=1)
    fitted = net.fit(fit)
    calls = _spies(monkeypatch)
    rows = net.score_all(test)
    assert calls == {'count': 3 * n, 'experts': 0}
    generic = _comparison(weights, THREE, c, batchsize=1, fused_head=False)
    generic.fit(fit)
    other = generic.score_all(test)
    assert list(rows) == list(other) == list(THREE) + ['bayes_fusion', 'dirichlet_fusion', 'average_fusion']
    for name in rows:
        assert np.array_equal(rows[name][1], other[name][1]), name
        assert rows[name][1].sum() == (test['labels'] >= 0).sum()
    # score() of the separately built models, from fit()'s return value: the independent reference
    from modular_semantic_segmentation_amd import get_model
    measurements = fitted
    singles = {}
    for m in THREE:
        expert = get_model('fcn')(m, _desc(THREE, c), m, num_units=U, batch_normalization=False, batchsize=1)
        expert.import_weights(weights[(m, c)], warnings=False)
        singles[m] = expert.score(test)[1]
    singles['bayes_fusion'] = _model(weights, 'bayes_fusion', THREE, c, batchsize=1,
                                     tables=dict(confusion_matrices=measurements['confusion_matrices'])).score(test)[1]
    singles['dirichlet_fusion'] = _model(weights, 'dirichlet_fusion', THREE, c, batchsize=1, tables=dict(
        dirichlet_params=measurements['dirichlet_params'], sigma=1.0, delta=1e-2, beta=1e-2)).score(test)[1]
    singles['average_fusion'] = _model(weights, 'average_fusion', THREE, c, batchsize=1).score(test)[1]
    for name in rows:
        assert np.array_equal(rows[name][1], singles[name]), name
    mats = [rows[name][1] for name in rows]
    assert all(not np.array_equal(mats[i], mats[j]) for i in range(len(mats)) for j in range(i))     # six different rows
    per_image = net.score_all_groups(test, 'image')
    assert len(per_image) == n
    for i, key in enumerate(per_image):
        alone = net.score_all(_only(test, THREE, rows=[i]))
        for name in rows:
            assert np.array_equal(per_image[key][name][1], alone[name][1]), (key, name)


def test_three_modalities_flow_through_the_experiments(weights, monkeypatch):
    """experiments.grid_search_fusion and fit_and_evaluate_all_fusions take a three-modality config onto the counting head"""
    from modular_semantic_segmentation_amd.experiments import fit_and_evaluate_all_fusions, grid_search_fusion
    c, n = 12, 2
    fit, test = _only(_data(2, c, seed=90), THREE), _only(_data(n, c, seed=91), THREE)
    calls = _spies(monkeypatch)
    net = _model(weights, 'dirichlet_fusion', THREE, c, batchsize=n)
    grid = grid_search_fusion(net, test, GRIDS['dirichlet_fusion'])
    assert calls == {'count': 1, 'experts': 0}
    assert grid['sigma'] == [0.5, 0.5, 1.0, 1.0] and len(grid['mean_IoU']) == 4
    wanted = [r[1]['mean_IoU'] for r in net.score_grid(test, GRIDS['dirichlet_fusion'])]
    assert grid['mean_IoU'] == wanted
    config = dict(num_units=U, num_channels={m: CHANNELS[m] for m in THREE}, expert_model='fcn', batchsize=n, class_prior='data',
                  sigma=1.0, delta=1e-2, beta=1e-2, prefixes={m: m for m in THREE})
    before = dict(calls)
    info = fit_and_evaluate_all_fusions(config, _desc(THREE, c), fit, test, {m: weights[(m, c)] for m in THREE})
    assert calls['count'] == before['count'] + 3                              # score_all: three launches for the one batch
    assert list(info['confusion_matrix']) == list(THREE) + ['bayes_fusion', 'dirichlet_fusion', 'average_fusion']
    reference = _comparison(weights, THREE, c, batchsize=n, fused_head=False)
    reference.fit(fit)
    for name, (_, cm) in reference.score_all(test).items():
        assert np.array_equal(info['confusion_matrix'][name], cm), name
