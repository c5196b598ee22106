"""Grid search over the fusion parameters (experiments/different_evaluation_parameters.py): the host-side flows on hand-written
expectations, and the capacity query of the grid-scoring head."""
import numpy as np
import pytest


def test_parameter_combinations_order_and_copies():
    from modular_semantic_segmentation_amd.experiments import parameter_combinations
    base = {'sigma': 1.0, 'class_prior': 'data', 'prefixes': {'rgb': 'rgb'}}
    combos = parameter_combinations({'sigma': [0.5, 2.0], 'class_prior': ['data', 'uniform', 0.3]}, base)
    # the first key varies slowest
    assert [(c['sigma'], c['class_prior']) for c in combos] == [(0.5, 'data'), (0.5, 'uniform'), (0.5, 0.3),
                                                                (2.0, 'data'), (2.0, 'uniform'), (2.0, 0.3)]
    assert all(c['prefixes'] == {'rgb': 'rgb'} and c['prefixes'] is not base['prefixes'] for c in combos)
    assert base == {'sigma': 1.0, 'class_prior': 'data', 'prefixes': {'rgb': 'rgb'}}
    swapped = parameter_combinations({'class_prior': ['data', 'uniform'], 'sigma': [0.5, 2.0]}, base)
    assert [(c['class_prior'], c['sigma']) for c in swapped] == [('data', 0.5), ('data', 2.0), ('uniform', 0.5), ('uniform', 2.0)]
    assert parameter_combinations({}, base) == [base]
    # a key the base config lacks is added
    assert [c['delta'] for c in parameter_combinations({'delta': [1, 2]}, {})] == [1, 2]


def test_grid_search_merges_results_into_lists():
    from modular_semantic_segmentation_amd.experiments import grid_search
    seen = []

    def evaluation(config):
        seen.append(dict(config))
        return {'accuracy': config['a'] * 10 + config['b'], 'per_class': {'iou': config['a'], 'deep': {'f1': config['b']}}}

    got = grid_search(evaluation, {'a': [1, 2], 'b': [3, 4, 5]}, {'a': 0, 'fixed': {'x': 1}})
    assert got == {
        'a': [1, 1, 1, 2, 2, 2],
        'b': [3, 4, 5, 3, 4, 5],
        'fixed': [{'x': 1}] * 6,                    # a config value stays one entry per grid point, a dict too
        'accuracy': [13, 14, 15, 23, 24, 25],
        'per_class': {'iou': [1, 1, 1, 2, 2, 2], 'deep': {'f1': [3, 4, 5, 3, 4, 5]}},
    }
    assert [(c['a'], c['b']) for c in seen] == [(1, 3), (1, 4), (1, 5), (2, 3), (2, 4), (2, 5)]


def test_grid_search_fusion_has_the_shape_of_grid_search():
    from modular_semantic_segmentation_amd.base_model import score_measures
    from modular_semantic_segmentation_amd.experiments import grid_search_fusion

    class Net(object):
        def score_grid(self, data, search_parameters):
            assert data == 'testset' and search_parameters == {'sigma': [1, 2]}
            cms = [np.array([[1., 0.], [1., 2.]]), np.array([[1., 0.], [0., 3.]])]
            return [({'sigma': s, 'batchsize': 2}, score_measures(cm), cm) for s, cm in zip([1, 2], cms)]

    got = grid_search_fusion(Net(), 'testset', {'sigma': [1, 2]})
    assert got['sigma'] == [1, 2] and got['batchsize'] == [2, 2]
    assert got['total_accuracy'] == [2. / 3, 1.0] and len(got['confusion_matrix']) == 2 and len(got['IoU']) == 2


def test_bayes_host_decision_and_confusion_from_joint_hist():
    from modular_semantic_segmentation_amd.bayes_mix import confusion_from_joint_hist, fused_decision_table
    rng = np.random.default_rng(0)
    C = 4
    loglik, logprior = rng.standard_normal((2, C, C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    loglik[0, 1] = loglik[0, 2]                     # equal rows: equal decisions
    dec = fused_decision_table(loglik, logprior)
    for a in range(C):
        for b in range(C):
            v = [np.float32(np.float32(loglik[0, a, k] + loglik[1, b, k]) + logprior[k]) for k in range(C)]
            assert dec[a, b] == int(np.argmax(v))
    assert np.array_equal(dec[1], dec[2])
    hist = rng.integers(0, 50, (C, C, C))
    cm = confusion_from_joint_hist(hist, dec)
    ref = np.zeros((C, C), np.int64)
    for l in range(C):
        for a in range(C):
            for b in range(C):
                ref[l, dec[a, b]] += hist[l, a, b]
    assert np.array_equal(cm, ref) and cm.sum() == hist.sum()


def test_grid_capacity():
    """No GPU call: the capacity is LDS arithmetic on the host."""
    from modular_semantic_segmentation_amd import _lib
    lib = _lib.lib()
    cap = [lib.xv_fused_head_grid_capacity(c) for c in range(2, 33)]
    assert lib.xv_fused_head_grid_capacity(12) >= 16 and lib.xv_fused_head_grid_capacity(32) >= 1
    assert all(a >= b for a, b in zip(cap, cap[1:])), cap
    assert lib.xv_fused_head_grid_capacity(1) == 0 and lib.xv_fused_head_grid_capacity(33) == 0
