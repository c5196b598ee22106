"""Uncertainty benchmarks without a GPU (uncertainty_model.py): the bit-pattern histogram bins, the ROC from two histogram rows
against the exact rank statistic, and the model's host logic.

The tie bound: binning is monotone in the value, so a (positive, negative) pair whose members fall into different bins is
ordered by the bins as by the values; only pairs that share a bin can differ, each by at most one half of 1 / (P N) (the
histogram gives it one half; the truth is 0, one half or 1): |auroc_binned - auroc_exact| <= 0.5 sum_b pos_b neg_b / (P N)."""
import numpy as np
import pytest

from modular_semantic_segmentation_amd import uncertainty_model as um

SHAPES = [(5, 24), (3, 8), (8, 32), (4, 16)]           # (mantissa_bits, octaves): the default and the corners


# ---- bins ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('m,o', SHAPES)
def test_bin_index_agrees_with_bin_edges(m, o):
    bins = o << m
    edges = um.bin_edges(m, o)
    assert edges.shape == (bins + 1,) and edges[0] == 0 and np.isinf(edges[-1])
    assert (np.diff(edges) > 0).all()
    assert edges[1] == 2.0 ** (1 - o) * (1 + 2.0 ** -m)             # bin 0 ends one step above 2^(1 - octaves)
    assert edges[bins - 1] == 2 - 2.0 ** -m                          # the top bin starts one step below 2
    inner = edges[1:-1].astype(np.float32)
    assert np.array_equal(inner.astype(np.float64), edges[1:-1])    # every edge is a float32
    b = np.arange(1, bins)
    assert np.array_equal(um.bin_index(inner, m, o), b)                                     # an edge opens its bin
    assert np.array_equal(um.bin_index(np.nextafter(inner, np.float32(0)), m, o), b - 1)    # the float below closes the one before
    assert np.array_equal(um.bin_index(np.nextafter(inner, np.float32(4)), m, o), b)
    # monotone on a sorted sample over every binade, denormals and values past 2 included
    rng = np.random.default_rng(m * 100 + o)
    v = np.sort(np.concatenate([np.exp(rng.uniform(np.log(1e-45), np.log(8.0), 20000)), rng.uniform(0, 2, 20000)]).astype(np.float32))
    k = um.bin_index(v, m, o)
    assert (np.diff(k) >= 0).all() and k.min() == 0 and k.max() == bins - 1
    assert ((edges[k] <= v) & (v < edges[k + 1])).all()
    special = np.array([0.0, -0.0, -1.0, -np.inf, -1e-30, 1e-45, 2.0, 3.5, np.inf, np.nan, -np.nan], np.float32)
    assert um.bin_index(special, m, o).tolist() == [0, 0, 0, 0, 0, 0] + [bins - 1] * 5
    assert um.bin_index(np.zeros((2, 3), np.float32), m, o).shape == (2, 3)


def test_bin_shape_is_checked():
    for m, o in [(2, 24), (9, 24), (5, 7), (5, 33)]:
        with pytest.raises(ValueError):
            um.bin_edges(m, o)
        with pytest.raises(ValueError):
            um.bin_index(np.ones(1, np.float32), m, o)


# ---- ROC ------------------------------------------------------------------------------------------------------------------------

def exact_auroc(neg, pos):
    """P(pos > neg) + 0.5 P(pos == neg) from average ranks, in float64 (Mann-Whitney)"""
    allv = np.concatenate([neg, pos]).astype(np.float64)
    _, inv, cnt = np.unique(allv, return_inverse=True, return_counts=True)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rank = (start + (cnt + 1) / 2.0)[inv]                           # average 1-based rank
    n, p = len(neg), len(pos)
    return (rank[n:].sum() - p * (p + 1) / 2.0) / (n * float(p))


def test_roc_exact_cases():
    sep = np.zeros((2, 64), np.int64)
    sep[0, 3:20] = np.arange(17) + 1
    sep[1, 20:40] = np.arange(20) + 2
    fpr, tpr, auroc, thr = um.roc_from_histogram(sep)
    assert auroc == 1.0
    assert fpr.shape == tpr.shape == thr.shape == (65,)
    assert fpr[0] == 0 and tpr[0] == 0 and fpr[-1] == 1 and tpr[-1] == 1 and np.isinf(thr[0])
    assert (np.diff(fpr) >= 0).all() and (np.diff(tpr) >= 0).all() and (np.diff(thr) < 0).all()
    assert um.auroc_tie_bound(sep) == 0.0
    assert um.roc_from_histogram(sep[::-1])[2] == 0.0
    rng = np.random.default_rng(1)
    row = rng.integers(0, 1000, 64)
    same = np.stack([row, row])
    assert um.roc_from_histogram(same)[2] == 0.5
    assert um.roc_from_histogram(np.stack([row, 7 * row]))[2] == 0.5
    h = rng.integers(0, 1000, (2, 64))
    a, b = um.roc_from_histogram(h)[2], um.roc_from_histogram(h[::-1])[2]
    assert abs(b - (1 - a)) <= 2.0 ** -52
    assert np.isnan(um.roc_from_histogram(np.stack([row, 0 * row]))[2])
    big = np.full((2, 8), 3_000_000_000, np.int64)                  # products of counts beyond 2^63
    assert um.roc_from_histogram(big)[2] == 0.5
    # thresholds are the bins' lower edges
    e = um.bin_edges()
    thr = um.roc_from_histogram(np.ones((2, 768), np.int64), e)[3]
    assert np.array_equal(thr[1:], e[:-1][::-1])


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
@pytest.mark.parametrize('m,o', [(5, 24), (3, 8)])
def test_binned_auroc_is_within_the_tie_bound_of_the_rank_statistic(seed, m, o):
    rng = np.random.default_rng(seed)
    n, p = 30000, 4000 + 3000 * seed
    neg = (rng.beta(1.2, 6 + seed, n) * rng.choice([1.0, 1e-3, 1e-6], n)).astype(np.float32)     # several binades, like a variance
    pos = (rng.beta(2.0, 3.0, p) * rng.choice([1.0, 1e-3], p)).astype(np.float32)
    neg[:50] = 0                                                    # exact ties across the rows
    pos[:50] = 0
    hist = np.zeros((2, o << m), np.int64)
    np.add.at(hist[0], um.bin_index(neg, m, o), 1)
    np.add.at(hist[1], um.bin_index(pos, m, o), 1)
    auroc = um.roc_from_histogram(hist, um.bin_edges(m, o))[2]
    exact = exact_auroc(neg, pos)
    bound = um.auroc_tie_bound(hist)
    print('seed %d M=%d octaves=%d: binned %.6f exact %.6f |diff| %.3g bound %.3g' % (seed, m, o, auroc, exact, abs(auroc - exact), bound))
    assert 0.55 < exact < 0.999 and 0 < bound < 0.25              # the inputs are neither separable nor noise
    assert abs(auroc - exact) <= bound + 1e-12                      # (1e-12: the float64 rounding of the rank sum)


# ---- model host logic ---------------------------------------------------------------------------------------------------------

def _hostonly_model(**config):
    """A BayesianFCN without its engine (no device): what the host-side checks need"""
    from modular_semantic_segmentation_amd.bayesian_fcn import BayesianFCN
    net = BayesianFCN.__new__(BayesianFCN)
    net.config = dict({'num_classes': 12, 'batchsize': 1, 'num_samples': 4, 'dropout_rate': 0.5}, **config)
    net.modality = 'rgb'
    return net


def test_model_host_logic():
    from modular_semantic_segmentation_amd import get_model
    from modular_semantic_segmentation_amd.bayesian_fcn import BayesianFCN
    from modular_semantic_segmentation_amd.simple_fcn import SimpleFCN
    assert get_model('bayesian_fcn') is BayesianFCN
    assert issubclass(BayesianFCN, um.UncertaintyModel) and issubclass(BayesianFCN, SimpleFCN)
    assert BayesianFCN.uncertainty_metrics == ('entropy', 'cond_entropy', 'variance')
    for name in ('misclassification_detection_score', 'out_of_distribution_detection_score', 'nll_score', 'value_distribution',
                 'uncertainty_tables', 'temperature_search'):
        assert callable(getattr(BayesianFCN, name)), name
    batch = {'rgb': np.zeros((1, 64, 96, 3), np.float32)}
    hot = _hostonly_model(temperature_scaling=1.7)
    assert hot._temperature() == 1.7 and hot._temperature(2) == 2.0
    with pytest.raises(NotImplementedError, match='temperature_scaling'):
        hot._predict_batch_impl(batch)
    with pytest.raises(NotImplementedError, match='temperature_scaling'):
        hot.predict_uncertainty(batch)
    plain = _hostonly_model()
    assert plain._temperature() == 1.0 and plain._uncertainty_bins() == (5, 24)
    with pytest.raises(ValueError):
        plain._temperature(0)
    for call in (lambda: plain.misclassification_detection_score(batch, 'std'),
                 lambda: plain.out_of_distribution_detection_score(batch, 'std', batch),
                 lambda: plain.value_distribution(batch, 'mean')):
        with pytest.raises(UserWarning):
            call()
    # a model with maps but no temperature refuses one instead of ignoring it
    with pytest.raises(NotImplementedError):
        um.UncertaintyModel._uncertainty_accumulate(plain, {}, None, {}, 1.7, -1)


def test_experiment_flows_call_the_model():
    from modular_semantic_segmentation_amd import experiments

    class Net(object):
        name = 'net'

        def misclassification_detection_score(self, data, metric):
            return np.array([0, 1.0]), np.array([0, 1.0]), 0.75, np.array([np.inf, 0])

        def out_of_distribution_detection_score(self, data, metric, ood_data):
            return np.array([0, 1.0]), np.array([0, 1.0]), 0.25, np.array([np.inf, 0])

        def nll_score(self, data):
            return np.ones(3), np.arange(3)

        def value_distribution(self, data, metric):
            return np.arange(4), np.arange(5.0)
    r = experiments.evaluate_uncertainty(Net(), {}, 'entropy', print_results=False)
    assert sorted(r) == ['AUROC', 'FPR', 'TPR', 'thresholds'] and r['AUROC'] == 0.75
    assert experiments.evaluate_uncertainty(Net(), {}, 'entropy', 'out_of_distribution', False, ood_data={})['AUROC'] == 0.25
    with pytest.raises(ValueError):
        experiments.evaluate_uncertainty(Net(), {}, 'entropy', 'out_of_distribution', False)
    m = experiments.measure_metrics(Net(), {}, ['entropy', 'variance'])
    assert sorted(m) == ['class_counts', 'entropy', 'nll', 'variance']
