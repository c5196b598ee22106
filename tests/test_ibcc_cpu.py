"""The host side of the IBCC fusion (modular_semantic_segmentation_amd/ibcc.py, experiments.collect_predictions), without a
GPU: the variational solver on the tuple histogram against a per-pixel twin written here straight from the update equations,
its properties, the priors, a domain-shift case in which adapting has to pay, and the host interfaces."""
import os

import numpy as np
import pytest
from scipy.special import psi

from modular_semantic_segmentation_amd import ibcc


# ---- the per-pixel twin: the equations of ibcc.py's docstring over the expanded pixel list, no histogram anywhere -----------
def twin_vb_ibcc(labels, alpha0, nu0, iterations):
    """labels int [P, E].  Returns (alpha, nu, q [P, C]) after `iterations` updates from the priors, q under the final
    Dirichlets."""
    alpha0, nu0 = np.asarray(alpha0, np.float64), np.asarray(nu0, np.float64)
    E, C = alpha0.shape[:2]
    alpha, nu = alpha0.copy(), nu0.copy()

    def responsibilities():
        lnrho = np.tile(psi(nu) - psi(nu.sum()), (len(labels), 1))
        for e in range(E):
            elnpi = psi(alpha[e]) - psi(alpha[e].sum(1, keepdims=True))
            lnrho += elnpi[:, labels[:, e]].T
        lnrho -= lnrho.max(1, keepdims=True)
        q = np.exp(lnrho)
        return q / q.sum(1, keepdims=True)

    for _ in range(iterations):
        q = responsibilities()
        nu = nu0 + q.sum(0)
        alpha = alpha0.copy()
        for e in range(E):
            for j in range(C):
                np.add.at(alpha[e, j], labels[:, e], q[:, j])
    return alpha, nu, responsibilities()


def draw_answers(rng, truth, matrix):
    """one expert's answers to `truth` from its confusion matrix (rows = true class, each a distribution over answers)"""
    cdf = np.cumsum(matrix, 1)
    return (rng.random(len(truth))[:, None] > cdf[truth]).sum(1).clip(0, len(matrix) - 1)


def soft_identity(C, diag):
    return np.full((C, C), (1.0 - diag) / (C - 1)) + (diag - (1.0 - diag) / (C - 1)) * np.eye(C)


def _random_case(seed, C, E, P):
    rng = np.random.default_rng(seed)
    truth = rng.choice(C, P, p=rng.dirichlet(np.full(C, 3.0)))
    mats = [0.5 * soft_identity(C, 0.7) + 0.5 * rng.dirichlet(np.full(C, 1.0), C) for _ in range(E)]
    labels = np.stack([draw_answers(rng, truth, m) for m in mats], 1)
    alpha0 = 1.0 + rng.random((E, C, C)) * 2 + 4.0 * np.eye(C)
    nu0 = 1.0 + rng.random(C) * 3
    return truth, labels, alpha0, nu0


def _relative(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def test_histogram_solver_equals_the_per_pixel_twin():
    """C = 4, E = 3, 2 000 seeded pixels, 30 iterations from the priors (tol = 0: none ends early).  The two differ only in
    summation order -- the histogram multiplies a tuple's responsibility by its count where the twin adds it once per pixel.
    Largest relative difference measured where this was written: posterior 9.7e-14, alpha 5.2e-14, nu 3.1e-14 (float64;
    thirty iterations carry the rounding of each into the next).  The bound is ten times the largest, and never above 1e-8."""
    C, E, P, iterations = 4, 3, 2000, 30
    _, labels, alpha0, nu0 = _random_case(3, C, E, P)
    t = ibcc.tuple_index(labels.T, C)
    hist = np.bincount(t, minlength=C ** E)
    got = ibcc.vb_ibcc(hist, alpha0, nu0, max_iter=iterations, tol=0.0)
    alpha, nu, q = twin_vb_ibcc(labels, alpha0, nu0, iterations)
    assert got.iterations == iterations and len(got.lower_bounds) == iterations and not got.converged
    diff_posterior, diff_alpha = _relative(got.posterior[t], q), _relative(got.alpha, alpha)
    print('relative difference: posterior %.3g, alpha %.3g, nu %.3g' % (diff_posterior, diff_alpha, _relative(got.nu, nu)))
    bound = 10 * 9.7e-14
    assert bound <= 1e-8
    assert diff_posterior <= bound and diff_alpha <= bound and _relative(got.nu, nu) <= bound
    assert np.array_equal(got.lut[t], np.argmax(q, 1))
    assert got.lut.dtype == np.uint8 and got.lut.shape == (C ** E,) and got.posterior.shape == (C ** E, C)
    assert got.alpha.shape == (E, C, C) and got.nu.shape == (C,)
    # the updates conserve the pixels: every one is handed out once per expert, and once to the class proportions
    assert np.allclose(got.nu.sum() - nu0.sum(), P, rtol=1e-12)
    assert np.allclose(got.alpha.sum((1, 2)) - alpha0.sum((1, 2)), P, rtol=1e-12)


@pytest.mark.parametrize('seed,C,E', [(0, 4, 3), (1, 3, 2), (2, 5, 4), (3, 12, 2)])
def test_lower_bound_never_decreases(seed, C, E):
    _, labels, alpha0, nu0 = _random_case(seed, C, E, 3000)
    hist = np.bincount(ibcc.tuple_index(labels.T, C), minlength=C ** E)
    got = ibcc.vb_ibcc(hist, alpha0, nu0, max_iter=60, tol=1e-9)
    lb = got.lower_bounds
    assert len(lb) == got.iterations >= 2 and np.all(np.isfinite(lb))
    assert np.all(np.diff(lb) >= -1e-9 * np.abs(lb[:-1])), np.diff(lb).min()
    assert lb[-1] > lb[0]
    # ending early: a loose tolerance is reached, reported, and its bounds are the first ones of the longer run
    loose = ibcc.vb_ibcc(hist, alpha0, nu0, max_iter=60, tol=0.5)
    assert loose.converged and loose.iterations < 60 and np.array_equal(loose.lower_bounds, lb[:loose.iterations])


def test_no_data_returns_the_priors():
    C, E = 4, 3
    _, _, alpha0, nu0 = _random_case(5, C, E, 10)
    got = ibcc.vb_ibcc(np.zeros(C ** E, np.int64), alpha0, nu0)
    assert np.array_equal(got.alpha, alpha0) and np.array_equal(got.nu, nu0) and got.converged
    assert got.iterations == 0 and len(got.lower_bounds) == 0                   # nothing to iterate on
    _, _, q = twin_vb_ibcc(ibcc.tuple_labels(C, E).T, alpha0, nu0, 0)           # every tuple once, under the priors
    assert np.allclose(got.posterior, q, rtol=1e-13, atol=0)
    assert np.array_equal(got.lut, np.argmax(q, 1))
    none = ibcc.vb_ibcc(np.zeros(C ** E), alpha0, nu0, max_iter=0)
    assert none.iterations == 0 and len(none.lower_bounds) == 0 and np.array_equal(none.lut, got.lut)
    with pytest.raises(ValueError):
        ibcc.vb_ibcc(np.zeros(C ** E + 1), alpha0, nu0)
    with pytest.raises(ValueError):
        ibcc.vb_ibcc(np.zeros(C ** E), alpha0, nu0[:-1])
    with pytest.raises(ValueError):
        ibcc.vb_ibcc(np.zeros(C ** E), alpha0 * 0, nu0)
    with pytest.raises(ValueError):
        ibcc.vb_ibcc(-np.ones(C ** E), alpha0, nu0)


def test_first_maximum_breaks_ties():
    C, E = 3, 2
    got = ibcc.vb_ibcc(np.zeros(C ** E), np.ones((E, C, C)), np.ones(C))         # flat priors: every class ties everywhere
    assert np.allclose(got.posterior, 1.0 / C) and np.array_equal(got.lut, np.zeros(C ** E, np.uint8))


def test_priors_from_confusion_matrices():
    cm_a = np.array([[8., 2., 0.], [0., 0., 0.], [1., 1., 2.]])                  # class 1 was never seen: an empty row
    cm_b = np.array([[5., 5., 0.], [0., 0., 0.], [0., 0., 4.]])
    alpha0, nu0 = ibcc.ibcc_priors([cm_a, cm_b])
    assert np.array_equal(alpha0, 1 + np.stack([cm_a, cm_b])) and np.array_equal(nu0, [11., 1., 5.])
    alpha0, nu0 = ibcc.ibcc_priors([cm_a, cm_b], prior_strength=20)
    assert np.allclose(alpha0[0], 1 + 20 * np.array([[.8, .2, 0.], [0., 0., 0.], [.25, .25, .5]]))
    assert np.array_equal(alpha0[:, 1], np.ones((2, 3)))                          # the empty rows stay flat
    assert np.allclose(alpha0.sum(2)[:, [0, 2]], 3 + 20)
    assert np.allclose(nu0, 1 + 20 * 3 * np.array([10., 0., 4.]) / 14) and np.isclose(nu0.sum() - 3, 60)
    alpha0, nu0 = ibcc.ibcc_priors([np.zeros((3, 3))] * 2, prior_strength=5)      # nothing measured at all
    assert np.array_equal(alpha0, np.ones((2, 3, 3))) and np.array_equal(nu0, np.ones(3))
    alpha0, nu0 = ibcc.ibcc_priors([cm_a, cm_b], prior_strength=0)
    assert np.array_equal(alpha0, np.ones((2, 3, 3))) and np.array_equal(nu0, np.ones(3))
    for bad in ([], [cm_a, cm_b[:2]], [cm_a, -cm_b]):
        with pytest.raises(ValueError):
            ibcc.ibcc_priors(bad)
    with pytest.raises(ValueError):
        ibcc.ibcc_priors([cm_a], prior_strength=-1)


def test_adapting_pays_under_domain_shift():
    """Ground truth from a class prior, two experts from known confusion matrices, a third whose matrix on the adaptation set
    is far worse than the one its prior was measured under (it mostly answers the NEXT class).  Without one label the adapted
    table must beat the prior-only table on the drawn pixels, and the adapted posterior-mean matrix of the degraded expert
    must be closer (L1) to its true matrix than its prior mean is.  The per-pixel twin must show both effects, and the
    product is compared with the twin, not with a fixed number."""
    C, E, P, iterations = 4, 3, 6000, 40
    rng = np.random.default_rng(11)
    class_prior = np.array([0.4, 0.3, 0.2, 0.1])
    truth = rng.choice(C, P, p=class_prior)
    good = [soft_identity(C, 0.75), soft_identity(C, 0.7), soft_identity(C, 0.9)]   # what the priors were measured under
    degraded = 0.15 * soft_identity(C, 0.25) + 0.85 * np.roll(np.eye(C), 1, axis=1)
    actual = [good[0], good[1], degraded]
    labels = np.stack([draw_answers(rng, truth, m) for m in actual], 1)
    measured = [400 * class_prior[:, None] * m for m in good]                        # expected counts of a small measure set
    alpha0, nu0 = ibcc.ibcc_priors(measured)
    t = ibcc.tuple_index(labels.T, C)
    hist = np.bincount(t, minlength=C ** E)

    prior_only = ibcc.vb_ibcc(np.zeros_like(hist), alpha0, nu0)
    adapted = ibcc.vb_ibcc(hist, alpha0, nu0, max_iter=iterations, tol=0.0)
    alpha, _, q = twin_vb_ibcc(labels, alpha0, nu0, iterations)
    _, _, q_prior = twin_vb_ibcc(labels, alpha0, nu0, 0)

    def mean_matrix(a):
        return a / a.sum(1, keepdims=True)

    def l1(a):
        return float(np.abs(mean_matrix(a) - degraded).sum())

    acc = {'prior': float(np.mean(prior_only.lut[t] == truth)), 'adapted': float(np.mean(adapted.lut[t] == truth)),
           'twin prior': float(np.mean(np.argmax(q_prior, 1) == truth)), 'twin adapted': float(np.mean(np.argmax(q, 1) == truth))}
    dist = {'prior': l1(alpha0[2]), 'adapted': l1(adapted.alpha[2]), 'twin adapted': l1(alpha[2])}
    print(acc, dist)
    assert acc['adapted'] > acc['prior'] and acc['twin adapted'] > acc['twin prior']
    assert dist['adapted'] < dist['prior'] and dist['twin adapted'] < dist['prior']
    # the product against the twin: the same decisions on every pixel, the same matrix to summation order
    assert np.array_equal(adapted.lut[t], np.argmax(q, 1)) and np.array_equal(prior_only.lut[t], np.argmax(q_prior, 1))
    assert acc['adapted'] == acc['twin adapted'] and acc['prior'] == acc['twin prior']
    assert abs(dist['adapted'] - dist['twin adapted']) <= 1e-8 * dist['twin adapted']
    # the two healthy experts keep matrices close to their own
    for e in (0, 1):
        assert np.abs(mean_matrix(adapted.alpha[e]) - actual[e]).sum() < 0.5 * l1(alpha0[2])


def test_tuple_index_is_the_decision_matrix_flattened():
    from modular_semantic_segmentation_amd.bayes_mix import bayes_decision_matrix
    rng = np.random.default_rng(2)
    for C, E in ((3, 2), (4, 3), (3, 4)):
        mats = [(rng.integers(1, 30, (C, C)) + 40 * np.eye(C)).astype(np.float32).T for _ in range(E)]
        decision = bayes_decision_matrix(mats)
        assert decision.shape == (C,) * E
        labels = rng.integers(0, C, (E, 500))
        t = ibcc.tuple_index(labels, C)
        assert t.dtype == np.int64 and np.array_equal(decision.reshape(-1)[t], decision[tuple(labels)])
        digits = ibcc.tuple_labels(C, E)
        assert digits.shape == (E, C ** E) and np.array_equal(ibcc.tuple_index(digits, C), np.arange(C ** E))
        assert np.array_equal(digits[0], np.arange(C ** E) // C ** (E - 1))        # expert 0 is the most significant digit


class _StubNet(object):
    """What collect_predictions asks of a fusion model: modalities, config, predict(batch) leaving `expert_outputs`."""

    def __init__(self, C):
        self.modalities = ['rgb', 'depth']
        self.config = {'batchsize': 2, 'fused_head': True}
        self.C = C
        self.heads_seen = []

    def predict(self, batch):
        self.heads_seen.append(self.config['fused_head'])
        self.expert_outputs = {'rgb': {'classification': (batch['rgb'].sum(-1) % self.C).astype(np.int64)},
                               'depth': {'classification': (batch['depth'][..., 0] % self.C).astype(np.int64)}}
        return self.expert_outputs['rgb']['classification']


def test_collect_predictions_writes_the_reference_file(tmp_path):
    from modular_semantic_segmentation_amd.experiments import collect_predictions
    rng = np.random.default_rng(4)
    C = 5

    def dataset(n):
        return {'rgb': rng.integers(0, 256, (n, 8, 16, 3)).astype(np.float32),
                'depth': rng.integers(0, 256, (n, 8, 16, 1)).astype(np.float32),
                'labels': rng.integers(-1, C, (n, 8, 16)).astype(np.int32)}
    measure, test = dataset(3), dataset(5)
    net = _StubNet(C)
    path = collect_predictions(net, measure, test, str(tmp_path / 'run'))
    assert os.path.basename(path) == 'predictions.npz' and os.path.exists(path)
    assert net.heads_seen == [False] * 5 and net.config['fused_head'] is True       # 2 + 3 batches, the experts materialised
    with np.load(path) as f:
        assert sorted(f.files) == ['measure_depth', 'measure_gt', 'measure_rgb', 'test_depth', 'test_gt', 'test_rgb']
        for part, data in (('measure', measure), ('test', test)):
            for m in ('rgb', 'depth'):
                got = f['%s_%s' % (part, m)]
                assert got.dtype == np.int64 and got.shape == data['labels'].shape
            assert np.array_equal(f['%s_rgb' % part], (data['rgb'].sum(-1) % C).astype(np.int64))
            assert np.array_equal(f['%s_depth' % part], (data['depth'][..., 0] % C).astype(np.int64))
            assert f['%s_gt' % part].dtype == np.int32 and np.array_equal(f['%s_gt' % part], data['labels'])


def test_the_model_is_registered():
    from modular_semantic_segmentation_amd import get_model
    from modular_semantic_segmentation_amd.ibcc_mix import IbccFusion
    assert get_model('ibcc_fusion') is IbccFusion and get_model('ibcc_mix') is IbccFusion
