"""ibcc_fusion with two and three small random-weight FCN experts on 32x64 inputs: before adapt() the model decides by its
priors' table; adapt() on unlabelled images, then predict / score / score_groups through the label-tuple heads give the integers
of the same model with fused_head=False and of self.ibcc.lut applied by numpy to the experts' materialised labels."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo

U = 64
H, W = 32, 64
CHANNELS = {'rgb': 3, 'depth': 1, 'ir': 1}
FIRST_SCALE = {'rgb': 0.02, 'depth': 2e-4, 'ir': 2e-4}       # conv1_1 against inputs up to 255 / 65 535
TWO, THREE = ('rgb', 'depth'), ('rgb', 'depth', 'ir')
CASES = [(TWO, 12, 3), (THREE, 12, 2), (THREE, 5, 3)]
IDS = ['e%d-c%d-n%d' % (len(m), c, n) for m, c, n in CASES]


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _desc(mods, c):
    return (dict({m: 'float32' for m in mods}, labels='int32'),
            dict({m: (None, None, CHANNELS[m]) for m in mods}, labels=(None, None)), c)


def _data(n, c, seed, mods, labels=True):
    rng = np.random.default_rng(seed)
    d = {m: rng.integers(0, 256 if FIRST_SCALE[m] > 1e-3 else 65536, (n, H, W, CHANNELS[m])).astype(np.float32) for m in THREE}
    d['labels'] = rng.integers(-1, c, (n, H, W)).astype(np.int32)
    return {k: v for k, v in d.items() if k in mods or (labels and k == 'labels')}


@pytest.fixture(scope='module')
def weights(gpu, tmp_path_factory):
    """{(modality, classes): npz path} of random weights by seed, scaled so that the experts disagree"""
    tmp = tmp_path_factory.mktemp('ibcc_models')
    paths = {}
    for c in (12, 5):
        for i, m in enumerate(THREE):
            w = fo.init_fcn_weights(m, CHANNELS[m], U, c, seed=21 + i, bias_scale=0.02)
            w['%s/conv1_1/kernel' % m] *= FIRST_SCALE[m]
            for k in w:
                if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
                    w[k] *= 1.6
            paths[(m, c)] = os.path.join(str(tmp), '%s_%d.npz' % (m, c))
            np.savez(paths[(m, c)], **w)
    return paths


def _model(weights, mods, c, batchsize, **config):
    from modular_semantic_segmentation_amd import get_model
    rng = np.random.default_rng(5 * c + len(mods))
    cms = {m: rng.integers(1, 50, (c, c)) + 100 * np.eye(c, dtype=np.int64) for m in mods}
    cfg = dict(num_units=U, num_channels={m: CHANNELS[m] for m in mods}, expert_model='fcn', batchsize=batchsize,
               prefixes={m: m for m in mods}, confusion_matrices=cms, prior_strength=20.0, ibcc_max_iter=50)
    cfg.update(config)
    net = get_model('ibcc_fusion')(data_description=_desc(mods, c), **cfg)
    for m in mods:
        net.import_weights(weights[(m, c)], warnings=False)
    return net


def _expert_labels(net, data, mods):
    """the experts' materialised label maps of ONE batch (host), through the model's own unfused route"""
    net.predict(data, output_attr='probs')
    return [net.expert_outputs[m]['classification'].cpu().numpy() for m in mods]


def _numpy_cm(labels, pred, c):
    cm = np.zeros((c, c), np.float64)
    valid = labels >= 0
    np.add.at(cm, (labels[valid], pred[valid]), 1)
    return cm


@pytest.mark.parametrize('mods,c,n', CASES, ids=IDS)
def test_both_routes_and_numpy_agree_before_and_after_adapt(weights, mods, c, n):
    from modular_semantic_segmentation_amd import ibcc
    from modular_semantic_segmentation_amd.basic_fusion_model import tuple_head_applicable
    test = _data(n, c, 60 + c, mods)
    unlabelled = _data(n, c, 60 + c, mods, labels=False)
    fused = _model(weights, mods, c, n)
    unfused = _model(weights, mods, c, n, fused_head=False)
    assert tuple_head_applicable(fused) and not tuple_head_applicable(unfused)
    maps = _expert_labels(unfused, test, mods)
    t = ibcc.tuple_index(maps, c)
    assert len(np.unique(t)) >= 4                                            # the experts disagree somewhere

    # before adapt(): the priors' own table
    prior = ibcc.vb_ibcc(np.zeros(c ** len(mods)), fused.alpha0, fused.nu0)
    assert fused.ibcc is fused.ibcc_prior and np.array_equal(fused.ibcc.lut, prior.lut)
    a, b = fused.predict(test), unfused.predict(test)
    assert fused.expert_outputs is None and set(unfused.expert_outputs) == set(mods)
    assert a.dtype == np.int64 and a.shape == (n, H, W)
    assert np.array_equal(a, b) and np.array_equal(a, prior.lut[t].astype(np.int64))
    assert np.array_equal(fused.score(test)[1], _numpy_cm(test['labels'], prior.lut[t], c))

    # adapt on the images alone: both routes count the same histogram, so the same result to the last bit
    ra, rb = fused.adapt(unlabelled), unfused.adapt(unlabelled)
    want = ibcc.vb_ibcc(np.bincount(t.reshape(-1), minlength=c ** len(mods)), fused.alpha0, fused.nu0, max_iter=50)
    for r in (ra, rb):
        assert np.array_equal(r.lut, want.lut) and np.array_equal(r.alpha, want.alpha) and np.array_equal(r.nu, want.nu)
    assert fused.ibcc is ra and np.isclose(ra.nu.sum() - fused.nu0.sum(), n * H * W)
    assert np.array_equal(fused.lut.cpu().numpy(), want.lut)
    a, b = fused.predict(test), unfused.predict(test)
    assert np.array_equal(a, b) and np.array_equal(a, want.lut[t].astype(np.int64))
    assert np.array_equal(fused.predict(test), a)                            # and again
    (ma, cma), (mb, cmb) = fused.score(test), unfused.score(test)
    assert np.array_equal(cma, cmb) and np.array_equal(cma, _numpy_cm(test['labels'], want.lut[t], c))
    assert cma.sum() == (test['labels'] >= 0).sum() and np.array_equal(ma['IoU'], mb['IoU'], equal_nan=True)
    ga, gb = fused.score_groups(test, 'image'), unfused.score_groups(test, 'image')
    assert sorted(ga) == sorted(gb) == list(range(n))
    for i in range(n):
        assert np.array_equal(ga[i][1], gb[i][1]) and np.array_equal(ga[i][1], _numpy_cm(test['labels'][i], want.lut[t[i]], c))
    keys = ['a', 'b', 'a'][:n]
    ga, gb = fused.score_groups(test, keys), unfused.score_groups(test, keys)
    for key in set(keys):
        rows = [i for i, k in enumerate(keys) if k == key]
        assert np.array_equal(ga[key][1], gb[key][1])
        assert np.array_equal(ga[key][1], sum(_numpy_cm(test['labels'][i], want.lut[t[i]], c) for i in rows))
    # the fused score is the log posterior of the pixel's tuple, on the materialised route
    score = fused.predict(test, output_attr='fused_score')
    with np.errstate(divide='ignore'):
        assert score.shape == (n, H, W, c) and np.array_equal(score, np.log(want.posterior).astype(np.float32)[t])
    # adapting again starts from the priors: the same data give the same result, and the priors can be put back
    again = fused.adapt(unlabelled)
    assert np.array_equal(again.alpha, ra.alpha) and np.array_equal(again.lut, ra.lut)
    fused.use_adaptation(fused.ibcc_prior)
    assert np.array_equal(fused.predict(test), prior.lut[t].astype(np.int64))


def test_adapt_by_image_equals_adapting_on_each_image(weights):
    mods, c, n = THREE, 5, 3
    data = _data(n, c, 77, mods, labels=False)
    for config in ({}, {'fused_head': False}):
        net = _model(weights, mods, c, 2, **config)                           # two batches: 2 + 1 images
        grouped = net.adapt(data, groups='image')
        assert sorted(grouped) == list(range(n))
        whole = net.ibcc
        for i in range(n):
            one = net.adapt({m: data[m][i:i + 1] for m in mods})
            assert np.array_equal(grouped[i].alpha, one.alpha) and np.array_equal(grouped[i].lut, one.lut), i
            assert np.isclose(one.nu.sum() - net.nu0.sum(), H * W)
        assert np.array_equal(whole.alpha, net.adapt(data).alpha)            # the model itself: all the images
        by_key = net.adapt(data, groups=['x', 'y', 'x'])
        assert sorted(by_key) == ['x', 'y'] and np.array_equal(by_key['y'].alpha, grouped[1].alpha)
        assert np.array_equal(by_key['x'].alpha, net.adapt({m: data[m][[0, 2]] for m in mods}).alpha)


def test_agreement_runs_on_the_materialised_route(weights):
    mods, c, n = TWO, 12, 2
    test = _data(n, c, 81, mods)
    net = _model(weights, mods, c, n)
    net.adapt(test)
    measures, table = net.score_agreement(test)
    assert table.shape == (c, 4, 2, 3) and table.sum() == (test['labels'] >= 0).sum()
    assert np.array_equal(table[..., 0].sum((1, 2)), np.diag(net.score(test)[1]))


def test_measure_adapt_and_evaluate_flow(weights):
    from modular_semantic_segmentation_amd import ibcc
    from modular_semantic_segmentation_amd.experiments import fit_and_evaluate_ibcc
    mods, c = TWO, 12
    measure_set, test_set = _data(3, c, 91, mods), _data(2, c, 92, mods)
    config = dict(num_units=U, num_channels={m: CHANNELS[m] for m in mods}, expert_model='fcn', batchsize=2,
                  prefixes={m: m for m in mods}, prior_strength=20.0, ibcc_max_iter=50)
    info = fit_and_evaluate_ibcc(config, _desc(mods, c), measure_set, test_set, {m: weights[(m, c)] for m in mods})
    # the measured matrices are those of the experts' own label maps, and the priors are built from them
    ref = _model(weights, mods, c, 3, fused_head=False)
    for m, labels in zip(mods, _expert_labels(ref, measure_set, mods)):
        assert np.array_equal(info['confusion_matrices'][m], _numpy_cm(measure_set['labels'], labels, c)), m
    alpha0, nu0 = ibcc.ibcc_priors([info['confusion_matrices'][m] for m in mods], 20.0)
    t = ibcc.tuple_index(_expert_labels(ref, test_set, mods), c)
    prior = ibcc.vb_ibcc(np.zeros(c * c), alpha0, nu0)
    adapted = ibcc.vb_ibcc(np.bincount(t.reshape(-1), minlength=c * c), alpha0, nu0, max_iter=50)
    assert np.array_equal(info['ibcc'].alpha, adapted.alpha) and np.array_equal(info['ibcc'].lut, adapted.lut)
    assert np.array_equal(info['prior'][1], _numpy_cm(test_set['labels'], prior.lut[t], c))
    assert np.array_equal(info['adapted'][1], _numpy_cm(test_set['labels'], adapted.lut[t], c))
    assert set(info['adapted'][0]) >= {'mean_IoU', 'total_accuracy'}


def test_refusals(weights):
    from modular_semantic_segmentation_amd import get_model
    mods, c = TWO, 12
    net = _model(weights, mods, c, 2)
    with pytest.raises(NotImplementedError, match='score_grid'):
        net.score_grid(_data(2, c, 90, mods), {'class_prior': ['data', 'uniform']})
    with pytest.raises(ValueError, match='decision_matrix'):
        _model(weights, mods, c, 2, decision_matrix=True)
    from modular_semantic_segmentation_amd.fusion_comparison import FusionComparison
    with pytest.raises(NotImplementedError, match='IBCC'):
        FusionComparison(data_description=_desc(mods, c), num_units=U, num_channels={m: CHANNELS[m] for m in mods},
                         expert_model='fcn', prefixes={m: m for m in mods}, sigma=1.0, delta=1e-2, beta=1e-2,
                         prior_strength=20.0)
    assert get_model('ibcc_mix') is get_model('ibcc_fusion')
