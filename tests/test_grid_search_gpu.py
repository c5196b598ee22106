"""Grid search over the fusion parameters on ONE pass of the experts: the grid-scoring heads against the per-point route
(xv_fused_head_fwd / xv_decoder_head_fwd + xv_confusion_matrix), integer for integer, and score_grid of the two fusion models
against score() of a model per grid point."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo

C, U = 12, 64
H, W = 64, 96
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


# ---- op level ---------------------------------------------------------------------------------------------------------------

def _scores(c, seed, n=2, hi=5, wi=7):
    """random zero-bordered low-resolution scores of two experts, their biases and labels drawn from [-1, c]"""
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    S = [torch.zeros((n, hi + 2, wi + 2, cp)) for _ in range(2)]
    for t in S:
        t[:, 1:-1, 1:-1, :c] = torch.randn((n, hi, wi, c), generator=g) * 3
    bias = [torch.randn(c, generator=g).to(DEV) for _ in range(2)]
    labels = torch.randint(-1, c + 1, (n, 8 * hi, 8 * wi), generator=g, dtype=torch.int32).to(DEV)
    return g, [t.to(DEV) for t in S], bias, labels, (n, hi, wi)


def _dirichlet_tables(g, c, points):
    """`points` random parameter sets, each as test_fused_head_op_equals_decoder_heads_and_fusion_kernels builds one"""
    am1 = torch.stack([torch.rand((2, c, c), generator=g) - 0.5 + 4 * torch.eye(c) for _ in range(points)]).to(DEV)
    lognorm = (torch.randn((points, 2, c), generator=g) * 0.1).to(DEV)
    logprior = torch.randn((points, c), generator=g).to(DEV)
    return am1, lognorm, logprior


def _per_point(S, bias, geo, c, tables, labels):
    """the per-point route: ops.fused_head with point g's tables, then ops.confusion_matrix"""
    from modular_semantic_segmentation_amd import ops
    am1, lognorm, logprior = tables
    cm = torch.zeros((am1.shape[0], c, c), dtype=torch.int64, device=DEV)
    preds = []
    for g in range(am1.shape[0]):
        pred = ops.fused_head(S[0], S[1], bias[0], bias[1], *geo, c, am1[g], logprior[g], lognorm=lognorm[g])
        ops.confusion_matrix(labels, pred, cm[g])
        preds.append(pred)
    return cm, preds


@pytest.mark.parametrize('c', [3, 5, 12, 14, 16, 30])
def test_dirichlet_grid_score_equals_per_point_route(gpu, c):
    from modular_semantic_segmentation_amd import ops
    g, S, bias, labels, geo = _scores(c, 11 * c)
    tables = _dirichlet_tables(g, c, 5)
    ref, preds = _per_point(S, bias, geo, c, tables, labels)
    assert sum(int((preds[0] != p).sum()) > 0 for p in preds[1:]) >= 1      # the points do not predict the same map
    valid = int(((labels >= 0) & (labels < c)).sum())
    assert 0 < valid < labels.numel() and all(int(ref[i].sum()) == valid for i in range(5))
    for max_workgroups in (0, 1, 3):            # 1 and 3: the stride loop, several pixels per thread
        cm = ops.fused_head_grid_score(S[0], S[1], bias[0], bias[1], *geo, c, *tables, labels, max_workgroups=max_workgroups)
        assert cm.dtype == torch.int64 and torch.equal(cm, ref), max_workgroups
    again = ops.fused_head_grid_score(S[0], S[1], bias[0], bias[1], *geo, c, *tables, labels, cm=cm)
    assert again is cm and torch.equal(cm, 2 * ref)                         # accumulated, not cleared


@pytest.mark.parametrize('c', [12, 30])
def test_dirichlet_grid_score_splits_more_points_than_one_launch_holds(gpu, c):
    from modular_semantic_segmentation_amd import _lib, ops
    cap = ops.fused_head_grid_capacity(c)
    points = cap + 2
    g, S, bias, labels, geo = _scores(c, 5 * c + 1, n=1, hi=3, wi=4)
    tables = _dirichlet_tables(g, c, points)
    ref, _ = _per_point(S, bias, geo, c, tables, labels)
    cm = ops.fused_head_grid_score(S[0], S[1], bias[0], bias[1], *geo, c, *tables, labels)
    assert torch.equal(cm, ref)
    # the raw entry point refuses what does not fit one launch
    raw = torch.zeros_like(cm)
    rc = _lib.lib().xv_fused_head_grid_score_fwd(
        S[0].data_ptr(), S[1].data_ptr(), bias[0].data_ptr(), bias[1].data_ptr(), *geo, c, points, tables[0].data_ptr(),
        tables[1].data_ptr(), tables[2].data_ptr(), labels.data_ptr(), raw.data_ptr(), 0, None)
    assert rc == -1 and int(raw.sum()) == 0


@pytest.mark.parametrize('c', [3, 12, 20])
def test_joint_hist_equals_bincount_of_the_experts_labels(gpu, c):
    from modular_semantic_segmentation_amd import ops
    n, hi, wi, u = 2, 5, 7, 64
    g = torch.Generator().manual_seed(13 * c)
    feats = [ops.Act.from_dense((torch.rand((n, hi, wi, u), generator=g) * 2).to(DEV)) for _ in range(2)]
    ws = [(torch.randn((u, c), generator=g) * 0.3).to(DEV) for _ in range(2)]
    bs = [torch.randn(c, generator=g).to(DEV) for _ in range(2)]
    cp = (c + 3) // 4 * 4
    S = [torch.zeros((n, hi + 2, wi + 2, cp), device=DEV) for _ in range(2)]
    for e in range(2):
        ops.score_lowres(feats[e], ws[e], c, S[e])
    a, b = (ops.decoder_head_fwd(feats[e], ws[e], bs[e], c)['label'] for e in range(2))
    labels = torch.randint(-1, c + 1, (n, 8 * hi, 8 * wi), generator=g, dtype=torch.int32).to(DEV)
    ok = (labels >= 0) & (labels < c)
    key = (labels.long()[ok] * c + a[ok]) * c + b[ok]
    ref = torch.bincount(key, minlength=c ** 3).reshape(c, c, c)
    assert a.unique().numel() > 1 and b.unique().numel() > 1 and 0 < int(ok.sum()) < labels.numel()
    for max_workgroups in (0, 2):
        hist = ops.fused_head_joint_hist(S[0], S[1], bs[0], bs[1], n, hi, wi, c, labels, max_workgroups=max_workgroups)
        assert torch.equal(hist, ref), max_workgroups
    ops.fused_head_joint_hist(S[0], S[1], bs[0], bs[1], n, hi, wi, c, labels, hist=hist)
    assert torch.equal(hist, 2 * ref)


def test_bad_arguments_are_refused(gpu):
    from modular_semantic_segmentation_amd import _lib
    lib = _lib.lib()
    c = 12
    g, S, bias, labels, geo = _scores(c, 3, n=1, hi=2, wi=2)
    am1, lognorm, logprior = _dirichlet_tables(g, c, 2)
    cm = torch.zeros((2, c, c), dtype=torch.int64, device=DEV)
    good = [S[0].data_ptr(), S[1].data_ptr(), bias[0].data_ptr(), bias[1].data_ptr(), *geo, c, 2, am1.data_ptr(),
            lognorm.data_ptr(), logprior.data_ptr(), labels.data_ptr(), cm.data_ptr(), 0, None]
    assert lib.xv_fused_head_grid_score_fwd(*good) == 0
    for i in (0, 1, 2, 3, 9, 10, 11, 12, 13):                                # every pointer
        bad = list(good)
        bad[i] = None
        assert lib.xv_fused_head_grid_score_fwd(*bad) == -1, i
    for i, v in ((7, 1), (8, 0), (8, -1)):                                   # C < 2, G < 1
        bad = list(good)
        bad[i] = v
        assert lib.xv_fused_head_grid_score_fwd(*bad) == -1, (i, v)
    torch.cuda.synchronize()
    assert int(cm.sum()) == int(((labels >= 0) & (labels < c)).sum()) * 2    # only the good call counted
    hist = torch.zeros((c, c, c), dtype=torch.int64, device=DEV)
    good = [S[0].data_ptr(), S[1].data_ptr(), bias[0].data_ptr(), bias[1].data_ptr(), *geo, c, labels.data_ptr(),
            hist.data_ptr(), 0, None]
    assert lib.xv_fused_head_joint_hist_fwd(*good) == 0
    for i in (0, 1, 2, 3, 8, 9):
        bad = list(good)
        bad[i] = None
        assert lib.xv_fused_head_joint_hist_fwd(*bad) == -1, i
    for v in (1, 24):                                                        # C < 2; more classes than the counters hold
        bad = list(good)
        bad[7] = v
        assert lib.xv_fused_head_joint_hist_fwd(*bad) == -1, v
    torch.cuda.synchronize()


# ---- model level ------------------------------------------------------------------------------------------------------------

def _desc():
    return ({'labels': 'int32', 'rgb': 'float32', 'depth': 'float32'},
            {'labels': (None, None), 'rgb': (None, None, 3), 'depth': (None, None, 1)}, C)


def _data(n, seed=0):
    rng = np.random.default_rng(seed)
    return {'rgb': rng.integers(0, 256, (n, H, W, 3)).astype(np.float32),
            'depth': rng.integers(0, 65536, (n, H, W, 1)).astype(np.float32),
            'labels': rng.integers(-1, C, (n, H, W)).astype(np.int32)}


def _weights(tmp_path, prefix, cin, seed, scale_first):
    w = fo.init_fcn_weights(prefix, cin, U, C, seed=seed, bias_scale=0.02)
    w['%s/conv1_1/kernel' % prefix] *= scale_first
    for k in w:
        if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] *= 1.6
    path = os.path.join(str(tmp_path), prefix + '.npz')
    np.savez(path, **w)
    return path


@pytest.fixture(scope='module')
def setup(tmp_path_factory, golden_dir):
    from modular_semantic_segmentation_amd import get_model
    tmp = tmp_path_factory.mktemp('grid_search')
    paths = [_weights(tmp, 'rgb', 3, 1, 0.02), _weights(tmp, 'depth', 1, 2, 2e-4)]
    g = np.load(os.path.join(golden_dir, 'notebook_868.npz'))
    common = dict(data_description=_desc(), num_units=U, num_channels={'rgb': 3, 'depth': 1}, expert_model='fcn', batchsize=2,
                  class_prior='data')
    params = {'rgb': np.random.default_rng(4).uniform(0.5, 4.0, (C, C)), 'depth': np.random.default_rng(5).uniform(0.5, 4.0, (C, C)),
              'class_counts': g['cm_depth'].sum(1)}

    def make(kind, **config):
        if kind == 'bayes':
            net = get_model('bayes_fusion')(confusion_matrices={'rgb': g['cm_rgb'], 'depth': g['cm_depth']},
                                            prefixes={'rgb': 'rgb', 'depth': 'depth'}, **dict(common, **config))
        else:
            net = get_model('dirichlet_fusion')(modalities=['rgb', 'depth'],
                                                **dict(common, **dict(dict(sigma=1.0, delta=1e-2, beta=1e-2), **config)))
        for p in paths:
            net.import_weights(p, warnings=False)
        return net
    return make, params, _data(3, seed=21)          # three images in batches of two: the last batch is partial


DIRICHLET_SEARCH = {'sigma': [0.5, 1.0, 2.0], 'class_prior': ['data', 'uniform', 0.3]}
BAYES_SEARCH = {'class_prior': ['data', 'uniform', 0.3]}


def _check_points(results, configs, search, score_of):
    assert len(results) == len(configs)
    matrices = []
    for (config, measures, cm), expected in zip(results, configs):
        # parameter_combinations order, full configs (compared by the searched keys: a config may hold arrays)
        assert set(config) == set(expected) and all(config[k] == expected[k] for k in search)
        ref_measures, ref = score_of(config)
        assert cm.dtype == np.float64 and np.array_equal(cm, ref)
        assert np.array_equal(measures['confusion_matrix'], ref)
        assert np.array_equal(measures['IoU'], ref_measures['IoU'], equal_nan=True)
        matrices.append(cm)
    assert any(not np.array_equal(matrices[0], m) for m in matrices[1:])    # the points do differ


@pytest.mark.parametrize('fused_head', [True, False])
def test_dirichlet_score_grid_equals_a_model_per_point(gpu, setup, fused_head):
    from modular_semantic_segmentation_amd.experiments import parameter_combinations
    make, params, data = setup
    net = make('dirichlet', dirichlet_params=params, fused_head=fused_head)
    other = make('dirichlet', dirichlet_params=params)

    def score_of(config):            # a model with that point's config: its tables rebuilt as the constructor builds them
        other.config.update({k: config[k] for k in DIRICHLET_SEARCH})
        other._initialize_graph()
        return other.score(data)
    results = net.score_grid(data, DIRICHLET_SEARCH)
    _check_points(results, parameter_combinations(DIRICHLET_SEARCH, net.config), DIRICHLET_SEARCH, score_of)
    assert results[0][2].sum() == (data['labels'] >= 0).sum()


@pytest.mark.parametrize('fused_head', [True, False])
def test_bayes_score_grid_equals_a_model_per_point(gpu, setup, fused_head):
    from modular_semantic_segmentation_amd.experiments import grid_search_fusion, parameter_combinations
    make, _, data = setup
    net = make('bayes', fused_head=fused_head)
    results = net.score_grid(data, BAYES_SEARCH)
    _check_points(results, parameter_combinations(BAYES_SEARCH, net.config), BAYES_SEARCH,
                  lambda config: make('bayes', class_prior=config['class_prior']).score(data))
    merged = grid_search_fusion(net, data, BAYES_SEARCH)
    assert merged['class_prior'] == BAYES_SEARCH['class_prior']
    assert merged['mean_IoU'] == [r[1]['mean_IoU'] for r in results]


def test_dirichlet_score_grid_refits_delta_and_beta(gpu, setup):
    make, params, data = setup
    search = {'delta': [1e-2, 1e-1], 'beta': [1e-2]}
    unfitted = make('dirichlet', dirichlet_params=params)
    with pytest.raises(UserWarning):
        unfitted.score_grid(data, search)                                   # no sufficient statistics to refit from
    with pytest.raises(ValueError, match='num_units'):
        unfitted.score_grid(data, {'num_units': [32]})
    with pytest.raises(ValueError, match='sigma'):
        make('bayes').score_grid(data, {'sigma': [1.0]})
    net = make('dirichlet')
    net.fit(data)
    assert set(net.sufficient_statistics[0]) == {'rgb', 'depth'}
    results = net.score_grid(data, search)
    assert [(r[0]['delta'], r[0]['beta']) for r in results] == [(1e-2, 1e-2), (1e-1, 1e-2)]
    for config, _, cm in results:
        other = make('dirichlet', delta=config['delta'], beta=config['beta'])
        other.fit(data)
        assert np.array_equal(cm, other.score(data)[1]), (config['delta'], config['beta'])
