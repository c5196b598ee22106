"""Scoring by group of images on one pass: the grouped confusion kernel against numpy, the grouped joint histogram against the
ungrouped one per group, score_groups of the models against score() of each group's images, and FusionComparison's
score_all_groups against score_all.  Integer results throughout: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo

C, U = 12, 64
H, W = 64, 96
DEV = 'cuda:0'
MODS = ('rgb', 'depth')


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


# ---- xv_confusion_matrix_grouped ----------------------------------------------------------------------------------------------

def _maps(c, shape, seed, n=3):
    """labels drawn from [-1, c] with a few c + 5 among them (none of -1, c, c + 5 is counted), predictions from [0, c)"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(-1, c + 1, (n,) + shape).astype(np.int32)
    labels[rng.random(labels.shape) < 0.05] = c + 5
    labels.reshape(n, -1)[:, :3] = (-1, c, c + 5)                            # every image holds all three
    pred = rng.integers(0, c, (n,) + shape).astype(np.int64)
    return labels, pred


def _numpy_counts(labels, pred, groups, num_groups, c):
    ref = np.zeros((num_groups, c, c), np.int64)
    gid = np.broadcast_to(np.asarray(groups).reshape((-1,) + (1,) * (labels.ndim - 1)), labels.shape)
    ok = (labels >= 0) & (labels < c)
    np.add.at(ref, (gid[ok], labels[ok], pred[ok]), 1)
    return ref


# 5x7: 35 pixels per image, below one workgroup and a multiple of no vector width; 64x96: 1 536 label quads per image, two
# workgroups of 1 024 threads, the second one half full
@pytest.mark.parametrize('groups,num_groups', [([1, 0, 1], 2), ([0, 1, 2], 3), ([3, 0, 1], 4)], ids=['two', 'per-image', 'empty'])
@pytest.mark.parametrize('shape', [(5, 7), (64, 96)], ids=['5x7', '64x96'])
@pytest.mark.parametrize('c', [2, 12, 64])
def test_grouped_confusion_equals_numpy(gpu, c, shape, groups, num_groups):
    from modular_semantic_segmentation_amd import ops
    labels, pred = _maps(c, shape, 7 * c + shape[0] + num_groups)
    ref = _numpy_counts(labels, pred, groups, num_groups, c)
    assert ref.sum() == ((labels >= 0) & (labels < c)).sum() and (ref.sum((1, 2)) == 0).sum() == num_groups - len(set(groups))
    dl, dp = torch.from_numpy(labels).to(DEV), torch.from_numpy(pred).to(DEV)
    cm = ops.confusion_matrix_grouped(dl, dp, groups, num_groups, num_classes=c)
    assert cm.dtype == torch.int64 and tuple(cm.shape) == (num_groups, c, c)
    assert np.array_equal(cm.cpu().numpy(), ref)
    # ids checked and uploaded once (what a pass over many batches does) are taken as they are
    assert torch.equal(ops.confusion_matrix_grouped(dl, dp, ops.upload_group_ids(groups, num_groups, DEV), num_groups, num_classes=c), cm)
    # accumulated onto what cm holds, not cleared
    filled = np.random.default_rng(1).integers(0, 1000, ref.shape)
    cm2 = torch.from_numpy(filled).to(DEV)
    assert ops.confusion_matrix_grouped(dl, dp, np.asarray(groups), num_groups, cm=cm2) is cm2
    assert np.array_equal(cm2.cpu().numpy(), filled + ref)
    # the groups sum to the ungrouped kernel's matrix of the same tensors
    whole = torch.zeros((c, c), dtype=torch.int64, device=DEV)
    ops.confusion_matrix(dl, dp, whole)
    assert torch.equal(cm.sum(0), whole)


def test_grouped_confusion_refuses_bad_arguments(gpu):
    from modular_semantic_segmentation_amd import _lib, ops
    lib = _lib.lib()
    c, n, ppi, G = 12, 3, 35, 2
    labels, pred = _maps(c, (5, 7), 3)
    dl, dp = torch.from_numpy(labels).to(DEV), torch.from_numpy(pred).to(DEV)
    ids = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    cm = torch.zeros((G, c, c), dtype=torch.int64, device=DEV)
    good = [dl.data_ptr(), dp.data_ptr(), ids.data_ptr(), n, ppi, c, G, cm.data_ptr(), None]
    for i in (0, 1, 2, 7):                                                   # every pointer: null, then misaligned
        for v in (None, good[i] + (4 if i in (1, 7) else 2)):
            bad = list(good)
            bad[i] = v
            assert lib.xv_confusion_matrix_grouped(*bad) == _lib.CONSTANTS['XV_EINVAL'], (i, v)
    for i in (3, 4, 6):                                                      # n, ppi, num_groups below 1
        for v in (0, -1):
            bad = list(good)
            bad[i] = v
            assert lib.xv_confusion_matrix_grouped(*bad) == _lib.CONSTANTS['XV_EINVAL'], (i, v)
    bad = list(good)
    bad[5] = 65                                                              # the class range of xv_confusion_matrix
    assert lib.xv_confusion_matrix(dl.data_ptr(), dp.data_ptr(), 65, n * ppi, cm.data_ptr(), None) == _lib.CONSTANTS['XV_ESHAPE']
    assert lib.xv_confusion_matrix_grouped(*bad) == _lib.CONSTANTS['XV_ESHAPE']
    torch.cuda.synchronize()
    assert int(cm.abs().sum()) == 0                                          # nothing was written
    # an id outside [0, G): ops raises before any launch ...
    for ids_bad in ([1, 0, 2], [1, -1, 0], [1, 0], [0.0, 1.0, 0.0]):
        with pytest.raises(ValueError):
            ops.confusion_matrix_grouped(dl, dp, ids_bad, G, cm=cm)
    with pytest.raises(ValueError):
        ops.confusion_matrix_grouped(dl, dp, [0, 0, 0], 0, cm=cm)
    assert int(cm.abs().sum()) == 0
    # ... and the kernel itself counts nothing for such an image: it never indexes cm with an unchecked id
    guard = torch.zeros((G + 2, c, c), dtype=torch.int64, device=DEV)         # cm = the middle G matrices
    stray = torch.tensor([G, 0, -1], dtype=torch.int32, device=DEV)
    args = [dl.data_ptr(), dp.data_ptr(), stray.data_ptr(), n, ppi, c, G, guard[1:].data_ptr(), None]
    assert lib.xv_confusion_matrix_grouped(*args) == 0
    ref = _numpy_counts(labels[1:2], pred[1:2], [0], G, c)
    got = guard.cpu().numpy()
    assert np.array_equal(got[1:G + 1], ref) and got[0].sum() == 0 and got[G + 1].sum() == 0


# ---- xv_fused_head_joint_hist_grouped_fwd -------------------------------------------------------------------------------------

def _scores(c, seed, n, hi, wi):
    """random zero-bordered low-resolution scores of two experts, their biases and labels drawn from [-1, c]"""
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    S = [torch.zeros((n, hi + 2, wi + 2, cp)) for _ in range(2)]
    for t in S:
        t[:, 1:-1, 1:-1, :c] = torch.randn((n, hi, wi, c), generator=g) * 3
    bias = [torch.randn(c, generator=g).to(DEV) for _ in range(2)]
    labels = torch.randint(-1, c + 1, (n, 8 * hi, 8 * wi), generator=g, dtype=torch.int32).to(DEV)
    return [t.to(DEV) for t in S], bias, labels


# 8x12: whole steps of 256 pixel groups per image; 5x7: the last step of an image is partial
@pytest.mark.parametrize('hi,wi', [(8, 12), (5, 7)], ids=['8x12', '5x7'])
@pytest.mark.parametrize('c', [12, 20])
def test_grouped_joint_hist_equals_the_ungrouped_head_per_group(gpu, c, hi, wi):
    from modular_semantic_segmentation_amd import ops
    n = 3
    S, bias, labels = _scores(c, 17 * c + hi, n, hi, wi)
    whole = ops.fused_head_joint_hist(S[0], S[1], bias[0], bias[1], n, hi, wi, c, labels)
    assert int(whole.sum()) == int(((labels >= 0) & (labels < c)).sum()) and int((whole.sum(0) > 0).sum()) > c
    for groups, G in (([1, 0, 1], 2), ([0, 1, 2], 3), ([3, 0, 1], 4)):
        ref = torch.zeros((G, c, c, c), dtype=torch.int64, device=DEV)
        for g in set(groups):
            idx = torch.tensor([i for i in range(n) if groups[i] == g], device=DEV)
            ops.fused_head_joint_hist(S[0][idx].contiguous(), S[1][idx].contiguous(), bias[0], bias[1], len(idx), hi, wi, c,
                                      labels[idx].contiguous(), hist=ref[g])
        for max_workgroups in (0, 1, 2, 7):          # 1, 2: a workgroup walks several images; 7: images of two parts
            hist = ops.fused_head_joint_hist_grouped(S[0], S[1], bias[0], bias[1], n, hi, wi, c, labels, groups, G,
                                                     max_workgroups=max_workgroups)
            assert hist.dtype == torch.int64 and torch.equal(hist, ref), (groups, max_workgroups)
            assert torch.equal(hist.sum(0), whole)
        again = ops.fused_head_joint_hist_grouped(S[0], S[1], bias[0], bias[1], n, hi, wi, c, labels, groups, G, hist=hist)
        assert again is hist and torch.equal(hist, 2 * ref)                  # accumulated, not cleared


def test_grouped_joint_hist_refuses_bad_arguments(gpu):
    from modular_semantic_segmentation_amd import _lib, ops
    lib = _lib.lib()
    c, n, hi, wi, G = 12, 3, 2, 2, 2
    S, bias, labels = _scores(c, 5, n, hi, wi)
    ids = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    hist = torch.zeros((G, c, c, c), dtype=torch.int64, device=DEV)
    good = [S[0].data_ptr(), S[1].data_ptr(), bias[0].data_ptr(), bias[1].data_ptr(), n, hi, wi, c, labels.data_ptr(),
            ids.data_ptr(), G, hist.data_ptr(), 0, None]
    for i in (0, 1, 2, 3, 8, 9, 11):
        bad = list(good)
        bad[i] = None
        assert lib.xv_fused_head_joint_hist_grouped_fwd(*bad) == -1, i
    for i, v in ((7, 1), (7, 21), (10, 0), (12, -1), (8, good[8] + 4), (9, good[9] + 2), (11, good[11] + 4)):
        bad = list(good)
        bad[i] = v
        assert lib.xv_fused_head_joint_hist_grouped_fwd(*bad) == -1, (i, v)
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0
    with pytest.raises(ValueError):
        ops.fused_head_joint_hist_grouped(S[0], S[1], bias[0], bias[1], n, hi, wi, c, labels, [0, 1, 2], G, hist=hist)
    assert int(hist.abs().sum()) == 0
    assert lib.xv_fused_head_joint_hist_grouped_fwd(*good) == 0
    assert int(hist.sum()) == int(((labels >= 0) & (labels < c)).sum())


# ---- models -------------------------------------------------------------------------------------------------------------------

def _desc():
    return ({'labels': 'int32', 'rgb': 'float32', 'depth': 'float32'},
            {'labels': (None, None), 'rgb': (None, None, 3), 'depth': (None, None, 1)}, C)


def _data(n, seed):
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


COMMON = dict(num_units=U, num_channels={'rgb': 3, 'depth': 1}, expert_model='fcn', batchsize=2, class_prior='data')
DIRICHLET = dict(sigma=1.0, delta=1e-2, beta=1e-2)
KEYS = ['seq-a', 'seq-b', 'seq-a', ('seq', 3), 'seq-b']        # five images in batches of two: the groups straddle the batches


@pytest.fixture(scope='module')
def setup(gpu, tmp_path_factory, golden_dir):
    tmp = tmp_path_factory.mktemp('grouped_score')
    paths = {'rgb': _weights(tmp, 'rgb', 3, 1, 0.02), 'depth': _weights(tmp, 'depth', 1, 2, 2e-4)}
    g = np.load(os.path.join(golden_dir, 'notebook_868.npz'))
    measurements = {
        'confusion_matrices': {'rgb': g['cm_rgb'], 'depth': g['cm_depth']},
        'dirichlet_params': {'rgb': np.random.default_rng(4).uniform(0.5, 4.0, (C, C)),
                             'depth': np.random.default_rng(5).uniform(0.5, 4.0, (C, C)), 'class_counts': g['cm_depth'].sum(1)}}
    return paths, measurements, _data(5, seed=41)


def _model(kind, setup, **config):
    from modular_semantic_segmentation_amd import get_model
    paths, measurements, _ = setup
    prefixes = {'rgb': 'rgb', 'depth': 'depth'}
    if kind == 'fcn':
        net = get_model('fcn')('rgb', _desc(), 'rgb', num_units=U, batch_normalization=False, batchsize=2)
        net.import_weights(paths['rgb'], warnings=False)
        return net
    if kind == 'bayes_fusion':
        net = get_model(kind)(data_description=_desc(), confusion_matrices=measurements['confusion_matrices'], prefixes=prefixes,
                              **dict(COMMON, **config))
    elif kind == 'dirichlet_fusion':
        net = get_model(kind)(data_description=_desc(), modalities=list(MODS), dirichlet_params=measurements['dirichlet_params'],
                              **dict(COMMON, **dict(DIRICHLET, **config)))
    elif kind == 'average_fusion':
        net = get_model(kind)(data_description=_desc(), prefixes=prefixes, **dict(COMMON, **config))
    else:
        from modular_semantic_segmentation_amd.fusion_comparison import FusionComparison
        net = FusionComparison(data_description=_desc(), prefixes=prefixes, confusion_matrices=measurements['confusion_matrices'],
                               dirichlet_params=measurements['dirichlet_params'], **dict(COMMON, **dict(DIRICHLET, **config)))
    for p in paths.values():
        net.import_weights(p, warnings=False)
    return net


def _same_pair(got, ref):
    """(measures, confusion matrix) as score() returns them: the same integers, identical measures, NaNs in the same places"""
    assert got[1].dtype == np.float64 and np.array_equal(got[1], ref[1])
    assert set(got[0]) == set(ref[0])
    for name in ref[0]:
        assert np.array_equal(np.asarray(got[0][name]), np.asarray(ref[0][name]), equal_nan=True), name


def _subset(data, idx):
    return {k: v[idx] for k, v in data.items()}


@pytest.mark.parametrize('kind,config', [('fcn', {}), ('bayes_fusion', {}), ('bayes_fusion', {'fused_head': False}),
                                         ('dirichlet_fusion', {}), ('average_fusion', {})],
                         ids=['fcn', 'bayes', 'bayes-unfused', 'dirichlet', 'average'])
def test_score_groups_equals_score_of_each_group(setup, monkeypatch, kind, config):
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd.basic_fusion_model import fused_head_applicable
    data = setup[2]
    net = _model(kind, setup, **config)
    whole = net.score(data)
    calls = {'hist': 0, 'confusion': 0}
    for name, entry in (('hist', 'fused_head_joint_hist_grouped'), ('confusion', 'confusion_matrix_grouped')):
        def counted(*args, _inner=getattr(ops, entry), _name=name, **kwargs):
            calls[_name] += 1
            return _inner(*args, **kwargs)
        monkeypatch.setattr(ops, entry, counted)
    results = net.score_groups(data, KEYS)
    # the route: the fused Bayes model counts the grouped joint histogram (three batches), everything else the label maps
    if kind == 'bayes_fusion' and not config:
        assert fused_head_applicable(net) and calls == {'hist': 3, 'confusion': 0}
    else:
        assert calls == {'hist': 0, 'confusion': 3}
    assert list(results) == ['seq-a', 'seq-b', ('seq', 3)]                    # in the order the keys first appear
    for key in results:
        _same_pair(results[key], net.score(_subset(data, [i for i, k in enumerate(KEYS) if k == key])))
    assert np.array_equal(sum(cm for _, cm in results.values()), whole[1])
    assert whole[1].sum() == (data['labels'] >= 0).sum()
    per_image = net.score_groups(data, 'image')
    assert list(per_image) == [0, 1, 2, 3, 4]
    for i in (0, 3, 4):
        _same_pair(per_image[i], net.score(_subset(data, [i])))
    assert np.array_equal(sum(cm for _, cm in per_image.values()), whole[1])
    first = net.score_groups(data, KEYS, max_iterations=1)                   # one batch: the first two images
    assert list(first) == ['seq-a', 'seq-b']
    assert np.array_equal(sum(cm for _, cm in first.values()), net.score(data, max_iterations=1)[1])
    assert list(net.score_groups(data, 'image', max_iterations=2)) == [0, 1, 2, 3]
    _same_pair(net.score(data), whole)                                      # score() itself is what it was
    with pytest.raises(ValueError):
        net.score_groups(data, KEYS[:4])                                    # a key per image
    with pytest.raises(ValueError):
        net.score_groups(data, 'sequence')


NAMES = ['rgb', 'depth', 'bayes_fusion', 'dirichlet_fusion', 'average_fusion']


@pytest.mark.parametrize('fused_head', [True, False], ids=['one-pass-heads', 'generic'])
def test_score_all_groups_equals_score_all(setup, fused_head):
    data = setup[2]
    net = _model('comparison', setup, fused_head=fused_head)
    assert net.one_pass_heads_applicable() == fused_head
    whole = net.score_all(data)
    results = net.score_all_groups(data, KEYS)
    assert list(results) == ['seq-a', 'seq-b', ('seq', 3)] and all(list(rows) == NAMES for rows in results.values())
    for name in NAMES:
        assert np.array_equal(sum(rows[name][1] for rows in results.values()), whole[name][1]), name
    for key in results:                                                      # and each key against score_all of its images
        ref = net.score_all(_subset(data, [i for i, k in enumerate(KEYS) if k == key]))
        for name in NAMES:
            _same_pair(results[key][name], ref[name])
    one = net.score_all_groups(data, ['all'] * 5)
    assert list(one) == ['all']
    for name in NAMES:
        _same_pair(one['all'][name], whole[name])
    mats = [whole[name][1] for name in NAMES]
    assert all(not np.array_equal(mats[i], mats[j]) for i in range(5) for j in range(i))        # five different rows
    assert list(net.score_all_groups(data, 'image', max_iterations=1)) == [0, 1]
