"""MC-dropout Bayesian FCN (bayesian_fcn.py; get_model('bayesian_fcn')): the sample-only replication kernel against xv_dropout,
the uncertainty head against the unfused decoder head and a float64 restatement, xv_sampling_uncertainty against the head,
FcnEngine.mc_sample_scores against sequential dropout passes for every kind of site list, and the model end to end at 768x384.

The float64 restatement (bayesian_fcn.py:48-57, custom_layers.py:251-256), from per-sample probabilities p_t:
    mean = (1/T) sum_t p_t;  entropy = -sum_c mean_c ln(clip(mean_c, 1e-10, 1)) / ln C;
    cond_entropy = (1/T) sum_t (-sum_c p_tc ln(clip(p_tc, 1e-10, 1)) / ln C);  variance = sum_c population variance over t."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo

C, U = 12, 64
DEV = 'cuda:0'
DEFAULT_LAYERS = ['pool3', 'pool4', 'conv4_3', 'conv5_3', 'features']
EPS = 2.0 ** -24          # half an ulp of a float32 in [0.5, 1): the rounding error of one operation with a result below 1


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _border_zero(a):
    t = a.t
    return not (t[:, 0].any() or t[:, -1].any() or t[:, :, 0].any() or t[:, :, -1].any())


# ---- 1. sample-only replication ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('c', [256, 512])
@pytest.mark.parametrize('T', [1, 4])
@pytest.mark.parametrize('rate', [0.0, 0.5])
def test_sample_only_replication_equals_dropout_per_slot(gpu, n, c, T, rate):
    from modular_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(n * 1000 + c + T)
    x = ops.Act.from_dense((torch.rand((n, 6, 10, c), generator=g) * 4 - 1).to(DEV))
    seed0, stride = 0xfedcba9876543210 + 17 * T, 1000003
    y = ops.Act(T * n, 6, 10, c, DEV)
    y.t.fill_(float('nan'))                      # every byte, the borders included, must be written
    ops.dropout_samples(x, T, rate, seed0, stride, y=y, sample_only=True)
    refs = []
    for t in range(T):
        ref = ops.dropout(x, rate, (seed0 + t * stride) & 0xffffffffffffffff)
        refs.append(ref)
        assert torch.equal(y.images(t * n, (t + 1) * n).t, ref.t), t
    assert _border_zero(y)
    if rate > 0:
        assert not torch.equal(refs[0].t, x.t)
    else:
        assert torch.equal(refs[0].t, x.t)
    # in place: every slot holds a copy of x and is dropped with its own seed
    z = ops.Act(T * n, 6, 10, c, DEV)
    for t in range(T):
        z.images(t * n, (t + 1) * n).t.copy_(x.t)
    assert ops.dropout_samples(z, T, rate, seed0, stride, in_place=True, sample_only=True) is z
    for t in range(T):
        assert torch.equal(z.images(t * n, (t + 1) * n).t, refs[t].t), t
    assert _border_zero(z)


# ---- 2. / 3. the head -----------------------------------------------------------------------------------------------------------

def _head_inputs(c, T, n, hi, wi, seed, kind):
    """T n images of 1/8-resolution features (sample-major) -> (features Act, their low-resolution scores S, score weights,
    bias).  kind 'random': independent random features per slot; 'dropped': ONE random map dropped T times by ops.dropout with
    different seeds (what MC dropout at 'features' produces); 'same': every slot holds the same map."""
    from modular_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    ws = (torch.randn((U, c), generator=g) * 0.3).to(DEV)
    bs = torch.randn(c, generator=g).to(DEV)
    if kind == 'random':
        f = ops.Act.from_dense((torch.rand((T * n, hi, wi, U), generator=g) * 2).to(DEV))
    else:
        one = ops.Act.from_dense((torch.rand((n, hi, wi, U), generator=g) * 2).to(DEV))
        f = ops.Act(T * n, hi, wi, U, DEV)
        for t in range(T):
            src = one if kind == 'same' else ops.dropout(one, 0.5, 77 * seed + 1000003 * t)
            f.images(t * n, (t + 1) * n).t.copy_(src.t)
    S = torch.zeros((T * n, hi + 2, wi + 2, cp), device=DEV)
    ops.score_lowres(f, ws, c, S)
    return f, S, ws, bs


def _slot_probs(f, ws, bs, c, T, n):
    """p_t of every slot from the UNFUSED decoder head (an existing kernel), stacked: float32 [T, n, H, W, c]"""
    from modular_semantic_segmentation_amd import ops
    return torch.stack([ops.decoder_head_fwd(f.images(t * n, (t + 1) * n), ws, bs, c, want_prob=True,
                                             want_label=False)['prob'].clone() for t in range(T)], 0)


def _restatement(samples):
    """the four quantities in float64 from samples [T, ..., C]"""
    p = samples.double()
    c = p.shape[-1]

    def ent(q):
        return -(q * torch.log(q.clamp(1e-10, 1.0))).sum(-1) / math.log(c)
    mean = p.mean(0)
    return {'mean': mean, 'entropy': ent(mean), 'cond_entropy': ent(p).mean(0),
            'variance': ((p * p).mean(0) - mean * mean).sum(-1)}


def _mean_bound(T):
    """|mean - float64 mean| <= (T + 1) 2^-24, the figure of an fp32 sum of T values in [0, 1] times 1 / T: T - 1 additions
    whose partial sums stay below k = 2 .. T, each rounding by at most k 2^-25, i.e. (T + 2)(T - 1) 2^-26 in all, which the
    division by T brings to less than (T + 1) 2^-26 ... 2^-25, plus the scaling's own rounding of 2^-25: within (T + 1) 2^-24.
    The kernel's running form mean_t = mean_{t-1} + (p_t - mean_{t-1}) / t stays inside the same figure: a step rounds the
    difference d (2^-25, then divided by t >= 2: 2^-26), the reciprocal of t and the product (|d / t| <= 1/2: 2^-25 + 2^-26)
    and the sum (2^-25), together e <= 1.5 * 2^-24; the error carried from the step before is damped by (1 - 1/t), so after
    T samples the error is at most e sum_{t=2..T} t / T < 0.75 (T + 1) 2^-24."""
    return (T + 1) * EPS


def _entropy_bounds(c, T):
    """(bound of entropy, bound of cond_entropy), each for |kernel - float64 restatement|, DERIVED (not read off a run):
    * one term p ln(clip p): xv_fast_log is the transcendental unit's log2 ('about 1 ulp', xv_common.h: relative 2^-23) times
      ln 2 (the rounded constant and the product: 2 * 2^-24), then times p (2^-24): relative r = 2^-23 + 3 * 2^-24 of a term
      of magnitude at most 1/e;  C terms: C r / e;
    * the fp32 sum over the C terms: C - 1 additions of partial sums below ln C: (C - 1) ln C 2^-24;
    * both divided by ln C, which itself is a rounded float, and the division rounds: + 2 * 2^-24 of a value <= 1;
    * cond_entropy: the sum over T samples of entropies below ln C each (T - 1 additions of partial sums up to T ln C, times
      1 / T afterwards: at most (T - 1) 2^-24 of the normed value) and the scaling by 1 / T (the reciprocal and the product:
      2 * 2^-24);
    * entropy: the error of `mean`, delta = (T + 1) 2^-24 per class (_mean_bound), through f(p) = p ln(clip(p, 1e-10, 1)),
      whose slope is |ln p + 1| <= 22.03 above the clip and |ln 1e-10| = 23.03 below it: C * 23.03 * delta / ln C."""
    lnc = math.log(c)
    r = 2.0 ** -23 + 3 * EPS
    per_sample = (c * r / math.e + (c - 1) * lnc * EPS) / lnc + 2 * EPS
    cond = per_sample + (T - 1) * EPS + 2 * EPS
    ent = per_sample + c * 23.03 * _mean_bound(T) / lnc
    return ent, cond


def _clear(score, margin=1e-4):
    top2 = score.topk(2, -1).values
    return (top2[..., 0] - top2[..., 1]) > margin


def _check_maps(out, ref, c, T, clear_share):
    """`out` (dict of device tensors: label, mean, entropy, cond_entropy, variance) against the float64 restatement `ref`"""
    eb, cb = _entropy_bounds(c, T)
    d_mean = (out['mean'].double() - ref['mean']).abs().max().item()
    d_ent = (out['entropy'].double() - ref['entropy']).abs().max().item()
    d_cond = (out['cond_entropy'].double() - ref['cond_entropy']).abs().max().item()
    clear = _clear(ref['mean'])
    share = clear.float().mean().item()
    print('C=%d T=%d: |mean| %.3g (bound %.3g)  |entropy| %.3g (bound %.3g)  |cond_entropy| %.3g (bound %.3g)  clear %.4f'
          % (c, T, d_mean, _mean_bound(T), d_ent, eb, d_cond, cb, share))
    assert d_mean <= _mean_bound(T)
    assert torch.allclose(out['variance'].double(), ref['variance'], rtol=1e-5, atol=1e-9)
    assert d_ent <= eb
    assert d_cond <= cb
    assert share > clear_share
    assert torch.equal(out['label'][clear], ref['mean'].argmax(-1)[clear])
    assert out['cond_entropy'].min().item() >= 0
    assert out['entropy'].max().item() <= 1 + eb
    assert (out['entropy'] - out['cond_entropy']).min().item() >= -(eb + cb)        # mutual information is non-negative
    assert out['variance'].min().item() >= 0 and out['variance'].max().item() <= 1


# Clear-pixel share (top-2 gap of the float64 mean > 1e-4) of these inputs, evaluated on the CPU in float64 with torch alone
# (the same generators, seeds, weights and bilinear x8 taps; the 'dropped' kind with Bernoulli(0.5) masks from the generator
# in place of the kernel's hash) for all 15 (C, T) pairs and both kinds: the smallest share is 0.9989 (C = 14, T = 2,
# 'random'), far above the 0.9 required.
@pytest.mark.parametrize('kind', ['random', 'dropped'])
@pytest.mark.parametrize('c', [3, 5, 12, 14, 16, 20, 30, 32])
@pytest.mark.parametrize('T', [1, 2, 7])
def test_uncertainty_head_against_unfused_path(gpu, c, T, kind):
    from modular_semantic_segmentation_amd import ops
    n, hi, wi = 2, 5, 7
    f, S, ws, bs = _head_inputs(c, T, n, hi, wi, seed=31 * c + T, kind=kind)
    out = ops.mc_uncertainty_head(S, bs, n, hi, wi, c, T, want_mean=True, want_entropy=True, want_cond_entropy=True,
                                  want_variance=True)
    samples = _slot_probs(f, ws, bs, c, T, n)
    ref = _restatement(samples)
    _check_maps(out, ref, c, T, clear_share=0.9)
    if T == 1:
        assert torch.equal(out['mean'], samples[0])
        assert torch.count_nonzero(out['variance']).item() == 0
        assert torch.equal(out['entropy'], out['cond_entropy'])
    else:
        assert (ref['variance'] > 0).float().mean() > 0.99
    # the label alone: the same labels
    assert torch.equal(ops.mc_uncertainty_head(S, bs, n, hi, wi, c, T)['label'], out['label'])
    # the stand-alone reduction on the materialised p_t: every output of the head, bit for bit
    alone = ops.sampling_uncertainty(samples.contiguous())
    for key in ('label', 'mean', 'entropy', 'cond_entropy', 'variance'):
        assert torch.equal(alone[key], out[key]), key
    # and any subset of its outputs
    part = ops.sampling_uncertainty(samples.contiguous(), want_label=False, want_mean=False, want_cond_entropy=False)
    assert sorted(part) == ['entropy', 'variance']
    assert torch.equal(part['entropy'], out['entropy']) and torch.equal(part['variance'], out['variance'])


@pytest.mark.parametrize('c', [5, 12])
def test_uncertainty_head_degenerate_samples(gpu, c):
    """Identical samples: the variance is exactly 0, the mean is the one pass's softmax and the label its label."""
    from modular_semantic_segmentation_amd import ops
    n, hi, wi, T = 2, 4, 6, 5
    f, S, ws, bs = _head_inputs(c, T, n, hi, wi, seed=5 + c, kind='same')
    out = ops.mc_uncertainty_head(S, bs, n, hi, wi, c, T, want_mean=True, want_entropy=True, want_cond_entropy=True,
                                  want_variance=True)
    assert torch.count_nonzero(out['variance']).item() == 0
    one = ops.decoder_head_fwd(f.images(0, n), ws, bs, c, want_prob=True, want_label=True)
    assert ((out['mean'] - one['prob']).abs() <= 2.0 ** -23 * one['prob']).all()
    clear = _clear(one['prob'].double())
    assert clear.float().mean() > 0.9
    assert torch.equal(out['label'][clear], one['label'][clear])


def test_uncertainty_head_refuses_bad_arguments(gpu):
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd._lib import XvError
    S = torch.zeros((2, 4, 4, 4), device=DEV)
    b = torch.zeros(4, device=DEV)
    with pytest.raises(XvError):
        ops.mc_uncertainty_head(torch.zeros((0, 4, 4, 4), device=DEV), b, 2, 2, 2, 3, 0)       # T < 1
    with pytest.raises(XvError):
        ops.mc_uncertainty_head(S, b, 2, 2, 2, 1, 1)                                           # C < 2
    with pytest.raises(ValueError):
        ops.mc_uncertainty_head(S, b, 2, 2, 2, 3, 2)                                           # S holds T n = 2 images, not 4


# ---- 4. the sampler -----------------------------------------------------------------------------------------------------------

def _engine(prefix='rgb', cin=3, seed=9, first=0.02):
    from modular_semantic_segmentation_amd.fcn import FcnEngine
    w = fo.init_fcn_weights(prefix, cin, U, C, seed=seed, bias_scale=0.02)
    w['%s/conv1_1/kernel' % prefix] *= first
    for k in w:
        if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] *= 1.6
    return FcnEngine(prefix, cin, U, C, w, device=DEV)


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('layers', [['pool3'], ['conv4_3'], ['conv5_3', 'features'], ['pool4'], DEFAULT_LAYERS],
                         ids=lambda l: '+'.join(l))
def test_mc_sample_scores_equal_sequential_dropout_passes(gpu, monkeypatch, n, layers):
    """Slot t of the batched sampler holds the bits of sequential pass p0 + t (the pass counter continues over calls); a chunk
    cap that splits the samples changes no bit; without 'pool3' the 3x3 trunk runs once on n images, whatever T."""
    from modular_semantic_segmentation_amd import ops
    eng = _engine()
    T, rate, seed = 4, 0.5, 11
    x = torch.from_numpy(np.random.default_rng(3 + n).integers(0, 256, (n, 64, 96, 3)).astype(np.float32)).to(DEV)
    calls = []
    real = ops.conv2d_fwd

    def counting(xa, w_packed, bias, k, *args, **kwargs):
        calls.append((int(k), xa.n))
        return real(xa, w_packed, bias, k, *args, **kwargs)
    monkeypatch.setattr(ops, 'conv2d_fwd', counting)
    plain = eng.lowres_scores(x)[0].clone()
    plain_3x3 = [c for c in calls if c[0] == 3]
    assert plain_3x3 and all(c[1] == n for c in plain_3x3)
    eng._dropout_pass = 0
    eng.set_dropout(layers, rate, seed)
    seq = [eng.lowres_scores(x)[0].clone() for _ in range(2 * T)]
    assert eng._dropout_pass == 2 * T
    eng.set_dropout([], 0.0)
    eng._dropout_pass = 0
    del calls[:]
    S, geo = eng.mc_sample_scores(x, T, rate, seed, layers)
    S = S.clone()
    sampler_3x3 = [c for c in calls if c[0] == 3]
    assert geo == (n, 8, 12) and eng._dropout_pass == T and tuple(S.shape[:1]) == (T * n,)
    for t in range(T):
        assert torch.equal(S[t * n:(t + 1) * n], seq[t]), t
    if 'pool3' not in layers:
        assert sampler_3x3 == plain_3x3                                # the 3x3 trunk ran once, on n images
    if layers == ['pool4']:
        for t in range(T):
            assert torch.equal(S[t * n:(t + 1) * n], plain), t         # 'pool4' alone enables nothing
    else:
        assert not torch.equal(S[:n], S[n:2 * n])
        assert not torch.equal(S[:n], plain)
    S2 = eng.mc_sample_scores(x, T, rate, seed, layers)[0].clone()     # passes T .. 2T-1
    assert eng._dropout_pass == 2 * T
    for t in range(T):
        assert torch.equal(S2[t * n:(t + 1) * n], seq[T + t]), t
    for cap in (n, 3 * n):                                             # one sample per launch; three and one
        eng._dropout_pass, eng.mc_chunk_images = 0, cap
        S3 = eng.mc_sample_scores(x, T, rate, seed, layers)[0]
        for t in range(T):
            assert torch.equal(S3[t * n:(t + 1) * n], seq[t]), (cap, t)
    # rate 0: T copies of the plain pass, the counter still advances
    eng._dropout_pass = 0
    S4 = eng.mc_sample_scores(x, T, 0.0, seed, layers)[0]
    assert eng._dropout_pass == T
    for t in range(T):
        assert torch.equal(S4[t * n:(t + 1) * n], plain), t


def test_mc_sample_scores_refuses_what_it_cannot_sample(gpu):
    eng = _engine()
    x = torch.zeros((1, 64, 96, 3), device=DEV)
    eng.set_dropout(['pool3'], 0.5, 1)
    with pytest.raises(ValueError):
        eng.mc_sample_scores(x, 2, 0.5, 1, ['pool3'])
    eng.set_dropout([], 0.0)
    with pytest.raises(ValueError):
        eng.mc_sample_scores(x, 0, 0.5, 1, ['pool3'])
    eng.affine['upscore'] = (None, None)                               # an un-commuted head
    with pytest.raises(NotImplementedError):
        eng.mc_sample_scores(x, 2, 0.5, 1, ['pool3'])


# ---- 5. the model -----------------------------------------------------------------------------------------------------------

DESC = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, C)


def _rescale(net, seed):
    """the weight recipe of the variance fusion model's test (activations that neither die nor overflow at 768x384)"""
    w = dict(net.variables)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith('/bias') and 'upscore' not in k:
            w[k] = (rng.standard_normal(w[k].shape) * 0.02).astype(np.float32)
        elif k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] = w[k] * 1.6
    w['rgb/conv1_1/kernel'] = w['rgb/conv1_1/kernel'] / 50.0
    net.variables.update(w)
    net._variables_changed()
    return net


def _model(T=5, rate=0.5, seed=1, **extra):
    from modular_semantic_segmentation_amd import get_model
    net = get_model('bayesian_fcn')('rgb', DESC, 'rgb', num_units=U, dropout_rate=rate, num_samples=T, seed=seed,
                                    batchsize=2, **extra)
    return _rescale(net, seed)


def _data(n, seed):
    rng = np.random.default_rng(seed)
    return {'rgb': rng.integers(0, 256, (n, 384, 768, 3)).astype(np.float32),
            'labels': rng.integers(-1, C, (n, 384, 768)).astype(np.int32)}


@pytest.mark.parametrize('n', [1, 2])
def test_bayesian_model_768x384(gpu, n):
    T, rate = 5, 0.5
    data = _data(n, 20 + n)
    net = _model(T, rate)
    assert list(net.config['dropout_layers']) == DEFAULT_LAYERS
    out = net.predict_uncertainty(data)
    assert out['label'].shape == (n, 384, 768) and out['label'].dtype == np.int64
    assert out['mean'].shape == (n, 384, 768, C) and out['mean'].dtype == np.float32
    for key in ('entropy', 'cond_entropy', 'variance'):
        assert out[key].shape == (n, 384, 768) and out[key].dtype == np.float32, key
    # float64 restatement from T sequential passes of a twin model (same weights and seed, fresh pass counter)
    twin = _model(T, rate)
    x = torch.from_numpy(data['rgb']).to(DEV)
    twin.engine.set_dropout(DEFAULT_LAYERS, rate, twin._dropout_seed)
    samples = torch.stack([twin.engine.forward(x, want=('prob',))['prob'].clone() for _ in range(T)], 0)
    twin.engine.set_dropout([], 0.0)
    ref = _restatement(samples)
    _check_maps({k: torch.from_numpy(v).to(DEV) for k, v in out.items()}, ref, C, T, clear_share=0.5)
    # the same seed in a fresh model: the same labels; consecutive calls: new masks
    fresh = _model(T, rate)
    labels = fresh.predict(data)
    assert labels.shape == (n, 384, 768) and labels.dtype == np.int64
    assert np.array_equal(labels, out['label'])
    v1 = net.predict(data, output_attr='variance')
    v2 = net.predict(data, output_attr='variance')
    assert v1.shape == (n, 384, 768) and not np.array_equal(v1, v2)
    assert net.predict(data, output_attr='mean').shape == (n, 384, 768, C)
    assert net.predict(data, output_attr='prob').shape == (n, 384, 768, C)
    assert net.predict(data, output_attr='entropy').shape == (n, 384, 768)
    assert net.predict(data, output_attr='cond_entropy').shape == (n, 384, 768)
    for _ in range(3):                                                 # enough equal batches for an automatic capture
        net.predict(data)
    assert net._graph is None
    measures, cm = net.score(data)
    assert cm.shape == (C, C) and cm.sum() == (data['labels'] >= 0).sum()
    assert 'mean_IoU' in measures and 'total_accuracy' in measures


def test_bayesian_model_loads_fcn_weights(gpu, tmp_path):
    """The npz schema is the expert's; at dropout_rate 0 every sample is the plain pass."""
    from modular_semantic_segmentation_amd import get_model
    data = _data(1, 31)
    fcn = _rescale(get_model('fcn')('rgb', DESC, 'rgb', num_units=U, batch_normalization=False, seed=3, batchsize=2), 3)
    path = fcn.export_weights(str(tmp_path))
    prob = fcn.predict(data, output_attr='prob')
    net = get_model('bayesian_fcn')('rgb', DESC, 'rgb', num_units=U, dropout_rate=0.0, num_samples=3, seed=8, batchsize=2)
    net.import_weights(path, warnings=False)
    for k, v in fcn.variables.items():
        assert np.array_equal(net.variables[k], v), k
    out = net.predict_uncertainty(data)
    assert np.count_nonzero(out['variance']) == 0
    assert (np.abs(out['mean'] - prob) <= 2.0 ** -23 * prob).all()
    eb, cb = _entropy_bounds(C, 3)
    assert np.abs(out['entropy'] - out['cond_entropy']).max() <= eb + cb          # identical samples: no mutual information


# ---- 6. API -----------------------------------------------------------------------------------------------------------------

def test_bayesian_model_api(gpu):
    from modular_semantic_segmentation_amd import get_model
    from modular_semantic_segmentation_amd.bayesian_fcn import BayesianFCN
    cls = get_model('bayesian_fcn')
    assert cls is BayesianFCN
    with pytest.raises(UserWarning):
        cls('rgb', DESC, 'rgb', num_units=U, dropout_rate=0.5)
    with pytest.raises(UserWarning):
        cls('rgb', DESC, 'rgb', num_units=U, num_samples=4)
    with pytest.raises(UserWarning):
        cls('rgb', DESC, 'rgb', num_units=U, dropout_rate=0.5, num_samples=4, method='other')
    with pytest.raises(NotImplementedError):
        cls('rgb', DESC, 'rgb', num_units=U, dropout_rate=0.5, num_samples=4, batch_normalization=True)
    net = cls('rgb', DESC, 'rgb', num_units=U, dropout_rate=0.5, num_samples=4)
    assert net.config['method'] == 'sampling' and net._dropout_seed == 0
    assert cls('rgb', DESC, 'rgb', num_units=U, dropout_rate=0.5, num_samples=4, seed=5)._dropout_seed == 5
    assert cls('rgb', DESC, 'rgb', num_units=U, dropout_rate=0.5, num_samples=4, seed=5, dropout_seed=9)._dropout_seed == 9
    with pytest.raises(NotImplementedError):
        net.fit(None, 1)
    with pytest.raises(UserWarning):
        net.predict({'rgb': np.zeros((1, 64, 96, 3), np.float32)}, output_attr='fused_score')


def test_sampling_uncertainty_functional(gpu):
    """The reference's signature and tuple; the maps against float64 from the very probabilities the pipeline returned."""
    from modular_semantic_segmentation_amd import simple_fcn
    from modular_semantic_segmentation_amd.bayesian_fcn import sampling_uncertainty
    T = 4
    w = fo.init_fcn_weights('rgb', 3, U, C, seed=9, bias_scale=0.02)
    w['rgb/conv1_1/kernel'] *= 0.02
    for k in w:
        if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] *= 1.6
    x = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (2, 64, 96, 3)).astype(np.float32)).to(DEV)
    seen = []

    def pipeline(inputs, **kwargs):
        layers = simple_fcn.fcn(inputs, 'rgb', U, C, variables=w, **kwargs)
        seen.append(layers['prob'].clone())
        return layers
    mean, unc = sampling_uncertainty(x, pipeline, T, C, dropout_rate=0.5, dropout_layers=DEFAULT_LAYERS, dropout_seed=3)
    assert len(seen) == T and not torch.equal(seen[0], seen[1])
    assert sorted(unc) == ['cond_entropy', 'entropy', 'variance']
    assert tuple(mean.shape) == (2, 64, 96, C) and all(tuple(v.shape) == (2, 64, 96) for v in unc.values())
    ref = _restatement(torch.stack(seen, 0))
    eb, cb = _entropy_bounds(C, T)
    assert (mean.double() - ref['mean']).abs().max().item() <= _mean_bound(T)
    assert torch.allclose(unc['variance'].double(), ref['variance'], rtol=1e-5, atol=1e-9)
    assert (unc['entropy'].double() - ref['entropy']).abs().max().item() <= eb
    assert (unc['cond_entropy'].double() - ref['cond_entropy']).abs().max().item() <= cb
