"""Uncertainty benchmarks on the device (uncertainty_model.py): xv_uncertainty_stats against numpy, the scoring form of the
uncertainty head (xv_mc_uncertainty_score_fwd) against the maps route (mc_uncertainty_head + uncertainty_stats) and, at a
temperature that is no power of two, against a float64 restatement, and the BayesianFCN's benchmark methods end to end.

Bounds, all derived:
* NLL sums on given probabilities: xv_fast_log is the transcendental unit's log2 (1 ulp: relative 2^-23) times ln 2 (the
  rounded constant and the product: 2 * 2^-24) -- the figure of tests/test_bayesian_fcn_gpu.py -- so a term -ln(clip p) of
  magnitude at most ln 1e10 is off by at most R * ln 1e10, times the count; the double sums add nothing visible.
* The same sums by two kernels that add the same terms in another order: 1e-9 relative (tests/test_config4_gpu.py).
* Temperature 1.7, float64 restatement from the fp32 logits: a sample's probability carries the relative error
  RHO = (4 xmax + 4) 2^-23 + C 2^-24 of the fp32 softmax (logit times 1 / temperature: two roundings of a value up to xmax;
  x - max; the product with log2 e, amplified by |x - max| <= 2 xmax; exp2, reciprocal and product 1 ulp each; the sum of C
  terms), and the running mean adds (T + 1) 2^-24 absolutely (_mean_bound there).  Per pixel, from the float64 values:
    entropy      per-sample figure of _entropy_bounds + sum_c |ln(clip mean_c) + 1| (T + 1) 2^-24 / ln C + RHO (H + 1 / ln C)
    cond_entropy _entropy_bounds' figure + RHO (H + 1 / ln C)
    variance     1e-5 relative + 1e-9 (the kernel against float64 on equal samples, as that file asserts)
                 + (2 RHO / T) sum_c sum_t |p_tc - mean_c| p_tc   (d var_c = (2 / T) sum_t (p_t - mean)(dp_t - dmean) to first
                 order, sum_t (p_t - mean) = 0 removes dmean, and |dp_t| <= RHO p_t)
    NLL term     R |ln mean| + RHO + (T + 1) 2^-24 / mean
  A pixel further than its tolerance from every bin edge falls into the same bin in both; the others can move a cumulative
  count by one each."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modular_semantic_segmentation_amd import uncertainty_model as um

U = 64
DEV = 'cuda:0'
EPS = 2.0 ** -24
R_LOG = 2.0 ** -23 + 2 * EPS
LN_CLIP = math.log(1e10)
METRICS = ('entropy', 'cond_entropy', 'variance')


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _np_hist(values, rows, m=5, o=24):
    h = np.zeros((2, o << m), np.int64)
    np.add.at(h, (rows, um.bin_index(values, m, o)), 1)
    return h


# ---- 1. the statistics kernel -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('m,o', [(5, 24), (3, 8), (8, 31)])
@pytest.mark.parametrize('misaligned', [False, True])
def test_uncertainty_stats_against_numpy(gpu, m, o, misaligned):
    from modular_semantic_segmentation_amd import ops
    c, npix = 12, 100003                                               # not a multiple of 4
    rng = np.random.default_rng(7 + m)
    # smooth (neighbouring lanes share a bin) and rough parts, every binade, and the special values
    metric = np.concatenate([np.repeat(rng.random(npix // 128).astype(np.float32), 64),
                             np.exp(rng.uniform(np.log(1e-12), np.log(4.0), npix)).astype(np.float32)])[:npix]
    metric[:12] = [0.0, -0.0, -1.0, np.nan, np.inf, 2.0, 1e-45, 1.0, 0.5, -np.inf, 1.9999999, 3e-39]
    labels = rng.integers(-2, c + 3, npix).astype(np.int32)           # negatives and values >= C
    pred = rng.integers(0, c, npix).astype(np.int64)
    pred[::3] = np.clip(labels[::3], 0, c - 1)                         # a good share of correct pixels
    logits = rng.standard_normal((npix, c)) * 3
    mean = (np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)).astype(np.float32)
    mean[5, labels[5] % c] = 0.0                                       # below the clip
    off = 1 if misaligned else 0

    def dev(a):
        t = torch.zeros(a.size + 4 * a.shape[-1] if a.ndim == 2 else a.size + 4, dtype=torch.from_numpy(a).dtype, device=DEV)
        v = t[off:off + a.size]
        v.copy_(torch.from_numpy(a).reshape(-1))
        assert (v.data_ptr() % 16 != 0) == misaligned or a.ndim == 2
        return v.view(a.shape)
    d_metric, d_labels, d_pred, d_mean = dev(metric), dev(labels), dev(pred), dev(mean)
    valid = (labels >= 0) & (labels < c)
    ref_hist = _np_hist(metric[valid], (pred[valid] != labels[valid]).astype(np.int64), m, o)
    ref_counts = np.bincount(labels[valid], minlength=c)
    terms = -np.log(np.clip(mean[valid, labels[valid]].astype(np.float64), 1e-10, 1.0))
    ref_nll = np.bincount(labels[valid], weights=terms, minlength=c)
    t = ops.uncertainty_stats(d_metric, d_pred, d_labels, c, mean_prob=d_mean, mantissa_bits=m, octaves=o)
    assert np.array_equal(t['hist'].cpu().numpy(), ref_hist)
    assert ref_hist.sum() == valid.sum() and ref_hist[0].sum() > 1000 and ref_hist[1].sum() > 1000
    assert np.array_equal(t['counts'].cpu().numpy(), ref_counts)
    err = np.abs(t['nll'].cpu().numpy() - ref_nll)
    bound = ref_counts * R_LOG * LN_CLIP
    print('M=%d octaves=%d misaligned=%s: NLL |error| max %.3g, bound min %.3g' % (m, o, misaligned, err.max(), bound.min()))
    assert (err <= bound).all()
    # a second call accumulates; without mean_prob the NLL tables are not touched
    nll_before = t['nll'].clone()
    ops.uncertainty_stats(d_metric, d_pred, d_labels, c, mantissa_bits=m, octaves=o, tables=t)
    assert np.array_equal(t['hist'].cpu().numpy(), 2 * ref_hist)
    assert torch.equal(t['nll'], nll_before) and np.array_equal(t['counts'].cpu().numpy(), ref_counts)
    ops.uncertainty_stats(d_metric, d_pred, d_labels, c, mean_prob=d_mean, mantissa_bits=m, octaves=o, tables=t)
    assert np.array_equal(t['counts'].cpu().numpy(), 2 * ref_counts)
    assert (np.abs(t['nll'].cpu().numpy() - 2 * ref_nll) <= 2 * bound).all()
    # a fixed row: every pixel counts, whatever its label; labels and predictions may be absent
    for row in (0, 1):
        ref = _np_hist(metric, np.full(npix, row), m, o)
        assert np.array_equal(ops.uncertainty_stats(d_metric, d_pred, d_labels, c, fixed_row=row, mantissa_bits=m,
                                                    octaves=o)['hist'].cpu().numpy(), ref)
        assert np.array_equal(ops.uncertainty_stats(d_metric, None, None, c, fixed_row=row, mantissa_bits=m,
                                                    octaves=o)['hist'].cpu().numpy(), ref)


def test_bad_arguments_return_einval(gpu):
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd._lib import XvError
    v = torch.rand(64, device=DEV)
    p = torch.zeros(64, dtype=torch.int64, device=DEV)
    l = torch.zeros(64, dtype=torch.int32, device=DEV)
    mean = torch.rand((64, 12), device=DEV)
    for kwargs in (dict(mantissa_bits=2), dict(mantissa_bits=9), dict(octaves=7), dict(octaves=33), dict(fixed_row=2),
                   dict(mantissa_bits=8, octaves=32, mean_prob=mean)):    # (the last: 64 KB of histogram leave no room for the NLL)
        with pytest.raises(XvError, match='XV_EINVAL'):
            ops.uncertainty_stats(v, p, l, 12, **kwargs)
    with pytest.raises(XvError, match='XV_EINVAL'):
        ops.uncertainty_stats(v, p, l, 1)                                                     # C < 2
    with pytest.raises(XvError, match='XV_EINVAL'):
        ops.uncertainty_stats(v, None, None, 12)                                              # rows by correctness need both maps
    ops.uncertainty_stats(v, p, l, 12, mantissa_bits=8, octaves=32)                           # exactly 64 KB: fits
    S = torch.zeros((2, 4, 4, 12), device=DEV)
    b = torch.zeros(12, device=DEV)
    lab = torch.zeros((1, 16, 16), dtype=torch.int32, device=DEV)
    for kwargs in (dict(mantissa_bits=2), dict(octaves=33), dict(fixed_row=-2), dict(mantissa_bits=8, octaves=24),
                   dict(temperature=-1.0)):
        with pytest.raises(XvError, match='XV_EINVAL'):
            ops.mc_uncertainty_score(S, b, 1, 2, 2, 12, 2, labels=lab, **kwargs)
    with pytest.raises(XvError, match='XV_EINVAL'):
        ops.mc_uncertainty_score(S, b, 1, 2, 2, 12, 2)                                        # no labels, no fixed row
    with pytest.raises(XvError, match='XV_EINVAL'):
        ops.mc_uncertainty_score(torch.zeros((2, 4, 4, 4), device=DEV), torch.zeros(1, device=DEV), 1, 2, 2, 1, 2, labels=lab)
    with pytest.raises(ValueError):
        ops.mc_uncertainty_score(S, b, 1, 2, 2, 12, 3, labels=lab)                            # S holds 2 images, not 3


# ---- 2. the scoring head ------------------------------------------------------------------------------------------------------

def _head_inputs(c, T, n, hi, wi, seed, kind, wscale=0.3):
    """T n images of 1/8-resolution features, sample-major (the recipe of tests/test_bayesian_fcn_gpu.py): 'dropped' = ONE
    random map dropped T times with different seeds (what MC dropout at 'features' gives), 'same' = T copies of it."""
    from modular_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    ws = (torch.randn((U, c), generator=g) * wscale).to(DEV)
    bs = torch.randn(c, generator=g).to(DEV)
    one = ops.Act.from_dense((torch.rand((n, hi, wi, U), generator=g) * 2).to(DEV))
    f = ops.Act(T * n, hi, wi, U, DEV)
    for t in range(T):
        src = one if kind == 'same' else ops.dropout(one, 0.5, 77 * seed + 1000003 * t)
        f.images(t * n, (t + 1) * n).t.copy_(src.t)
    S = torch.zeros((T * n, hi + 2, wi + 2, cp), device=DEV)
    ops.score_lowres(f, ws, c, S)
    labels = torch.randint(-1, c + 1, (n, 8 * hi, 8 * wi), generator=g).to(torch.int32).to(DEV)
    return f, S, ws, bs, labels


def _maps_route(S, bs, labels, n, hi, wi, c, T, fixed_row=-1):
    """the tables of the maps route: the head writes every map, three statistics launches bin them"""
    from modular_semantic_segmentation_amd import ops
    out = ops.mc_uncertainty_head(S, bs, n, hi, wi, c, T, want_mean=True, want_entropy=True, want_cond_entropy=True,
                                  want_variance=True)
    t = ops.uncertainty_tables(c, S.device, 3)
    for i, key in enumerate(METRICS):
        ops.uncertainty_stats(out[key], out['label'], labels, c, mean_prob=out['mean'] if i == 0 and labels is not None else None, fixed_row=fixed_row,
                              tables={'hist': t['hist'][i], 'nll': t['nll'], 'counts': t['counts']})
    return t, out


def _assert_tables_equal(a, b, what):
    assert torch.equal(a['hist'], b['hist']), what
    assert torch.equal(a['counts'], b['counts']), what
    assert torch.allclose(a['nll'], b['nll'], rtol=1e-9, atol=0), what


@pytest.mark.parametrize('c', [12, 16])
@pytest.mark.parametrize('T', [1, 5, 10])
def test_scoring_head_equals_the_maps_route(gpu, c, T):
    from modular_semantic_segmentation_amd import ops
    n, hi, wi = 2, 6, 9
    f, S, ws, bs, labels = _head_inputs(c, T, n, hi, wi, seed=3 * c + T, kind='dropped')
    ref, out = _maps_route(S, bs, labels, n, hi, wi, c, T)
    got = ops.mc_uncertainty_score(S, bs, n, hi, wi, c, T, labels=labels)
    _assert_tables_equal(got, ref, (c, T))
    nvalid = int(((labels >= 0) & (labels < c)).sum())
    assert got['hist'].sum().item() == 3 * nvalid and got['counts'].sum().item() == nvalid
    assert got['hist'][:, 0].sum().item() > 0 and got['hist'][:, 1].sum().item() > 0
    if T == 1:
        assert got['hist'][2, :, 1:].sum().item() == 0                       # one sample: no variance
        assert torch.equal(got['hist'][0], got['hist'][1])                   # entropy == cond_entropy bit for bit
    else:
        assert (got['hist'][2].sum(0) > 0).sum().item() > 10
    # a second call accumulates
    ops.mc_uncertainty_score(S, bs, n, hi, wi, c, T, labels=labels, tables=got)
    assert torch.equal(got['hist'], 2 * ref['hist']) and torch.equal(got['counts'], 2 * ref['counts'])
    # a fixed row takes every pixel; without labels nothing else is touched
    ref1, _ = _maps_route(S, bs, None, n, hi, wi, c, T, fixed_row=1)
    got1 = ops.mc_uncertainty_score(S, bs, n, hi, wi, c, T, fixed_row=1)
    assert torch.equal(got1['hist'], ref1['hist']) and got1['hist'][:, 0].sum().item() == 0
    assert got1['hist'].sum().item() == 3 * labels.numel() and got1['counts'].sum().item() == 0
    # other bin shapes
    for m, o in ((3, 8), (6, 32)):
        a = ops.mc_uncertainty_score(S, bs, n, hi, wi, c, T, labels=labels, mantissa_bits=m, octaves=o)
        for i, key in enumerate(METRICS):
            b = ops.uncertainty_stats(out[key], out['label'], labels, c, mantissa_bits=m, octaves=o)
            assert torch.equal(a['hist'][i], b['hist']), (m, o, key)


@pytest.mark.parametrize('c', [12, 16])
def test_scoring_head_degenerate_samples(gpu, c):
    """identical samples: the variance is exactly 0 -- all of it in bin 0"""
    from modular_semantic_segmentation_amd import ops
    n, hi, wi, T = 2, 4, 6, 5
    f, S, ws, bs, labels = _head_inputs(c, T, n, hi, wi, seed=5 + c, kind='same')
    ref, _ = _maps_route(S, bs, labels, n, hi, wi, c, T)
    got = ops.mc_uncertainty_score(S, bs, n, hi, wi, c, T, labels=labels)
    _assert_tables_equal(got, ref, c)
    assert got['hist'][2, :, 1:].sum().item() == 0 and got['hist'][2, :, 0].sum().item() == got['counts'].sum().item()


@pytest.mark.parametrize('c', [12, 16])
def test_power_of_two_temperatures_are_exact(gpu, c):
    from modular_semantic_segmentation_amd import ops
    n, hi, wi, T = 2, 6, 9, 5
    f, S, ws, bs, labels = _head_inputs(c, T, n, hi, wi, seed=40 + c, kind='dropped')
    for temp, scale in ((2.0, 0.5), (0.5, 2.0)):
        ref, _ = _maps_route((S * scale).contiguous(), bs * scale, labels, n, hi, wi, c, T)
        got = ops.mc_uncertainty_score(S, bs, n, hi, wi, c, T, labels=labels, temperature=temp)
        _assert_tables_equal(got, ref, (c, temp))
    plain = ops.mc_uncertainty_score(S, bs, n, hi, wi, c, T, labels=labels)
    assert not torch.equal(plain['hist'], got['hist'])


def test_temperature_against_float64(gpu):
    from modular_semantic_segmentation_amd import ops
    c, T, n, hi, wi, temp = 12, 5, 2, 12, 16, 1.7
    f, S, ws, bs, labels = _head_inputs(c, T, n, hi, wi, seed=99, kind='dropped', wscale=0.1)
    got = ops.mc_uncertainty_score(S, bs, n, hi, wi, c, T, labels=labels, temperature=temp)
    # the fp32 logits of every sample from the unfused decoder head (the bits of the head's own), then float64
    x = torch.stack([ops.decoder_head_fwd(f.images(t * n, (t + 1) * n), ws, bs, c, want_score=True,
                                          want_label=False)['score'].clone() for t in range(T)], 0).double().cpu().numpy()
    xmax = np.abs(x).max() / temp
    rho = (4 * xmax + 4) * 2.0 ** -23 + c * EPS
    z = x / temp
    p = np.exp(z - z.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    lnc = math.log(c)

    def ent(q):
        return -(q * np.log(np.clip(q, 1e-10, 1.0))).sum(-1) / lnc
    mean = p.mean(0)
    var_c = (p * p).mean(0) - mean * mean
    ref = {'entropy': ent(mean), 'cond_entropy': ent(p).mean(0), 'variance': var_c.sum(-1)}
    per_sample = (c * (2.0 ** -23 + 3 * EPS) / math.e + (c - 1) * lnc * EPS) / lnc + 2 * EPS
    tol = {'entropy': per_sample + np.abs(np.log(np.clip(mean, 1e-10, 1.0)) + 1).sum(-1) * (T + 1) * EPS / lnc +
           rho * (ref['entropy'] + 1 / lnc),
           'cond_entropy': per_sample + (T + 1) * EPS + rho * (ref['cond_entropy'] + 1 / lnc),
           'variance': 1e-5 * ref['variance'] + 1e-9 + 2 * rho / T * (np.abs(p - mean) * p).sum((0, -1))}
    lab = labels.cpu().numpy()
    valid = (lab >= 0) & (lab < c)
    edges = um.bin_edges()[1:-1]
    hist = got['hist'].cpu().numpy()
    for i, key in enumerate(METRICS):
        v, t = ref[key][valid], tol[key][valid]
        j = np.clip(np.searchsorted(edges, v), 1, len(edges) - 1)
        near = np.minimum(np.abs(v - edges[j - 1]), np.abs(v - edges[j])) <= t
        share = near.mean()
        cum = np.cumsum(hist[i].sum(0))
        cum_ref = np.cumsum(np.bincount(um.bin_index(v.astype(np.float32)), minlength=hist.shape[-1]))
        worst = np.abs(cum - cum_ref).max()
        print('%s: %d of %d pixels within their tolerance of a bin edge (share %.4f); cumulative counts differ by at most %d'
              % (key, near.sum(), near.size, share, worst))
        assert share <= 0.01, key
        assert cum[-1] == cum_ref[-1] == valid.sum()
        assert worst <= near.sum(), key
    # NLL: independent of the argmax
    pl = np.take_along_axis(mean, np.clip(lab, 0, c - 1)[..., None], -1)[..., 0][valid]
    term = -np.log(np.clip(pl, 1e-10, 1.0))
    bound = R_LOG * term + rho + (T + 1) * EPS / pl
    ref_nll = np.bincount(lab[valid], weights=term, minlength=c)
    nll_bound = np.bincount(lab[valid], weights=bound, minlength=c)
    err = np.abs(got['nll'].cpu().numpy() - ref_nll)
    print('NLL |error| / bound, worst class: %.3g' % (err / nll_bound).max())
    assert np.array_equal(got['counts'].cpu().numpy(), np.bincount(lab[valid], minlength=c))
    assert (err <= nll_bound).all()


# ---- 3. the model -------------------------------------------------------------------------------------------------------------

C = 12
DESC = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, C)


def _model(T=4, rate=0.5, seed=1, **extra):
    """random weights in the recipe of tests/test_bayesian_fcn_gpu.py (activations that neither die nor overflow)"""
    from modular_semantic_segmentation_amd import get_model
    net = get_model('bayesian_fcn')('rgb', DESC, 'rgb', num_units=U, dropout_rate=rate, num_samples=T, seed=seed, batchsize=2,
                                    **extra)
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


def _data(n, seed, h=128, w=192):
    rng = np.random.default_rng(seed)
    return {'rgb': rng.integers(0, 256, (n, h, w, 3)).astype(np.float32),
            'labels': rng.integers(-1, C, (n, h, w)).astype(np.int32)}


def _exact_auroc(neg, pos):
    allv = np.concatenate([neg, pos]).astype(np.float64)
    _, inv, cnt = np.unique(allv, return_inverse=True, return_counts=True)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rank = (start + (cnt + 1) / 2.0)[inv]
    n, p = len(neg), len(pos)
    return (rank[n:].sum() - p * (p + 1) / 2.0) / (n * float(p))


def test_model_tables_equal_the_maps_route(gpu):
    from modular_semantic_segmentation_amd import ops
    data = _data(3, 11)                                               # two batches, the second of one image
    t = _model().uncertainty_tables(data)
    assert t['metrics'] == METRICS and t['hist'].shape == (3, 2, 768) and t['edges'].shape == (769,)
    maps = _model().predict_uncertainty(data)                         # the same seed and pass counter: the same masks
    lab = data['labels']
    valid = lab >= 0
    wrong = (maps['label'][valid] != lab[valid]).astype(np.int64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    for i, key in enumerate(METRICS):
        assert np.array_equal(t['hist'][i], _np_hist(maps[key][valid], wrong)), key
        s = ops.uncertainty_stats(dev(maps[key]), dev(maps['label']), dev(lab), C, mean_prob=dev(maps['mean']))
        assert np.array_equal(s['hist'].cpu().numpy(), t['hist'][i]), key
    assert np.array_equal(s['counts'].cpu().numpy(), t['counts']) and t['counts'].sum() == valid.sum()
    assert np.allclose(s['nll'].cpu().numpy(), t['nll_sum'], rtol=1e-9, atol=0)
    # the other methods are views of these tables (fresh models: the same masks)
    nll, counts = _model().nll_score(data)
    assert np.array_equal(counts, t['counts']) and np.allclose(nll, t['nll_sum'] / t['counts'], rtol=1e-9, atol=0)
    dist, edges = _model().value_distribution(data, 'variance')
    assert np.array_equal(dist, t['hist'][2].sum(0)) and np.array_equal(edges, t['edges'])
    for key in METRICS:
        fpr, tpr, auroc, thr = _model().misclassification_detection_score(data, key)
        assert (np.diff(fpr) >= 0).all() and (np.diff(tpr) >= 0).all() and fpr[-1] == 1 and tpr[-1] == 1
        assert fpr[0] == 0 and tpr[0] == 0 and (np.diff(thr) < 0).all()
        exact = _exact_auroc(maps[key][valid][wrong == 0], maps[key][valid][wrong == 1])
        bound = um.auroc_tie_bound(t['hist'][METRICS.index(key)])
        print('%s: AUROC %.6f, exact %.6f, tie bound %.3g' % (key, auroc, exact, bound))
        assert abs(auroc - exact) <= bound + 1e-12
    with pytest.raises(UserWarning):
        _model().misclassification_detection_score(data, 'mutual_information')


def test_model_temperature_search_and_ood(gpu):
    from modular_semantic_segmentation_amd import experiments
    data = _data(3, 12)
    net = _model()
    calls = []
    real = net.engine.mc_sample_scores
    net.engine.mc_sample_scores = lambda *a, **k: calls.append(1) or real(*a, **k)
    res = net.temperature_search(data, [1, 1.7])
    assert len(calls) == 2                                            # the convolutions ran once per batch, not per temperature
    assert [r['temperature'] for r in res] == [1.0, 1.7] and sorted(res[0]['auroc']) == sorted(METRICS)
    plain = _model().uncertainty_tables(data)
    hot_net = _model(temperature_scaling=1.7)
    hot = hot_net.uncertainty_tables(data)
    for got, ref in ((res[0]['tables'], plain), (res[1]['tables'], hot)):
        assert np.array_equal(got['hist'], ref['hist']) and np.array_equal(got['counts'], ref['counts'])
        assert np.allclose(got['nll_sum'], ref['nll_sum'], rtol=1e-9, atol=0)
    assert not np.array_equal(plain['hist'], hot['hist'])
    assert np.array_equal(_model().uncertainty_tables(data, temperature=1.7)['hist'], hot['hist'])
    with pytest.raises(NotImplementedError, match='temperature_scaling'):
        hot_net.predict(data)
    with pytest.raises(NotImplementedError, match='temperature_scaling'):
        hot_net.predict_uncertainty(data)
    # out of distribution: every pixel of `data` in row 0, every pixel of the foreign set in row 1
    ood = {'rgb': np.random.default_rng(5).normal(128, 90, (2, 128, 192, 3)).astype(np.float32)}
    fpr, tpr, auroc, thr = _model().out_of_distribution_detection_score(data, 'entropy', ood)
    assert fpr[-1] == 1 and tpr[-1] == 1 and 0 <= auroc <= 1
    r = experiments.evaluate_uncertainty(_model(), data, 'entropy', benchmark='out_of_distribution', print_results=False,
                                         ood_data=ood)
    assert r['AUROC'] == auroc
    # measure_metrics makes one pass for the NLL and one per metric, each with new masks: passes 1 and 2 of a fresh model
    twice = _model()
    first, second = twice.uncertainty_tables(data), twice.uncertainty_tables(data)
    assert np.array_equal(first['hist'], plain['hist']) and not np.array_equal(second['hist'], first['hist'])
    m = experiments.measure_metrics(_model(), data, ['entropy'])
    assert np.array_equal(m['class_counts'], plain['counts'])
    assert np.allclose(m['nll'], plain['nll_sum'] / plain['counts'], rtol=1e-9, atol=0)
    assert np.array_equal(m['entropy'][0], second['hist'][0].sum(0)) and np.array_equal(m['entropy'][1], plain['edges'])
