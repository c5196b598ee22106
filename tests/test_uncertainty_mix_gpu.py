"""Uncertainty-weighted Dirichlet fusion (uncertainty_dirichlet_mix.py; get_model('uncertainty_mix')): the pixel dropout of the
input, FcnEngine.mc_input_scores against sequential single passes, the moments pass against the variance head and a float64
restatement, the fusion head and the functional fusion against a float64 restatement of the mix / parameter / likelihood /
score steps, the two limits mix = 0 and mix = 1, and the model end to end at 768x384.

The score bound.  The restatement is evaluated in float64 on the head's OWN float32 probabilities, mvar and vmax, so only the
steps from the mix weight on are under test.  Per pixel and class the bound is K * 2^-24 * M, M the sum of the absolute values of
every term of the likelihood of both experts ((alpha - 1) log p per j, lgamma(sum alpha), lgamma(alpha) per j), computed in
the restatement.  The same formulas in float32 on the CPU (torch.lgamma, torch.log; 1e5 - 2e5 random pixels, mix ~ U(0, 1))
measure K = 3.2 - 3.8 for C = 3 .. 16; the kernel is held to K = 16: four times the float32-CPU reference, for another lgamma
/ log implementation and summation order.  Labels must equal the restatement's argmax wherever its top-2 gap exceeds twice the
bound, and at least 0.99 of the pixels must be that clear (the float32-CPU check gives > 0.9999 for these inputs).

The model test restates the variance too, in float64 from a twin's sequential passes, and holds the labels on the pixels that
are clear by the same criterion (gap > 2 * 16 * 2^-24 * M).  There the kernel's mvar and vmax carry their own float32 error
(the moments test holds each to rtol 1e-5), which moves a score by up to 2e-5 * mix * D, D = sum_e [sum_j |1 + delta_jc - A_jc|
(|log p_j| + |digamma(alpha_jc)|) + |C + 1 - sum_j A_jc| |digamma(sum_j alpha_jc)|] being the absolute terms of d score / d mix.
The test PRINTS the clear share and the number of differing labels with that term added to the bound as well, for
information; it asserts the criterion without it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo

C, U = 12, 64
DEV = 'cuda:0'
K_BOUND = 16.0
EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


# ---- 1. pixel dropout of the input -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('cin', [1, 3])
@pytest.mark.parametrize('T', [1, 4])
@pytest.mark.parametrize('rate', [0.25, 0.5])
def test_dropout_pixels(gpu, n, cin, T, rate):
    from modular_semantic_segmentation_amd import ops
    h, w = 256, 400                                              # 102 400 pixels per image
    g = torch.Generator().manual_seed(1000 * n + 10 * cin + T)
    x = (torch.rand((n, h, w, cin), generator=g) + 0.5).to(DEV)  # no zeros: a zero in the output is a dropped pixel
    seed0, stride = 0xfedcba9876543210 + 13 * T + cin, 1000003
    y = torch.full(((T + 1) * n, h, w, cin), float('nan'), device=DEV)
    assert ops.dropout_pixels_samples(x, T, rate, seed0, stride, y=y) is y
    assert torch.equal(y[:n], x)                                 # the plain slot
    scale = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(rate, dtype=torch.float32))
    for t in range(T):
        slot = y[(t + 1) * n:(t + 2) * n]
        kept, dropped = (slot != 0).all(-1), (slot == 0).all(-1)
        assert bool((kept | dropped).all())                      # every channel of a pixel shares its fate
        assert torch.equal(slot[kept], (x * scale.to(DEV))[kept])          # x * fl(1 / (1 - rate)), bit for bit
        one = torch.full((n, h, w, cin), float('nan'), device=DEV)
        ops.dropout_pixels(x, rate, (seed0 + t * stride) & 0xffffffffffffffff, y=one)
        assert torch.equal(slot, one), t                         # the single-pass form with that slot's seed
        share, npx = kept.float().mean().item(), kept.numel()
        assert npx >= 10 ** 5
        assert abs(share - (1 - rate)) <= 5 * (rate * (1 - rate) / npx) ** 0.5, (t, share)
    if T > 1:
        assert len({y[(t + 1) * n:(t + 2) * n].ne(0).sum().item() for t in range(T)}) > 1      # the samples differ
    # without the plain slot, and dealt out over two calls: the same bits
    z = torch.full((T * n, h, w, cin), float('nan'), device=DEV)
    a = (T + 1) // 2
    ops.dropout_pixels_samples(x, a, rate, seed0, stride, plain=False, y=z[:a * n])
    if T > a:
        ops.dropout_pixels_samples(x, T - a, rate, seed0 + a * stride, stride, plain=False, y=z[a * n:])
    assert torch.equal(z, y[n:])
    one_call = ops.dropout_pixels_samples(x, T, rate, seed0, stride, plain=False)
    assert torch.equal(one_call, z)
    # the mask is a function of (seed, pixel) alone: another channel count draws the same pixels
    other = torch.ones((n, h, w, 4 - cin), device=DEV)
    m = ops.dropout_pixels(other, rate, seed0)
    assert torch.equal(m[..., 0] != 0, y[n:2 * n, ..., 0] != 0)


def test_dropout_pixels_refuses_bad_arguments(gpu):
    from modular_semantic_segmentation_amd import _lib, ops
    x = torch.ones((1, 8, 8, 3), device=DEV)
    with pytest.raises(_lib.XvError):
        ops.dropout_pixels(x, 1.0, 1)
    with pytest.raises(_lib.XvError):
        ops.dropout_pixels_samples(x, 0, 0.5, 1, 1)
    with pytest.raises(ValueError):
        ops.dropout_pixels_samples(x, 2, 0.5, 1, 1, y=torch.empty((2, 8, 8, 3), device=DEV))    # plain slot missing
    both = torch.ones((2, 8, 8, 3), device=DEV)
    with pytest.raises(_lib.XvError):
        ops.dropout_pixels(both[:1], 0.5, 1, y=both[:1])                                         # in place


# ---- 2. the engine's sampler -----------------------------------------------------------------------------------------------

def _engine(prefix='rgb', cin=3, seed=9, first=0.02):
    from modular_semantic_segmentation_amd.fcn import FcnEngine
    w = fo.init_fcn_weights(prefix, cin, U, C, seed=seed, bias_scale=0.02)
    w['%s/conv1_1/kernel' % prefix] *= first
    for k in w:
        if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] *= 1.6
    return FcnEngine(prefix, cin, U, C, w, device=DEV)


@pytest.mark.parametrize('n', [1, 2])
def test_mc_input_scores_equal_sequential_single_passes(gpu, n):
    from modular_semantic_segmentation_amd import ops
    eng = _engine()
    T, rate, seed = 3, 0.5, 11
    x = torch.from_numpy(np.random.default_rng(3 + n).integers(0, 256, (n, 64, 96, 3)).astype(np.float32)).to(DEV)
    plain = eng.lowres_scores(x)[0].clone()
    seq = [eng.lowres_scores(ops.dropout_pixels(x, rate, eng._dropout_seed_of(seed, p, 'input_drop')))[0].clone()
           for p in range(2 * T)]
    eng._dropout_pass = 0
    S, geo = eng.mc_input_scores(x, T, rate, seed)                    # default chunk cap: one chunk
    assert geo == (n, 8, 12) and eng._dropout_pass == T
    assert tuple(S.shape) == ((T + 1) * n, 10, 14, C)
    assert torch.equal(S[:n], plain)
    for t in range(T):
        assert torch.equal(S[(t + 1) * n:(t + 2) * n], seq[t]), t
    assert not torch.equal(S[n:2 * n], plain)
    S2, _ = eng.mc_input_scores(x, T, rate, seed)                     # passes T .. 2T-1
    assert eng._dropout_pass == 2 * T
    for t in range(T):
        assert torch.equal(S2[(t + 1) * n:(t + 2) * n], seq[T + t]), t
    eng._dropout_pass, eng.mc_chunk_images = 0, n                     # one sample per launch: T chunks
    S3, _ = eng.mc_input_scores(x, T, rate, seed)
    assert torch.equal(S3[:n], plain)
    for t in range(T):
        assert torch.equal(S3[(t + 1) * n:(t + 2) * n], seq[t]), t
    eng._dropout_pass, eng.mc_chunk_images = 0, 2 * n                 # two samples, then one
    S4, _ = eng.mc_input_scores(x, T, rate, seed)
    for t in range(T):
        assert torch.equal(S4[(t + 1) * n:(t + 2) * n], seq[t]), t


def test_mc_input_scores_refuses_what_it_cannot_sample(gpu):
    eng = _engine()
    x = torch.zeros((1, 64, 96, 3), device=DEV)
    with pytest.raises(ValueError):
        eng.mc_input_scores(x, 0, 0.5, 1)
    eng.set_dropout(['pool3'], 0.5, 1)
    with pytest.raises(ValueError):
        eng.mc_input_scores(x, 2, 0.5, 1)
    eng.set_dropout([], 0.0)
    eng.affine['upscore'] = (None, None)                               # an un-commuted head
    with pytest.raises(NotImplementedError):
        eng.mc_input_scores(x, 2, 0.5, 1)


# ---- 3. - 5. moments, fusion head, functional fusion -------------------------------------------------------------------------

def _random_head_inputs(c, T, n, hi, wi, seed, same=False):
    """(T+1) n images of random 1/8-resolution features -> their low-resolution scores S and the features (for the unfused
    decoder head); same=True: every slot holds the same features."""
    from modular_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    ws = [(torch.randn((U, c), generator=g) * 0.3).to(DEV) for _ in range(2)]
    bs = [torch.randn(c, generator=g).to(DEV) for _ in range(2)]
    feats, S = [], []
    for e in range(2):
        if same:
            dense = (torch.rand((n, hi, wi, U), generator=g) * 2).repeat(T + 1, 1, 1, 1)
        else:
            dense = torch.rand(((T + 1) * n, hi, wi, U), generator=g) * 2
        f = ops.Act.from_dense(dense.to(DEV))
        s = torch.zeros(((T + 1) * n, hi + 2, wi + 2, cp), device=DEV)
        ops.score_lowres(f, ws[e], c, s)
        feats.append(f)
        S.append(s)
    return feats, S, ws, bs


def _slot_probs(feats, ws, bs, c, T, n):
    from modular_semantic_segmentation_amd import ops
    return [[ops.decoder_head_fwd(feats[e].images(t * n, (t + 1) * n), ws[e], bs[e], c, want_prob=True,
                                  want_label=False)['prob'].clone() for t in range(T + 1)] for e in range(2)]


def _params(c, seed):
    """A = 0.3 + 2 U(0, 1) + 8 I per expert (A[j, c]), class counts and the two priors under test"""
    from modular_semantic_segmentation_amd.dirichlet_mix import class_prior_vector
    g = torch.Generator().manual_seed(seed)
    A = [(0.3 + 2 * torch.rand((c, c), generator=g) + 8 * torch.eye(c)).float().numpy() for _ in range(2)]
    counts = torch.randint(1, 1000, (c,), generator=g).numpy()
    priors = {'uniform': class_prior_vector(counts, 'uniform', c), 'data': class_prior_vector(counts, 'data', c)}
    return A, counts, priors


def _tables(A, prior):
    params = torch.from_numpy(np.stack(A).astype(np.float32)).to(DEV)
    logprior = torch.from_numpy(np.log(np.float32(1e-20) + np.asarray(prior, np.float32), dtype=np.float32)).to(DEV)
    return params, logprior


def _restatement(probs, mvar, vmax, A, prior):
    """float64 mix, parameters, likelihood and score: probs [2][..., C], mvar [2][...], vmax [2], A two [C, C] arrays (A[j, c]),
    prior [C] -> (score [..., C], M [..., C]: the sum of the absolute likelihood terms, dmix [..., C]: sum_e mix_e D_e, the absolute
    terms of d score / d mix weighted by mix)"""
    c = probs[0].shape[-1]
    std = (torch.ones((c, c)) + torch.eye(c)).double().to(DEV)
    score, M, dmix = 0.0, 0.0, 0.0
    for e in range(2):
        p = probs[e].double()
        p = p / p.sum(-1, keepdim=True)
        vm = vmax[e].double()
        mix = mvar[e].double() / vm if vm.item() > 0 else torch.zeros_like(mvar[e], dtype=torch.float64)
        Ae = torch.from_numpy(np.asarray(A[e], np.float32)).double().to(DEV)
        m = mix[..., None, None]
        alpha = Ae * (1 - m) + m * std                                   # [..., j, c]
        lp = torch.log(1e-20 + p)[..., :, None]                          # [..., j, 1]
        t1, t2, t3 = (alpha - 1) * lp, torch.lgamma(alpha.sum(-2)), torch.lgamma(alpha)
        score = score + t1.sum(-2) + t2 - t3.sum(-2)
        M = M + t1.abs().sum(-2) + t2.abs() + t3.abs().sum(-2)
        D = ((std - Ae).abs() * (lp.abs() + torch.digamma(alpha).abs())).sum(-2) + \
            (c + 1 - Ae.sum(0)).abs() * torch.digamma(alpha.sum(-2)).abs()
        dmix = dmix + mix[..., None] * D
    return score + torch.log(1e-20 + torch.from_numpy(np.asarray(prior, np.float64)).to(DEV)), M, dmix


def _check_scores(tag, score, label, ref, bound, min_clear):
    err = (score.double() - ref).abs()
    ratio = (err / bound).max().item()
    top2 = ref.topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * bound.amax(-1)
    share = clear.float().mean().item()
    print('%s: max |score - float64| / bound = %.3f (K = %.2f of 16), clear share %.5f' % (tag, ratio, ratio * K_BOUND, share))
    assert ratio <= 1.0, tag
    assert share >= min_clear, (tag, share)
    assert torch.equal(label[clear], ref.argmax(-1)[clear]), tag


@pytest.mark.parametrize('c', [3, 5, 12, 14, 16, 20, 30, 32])
@pytest.mark.parametrize('T', [2, 7])
def test_uncertainty_moments(gpu, c, T):
    from modular_semantic_segmentation_amd import ops
    n, hi, wi = 2, 5, 7
    feats, S, ws, bs = _random_head_inputs(c, T, n, hi, wi, seed=31 * c + T)
    mvar, vmax = ops.uncertainty_moments(S[0], S[1], bs[0], bs[1], n, hi, wi, c, T)
    vh = ops.variance_head(S[0], S[1], bs[0], bs[1], n, hi, wi, c, T, want_variance=True)
    assert torch.equal(mvar, vh['variance'])                           # the variance head's bits
    probs = _slot_probs(feats, ws, bs, c, T, n)
    for e in range(2):
        v = torch.stack([probs[e][t].double() for t in range(1, T + 1)], 0).var(0, unbiased=False)
        print('C=%d T=%d expert %d: vmax %.9g, float64 %.9g' % (c, T, e, vmax[e].item(), v.amax().item()))
        assert torch.allclose(vmax[e].double(), v.amax(), rtol=1e-5, atol=1e-9)
        assert torch.allclose(mvar[e].double(), v.mean(-1), rtol=1e-5, atol=1e-9)
        assert vmax[e].item() >= mvar[e].max().item() > 0
    # stale contents of vmax are cleared by the entry point: a second call gives the same values
    mvar2, vmax2 = ops.uncertainty_moments(S[0], S[1], bs[0], bs[1], n, hi, wi, c, T)
    assert torch.equal(vmax2, vmax) and torch.equal(mvar2, mvar)


@pytest.mark.parametrize('c', [5, 12])
def test_uncertainty_moments_identical_samples(gpu, c):
    from modular_semantic_segmentation_amd import ops
    n, hi, wi, T = 2, 4, 6, 5
    _, S, _, bs = _random_head_inputs(c, T, n, hi, wi, seed=5 + c, same=True)
    mvar, vmax = ops.uncertainty_moments(S[0], S[1], bs[0], bs[1], n, hi, wi, c, T)
    assert torch.count_nonzero(mvar).item() == 0 and torch.count_nonzero(vmax).item() == 0


@pytest.mark.parametrize('c', [3, 5, 12, 14, 16, 20, 30, 32])
@pytest.mark.parametrize('T', [2, 7])
def test_uncertainty_dirichlet_head(gpu, c, T):
    from modular_semantic_segmentation_amd import ops
    n, hi, wi = 2, 5, 7
    feats, S, ws, bs = _random_head_inputs(c, T, n, hi, wi, seed=17 * c + T)
    mvar, vmax = ops.uncertainty_moments(S[0], S[1], bs[0], bs[1], n, hi, wi, c, T)
    A, counts, priors = _params(c, seed=c + T)
    plain = _slot_probs(feats, ws, bs, c, 0, n)
    for name, prior in priors.items():
        params, logprior = _tables(A, prior)
        out = ops.uncertainty_dirichlet_head(S[0], S[1], bs[0], bs[1], n, hi, wi, c, mvar, vmax, params, logprior,
                                             want_score=True, want_probs=True, want_mix=True)
        for e in range(2):
            assert torch.equal(out['probs'][e], plain[e][0]), e       # the plain slot: decoder_head_kernel's bits
            q = mvar[e] / vmax[e]                                     # float32 division: correctly rounded
            ulps = (out['mix'][e].view(torch.int32) - q.view(torch.int32)).abs().max().item()
            assert ulps <= 1, (e, ulps)
            assert 0 < out['mix'][e].max().item() <= 1
        ref, M, _ = _restatement(out['probs'], mvar, vmax, A, prior)
        _check_scores('head C=%d T=%d prior=%s' % (c, T, name), out['fused_score'], out['label'], ref, K_BOUND * EPS * M, 0.99)
        # the label alone: the same labels
        only = ops.uncertainty_dirichlet_head(S[0], S[1], bs[0], bs[1], n, hi, wi, c, mvar, vmax, params, logprior)
        assert set(only) == {'label'} and torch.equal(only['label'], out['label'])
        # the functional fusion on the head's materialised outputs: its scores and labels, bit for bit
        lab, score = ops.uncertainty_dirichlet_fuse([out['probs'][0], out['probs'][1]], mvar, vmax, params, logprior)
        assert torch.equal(score, out['fused_score'])
        assert torch.equal(lab, out['label'])
        lab2, none = ops.uncertainty_dirichlet_fuse([out['probs'][0], out['probs'][1]], mvar, vmax, params, logprior,
                                                    want_score=False)
        assert none is None and torch.equal(lab2, out['label'])


@pytest.mark.parametrize('c', [3, 12, 14, 32])
def test_uncertainty_weights_and_functional_fusion(gpu, c):
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd.uncertainty_dirichlet_mix import dirichlet_uncertainty_fusion
    g = torch.Generator().manual_seed(40 + c)
    shape = (2, 24, 40)
    unc = [(torch.rand(shape + (c,), generator=g) * 0.05).to(DEV) for _ in range(2)]
    mvar = torch.full((2,) + shape, float('nan'), device=DEV)
    vmax = torch.full((2,), float('nan'), device=DEV)
    for e in range(2):
        ops.uncertainty_weights(unc[e], mvar=mvar[e], vmax=vmax[e:e + 1])
        assert torch.equal(vmax[e], unc[e].amax())
        assert torch.allclose(mvar[e].double(), unc[e].double().mean(-1), rtol=1e-6, atol=0)
    m1, v1 = ops.uncertainty_weights(unc[1])
    assert torch.equal(m1, mvar[1]) and torch.equal(v1[0], vmax[1])
    if c > 16:
        return                                  # (the fusion's parameter grid stops at 16 classes here)
    probs = [torch.softmax(torch.randn(shape + (c,), generator=g), -1).to(DEV) for _ in range(2)]
    A, _, priors = _params(c, seed=c)
    params, logprior = _tables(A, priors['data'])
    _, parts = ops.uncertainty_dirichlet_fuse(probs, mvar, vmax, params, logprior, want_label=False)
    got = dirichlet_uncertainty_fusion(probs, A, unc, priors['data'])
    assert torch.equal(got, parts)
    ref, M, _ = _restatement(probs, mvar, vmax, A, priors['data'])
    _check_scores('functional C=%d' % c, got, got.argmax(-1), ref, K_BOUND * EPS * M, 0.99)


@pytest.mark.parametrize('c', [5, 12])
def test_limit_identical_samples_is_the_plain_dirichlet_fusion(gpu, c):
    """mix = 0 (max variance 0): the scores of ops.dirichlet_fuse on the same probabilities with sigma = 1"""
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd.dirichlet_mix import dirichlet_tables
    n, hi, wi, T = 2, 4, 6, 5
    _, S, _, bs = _random_head_inputs(c, T, n, hi, wi, seed=5 + c, same=True)
    mvar, vmax = ops.uncertainty_moments(S[0], S[1], bs[0], bs[1], n, hi, wi, c, T)
    A, counts, priors = _params(c, seed=2 * c)
    params, logprior = _tables(A, priors['data'])
    out = ops.uncertainty_dirichlet_head(S[0], S[1], bs[0], bs[1], n, hi, wi, c, mvar, vmax, params, logprior,
                                         want_score=True, want_probs=True, want_mix=True)
    assert torch.count_nonzero(out['mix']).item() == 0
    am1, lognorm, lp = dirichlet_tables(A, counts, 'data', 1.0)
    assert np.array_equal(lp, logprior.cpu().numpy())
    _, plain = ops.dirichlet_fuse([out['probs'][0].contiguous(), out['probs'][1].contiguous()], torch.from_numpy(am1).to(DEV),
                                  torch.from_numpy(lognorm).to(DEV), torch.from_numpy(lp).to(DEV), want_score=True)
    ref, M, _ = _restatement(out['probs'], mvar, vmax, A, priors['data'])
    bound = K_BOUND * EPS * M
    print('C=%d: |head - dirichlet_fuse| / bound = %.3f' % (c, ((out['fused_score'] - plain).abs().double() / bound).max().item()))
    assert ((out['fused_score'] - plain).abs().double() <= bound).all()
    _check_scores('mix=0 C=%d' % c, out['fused_score'], out['label'], ref, bound, 0.99)


@pytest.mark.parametrize('c', [5, 12])
def test_limit_full_uncertainty_forgets_the_parameters(gpu, c):
    """mvar = vmax everywhere (mix = 1): alpha = 1 + delta_jc whatever A holds"""
    from modular_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(c)
    shape = (2, 16, 24)
    probs = [torch.softmax(torch.randn(shape + (c,), generator=g), -1).to(DEV) for _ in range(2)]
    mvar = torch.full((2,) + shape, 0.0123, device=DEV)
    vmax = torch.full((2,), 0.0123, device=DEV)
    A1, _, priors = _params(c, seed=1)
    A2 = [a[::-1].copy() * 3 for a in A1]
    res = [ops.uncertainty_dirichlet_fuse(probs, mvar, vmax, *_tables(A, priors['uniform'])) for A in (A1, A2)]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], res[1][0])
    ref, M, _ = _restatement(probs, mvar, vmax, A1, priors['uniform'])
    _check_scores('mix=1 C=%d' % c, res[0][1], res[0][0], ref, K_BOUND * EPS * M, 0.99)


# ---- 6. the model -----------------------------------------------------------------------------------------------------------

DESC = ({'rgb': 'float32', 'depth': 'float32', 'labels': 'int32'},
        {'rgb': (None, None, 3), 'depth': (None, None, 1), 'labels': (None, None)}, C)
CFG = dict(modalities=['rgb', 'depth'], num_channels={'rgb': 3, 'depth': 1}, num_units=U, expert_model='fcn',
           class_prior='data', delta=1e-2, beta=1e-2)


def _rescale(net, seed):
    """the weight recipe of the other MC models' tests (activations that neither die nor overflow at 768x384)"""
    w = dict(net.variables)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith('/bias') and 'upscore' not in k:
            w[k] = (rng.standard_normal(w[k].shape) * 0.02).astype(np.float32)
        elif k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] = w[k] * 1.6
    w['rgb/conv1_1/kernel'] = w['rgb/conv1_1/kernel'] / 50.0
    w['depth/conv1_1/kernel'] = w['depth/conv1_1/kernel'] / 5000.0
    net.variables.update(w)
    net._variables_changed()
    return net


def _given_params():
    A, counts, _ = _params(C, seed=77)
    return {'rgb': A[0], 'depth': A[1], 'class_counts': counts}


def _model(T=5, rate=0.5, seed=1, batchsize=2, fitted=True, **extra):
    from modular_semantic_segmentation_amd import get_model
    if fitted:
        extra['dirichlet_params'] = _given_params()
    net = get_model('uncertainty_mix')(data_description=DESC, dropout_rate=rate, num_samples=T, seed=seed, batchsize=batchsize,
                                       **CFG, **extra)
    return _rescale(net, seed)


@pytest.mark.parametrize('n', [1, 2])
def test_uncertainty_mix_model_768x384(gpu, n):
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd.dirichlet_mix import class_prior_vector
    T, rate = 5, 0.5
    rng = np.random.default_rng(20 + n)
    data = {'rgb': rng.integers(0, 256, (n, 384, 768, 3)).astype(np.float32),
            'depth': rng.integers(0, 65536, (n, 384, 768, 1)).astype(np.float32),
            'labels': rng.integers(-1, C, (n, 384, 768)).astype(np.int32)}
    net = _model(T, rate)
    labels = net.predict(data)
    assert labels.shape == (n, 384, 768) and labels.dtype == np.int64
    # float64 restatement from sequential single passes of a twin's engines (same weights, same seeds, fresh pass counters)
    twin = _model(T, rate)
    probs, mvar, vmax = [], [], []
    for i, m in enumerate(twin.modalities):
        eng = twin.experts[m]
        x = torch.from_numpy(data[m]).to(DEV)
        smp = [eng.forward(ops.dropout_pixels(x, rate, eng._dropout_seed_of(twin._dropout_seed + i, t, 'input_drop')),
                           want=('prob',))['prob'].double() for t in range(T)]
        v = torch.stack(smp, 0).var(0, unbiased=False)
        del smp
        probs.append(eng.forward(x, want=('prob',))['prob'].clone())
        mvar.append(v.mean(-1))
        vmax.append(v.amax())
        del v
    given = _given_params()
    prior = class_prior_vector(given['class_counts'], 'data', C)
    ref, M, dmix = _restatement(probs, mvar, vmax, [given['rgb'], given['depth']], prior)
    top2 = ref.topk(2, -1).values
    gap = top2[..., 0] - top2[..., 1]
    want = ref.argmax(-1).cpu().numpy()
    clear = (gap > 2 * (K_BOUND * EPS * M).amax(-1)).cpu().numpy()                     # clear as in the head test
    wide = (gap > 2 * (K_BOUND * EPS * M + 2e-5 * dmix).amax(-1)).cpu().numpy()        # with the mix-error term (docstring)
    print('n=%d: clear share %.4f, %d labels differ there; with the mix-error term: share %.4f, %d differ' % (
        n, clear.mean(), (labels[clear] != want[clear]).sum(), wide.mean(), (labels[wide] != want[wide]).sum()))
    assert clear.mean() >= 0.5
    assert np.array_equal(labels[clear], want[clear])
    del ref, M, dmix
    # the same seed in a fresh model: the same labels; consecutive calls: new masks
    assert np.array_equal(_model(T, rate).predict(data), labels)
    v1 = net.predict(data, output_attr='variance')
    v2 = net.predict(data, output_attr='variance')
    assert v1.shape == (n, 2, 384, 768) and v1.dtype == np.float32
    assert not np.array_equal(v1, v2)
    assert v1.min() >= 0 and v1.max() <= 0.25
    mix = net.predict(data, output_attr='mix')
    assert mix.shape == (n, 2, 384, 768) and mix.dtype == np.float32 and mix.min() >= 0 and mix.max() <= 1
    score = net.predict(data, output_attr='fused_score')
    assert score.shape == (n, 384, 768, C) and score.dtype == np.float32 and np.isfinite(score).all()
    probs_out = net.predict(data, output_attr='probs')
    assert probs_out.shape == (n, 2, 384, 768, C) and probs_out.dtype == np.float32
    assert np.allclose(probs_out.sum(-1), 1.0, atol=1e-5)
    assert np.array_equal(probs_out[:, 0], probs[0].cpu().numpy())    # the plain pass does not depend on the masks
    for _ in range(5):
        net.predict(data)
    assert net._graph is None
    measures, cm = net.score(data)
    assert cm.shape == (C, C) and cm.sum() == (data['labels'] >= 0).sum()


def _fit_data(h=128, w=256, n=2):
    """blocky label maps and images whose colour / depth follow the label (the fit has something to find)"""
    rng = np.random.default_rng(h + 7)
    coarse = rng.integers(-1, C, (n, h // 32, w // 32))
    labels = np.repeat(np.repeat(coarse, 32, axis=1), 32, axis=2).astype(np.int32)
    palette = rng.integers(0, 256, (C + 1, 3)).astype(np.float32)
    dpal = rng.integers(0, 65536, (C + 1, 1)).astype(np.float32)
    rgb = np.clip(palette[labels] + rng.normal(0, 20, (n, h, w, 3)), 0, 255).astype(np.float32)
    depth = np.clip(dpal[labels] + rng.normal(0, 3000, (n, h, w, 1)), 0, 65535).astype(np.float32)
    return {'rgb': rgb, 'depth': depth, 'labels': labels}


def test_uncertainty_mix_fit_is_the_dirichlet_fit(gpu):
    from modular_semantic_segmentation_amd import get_model
    data = _fit_data()
    net = _model(fitted=False)
    with pytest.raises(UserWarning):
        net.predict(data)
    got = net.fit(data)
    twin = _rescale(get_model('dirichlet_fusion')(data_description=DESC, sigma=1.0, seed=1, batchsize=2, **CFG), 1)
    ref = twin.fit(data)
    assert np.array_equal(got['class_counts'], ref['class_counts'])
    for m in net.modalities:
        assert got[m].shape == (C, C) and np.all(got[m] > 0)
        # (the statistics are summed with float64 atomics: not bitwise reproducible)
        np.testing.assert_allclose(got[m], ref[m], rtol=1e-4, atol=1e-5, err_msg=m)
    labels = net.predict(data)
    assert labels.shape == data['labels'].shape and labels.min() >= 0 and labels.max() < C
