"""The fused head for two to four experts (xv_fused_head_multi_fwd / ops.fused_head_multi) on small maps.

The oracle is the unfused path on the same GPU: ops.decoder_head_from_scores per expert (labels for Bayes, `prob` for Dirichlet
and the mean), then ops.bayes_fuse / ops.dirichlet_fuse / ops.average_fuse.  tests/test_heads_fusion_edges_gpu.py holds those
kernels to float64 for up to four experts, so equality with them, label for label, is the whole numerical claim: no tolerance.
Inputs follow tests/test_fused_average_head_gpu.py::_host_case, extended to E experts."""
import pytest
import torch

DEV = 'cuda:0'
EXPERTS = [2, 3, 4]
MODES = [0, 1, 2]                                      # Bayes, Dirichlet, mean
MODE_NAMES = {0: 'bayes', 1: 'dirichlet', 2: 'mean'}
CLASSES = [2, 5, 12, 13, 32]                           # CM 4, 8 padded, 12 full, 16 padded, 32; Bayes with the decision table
#                                                        (C^E <= 1 024) and with the rows summed per pixel (4 experts x 32 classes)
GEOMETRIES = [(1, 3, 5), (3, 5, 4), (2, 7, 9)]         # (n, hi, wi); the last: eight workgroups of Bayes threads, one partial
SCALE = 3.0                                            # standard deviation of the low-resolution scores
SENTINEL = -7


def _host_case(c, geo, seed, experts):
    """zero-bordered low-resolution scores [n][hi+2][wi+2][CP] of `experts` experts and their biases"""
    n, hi, wi = geo
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    S = [torch.zeros((n, hi + 2, wi + 2, cp)) for _ in range(experts)]
    for t in S:
        t[:, 1:-1, 1:-1, :c] = torch.randn((n, hi, wi, c), generator=g) * SCALE
    bias = [torch.randn(c, generator=g) for _ in range(experts)]
    return S, bias


def _host_tables(c, experts, seed):
    """Bayes log-likelihoods [E][C][C] and log prior [C]; Dirichlet alpha - 1 [E][C][C], log normaliser [E][C]"""
    g = torch.Generator().manual_seed(1000 + seed)
    cond = torch.rand((experts, c, c), generator=g) + 0.05 + 2.0 * torch.eye(c)
    loglik = torch.log(1e-20 + cond / cond.sum(1, keepdim=True))
    prior = torch.rand(c, generator=g) + 0.1
    logprior = torch.log(prior / prior.sum())
    am1 = torch.rand((experts, c, c), generator=g) * 3.0 - 0.5 + 4.0 * torch.eye(c)
    lognorm = torch.randn((experts, c), generator=g)
    return dict(loglik=loglik.contiguous(), logprior=logprior.contiguous(), am1=am1.contiguous(), lognorm=lognorm.contiguous())


def _tables_for(mode, tables):
    """keyword arguments of ops.fused_head_multi"""
    if mode == 0:
        return dict(tab=tables['loglik'], logprior=tables['logprior'])
    if mode == 1:
        return dict(tab=tables['am1'], lognorm=tables['lognorm'], logprior=tables['logprior'])
    return {}


def _unfused(ops, S, bias, geo, c, mode, tables):
    """one decoder head per expert, then the fusion kernel"""
    n, hi, wi = geo
    outs = []
    for s, b in zip(S, bias):
        if mode == 0:
            t = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=DEV)
            ops.decoder_head_from_scores(s, b, n, hi, wi, c, label=t)
        else:
            t = torch.empty((n, 8 * hi, 8 * wi, c), dtype=torch.float32, device=DEV)
            ops.decoder_head_from_scores(s, b, n, hi, wi, c, prob=t)
        outs.append(t)
    if mode == 0:
        return ops.bayes_fuse(outs, tables['loglik'], tables['logprior'])[0]
    if mode == 1:
        return ops.dirichlet_fuse(outs, tables['am1'], tables['lognorm'], tables['logprior'])[0]
    return ops.average_fuse(outs)


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


@pytest.fixture(scope='module')
def inputs(gpu):
    """per (c, geo): device scores and biases of FOUR experts (E experts are the first E) and per (c, E) the tables; made
    once and left unchanged"""
    out = {}
    for c in CLASSES:
        for geo in GEOMETRIES:
            S, bias = _host_case(c, geo, 7 * c + geo[0], 4)
            out[(c, geo)] = ([t.to(DEV) for t in S], [t.to(DEV) for t in bias])
        for e in EXPERTS:
            out[(c, e)] = {k: v.to(DEV) for k, v in _host_tables(c, e, 10 * c + e).items()}
    return out


@pytest.fixture(scope='module')
def references(inputs):
    """the unfused path's labels per case, computed on first use and shared"""
    from modular_semantic_segmentation_amd import ops
    cache = {}

    def get(e, mode, c, geo):
        key = (e, mode, c, geo)
        if key not in cache:
            S, bias = inputs[(c, geo)]
            cache[key] = _unfused(ops, S[:e], bias[:e], geo, c, mode, inputs[(c, e)])
        return cache[key]
    return get


CASES = [(e, mode, c, geo) for e in EXPERTS for mode in MODES for c in CLASSES for geo in GEOMETRIES]
IDS = ['e%d-%s-c%d-n%dx%dx%d' % ((e, MODE_NAMES[mode], c) + geo) for e, mode, c, geo in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize('e,mode,c,geo', CASES, ids=IDS)
def test_labels_equal_the_unfused_path_on_every_pixel(inputs, references, e, mode, c, geo):
    from modular_semantic_segmentation_amd import ops
    S, bias = inputs[(c, geo)]
    ref = references(e, mode, c, geo)
    got = ops.fused_head_multi(S[:e], bias[:e], *geo, c, mode, **_tables_for(mode, inputs[(c, e)]))
    assert got.dtype == torch.int64 and tuple(got.shape) == (geo[0], 8 * geo[1], 8 * geo[2])
    assert torch.equal(got, ref)
    assert ref.unique().numel() >= 2                                 # the case decides something
    out = torch.full_like(got, SENTINEL)
    assert ops.fused_head_multi(S[:e], bias[:e], *geo, c, MODE_NAMES[mode], out=out, **_tables_for(mode, inputs[(c, e)])) is out
    assert torch.equal(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('c', CLASSES)
@pytest.mark.parametrize('mode', MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_two_experts_equal_the_two_expert_heads(inputs, mode, c):
    from modular_semantic_segmentation_amd import ops
    geo = (3, 5, 4)
    S, bias = inputs[(c, geo)]
    t = inputs[(c, 2)]
    got = ops.fused_head_multi(S[:2], bias[:2], *geo, c, mode, **_tables_for(mode, t))
    if mode == 0:
        two = ops.fused_head(S[0], S[1], bias[0], bias[1], *geo, c, t['loglik'], t['logprior'])
    elif mode == 1:
        two = ops.fused_head(S[0], S[1], bias[0], bias[1], *geo, c, t['am1'], t['logprior'], lognorm=t['lognorm'])
    else:
        two = ops.fused_head_average(S[0], S[1], bias[0], bias[1], *geo, c)
    assert torch.equal(got, two)


def _check(ops, S, bias, geo, c, mode, tables):
    ref = _unfused(ops, S, bias, geo, c, mode, tables)
    got = ops.fused_head_multi(S, bias, *geo, c, mode, **_tables_for(mode, tables))
    assert torch.equal(got, ref)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('e', [3, 4])
@pytest.mark.parametrize('mode', MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_ties(inputs, mode, e):
    """the first maximum wins wherever classes tie, as in the unfused kernels"""
    from modular_semantic_segmentation_amd import ops
    c, geo = 12, (1, 3, 5)
    S, bias = inputs[(c, geo)]
    S, bias, t = S[:e], bias[:e], inputs[(c, e)]
    # constant scores in every expert: every class of every expert ties
    flat = [torch.zeros_like(s) for s in S]
    for s in flat:
        s[:, 1:-1, 1:-1, :c] = 0.5
    zero = [torch.zeros_like(b) for b in bias]
    got = _check(ops, flat, zero, geo, c, mode, t)
    if mode == 2:
        assert int(got.abs().sum()) == 0                             # the mean of equal probabilities: label 0
    # two experts given the same scores
    _check(ops, [S[0], S[0]] + S[2:], [bias[0], bias[0]] + bias[2:], geo, c, mode, t)
    # tables that cannot tell class 3 from class 7
    tie = {k: v.clone() for k, v in t.items()}
    tie['loglik'][:, :, 7] = tie['loglik'][:, :, 3]                  # Bayes: two identical columns
    tie['am1'][:, 7, :] = tie['am1'][:, 3, :]                        # Dirichlet: equal rows for two classes
    tie['lognorm'][:, 7] = tie['lognorm'][:, 3]
    tie['logprior'][7] = tie['logprior'][3]
    got = _check(ops, S, bias, geo, c, mode, tie)
    if mode != 2:
        assert int((got == 7).sum()) == 0                            # equal scores: the lower index


@pytest.mark.gpu
@pytest.mark.parametrize('c', [5, 12])
@pytest.mark.parametrize('mode', MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_expert_order_is_kept(inputs, mode, c):
    """float sums do not commute: the experts permuted together with their tables give the unfused result of THAT order"""
    from modular_semantic_segmentation_amd import ops
    geo = (3, 5, 4)
    S, bias = inputs[(c, geo)]
    t = inputs[(c, 4)]
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2], [2, 0, 1]):
        idx = torch.tensor(perm, device=DEV)
        pt = {k: (v[idx].contiguous() if k != 'logprior' else v) for k, v in t.items()}
        _check(ops, [S[i] for i in perm], [bias[i] for i in perm], geo, c, mode, pt)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES, ids=[MODE_NAMES[m] for m in MODES])
def test_score_tensors_in_unrelated_allocations(inputs, references, mode):
    from modular_semantic_segmentation_amd import ops
    c, geo, e = 13, (2, 7, 9), 4
    S, bias = inputs[(c, geo)]
    views, keep = [], []
    for i, s in enumerate(S):
        pad = 4 * (3 + 5 * i)                                        # (16-byte aligned offsets that differ per expert)
        big = torch.full((pad + s.numel() + 64 * (e - i),), float('nan'), dtype=torch.float32, device=DEV)
        keep.append(big)
        view = big[pad:pad + s.numel()].view(s.shape)
        view.copy_(s)
        assert view.data_ptr() % 16 == 0 and view.is_contiguous()
        views.append(view)
    got = ops.fused_head_multi(views, bias, *geo, c, mode, **_tables_for(mode, inputs[(c, e)]))
    assert torch.equal(got, references(e, mode, c, geo))


@pytest.mark.gpu
def test_refusals(inputs):
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd._lib import XvError
    c, geo = 12, (1, 3, 5)
    S, bias = inputs[(c, geo)]
    out = torch.full((geo[0], 8 * geo[1], 8 * geo[2]), SENTINEL, dtype=torch.int64, device=DEV)

    def refused(scores, biases, classes, mode, **tables):
        with pytest.raises(XvError, match='XV_EINVAL'):
            ops.fused_head_multi(scores, biases, *geo, classes, mode, out=out, **tables)

    def tables(e, classes):
        return dict(tab=torch.zeros((e, classes, classes), device=DEV), lognorm=torch.zeros((e, classes), device=DEV),
                    logprior=torch.zeros(classes, device=DEV))

    for mode in MODES:
        refused(S[:1], bias[:1], c, mode, **tables(1, c))                               # one expert
        refused(S + S[:1], bias + bias[:1], c, mode, **tables(5, c))                    # five
        for classes in (1, 33):
            cp = (classes + 3) // 4 * 4
            s = [torch.zeros((geo[0], geo[1] + 2, geo[2] + 2, cp), device=DEV) for _ in range(3)]
            b = [torch.zeros(classes, device=DEV) for _ in range(3)]
            refused(s, b, classes, mode, **tables(3, classes))
    good = tables(3, c)
    refused(S[:3], bias[:3], c, 3, **good)                                              # no such mode
    refused(S[:3], bias[:3], c, 0, logprior=good['logprior'])                           # Bayes without its tables
    refused(S[:3], bias[:3], c, 1, lognorm=good['lognorm'], logprior=good['logprior'])  # Dirichlet without alpha - 1
    refused(S[:3], bias[:3], c, 1, tab=good['tab'], logprior=good['logprior'])          # Dirichlet without lognorm
    big = torch.zeros(S[1].numel() + 4, dtype=torch.float32, device=DEV)
    off = big[1:1 + S[1].numel()].view(S[1].shape)                                      # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    for mode in MODES:
        refused([S[0], off, S[2]], bias[:3], c, mode, **good)
    torch.cuda.synchronize()
    assert int((out != SENTINEL).sum()) == 0                                            # nothing ran
    assert ops.fused_head_multi(S[:3], bias[:3], *geo, c, 1, out=out, **good) is out    # and the good call does
    torch.cuda.synchronize()
    assert int((out == SENTINEL).sum()) == 0
