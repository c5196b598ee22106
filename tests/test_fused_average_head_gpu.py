"""The fused average head (xv_fused_head_average_fwd / _count_fwd) on small maps: its labels against the unfused path (two
decoder heads writing `prob`, then xv_average_fuse) bit for bit, its counts against xv_confusion_matrix of those labels, the
grid-stride loop of the counting form, an independent float64 evaluation from the scores, and the refusals.

The float64 check and its margin.  Reference: bilinear x8 interpolation of the low-resolution scores (the oracle's depthwise
deconvolution), + bias, softmax, mean of the two experts, argmax, all in numpy float64.  A pixel is left out only when the
float64 top-two gap of the MEAN probability is below MARGIN(L, C), L the largest |logit| of the case, u = 2^-23 (one ulp: the
hardware exp2 and reciprocal are good to one ulp, every other operation to half of one):
  logit        four products and three sums of the interpolation, one sum for the bias: |error| <= 5 u L
  x = z - max  both carry that error, one more rounding: <= 10 u L + u |x|, |x| <= 2 L
  exp(x)       x log2(e) rounds twice (the constant, the product): u |x| each on the exponent, exp2 one ulp:
               relative error rho <= (10 L + 3 |x|) u + u <= (16 L + 1) u
  1 / sum      C - 1 roundings of the sum on terms that each carry rho, the reciprocal one ulp: rho + C u
  p            one product: relative and (p <= 1) absolute error <= 2 rho + (C + 1) u
  mean         pa + pb and the halving (exact): <= 2 rho + (C + 2) u
  gap          two means: MARGIN = 2 (2 (16 L + 1) + C + 2) u
(1.3e-4 at L = 16, C = 12.)  At most 1 % of the pixels may be left out; test_float64_reference_leaves_out_at_most_one_percent
checks on the CPU that the logit scale of the cases keeps the reference itself within that."""
import numpy as np
import pytest
import torch

from oracle import fcn_oracle as fo

DEV = 'cuda:0'
GEOMETRIES = [(1, 3, 5), (3, 5, 4)]                  # (n, hi, wi): odd sizes, more than one image
CLASSES = [2, 5, 12, 13, 16, 20]                     # padded and full class vectors; CM = 4, 8, 12, 16, 20
SCALE = 3.0                                          # standard deviation of the low-resolution scores


def _host_case(c, geo, seed):
    """zero-bordered low-resolution scores [n][hi+2][wi+2][CP] of two experts, their biases, labels drawn from [-1, c]"""
    n, hi, wi = geo
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    S = [torch.zeros((n, hi + 2, wi + 2, cp)) for _ in range(2)]
    for t in S:
        t[:, 1:-1, 1:-1, :c] = torch.randn((n, hi, wi, c), generator=g) * SCALE
    bias = [torch.randn(c, generator=g) for _ in range(2)]
    labels = torch.randint(-1, c + 1, (n, 8 * hi, 8 * wi), generator=g, dtype=torch.int32)
    return S, bias, labels


def _float64_reference(S, bias, c):
    """(label of the float64 mean probability, its top-two gap, largest |logit|)"""
    mean, L = 0.0, 0.0
    for e in range(2):
        z = fo.depthwise_bilinear_up(S[e][:, 1:-1, 1:-1, :c].numpy().astype(np.float64), 8) + bias[e].numpy().astype(np.float64)
        L = max(L, float(np.abs(z).max()))
        ex = np.exp(z - z.max(-1, keepdims=True))
        mean = mean + ex / ex.sum(-1, keepdims=True)
    mean = mean / 2.0
    top = np.sort(mean, -1)
    return np.argmax(mean, -1), top[..., -1] - top[..., -2], L


def _margin(L, c):
    return 2.0 * (2.0 * (16.0 * L + 1.0) + c + 2.0) * 2.0 ** -23


CASES = [(c, geo) for c in CLASSES for geo in GEOMETRIES]
IDS = ['c%d-n%dx%dx%d' % ((c,) + geo) for c, geo in CASES]


@pytest.mark.parametrize('c,geo', CASES, ids=IDS)
def test_float64_reference_leaves_out_at_most_one_percent(c, geo):
    S, bias, _ = _host_case(c, geo, 7 * c + geo[0])
    _, gap, L = _float64_reference(S, bias, c)
    assert L < 32 and _margin(L, c) < 3e-4
    assert (gap < _margin(L, c)).mean() <= 0.01


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _unfused(ops, S, bias, geo, c):
    """two decoder heads writing `prob`, then xv_average_fuse"""
    n, hi, wi = geo
    probs = []
    for e in range(2):
        prob = torch.empty((n, 8 * hi, 8 * wi, c), dtype=torch.float32, device=DEV)
        ops.decoder_head_from_scores(S[e], bias[e], n, hi, wi, c, prob=prob)
        probs.append(prob)
    return ops.average_fuse(probs), probs


@pytest.fixture(scope='module')
def cases(gpu):
    """per (c, geo): device inputs and the unfused path's labels, computed once and left unchanged"""
    from modular_semantic_segmentation_amd import ops
    out = {}
    for c, geo in CASES:
        S, bias, labels = _host_case(c, geo, 7 * c + geo[0])
        dS, dbias = [t.to(DEV) for t in S], [t.to(DEV) for t in bias]
        ref, probs = _unfused(ops, dS, dbias, geo, c)
        out[(c, geo)] = dict(S=dS, bias=dbias, labels=labels.to(DEV), ref=ref, probs=probs, host=(S, bias))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('c,geo', CASES, ids=IDS)
def test_labels_equal_the_unfused_path_on_every_pixel(cases, c, geo):
    from modular_semantic_segmentation_amd import ops
    k = cases[(c, geo)]
    got = ops.fused_head_average(k['S'][0], k['S'][1], k['bias'][0], k['bias'][1], *geo, c)
    assert got.dtype == torch.int64 and tuple(got.shape) == (geo[0], 8 * geo[1], 8 * geo[2])
    assert torch.equal(got, k['ref'])
    assert c == 2 or k['ref'].unique().numel() > 2
    out = torch.full_like(got, -7)
    assert ops.fused_head_average(k['S'][0], k['S'][1], k['bias'][0], k['bias'][1], *geo, c, out=out) is out
    assert torch.equal(out, k['ref'])


@pytest.mark.gpu
@pytest.mark.parametrize('c,geo', CASES, ids=IDS)
def test_counts_equal_the_confusion_matrix_of_those_labels(cases, c, geo):
    from modular_semantic_segmentation_amd import ops
    k = cases[(c, geo)]
    labels = k['labels']
    assert int((labels == -1).sum()) > 0 and int((labels >= c).sum()) > 0       # both kinds of pixels that do not count
    ref = torch.zeros((c, c), dtype=torch.int64, device=DEV)
    ops.confusion_matrix(labels, k['ref'], ref)
    assert int(ref.sum()) == int(((labels >= 0) & (labels < c)).sum())
    args = (k['S'][0], k['S'][1], k['bias'][0], k['bias'][1]) + geo + (c,)
    cm = ops.fused_head_average_count(*args, labels)
    assert cm.dtype == torch.int64 and torch.equal(cm, ref)
    # accumulation into a matrix that is not zero
    start = torch.arange(c * c, dtype=torch.int64, device=DEV).reshape(c, c) * 3 + 1
    acc = start.clone()
    assert ops.fused_head_average_count(*args, labels, cm=acc) is acc
    assert torch.equal(acc, start + ref)
    # a label map that is a slice of a larger buffer, 4 bytes off a 16-byte boundary
    big = torch.zeros(labels.numel() + 4, dtype=torch.int32, device=DEV)
    view = big[1:1 + labels.numel()]
    view.copy_(labels.reshape(-1))
    assert view.data_ptr() % 16 == 4
    assert torch.equal(ops.fused_head_average_count(*args, view.reshape(labels.shape)), ref)
    # the grid-stride loop: one and three workgroups against 2 x 8 x 64 x hi x wi / 2 pixel groups
    for max_workgroups in (1, 3):
        assert torch.equal(ops.fused_head_average_count(*args, labels, max_workgroups=max_workgroups), ref), max_workgroups


@pytest.mark.gpu
@pytest.mark.parametrize('c', [12, 16, 5])
def test_grid_stride_loop_past_the_first_round(cases, c):
    """3 x 40 x 32 = 3 840 pixels are 1 920 groups of two: two workgroups of 256 threads take four rounds, the last one half
    empty (a wave with no live lane at all among them)"""
    from modular_semantic_segmentation_amd import ops
    geo = (3, 5, 4)
    k = cases[(c, geo)]
    ref = torch.zeros((c, c), dtype=torch.int64, device=DEV)
    ops.confusion_matrix(k['labels'], k['ref'], ref)
    groups = geo[0] * geo[1] * geo[2] * 64 // 2
    assert groups > 3 * 2 * 256 and groups % (2 * 256) == 384
    cm = ops.fused_head_average_count(k['S'][0], k['S'][1], k['bias'][0], k['bias'][1], *geo, c, k['labels'], max_workgroups=2)
    assert torch.equal(cm, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('c,geo', CASES, ids=IDS)
def test_labels_against_float64_from_the_scores(cases, c, geo):
    from modular_semantic_segmentation_amd import ops
    k = cases[(c, geo)]
    S, bias = k['host']
    ref, gap, L = _float64_reference(S, bias, c)
    clear = gap >= _margin(L, c)
    got = ops.fused_head_average(k['S'][0], k['S'][1], k['bias'][0], k['bias'][1], *geo, c).cpu().numpy()
    print('c %d geo %s: largest |logit| %.2f, margin %.3g, left out %d of %d, disagreeing among them %d' % (
        c, geo, L, _margin(L, c), int((~clear).sum()), clear.size, int((got != ref)[~clear].sum())))
    assert (~clear).mean() <= 0.01
    assert np.array_equal(got[clear], ref[clear])


@pytest.mark.gpu
def test_refusals(cases):
    from modular_semantic_segmentation_amd import _lib
    lib = _lib.lib()
    c, geo = 12, (1, 3, 5)
    k = cases[(c, geo)]
    fused = torch.full((geo[0], 8 * geo[1], 8 * geo[2]), -7, dtype=torch.int64, device=DEV)
    good = [k['S'][0].data_ptr(), k['S'][1].data_ptr(), k['bias'][0].data_ptr(), k['bias'][1].data_ptr(), *geo, c,
            fused.data_ptr(), None]
    for i in (0, 1, 2, 3, 8):                                                # every pointer
        bad = list(good)
        bad[i] = None
        assert lib.xv_fused_head_average_fwd(*bad) == -1, i
    for v in (0, -1, 33, 40):                                                # class counts no instantiation serves
        bad = list(good)
        bad[7] = v
        assert lib.xv_fused_head_average_fwd(*bad) == -1, v
    bad = list(good)
    bad[8] = fused.data_ptr() + 8                                            # the 16-byte stores
    assert lib.xv_fused_head_average_fwd(*bad) == -1
    torch.cuda.synchronize()
    assert int((fused != -7).sum()) == 0                                     # nothing ran
    # A width the pixel group does not divide: the output width is 8 wi and a group is two pixels, so no wi the entry point
    # accepts has one (the check in the launcher stands for a later group size); every width from 1 to 9 sources is served.
    for wi in range(1, 10):
        S, bias, _ = _host_case(c, (1, 1, wi), wi)
        S, bias = [t.to(DEV) for t in S], [t.to(DEV) for t in bias]
        out = torch.empty((1, 8, 8 * wi), dtype=torch.int64, device=DEV)
        assert lib.xv_fused_head_average_fwd(S[0].data_ptr(), S[1].data_ptr(), bias[0].data_ptr(), bias[1].data_ptr(), 1, 1, wi,
                                             c, out.data_ptr(), None) == 0, wi
    for wi in (0, -2):
        bad = list(good)
        bad[6] = wi
        assert lib.xv_fused_head_average_fwd(*bad) < 0, wi

    cm = torch.zeros((c, c), dtype=torch.int64, device=DEV)
    labels = k['labels']
    good = [k['S'][0].data_ptr(), k['S'][1].data_ptr(), k['bias'][0].data_ptr(), k['bias'][1].data_ptr(), *geo, c,
            labels.data_ptr(), cm.data_ptr(), 0, None]
    for i in (0, 1, 2, 3, 8, 9):
        bad = list(good)
        bad[i] = None
        assert lib.xv_fused_head_average_count_fwd(*bad) == -1, i
    for i, v in ((7, 0), (7, 33), (10, -1), (8, labels.data_ptr() + 4)):     # classes, max_workgroups, label alignment
        bad = list(good)
        bad[i] = v
        assert lib.xv_fused_head_average_count_fwd(*bad) == -1, (i, v)
    torch.cuda.synchronize()
    assert int(cm.sum()) == 0
    assert lib.xv_fused_head_average_count_fwd(*good) == 0
    torch.cuda.synchronize()
    assert int(cm.sum()) == int(((labels >= 0) & (labels < c)).sum())
