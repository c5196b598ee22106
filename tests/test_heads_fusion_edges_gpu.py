"""The anchor kernels of the unfused inference path at their edges: the low-resolution score conv, the decoder heads (all four
output forms, the general affine head), the dense softmax + argmax and the Bayes / lookup / Dirichlet / average / variance fusion
kernels, every host dispatch branch.  The fused heads are tested by bit-equality with these kernels, so a mistake shared by
both shows here or nowhere.

Conventions of test_training_kernels_edges_gpu.py and test_inference_pointwise_edges_gpu.py, whose helpers are imported: every
reference is numpy in float64 and calls no kernel; outputs are prefilled with a non-zero pattern and carry one guard row;
operands that make float32 arithmetic exact are compared bit for bit; random-valued cases are held to a per-element bound
counted from the roundings of the arithmetic (plus what xv_common.h documents for v_exp_f32 / v_log_f32 / v_rcp_f32: one ulp
each, denormal results flushed), the same formulas in float32 on the CPU are held to that bound first
(test_heads_fusion_reference_cpu.py does so without a GPU), and each such test prints the bound and both error-to-bound ratios.

csrc/Makefile builds with -O3 and no fast-math flag: float32 division is IEEE (correctly rounded), so bayes_fuse's sums and
average_fuse's ((p_0 + p_1) + ...) / E are compared with a float32 evaluation in the same order bit for bit.

Labels, three checks: (1) the label is the lowest-index argmax of the kernel's own prob / score output; (2) it is the float64
argmax wherever the float64 winner clears every other class by the two bounds; (3) exact ties give the lowest index.

Host dispatch branch -> the test that reaches it:
  decoder_head_kernel with score / with prob            test_decoder_head_from_scores_dyadic_all_forms (forms 1 and 2)
  decoder_head_label4_kernel (aligned label alone)      the same tests, form 3; test_decoder_head_near_ties_all_forms
  decoder_head_kernel, head_label_fast (offset label)   the same tests, form 4; the 1e-5 window: near ties [5e-6-*] / [2e-5-*]
  decoder_head_affine_kernel CLAMP only / plain + CLAMP test_decoder_head_affine_integers_bit_for_bit[8-*] / [16-*], [24-*] ...
  ... its second 128-column tile                        the same tests, map (1, 2, 17)
  softmax_argmax_kernel<12> / <16> / <32>               test_softmax_argmax_against_float64[12] / [1 .. 16] / [17, 31, 32]
  ... <16> on an unaligned 12-class map                 test_softmax_argmax_unaligned_12_classes_equal_the_vector_form
  bayes_fuse_kernel<16> / <32>                          test_bayes_fuse_every_form[*-1 .. 16] / [*-17, *-32]
  bayes_fuse2_kernel                                    test_bayes_fuse_every_form[2-*], the run without a score
  dirichlet_fuse: packed / <12, EXACT> / <16> vector /  test_dirichlet_fuse_branch[packed-*] / [exact12-*] / [vector16-*] /
    <16> scalar / <32>                                    [scalar16-*] / [kernel32-*]
  average_fuse / variance_fuse <16> / <32>, both loads  test_average_fuse_labels_of_the_same_order_float32_mean, test_variance_fuse_against_float64
  every grid-stride loop past its capped grid           the *_grid_stride_loop tests, test_bayes_fuse_lut_exact[12]

Largest error / bound seen on an MI355X (kernel; float32 on the CPU): score_lowres 0.25; 0.25, decoder head 0.57; 0.57, head
chain 0.23; 0.23, affine head 0.15; 0.15, softmax_argmax 0.66; 0.66, bayes_fuse 0.99; 0.99 (the same bits), dirichlet_fuse
0.47; 0.41, variance_fuse 0.33; 0.33.  No factor of a bound is measured: the transcendental unit enters with the one ulp that
xv_common.h documents.

head_label_fast returns a class only when the maximum is unique (a second class equal to it closes the 1e-5 window), so which
of several equal logits it would name cannot show in any output: the tie rule that can is head_softmax's, pinned by the
near-tie tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import fcn_oracle as fo
from test_training_kernels_edges_gpu import EPS, _act_from_bits, _bf16_bits, _bits_to_f64, _dev
from test_training_kernels_edges_gpu import ops  # noqa: F401  (the module-scoped fixture)
from test_inference_pointwise_edges_gpu import _report

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NORMAL = 2.0 ** -126                 # v_exp_f32 flushes denormal results ...
FLUSH = NORMAL * 1.001                # ... so anything made from an exp has this absolute floor (a value a rounding above 2^-126 may go too)
TINY = F32(1e-20)                    # the kernels' 1e-20f
LOG2E, LN2 = F32(1.4426950408889634), F32(0.6931471805599453)
SLACK = 1.001                        # second-order terms of the first-order rounding counts
LEFT_OUT = 0.01                      # check (2) may leave out at most this share of a random case's pixels
GRID_CAP = 8192                      # xv_grid_for's default cap, workgroups of 256


def _lib():
    from modular_semantic_segmentation_amd import _lib as m
    return m


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(name):
    return _lib().CONSTANTS[name]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _fma32(a, b, c):
    """One float32 fused multiply-add: the float64 product of two float32 values is exact."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


class _Out(object):
    """A prefilled output inside a larger plain allocation: `offset` elements in front of it (a misaligned contiguous view),
    one guard row (the last dimension) behind it.  get() asserts that everything around the output kept the prefill."""

    def __init__(self, shape, dtype=torch.float32, offset=0):
        self.shape, self.offset = tuple(int(s) for s in shape), offset
        self.n = int(np.prod(self.shape))
        self.fill = 3.0 if dtype.is_floating_point else -7
        self.whole = torch.full((offset + self.n + self.shape[-1],), self.fill, dtype=dtype, device='cuda')
        assert self.whole.data_ptr() % 16 == 0
        self.t = self.whole[offset:offset + self.n].view(self.shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (offset * self.whole.element_size()) % 16

    def get(self):
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        assert (w[:self.offset] == self.fill).all() and (w[self.offset + self.n:] == self.fill).all(), 'guard overwritten'
        return w[self.offset:self.offset + self.n].reshape(self.shape).copy()

    def untouched(self):
        return bool((self.get() == self.fill).all())


def _offset_input(a):
    """The array on the device as a contiguous view one element into a larger allocation."""
    a = np.ascontiguousarray(a)
    whole = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype, device='cuda')
    whole[1:] = torch.from_numpy(a.reshape(-1)).cuda()
    v = whole[1:].view(a.shape)
    assert v.data_ptr() % 16 == a.itemsize
    return v


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _same_bits(a, b):
    """float32 arrays equal bit for bit (a zero of either sign equal to itself only)."""
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- shared references ----------------------------------------------------------------------------------------------------------

def _taps8(size):
    """bilinear_taps<8> (xv_common.h): output o reads padded sources i1 (weight w0: the logical source i1 - 1) and i1 + 1
    (weight w1); the weights are multiples of 1/16."""
    t = np.arange(8 * size) + 4
    i1 = t // 8
    p1 = t - 8 * i1
    return i1, (1.0 - np.abs(p1 / 8.0 - 15.0 / 16.0)).astype(F32), (1.0 - np.abs((p1 + 8) / 8.0 - 15.0 / 16.0)).astype(F32)


def _up8_taps(xp):
    """The four source maps of every output pixel of a padded [n][h+2][w+2][c] array and their weights [8h][8w][1]."""
    h, w = xp.shape[1] - 2, xp.shape[2] - 2
    iy, wy1, wy0 = _taps8(h)
    ix, wx1, wx0 = _taps8(w)
    rows0, rows1 = xp[:, iy], xp[:, iy + 1]
    taps = (rows0[:, :, ix], rows0[:, :, ix + 1], rows1[:, :, ix], rows1[:, :, ix + 1])
    wts = tuple((a[:, None] * b[None, :])[..., None] for a, b in ((wy0, wx0), (wy0, wx1), (wy1, wx0), (wy1, wx1)))
    return taps, wts


def _pad_hw(x):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))


def _up8_abs(x):
    """x8 interpolation of |x| in float64 (x dense [n][h][w][c]): what the roundings of the interpolation scale with."""
    taps, wts = _up8_taps(_pad_hw(np.abs(x.astype(F64))))
    return sum(t * w.astype(F64) for t, w in zip(taps, wts))


def _up8_f32(x):
    """head_eval_taps in float32: fmaf(d, w11, fmaf(c, w10, fmaf(b, w01, a * w00)))."""
    (a, b, c, d), (w00, w01, w10, w11) = _up8_taps(_pad_hw(x.astype(F32)))
    return _fma32(d, w11, _fma32(c, w10, _fma32(b, w01, a * w00)))


@functools.lru_cache(maxsize=None)
def _taps_are_the_oracles_deconv():
    x = np.random.default_rng(11).integers(-8, 9, (2, 3, 5, 3)).astype(F64)
    taps, wts = _up8_taps(_pad_hw(x))
    assert np.array_equal(sum(t * w for t, w in zip(taps, wts)), fo.depthwise_bilinear_up(x, 8))      # multiples of 1/256
    return True


def _up8(x):
    assert _taps_are_the_oracles_deconv()
    return fo.depthwise_bilinear_up(np.asarray(x, F64), 8)


def _softmax_ref(z, dz=0.0):
    """float64 softmax over the last axis of the logits z and the bound of a float32 evaluation exp2((z - m) log2 e) / sum
    whose logits carry an absolute error of at most dz each: the exponent takes three roundings of size |z - m| (subtraction,
    the constant, the product), exp2 one ulp, the sum C - 1 roundings, the reciprocal one ulp, the product one rounding; an
    error of the logits moves an exponent by at most twice its size.  Flushed denormals: an absolute floor."""
    z = np.asarray(z, F64)
    C = z.shape[-1]
    d = z - z.max(-1, keepdims=True)
    e = np.exp(d)
    s = e.sum(-1, keepdims=True)
    p = e / s
    dz = np.broadcast_to(np.asarray(dz, F64), z.shape)
    r = 3 * EPS * np.abs(d) + 2 * EPS + dz + dz.max(-1, keepdims=True)
    r = np.expm1(r)
    rel = r + (e * r).sum(-1, keepdims=True) / s + (C + 2) * EPS
    return p, p * rel * SLACK + FLUSH


def _softmax_f32(z):
    """head_softmax / softmax_argmax_kernel in float32 on the CPU, classes summed in ascending order."""
    z = np.asarray(z, F32)
    e = np.exp2((z - z.max(-1, keepdims=True)) * LOG2E)
    e[e < NORMAL] = 0
    s = np.zeros(z.shape[:-1], F32)
    for k in range(z.shape[-1]):
        s = s + e[..., k]
    out = e * (F32(1) / s)[..., None]
    assert out.dtype == F32
    return out


def _clear(ref, bound):
    """(float64 argmax, mask of the pixels whose winner clears every other class by the two bounds)."""
    C = ref.shape[-1]
    ref, bound = ref.reshape(-1, C), np.broadcast_to(bound, ref.shape).reshape(-1, C)
    top = ref.argmax(-1)
    if C == 1:
        return top, np.ones(len(top), bool)
    lo = np.take_along_axis(ref - bound, top[:, None], -1)[:, 0]
    hi = ref + bound
    np.put_along_axis(hi, top[:, None], -np.inf, -1)
    return top, lo > hi.max(-1)


def _left_out(ref, bound):
    return 1.0 - float(_clear(ref, bound)[1].mean())


def _check_labels(label, own, ref, bound, limit=None):
    """Checks (1) and (2); limit: the largest share of pixels (2) may leave out."""
    C = ref.shape[-1]
    label, own = label.reshape(-1), own.reshape(-1, C)
    assert np.isfinite(own).all()
    assert np.array_equal(label, own.argmax(-1))                        # np.argmax: the lowest index among equal values
    top, clear = _clear(ref, bound)
    assert np.array_equal(label[clear], top[clear])
    if limit is not None:
        assert 1.0 - clear.mean() <= limit, 1.0 - clear.mean()


def _check_exact_ties(label, z):
    """(3) on exactly known logits: where the maximum is shared and everything else is far below, the lowest index."""
    C = z.shape[-1]
    z, label = z.reshape(-1, C), label.reshape(-1)
    m = z.max(-1, keepdims=True)
    tied = ((z == m).sum(-1) >= 2) & (((z == m) | (z < m - 1e-3)).all(-1))
    assert np.array_equal(label[tied], (z == m).argmax(-1)[tied])
    return int(tied.sum())


# ---- a. xv_score_lowres ---------------------------------------------------------------------------------------------------------

LOWRES_MAPS = [(1, 1, 1), (2, 3, 5), (1, 9, 15)]          # the last: 187 padded pixels, two workgroups of 128, the second partial


def _cm(C):
    return (C + 3) // 4 * 4


def _run_score_lowres(ops, fb, w, C):
    n, h, wd, U = fb.shape
    S = _Out((n, h + 2, wd + 2, _cm(C)))
    f, wt = _act_from_bits(ops, fb), _dev(w)
    rc = _lib().lib().xv_score_lowres(f.xv(), ops._ptr(wt), C, ops._ptr(S.t), _stream())
    return rc, S


def _padded_scores(s, C):
    """Dense [n][h][w][C] -> the padded [n][h+2][w+2][CM] layout, zero border, zero padding channels."""
    n, h, w, _ = s.shape
    out = np.zeros((n, h + 2, w + 2, _cm(C)), s.dtype)
    out[:, 1:-1, 1:-1, :C] = s
    return out


@pytest.mark.parametrize('C', [1, 3, 4, 12, 13, 17, 32])
@pytest.mark.parametrize('U', [8, 24, 64, 256])
def test_score_lowres_integers_bit_for_bit(ops, U, C):
    """|f| <= 4, |w| <= 2: every partial sum is an integer below 2^12.  The whole padded S, border and padding channels zero."""
    for n, h, w in LOWRES_MAPS:
        rng = np.random.default_rng(U + C + n * h * w)
        f = rng.integers(-4, 5, (n, h, w, U)).astype(F32)
        ws = rng.integers(-2, 3, (U, C)).astype(F32)
        rc, S = _run_score_lowres(ops, _bf16_bits(f), ws, C)
        assert rc == 0
        want = _padded_scores(np.einsum('nhwu,uc->nhwc', f.astype(F64), ws.astype(F64)), C)
        assert np.array_equal(S.get().astype(F64), want), (n, h, w)


def _score_lowres_case(U, C=13, shape=(2, 3, 5)):
    rng = np.random.default_rng(U + C)
    fb = _bf16_bits(rng.standard_normal(shape + (U,)).astype(F32))
    ws = rng.standard_normal((U, C)).astype(F32)
    f = _bits_to_f64(fb)
    ref = np.einsum('nhwu,uc->nhwc', f, ws.astype(F64))
    A = np.einsum('nhwu,uc->nhwc', np.abs(f), np.abs(ws.astype(F64)))
    f32 = np.zeros(shape + (C,), F32)
    for u in range(U):                                                  # the kernel's fmaf chain, channels in ascending order
        f32 = _fma32(f[..., u, None], ws[u], f32)
    return dict(fb=fb, ws=ws, ref=ref, bound=U * EPS * A * SLACK, f32=f32)          # one rounding per fused multiply-add


@pytest.mark.parametrize('U', [8, 24, 64, 256])
def test_score_lowres_random_within_the_rounding_bound(ops, U):
    C = 13
    case = _score_lowres_case(U)
    rc, S = _run_score_lowres(ops, case['fb'], case['ws'], C)
    assert rc == 0
    got = S.get()
    assert np.array_equal(got, _padded_scores(got[:, 1:-1, 1:-1, :C], C))           # border and padding channels: zeros
    rk, rc32 = _report('score_lowres U=%d' % U, case['bound'], np.abs(got[:, 1:-1, 1:-1, :C] - case['ref']),
                       np.abs(case['f32'] - case['ref']))
    assert rc32 <= 1.0 and rk <= 1.0


@pytest.mark.parametrize('U', [264, 12])
def test_score_lowres_refuses_channel_counts_it_cannot_hold(ops, U):
    rc, S = _run_score_lowres(ops, np.zeros((1, 2, 2, U), np.int16), np.ones((U, 3), F32), 3)
    assert rc == _code('XV_ESHAPE')
    assert S.untouched()


# ---- b. xv_decoder_head_from_scores and xv_decoder_head_fwd -----------------------------------------------------------------------

def _run_from_scores(ops, Sp, bias, C):
    """The four output forms on the same S: (score, prob, label), (prob, label), the label alone into an aligned buffer (the
    four-pixel kernel) and into a view offset by 8 bytes (the one-pixel kernel's fast path)."""
    n, hi, wi = Sp.shape[0], Sp.shape[1] - 2, Sp.shape[2] - 2
    S, b = _dev(Sp), _dev(bias)
    dense, lab = (n, 8 * hi, 8 * wi, C), (n, 8 * hi, 8 * wi)
    score, prob, l_spl = _Out(dense), _Out(dense), _Out(lab, torch.int64)
    ops.decoder_head_from_scores(S, b, n, hi, wi, C, score=score.t, prob=prob.t, label=l_spl.t)
    prob2, l_pl = _Out(dense), _Out(lab, torch.int64)
    ops.decoder_head_from_scores(S, b, n, hi, wi, C, prob=prob2.t, label=l_pl.t)
    l_four, l_one = _Out(lab, torch.int64), _Out(lab, torch.int64, offset=1)
    ops.decoder_head_from_scores(S, b, n, hi, wi, C, label=l_four.t)
    ops.decoder_head_from_scores(S, b, n, hi, wi, C, label=l_one.t)
    out = dict(score=score.get(), prob=prob.get(), label=l_spl.get())
    assert _same_bits(prob2.get(), out['prob'])
    for other in (l_pl, l_four, l_one):                                 # the three label maps that come without a score
        assert np.array_equal(other.get(), out['label'])
    return out


def _exact_logits(S, bias):
    """S (dense, [n][hi][wi][C]) whose interpolation is exact in float32: the kernel's logits are one rounding of the float64
    value, the bias added after the interpolation."""
    z = (_up8(S) + bias.astype(F64)).astype(F32)
    return z


def _check_head_exact(ops, S, bias, C):
    z = _exact_logits(S, bias)
    out = _run_from_scores(ops, _padded_scores(S.astype(F32), C), bias, C)
    assert _same_bits(out['score'], z)
    ref, bound = _softmax_ref(z)
    cpu = _softmax_f32(z)
    err, err32 = np.abs(out['prob'] - ref), np.abs(cpu - ref)
    _check_labels(out['label'], out['prob'], ref, bound)
    _check_exact_ties(out['label'], z)
    return out, z, bound, err, err32


HEAD_C = [1, 2, 3, 4, 5, 12, 13, 16, 17, 20, 32]
HEAD_MAPS = [(1, 1, 1), (1, 1, 3), (2, 3, 5), (3, 2, 2)]


@pytest.mark.parametrize('C', HEAD_C)
def test_decoder_head_from_scores_dyadic_all_forms(ops, C):
    """S multiples of 1/4 up to 4, bias multiples of 1/4 up to 2, the x8 weights multiples of 1/256: the logits are exact, at
    the image border too (the taps do not sum to 1 there)."""
    worst = [0.0, 0.0]
    for n, hi, wi in HEAD_MAPS:
        rng = np.random.default_rng(C + n * hi * wi)
        S = rng.integers(-16, 17, (n, hi, wi, C)) / 4.0
        bias = (rng.integers(-8, 9, C) / 4.0).astype(F32)
        z64 = _up8(S) + bias
        assert np.array_equal(z64.astype(F32).astype(F64), z64)
        _, _, bound, err, err32 = _check_head_exact(ops, S, bias, C)
        worst = [max(worst[0], float((err / bound).max())), max(worst[1], float((err32 / bound).max()))]
    print('decoder_head_from_scores dyadic C=%d: prob kernel err/bound %.4f; CPU float32 err/bound %.4f' % (C, worst[0], worst[1]))
    assert worst[1] <= 1.0 and worst[0] <= 1.0


def _near_tie_logits(C, kind, hi_first):
    """One pixel's logits: the top classes as `kind` says, every other class a multiple of 1/4 between -6 and -2.  hi_first:
    the winner sits below the runner-up's index."""
    rng = np.random.default_rng(C + len(kind))
    z = (rng.integers(-24, -7, C) / 4.0).astype(F32)
    i, j = (0, C - 1) if C < 4 else (1, C - 2)                          # two positions, i < j
    win, run = (i, j) if hi_first else (j, i)
    one = F32(1)
    if kind == 'tie2':
        z[i] = z[j] = one
    elif kind == 'tie3':
        z[i] = z[j] = z[(i + j) // 2] = one
    elif kind == 'ulp':
        z[win], z[run] = np.nextafter(one, F32(2)), one
    elif kind == '5e-6':
        z[win], z[run] = one + F32(5e-6), one
    elif kind == '2e-5':
        z[win], z[run] = one + F32(2e-5), one
    elif kind == 'equal':
        z[:] = F32(0.5)
    elif kind == 'saturated':
        z[:] = F32(-200)
        z[win] = F32(90)
    return z, win, run


NEAR_TIES = ['tie2', 'tie3', 'ulp', '5e-6', '2e-5', 'equal', 'saturated']


def _near_tie_case(C, kind, hi_first):
    """S constant over a 2x2 image and made of small integers, the fine structure in the bias: the 64 interior output pixels
    (rows and columns 4 .. 11, whose taps sum to 1) have logits of exactly z."""
    z, win, run = _near_tie_logits(C, kind, hi_first)
    s = (1 - np.arange(C) % 3).astype(F32)
    bias = (z - s).astype(F32)
    inexact = (bias.astype(F64) + s) != z.astype(F64)                   # there the whole logit goes into the bias
    s[inexact], bias[inexact] = 0, z[inexact]
    assert np.array_equal(bias.astype(F64) + s, z.astype(F64))
    return np.broadcast_to(s, (1, 2, 2, C)).astype(F64), bias, z, win, run


@pytest.mark.parametrize('hi_first', [True, False])
@pytest.mark.parametrize('kind', NEAR_TIES)
def test_decoder_head_near_ties_all_forms(ops, kind, hi_first):
    for C in HEAD_C:
        if C < (3 if kind == 'tie3' else 2):
            continue
        S, bias, z, win, run = _near_tie_case(C, kind, hi_first)
        out, zz, bound, err, err32 = _check_head_exact(ops, S, bias, C)
        assert _same_bits(zz[0, 4:12, 4:12], np.broadcast_to(z, (8, 8, C)))
        assert (err32 <= bound).all() and (err <= bound).all(), (C, kind)
        inner = out['label'][0, 4:12, 4:12]
        if kind in ('tie2', 'tie3', 'equal'):
            assert (inner == int(np.argmax(z))).all(), (C, kind)        # the lowest index of the tied classes
        else:
            # 2e-5 and the saturated row clear the runner-up by the counted bound at every class count, 5e-6 (about (C + 7) 2^-24
            # on either side) at the smaller ones; one ulp never does: there the softmax need not resolve the two
            clear = bool(_clear(*_softmax_ref(z[None]))[1].all())
            assert clear or kind in ('ulp', '5e-6'), (C, kind)
            assert (inner == win).all() if clear else np.isin(inner, (win, run)).all(), (C, kind)


def _head_random_case(C, shape=(2, 3, 5)):
    """Random S (std 3.5) and bias: the logits carry the five roundings of a * w00, three fmaf and the bias add."""
    rng = np.random.default_rng(50 + C)
    S = (rng.standard_normal(shape + (C,)) * 3.5).astype(F32)
    bias = rng.standard_normal(C).astype(F32)
    z = _up8(S) + bias.astype(F64)
    dz = 5 * EPS * (_up8_abs(S) + np.abs(bias.astype(F64))) * SLACK
    z32 = _up8_f32(S) + bias
    assert z32.dtype == F32
    ref, bound = _softmax_ref(z, dz)
    return dict(S=S, bias=bias, z=z, dz=dz, z32=z32, ref=ref, bound=bound, f32=_softmax_f32(z32))


HEAD_RANDOM_C = [3, 12, 13, 32]


@pytest.mark.parametrize('C', HEAD_RANDOM_C)
def test_decoder_head_from_scores_random_within_the_bound(ops, C):
    case = _head_random_case(C)
    out = _run_from_scores(ops, _padded_scores(case['S'], C), case['bias'], C)
    rk, rc = _report('decoder_head_from_scores score C=%d' % C, case['dz'], np.abs(out['score'] - case['z']),
                     np.abs(case['z32'] - case['z']))
    assert rc <= 1.0 and rk <= 1.0
    rk, rc = _report('decoder_head_from_scores prob C=%d' % C, case['bound'], np.abs(out['prob'] - case['ref']),
                     np.abs(case['f32'] - case['ref']))
    assert rc <= 1.0 and rk <= 1.0
    _check_labels(out['label'], out['prob'], case['ref'], case['bound'], LEFT_OUT)


def _head_chain_case(U, C, shape=(2, 3, 5), relu_input=True):
    """fused (non-negative bf16) -> 1x1 score at 1/8 resolution -> x8 -> + bias, float64; the logits' bound: the score conv's
    U roundings interpolated, then the head's five."""
    rng = np.random.default_rng(7 * U + C)
    f = rng.standard_normal(shape + (U,))
    fb = _bf16_bits((np.abs(f) if relu_input else f).astype(F32))
    ws = (rng.standard_normal((U, C)) * (3.0 / np.sqrt(U))).astype(F32)
    bias = rng.standard_normal(C).astype(F32)
    f64 = _bits_to_f64(fb)
    S = np.einsum('nhwu,uc->nhwc', f64, ws.astype(F64))
    eS = U * EPS * np.einsum('nhwu,uc->nhwc', np.abs(f64), np.abs(ws.astype(F64))) * SLACK
    z = _up8(S) + bias.astype(F64)
    dz = _up8_abs(eS) + 5 * EPS * (_up8_abs(np.abs(S) + eS) + np.abs(bias.astype(F64))) * SLACK
    S32 = np.zeros(shape + (C,), F32)
    for u in range(U):
        S32 = _fma32(f64[..., u, None], ws[u], S32)
    z32 = _up8_f32(S32) + bias
    ref, bound = _softmax_ref(z, dz)
    return dict(fb=fb, ws=ws, bias=bias, z=z, dz=dz, z32=z32, ref=ref, bound=bound, f32=_softmax_f32(z32))


CHAIN = [(U, C) for U in (8, 64, 256) for C in (3, 12, 32)]


def _run_head_fwd(ops, fb, ws, bias, C, short=0):
    n, hi, wi, _ = fb.shape
    dense = (n, 8 * hi, 8 * wi, C)
    score, prob, label = _Out(dense), _Out(dense), _Out(dense[:3], torch.int64)
    f, w, b = _act_from_bits(ops, fb), _dev(ws), _dev(bias)
    need = _lib().lib().xv_decoder_head_workspace_bytes(n, hi, wi, C)
    assert need == n * (hi + 2) * (wi + 2) * _cm(C) * 4
    wsp = torch.empty(need // 4, dtype=torch.float32, device='cuda')
    rc = _lib().lib().xv_decoder_head_fwd(f.xv(), ops._ptr(w), ops._ptr(b), C, ops._ptr(score.t), ops._ptr(prob.t),
                                          ops._ptr(label.t), ops._ptr(wsp), need - short, _stream())
    return rc, score, prob, label


@pytest.mark.parametrize('U,C', CHAIN)
def test_decoder_head_fwd_against_the_float64_chain(ops, U, C):
    case = _head_chain_case(U, C)
    rc, score, prob, label = _run_head_fwd(ops, case['fb'], case['ws'], case['bias'], C)
    assert rc == 0
    rk, rc32 = _report('decoder_head_fwd score U=%d C=%d' % (U, C), case['dz'], np.abs(score.get() - case['z']),
                       np.abs(case['z32'] - case['z']))
    assert rc32 <= 1.0 and rk <= 1.0
    rk, rc32 = _report('decoder_head_fwd prob U=%d C=%d' % (U, C), case['bound'], np.abs(prob.get() - case['ref']),
                       np.abs(case['f32'] - case['ref']))
    assert rc32 <= 1.0 and rk <= 1.0
    _check_labels(label.get(), prob.get(), case['ref'], case['bound'], LEFT_OUT)


def test_decoder_head_fwd_workspace_one_byte_short(ops):
    case = _head_chain_case(8, 3)
    rc, score, prob, label = _run_head_fwd(ops, case['fb'], case['ws'], case['bias'], 3, short=1)
    assert rc == _code('XV_EWORKSPACE')
    assert score.untouched() and prob.untouched() and label.untouched()


# ---- c. xv_decoder_head_affine_fwd ----------------------------------------------------------------------------------------------

AFFINE_MAPS = [(1, 1, 1), (2, 3, 5), (1, 2, 17)]          # the last: 136 output columns, a second, partial 128-column tile


def _run_affine(ops, fb, scale, shift, ws, bias, C, label_offset=0):
    n, hi, wi, _ = fb.shape
    dense = (n, 8 * hi, 8 * wi, C)
    score, prob, label = _Out(dense), _Out(dense), _Out(dense[:3], torch.int64, offset=label_offset)
    keep = [_act_from_bits(ops, fb)] + [_dev(a) for a in (scale, shift, ws, bias)]
    rc = _lib().lib().xv_decoder_head_affine_fwd(keep[0].xv(), *([ops._ptr(t) for t in keep[1:]] +
                                                 [C, ops._ptr(score.t), ops._ptr(prob.t), ops._ptr(label.t), _stream()]))
    return rc, score, prob, label


def _affine_features(f64, scale, shift):
    return np.maximum(_up8(f64) * scale.astype(F64) + shift.astype(F64), 0.0)


@pytest.mark.parametrize('C', [1, 3, 12, 13, 32])
@pytest.mark.parametrize('U', [8, 16, 24, 64, 72])
def test_decoder_head_affine_integers_bit_for_bit(ops, U, C):
    """Integer f up to 4, scale a power of two, integer shift and weights: relu(up8(f) scale + shift) is a multiple of 1/512
    below 16 and the score an exact float32, whatever the order.  The shift cuts about half of the features."""
    for n, hi, wi in AFFINE_MAPS:
        rng = np.random.default_rng(U + C + n * hi * wi)
        f = rng.integers(-4, 5, (n, hi, wi, U)).astype(F32)
        scale = rng.choice(np.array([0.5, 1.0, 2.0], F32), U)
        shift = rng.integers(-1, 2, U).astype(F32)
        ws = rng.integers(-2, 3, (U, C)).astype(F32)
        bias = rng.integers(-3, 4, C).astype(F32)
        up = _affine_features(f.astype(F64), scale, shift)
        assert hi * wi == 1 or 0.25 < (up == 0).mean() < 0.75
        z64 = np.einsum('nhwu,uc->nhwc', up, ws.astype(F64)) + bias
        z = z64.astype(F32)
        assert np.array_equal(z.astype(F64), z64)
        rc, score, prob, label = _run_affine(ops, _bf16_bits(f), scale, shift, ws, bias, C)
        assert rc == 0
        assert _same_bits(score.get(), z), (n, hi, wi)
        ref, bound = _softmax_ref(z)
        assert (np.abs(_softmax_f32(z) - ref) <= bound).all() and (np.abs(prob.get() - ref) <= bound).all()
        _check_labels(label.get(), prob.get(), ref, bound)
        _check_exact_ties(label.get(), z)


def _affine_random_case(U, C=13, shape=(2, 3, 5), identity=False):
    """relu(up8(f) * scale + shift) @ W + b in float64.  Roundings: four of the interpolation (two row blends, a product and a
    fused multiply-add across the columns), one of the affine (a fused multiply-add; two where the compiler does not fuse),
    one per feature of the score's fmaf chain, one of the bias add."""
    rng = np.random.default_rng(13 * U + C)
    f = rng.standard_normal(shape + (U,))
    fb = _bf16_bits((np.abs(f) if identity else f).astype(F32))
    scale = np.ones(U, F32) if identity else (1.0 + 0.3 * rng.standard_normal(U)).astype(F32)
    shift = np.zeros(U, F32) if identity else (0.5 * rng.standard_normal(U)).astype(F32)
    ws = (rng.standard_normal((U, C)) * (3.0 / np.sqrt(U))).astype(F32)
    bias = rng.standard_normal(C).astype(F32)
    f64, s64, t64, w64 = _bits_to_f64(fb), scale.astype(F64), shift.astype(F64), ws.astype(F64)
    I, IA = _up8(f64), _up8_abs(f64)
    pre = I * s64 + t64
    up = np.maximum(pre, 0.0)
    e_up = np.abs(s64) * 4 * EPS * IA + 2 * EPS * (np.abs(s64) * IA + np.abs(t64))
    z = np.einsum('nhwu,uc->nhwc', up, w64) + bias
    A = np.einsum('nhwu,uc->nhwc', up + e_up, np.abs(w64))
    dz = (np.einsum('nhwu,uc->nhwc', e_up, np.abs(w64)) + U * EPS * A + EPS * (A + np.abs(bias))) * SLACK
    # float32 on the CPU in the kernel's order: rows first, then columns, the affine fused, features in ascending order
    fp = _pad_hw(f64.astype(F32))
    hi, wi = shape[1], shape[2]
    iy, wy1, wy0 = _taps8(hi)
    ix, wx1, wx0 = _taps8(wi)
    rows = _fma32(fp[:, iy], wy0[None, :, None, None], fp[:, iy + 1] * wy1[None, :, None, None])        # [n][8hi][wi+2][U]
    v0, v1 = rows[:, :, ix], rows[:, :, ix + 1]
    up32 = _fma32(v0, wx0[None, None, :, None], v1 * wx1[None, None, :, None])
    up32 = np.maximum(_fma32(up32, scale, shift), F32(0))
    z32 = np.zeros(z.shape, F32)
    for u in range(U):
        z32 = _fma32(up32[..., u, None], ws[u], z32)
    z32 = z32 + bias
    ref, bound = _softmax_ref(z, dz)
    return dict(fb=fb, scale=scale, shift=shift, ws=ws, bias=bias, z=z, dz=dz, z32=z32, ref=ref, bound=bound,
                f32=_softmax_f32(z32), cut=float((pre < 0).mean()))


AFFINE_U = [8, 16, 24, 64, 72]


@pytest.mark.parametrize('U', AFFINE_U)
def test_decoder_head_affine_random_within_the_bound(ops, U):
    C = 13
    case = _affine_random_case(U)
    assert 0.3 < case['cut'] < 0.7                                      # the relu cuts about half of the features
    rc, score, prob, label = _run_affine(ops, case['fb'], case['scale'], case['shift'], case['ws'], case['bias'], C)
    assert rc == 0
    rk, rc32 = _report('decoder_head_affine score U=%d' % U, case['dz'], np.abs(score.get() - case['z']),
                       np.abs(case['z32'] - case['z']))
    assert rc32 <= 1.0 and rk <= 1.0
    rk, rc32 = _report('decoder_head_affine prob U=%d' % U, case['bound'], np.abs(prob.get() - case['ref']),
                       np.abs(case['f32'] - case['ref']))
    assert rc32 <= 1.0 and rk <= 1.0
    _check_labels(label.get(), prob.get(), case['ref'], case['bound'], LEFT_OUT)


@pytest.mark.parametrize('U', [8, 64])
def test_decoder_head_affine_identity_commutes_with_the_default_head(ops, U):
    """scale 1, shift 0, f >= 0: relu(up8(f)) = up8(f), and the default head's 1x1 conv in front of the interpolation computes
    the same scores -- each within its own counted bound of the one float64 value."""
    C = 13
    a = _affine_random_case(U, identity=True)
    f64, w64 = _bits_to_f64(a['fb']), a['ws'].astype(F64)                 # the default head's bound on the same operands
    S = np.einsum('nhwu,uc->nhwc', f64, w64)
    eS = U * EPS * np.einsum('nhwu,uc->nhwc', np.abs(f64), np.abs(w64)) * SLACK
    dz_head = _up8_abs(eS) + 5 * EPS * (_up8_abs(np.abs(S) + eS) + np.abs(a['bias'].astype(F64))) * SLACK
    rc, score, _, _ = _run_affine(ops, a['fb'], a['scale'], a['shift'], a['ws'], a['bias'], C)
    assert rc == 0
    rc, score_h, _, _ = _run_head_fwd(ops, a['fb'], a['ws'], a['bias'], C)
    assert rc == 0
    sa, sh = score.get().astype(F64), score_h.get().astype(F64)
    assert (np.abs(sa - a['z']) <= a['dz']).all() and (np.abs(sh - a['z']) <= dz_head).all()
    assert (np.abs(sa - sh) <= a['dz'] + dz_head).all()


def test_decoder_head_affine_refuses_a_label_pointer_it_cannot_store_pairs_to(ops):
    """The kernel stores labels in 16-byte pairs: a label pointer offset by 8 bytes is XV_EINVAL before any launch."""
    a = _affine_random_case(8)
    rc, score, prob, label = _run_affine(ops, a['fb'], a['scale'], a['shift'], a['ws'], a['bias'], 13, label_offset=1)
    assert rc == _code('XV_EINVAL')
    assert score.untouched() and prob.untouched() and label.untouched()


# ---- d. xv_softmax_argmax ---------------------------------------------------------------------------------------------------------

def _softmax_rows(C, npix, seed=0):
    """Random logits (std 3.5) with, in front, the rows of the near-tie list and logits spanning +-80."""
    rng = np.random.default_rng(1000 * C + npix + seed)
    z = (rng.standard_normal((npix, C)) * 3.5).astype(F32)
    special = [np.linspace(-80, 80, C).astype(F32) if C > 1 else np.array([80], F32)]
    for kind in NEAR_TIES:
        for hi_first in (True, False):
            if C >= (3 if kind == 'tie3' else 2):
                special.append(_near_tie_logits(C, kind, hi_first)[0])
    for i, row in enumerate(special[:npix]):
        z[i] = row
    return z, special


def _run_softmax(ops, zt, C, want_prob, want_label):
    npix = zt.shape[0]
    prob = _Out((npix, C)) if want_prob else None
    label = _Out((npix, 1), torch.int64) if want_label else None
    rc = _lib().lib().xv_softmax_argmax(ops._ptr(zt), npix, C, ops._ptr(prob.t if prob else None),
                                        ops._ptr(label.t if label else None), _stream())
    assert rc == 0
    return (prob.get() if prob else None), (label.get()[:, 0] if label else None)


def _check_softmax(ops, z, name=None, limit=None):
    C = z.shape[1]
    zt = _dev(z)
    assert zt.data_ptr() % 16 == 0
    prob, label = _run_softmax(ops, zt, C, True, True)
    prob_alone, _ = _run_softmax(ops, zt, C, True, False)
    _, label_alone = _run_softmax(ops, zt, C, False, True)
    assert _same_bits(prob_alone, prob) and np.array_equal(label_alone, label)
    ref, bound = _softmax_ref(z)
    err, err32 = np.abs(prob - ref), np.abs(_softmax_f32(z) - ref)
    if name:
        rk, rc = _report(name, bound, err, err32)
        assert rc <= 1.0 and rk <= 1.0
    else:
        assert (err32 <= bound).all() and (err <= bound).all()
    _check_labels(label, prob, ref, bound, limit)
    _check_exact_ties(label, z)
    return prob, label


SOFTMAX_C = [1, 2, 4, 11, 12, 13, 16, 17, 31, 32]


@pytest.mark.parametrize('C', SOFTMAX_C)
def test_softmax_argmax_against_float64(ops, C):
    for npix in (255, 257):
        _check_softmax(ops, _softmax_rows(C, npix)[0], 'softmax_argmax C=%d npix=%d' % (C, npix))
    z, special = _softmax_rows(C, 257)
    for row in special + [z[-1]]:                                       # npix = 1: every special row as a map of its own
        _check_softmax(ops, row[None].copy())


def test_softmax_argmax_random_rows_leave_few_pixels_out(ops):
    for C in SOFTMAX_C:
        z = (np.random.default_rng(C).standard_normal((4099, C)) * 3.5).astype(F32)
        _check_softmax(ops, z, limit=LEFT_OUT)


def test_softmax_argmax_unaligned_12_classes_equal_the_vector_form(ops):
    """C = 12 from a score view offset by 4 bytes: the <16> form.  The same bits as the aligned <12> vector form."""
    for npix in (1, 255, 257):
        z = _softmax_rows(12, npix)[0]
        prob, label = _check_softmax(ops, z)
        zt = _offset_input(z)
        prob_u, label_u = _run_softmax(ops, zt, 12, True, True)
        assert _same_bits(prob_u, prob) and np.array_equal(label_u, label)
        assert np.array_equal(_run_softmax(ops, zt, 12, False, True)[1], label)


def test_softmax_argmax_grid_stride_loop(ops):
    npix = GRID_CAP * 256 + 3
    z = (np.random.default_rng(5).standard_normal((npix, 5)) * 3.5).astype(F32)
    zt = _dev(z)
    prob, label = _run_softmax(ops, zt, 5, True, True)
    ref, bound = _softmax_ref(z)
    assert (np.abs(prob - ref) <= bound).all()
    _check_labels(label, prob, ref, bound, LEFT_OUT)


# ---- e. xv_bayes_fuse and xv_bayes_fuse_lut ---------------------------------------------------------------------------------------

NPIX_BAYES = [1, 2, 3, 255, 257, 4099]


def _bayes_labels(rng, E, npix, C):
    lab = rng.integers(0, C, (E, npix)).astype(np.int64)
    odd = np.array([-1, C, 1 << 40], np.int64)
    pick = rng.random((E, npix)) < 0.1
    lab[pick] = odd[rng.integers(0, 3, int(pick.sum()))]
    if npix >= 3:
        lab[0, :3], lab[-1, -3:] = odd, odd[::-1]
    return lab


def _bayes_case(E, C, npix, integers=False, seed=0):
    """score = ((ll_0 + ll_1) + ...) + logprior of the clamped labels: float32 in that order, float64, and the bound of the E
    roundings."""
    rng = np.random.default_rng(100 * E + C + npix + seed)
    if integers:
        loglik, prior = rng.integers(-3, 4, (E, C, C)).astype(F32), rng.integers(-2, 3, C).astype(F32)
    else:
        loglik, prior = rng.standard_normal((E, C, C)).astype(F32), rng.standard_normal(C).astype(F32)
    lab = _bayes_labels(rng, E, npix, C)
    cl = np.clip(lab, 0, C - 1)
    terms = [loglik[e][cl[e]] for e in range(E)] + [np.broadcast_to(prior, (npix, C))]
    f32, ref, A = terms[0], terms[0].astype(F64), np.abs(terms[0].astype(F64))
    for t in terms[1:]:
        f32, ref, A = f32 + t, ref + t, A + np.abs(t)
    assert f32.dtype == F32
    return dict(loglik=loglik, prior=prior, lab=lab, f32=f32, ref=ref, bound=E * EPS * A * SLACK)


def _run_bayes(ops, labs, loglik, prior, C, want_score):
    E, npix = len(labs), labs[0].numel()
    fused = _Out((npix, 1), torch.int64)
    score = _Out((npix, C)) if want_score else None
    ll, lp = _dev(loglik), _dev(prior)
    rc = _lib().lib().xv_bayes_fuse(ops._ptr_array(labs), E, ops._ptr(ll), ops._ptr(lp), C, npix, ops._ptr(fused.t),
                                    ops._ptr(score.t if score else None), _stream())
    assert rc == 0
    return fused.get()[:, 0], (score.get() if score else None)


def _check_bayes(ops, case, E, C, limit=None):
    labs = [_dev(l) for l in case['lab']]
    assert all(t.data_ptr() % 16 == 0 for t in labs)
    label, score = _run_bayes(ops, labs, case['loglik'], case['prior'], C, True)             # the generic kernel
    assert _same_bits(score, case['f32'])
    assert (np.abs(case['f32'] - case['ref']) <= case['bound']).all()
    _check_labels(label, score, case['ref'], case['bound'], limit)
    plain, _ = _run_bayes(ops, labs, case['loglik'], case['prior'], C, False)                # E = 2: the pair kernel
    assert np.array_equal(plain, label)
    if E == 2:                                                          # one label map offset by 8 bytes: the generic kernel
        shifted, _ = _run_bayes(ops, [labs[0], _offset_input(case['lab'][1])], case['loglik'], case['prior'], C, False)
        assert np.array_equal(shifted, label)
    return label, score


@pytest.mark.parametrize('C', [1, 2, 12, 16, 17, 32])
@pytest.mark.parametrize('E', [1, 2, 3, 4])
def test_bayes_fuse_every_form(ops, E, C):
    for npix in NPIX_BAYES:
        case = _bayes_case(E, C, npix)
        _, score = _check_bayes(ops, case, E, C, LEFT_OUT if npix == 4099 else None)
        if npix == 4099:
            rk, rc = _report('bayes_fuse E=%d C=%d' % (E, C), case['bound'], np.abs(score - case['ref']),
                             np.abs(case['f32'] - case['ref']))
            assert rc <= 1.0 and rk <= 1.0
        case = _bayes_case(E, C, npix, integers=True)                   # exact sums, many exact ties: the lowest index
        label, _ = _check_bayes(ops, case, E, C)
        assert np.array_equal(case['f32'].astype(F64), case['ref']) and np.array_equal(label, case['ref'].argmax(-1))


def test_bayes_fuse_pair_kernel_grid_stride_loop(ops):
    """Past the pair kernel's grid of 8 workgroups per CU, two pixels a thread, and an odd tail.  C = 2: the smallest class
    count at which a label carries information."""
    npix = _cus() * 8 * 256 * 2 + 5
    case = _bayes_case(2, 2, npix)
    labs = [_dev(l) for l in case['lab']]
    plain, _ = _run_bayes(ops, labs, case['loglik'], case['prior'], 2, False)
    assert np.array_equal(plain, case['f32'].argmax(-1))


def test_bayes_fuse_generic_kernel_grid_stride_loop(ops):
    npix = GRID_CAP * 256 + 3
    case = _bayes_case(1, 2, npix)
    label, score = _run_bayes(ops, [_dev(case['lab'][0])], case['loglik'], case['prior'], 2, True)
    assert _same_bits(score, case['f32']) and np.array_equal(label, case['f32'].argmax(-1))


def _run_lut(ops, a, b, lut, C):
    npix = a.shape[0]
    fused = _Out((npix, 1), torch.int64)
    ta, tb, tl = _dev(a), _dev(b), _dev(lut)
    rc = _lib().lib().xv_bayes_fuse_lut(ops._ptr(ta), ops._ptr(tb), ops._ptr(tl), C, npix, ops._ptr(fused.t), _stream())
    return rc, fused


def _lut_case(C, npix):
    rng = np.random.default_rng(C + npix)
    lab = _bayes_labels(rng, 2, npix, C)
    lut = rng.integers(0, C, (C, C)).astype(np.int64)
    cl = np.clip(lab, 0, C - 1)
    return lab, lut, lut[cl[0], cl[1]]


@pytest.mark.parametrize('C', [1, 12, 33, 64])
def test_bayes_fuse_lut_exact(ops, C):
    for npix in NPIX_BAYES + ([GRID_CAP * 256 + 3] if C == 12 else []):         # C = 12 also past the capped grid
        lab, lut, want = _lut_case(C, npix)
        rc, fused = _run_lut(ops, lab[0], lab[1], lut, C)
        assert rc == 0
        assert np.array_equal(fused.get()[:, 0], want), npix


def test_bayes_fuse_lut_refuses_65_classes(ops):
    lab, lut, _ = _lut_case(65, 255)
    rc, fused = _run_lut(ops, lab[0], lab[1], lut, 65)
    assert rc == _code('XV_ESHAPE')
    assert fused.untouched()


# ---- f. xv_dirichlet_fuse -------------------------------------------------------------------------------------------------------

NPIX = [1, 255, 257, 4099]


def _prob_rows(rng, E, npix, C, special=True):
    """Softmax rows of random logits (std 3) as float32; in front: a row with exact zeros, a one-hot row, rows that sum to 0.5
    and to 3 (never an all-zero row)."""
    z = rng.standard_normal((E, npix, C)) * 3.0
    e = np.exp(z - z.max(-1, keepdims=True))
    P = (e / e.sum(-1, keepdims=True)).astype(F32)
    if special:
        if npix > 0:
            P[:, 0, 1::2] = 0
        if npix > 1:
            P[:, 1] = 0
            P[np.arange(E), 1, rng.integers(0, C, E)] = 1
        if npix > 2:
            P[:, 2] *= F32(0.5)
        if npix > 3:
            P[:, 3] *= F32(3)
    assert (P.sum(-1) > 0).all()
    return P


def _dirichlet_case(E, C, npix, seed=0):
    """dirichlet_mix.py:14-36 in float64: q = p / sum p, lx = ln(1e-20 + q), L_e[c] = sum_k am1_e[c][k] lx[k] - lognorm_e[c],
    score = (sum_e L_e) + logprior.  Bound: the argument of the log carries C - 1 roundings of the sum, one ulp of the
    reciprocal and the fused multiply-add's rounding ((C + 2) 2^-24 relative, on the q part); the log one ulp of v_log_f32 and two
    roundings of the product with ln 2 (4 x 2^-24 |lx|); every dot product C roundings of its fmaf chain; one rounding each for
    - lognorm, every + L_e and + logprior."""
    rng = np.random.default_rng(100 * E + C + npix + seed)
    P = _prob_rows(rng, E, npix, C)
    am1 = (rng.random((E, C, C)) - 0.5 + 4 * np.eye(C)).astype(F32)
    lognorm, prior = (rng.standard_normal((E, C)) * 0.1).astype(F32), (rng.standard_normal(C) * 0.1).astype(F32)
    P64, a64, tiny = P.astype(F64), am1.astype(F64), F64(TINY)
    q = P64 / P64.sum(-1, keepdims=True)
    lx = np.log(tiny + q)
    e_lx = (C + 2) * EPS * q / (tiny + q) * SLACK + 4 * EPS * np.abs(lx)
    dot = np.einsum('eck,epk->epc', a64, lx)
    e_dot = np.einsum('eck,epk->epc', np.abs(a64), e_lx) + C * EPS * np.einsum('eck,epk->epc', np.abs(a64), np.abs(lx))
    L = dot - lognorm[:, None, :]
    e_L = e_dot + EPS * (np.abs(dot) + np.abs(lognorm[:, None, :]))
    ref = L.sum(0) + prior
    bound = (e_L.sum(0) + E * EPS * (np.abs(L).sum(0) + np.abs(prior))) * 1.01
    # float32 on the CPU in the kernels' order
    s = np.zeros((E, npix), F32)
    for k in range(C):
        s = s + P[..., k]
    lx32 = np.log2(_fma32(P, (F32(1) / s)[..., None], TINY)) * LN2
    d = np.zeros((E, npix, C), F32)
    for k in range(C):
        d = _fma32(am1[:, None, :, k], lx32[:, :, None, k], d)
    L32 = d - lognorm[:, None, :]
    f32 = L32[0]
    for e in range(1, E):
        f32 = f32 + L32[e]
    f32 = f32 + prior
    assert f32.dtype == F32
    return dict(P=P, am1=am1, lognorm=lognorm, prior=prior, ref=ref, bound=bound, f32=f32)


def _run_dirichlet(ops, probs, case, C, want_score=True, score_offset=0):
    E, npix = len(probs), probs[0].shape[0]
    fused = _Out((npix, 1), torch.int64)
    score = _Out((npix, C), offset=score_offset) if want_score else None
    keep = [_dev(case[k]) for k in ('am1', 'lognorm', 'prior')]
    rc = _lib().lib().xv_dirichlet_fuse(ops._ptr_array(probs), E, ops._ptr(keep[0]), ops._ptr(keep[1]), ops._ptr(keep[2]), C,
                                        npix, ops._ptr(fused.t), ops._ptr(score.t if score else None), _stream())
    assert rc == 0
    return fused.get()[:, 0], (score.get() if score else None)


def _dirichlet_probs(case, misalign):
    probs = [_dev(p) for p in case['P']]
    assert all(t.data_ptr() % 16 == 0 for t in probs)
    if misalign == 'prob':
        probs[-1] = _offset_input(case['P'][-1])
    return probs


def _check_dirichlet(ops, name, case, C, misalign=None, limit=None):
    probs = _dirichlet_probs(case, misalign)
    label, score = _run_dirichlet(ops, probs, case, C, score_offset=1 if misalign == 'score' else 0)
    rk, rc = _report(name, case['bound'], np.abs(score - case['ref']), np.abs(case['f32'] - case['ref']))
    assert rc <= 1.0 and rk <= 1.0
    _check_labels(label, score, case['ref'], case['bound'], limit)
    if misalign != 'score':                                             # (without a score output the packed kernel would run)
        assert np.array_equal(_run_dirichlet(ops, probs, case, C, want_score=False)[0], label)
    return label, score


DIRICHLET_BRANCHES = (
    [('packed', 12, 2, None)] + [('exact12', 12, E, None) for E in (1, 3, 4)] + [('exact12-score-offset', 12, 2, 'score'),
                                                                                  ('scalar16-prob-offset', 12, 2, 'prob')] +
    [('vector16', C, E, None) for C in (4, 8, 16) for E in (1, 2, 3, 4)] +
    [('scalar16', C, E, None) for C in (1, 3, 13) for E in (1, 2, 3, 4)] +
    [('kernel32', C, E, None) for C in (17, 20, 32) for E in (1, 2, 3, 4)])


@pytest.mark.parametrize('branch,C,E,misalign', DIRICHLET_BRANCHES, ids=['%s-C%d-E%d' % b[:3] for b in DIRICHLET_BRANCHES])
def test_dirichlet_fuse_branch(ops, branch, C, E, misalign):
    for npix in NPIX:
        _check_dirichlet(ops, 'dirichlet_fuse %s C=%d E=%d npix=%d' % (branch, C, E, npix), _dirichlet_case(E, C, npix), C,
                         misalign, LEFT_OUT if npix == 4099 else None)


def test_dirichlet_fuse_12_class_branches_give_the_same_bits(ops):
    """The packed kernel, <12, EXACT> (score offset by 4 bytes) and the <16> scalar form (a probability map offset by 4 bytes):
    the same fmaf chains, so the same scores bit for bit on the same values."""
    for npix in NPIX:
        case = _dirichlet_case(2, 12, npix)
        outs = [_check_dirichlet(ops, 'dirichlet_fuse C=12 %s npix=%d' % (m, npix), case, 12, m) for m in (None, 'score', 'prob')]
        for label, score in outs[1:]:
            assert _same_bits(score, outs[0][1]) and np.array_equal(label, outs[0][0])


@pytest.mark.parametrize('branch,C,cap', [('exact12', 12, None), ('vector16', 4, GRID_CAP)])
def test_dirichlet_fuse_grid_stride_loop(ops, branch, C, cap):
    npix = (cap or _cus() * 8) * 256 + 3
    case = _dirichlet_case(1, C, npix)
    probs = _dirichlet_probs(case, None)
    label, score = _run_dirichlet(ops, probs, case, C)
    assert (np.abs(case['f32'] - case['ref']) <= case['bound']).all() and (np.abs(score - case['ref']) <= case['bound']).all()
    _check_labels(label, score, case['ref'], case['bound'], LEFT_OUT)


# ---- g. xv_average_fuse and xv_variance_fuse --------------------------------------------------------------------------------------

FUSE_C = [1, 3, 4, 12, 14, 16, 17, 32]


def _tied_rows(P):
    """Rows 4 .. 7 (where there are that many): every expert holds the same row with two equal largest classes."""
    E, npix, C = P.shape
    if npix > 7 and C > 1:
        P[:, 4:8] = P[0, 4:8]
        top = P[0, 4:8].argmax(-1)
        P[:, np.arange(4, 8), (top + 1) % C] = P[0, np.arange(4, 8), top]
    return P


def _average_case(E, C, npix, seed=0):
    """((p_0 + p_1) + ...) / E in float32, experts in ascending order, an IEEE division."""
    rng = np.random.default_rng(100 * E + C + npix + seed)
    P = _tied_rows(_prob_rows(rng, E, npix, C))
    s = P[0]
    for e in range(1, E):
        s = s + P[e]
    f32 = s / F32(E)
    assert f32.dtype == F32
    return dict(P=P, f32=f32, label=f32.argmax(-1))


def _run_average(ops, probs, C):
    npix = probs[0].shape[0]
    fused = _Out((npix, 1), torch.int64)
    rc = _lib().lib().xv_average_fuse(ops._ptr_array(probs), len(probs), C, npix, ops._ptr(fused.t), _stream())
    assert rc == 0
    return fused.get()[:, 0]


@pytest.mark.parametrize('C', FUSE_C)
@pytest.mark.parametrize('E', [1, 2, 3, 4])
def test_average_fuse_labels_of_the_same_order_float32_mean(ops, E, C):
    for npix in NPIX:
        case = _average_case(E, C, npix)
        probs = [_dev(p) for p in case['P']]
        assert np.array_equal(_run_average(ops, probs, C), case['label']), npix
        probs[-1] = _offset_input(case['P'][-1])                        # one map offset by 4 bytes: the scalar row loads
        assert np.array_equal(_run_average(ops, probs, C), case['label']), npix


def test_average_fuse_grid_stride_loop(ops):
    """C = 2: the smallest class count at which a label carries information."""
    case = _average_case(1, 2, GRID_CAP * 256 + 3)
    assert np.array_equal(_run_average(ops, [_dev(case['P'][0])], 2), case['label'])


VARIANCES = np.array([0.0, 1e-30, 1.0, 1e30], F32)


def _variance_case(E, C, npix, seed=0):
    """variance_mix.py:7-15 in float64: sum_e p_e c_e / sum_e c_e, c_e = 1 / (1e-20 + var_e).  Every term is non-negative: c_e
    two roundings, the numerator E more, the denominator E - 1, the division one -- (2 E + 4) 2^-24 relative; products below
    the normal range round at 2^-149 before the division by the sum of the certainties."""
    rng = np.random.default_rng(100 * E + C + npix + seed)
    P = _tied_rows(_prob_rows(rng, E, npix, C))
    var = VARIANCES[rng.integers(0, 4, (E, npix))]
    if npix >= 4:
        var[:, :4] = VARIANCES                                          # every value in every expert, and all four against each other
        var[-1, :4] = VARIANCES[::-1]
    c64 = 1.0 / (F64(TINY) + var.astype(F64))
    ref = (P.astype(F64) * c64[..., None]).sum(0) / c64.sum(0)[:, None]
    bound = ref * (2 * E + 4) * EPS * SLACK + ((E + 1) * 2.0 ** -149 / c64.sum(0))[:, None] + 2.0 ** -149
    c = F32(1) / (TINY + var)
    acc, cs = P[0] * c[0][:, None], c[0]
    for e in range(1, E):
        acc, cs = _fma32(P[e], c[e][:, None], acc), cs + c[e]
    f32 = acc / cs[:, None]
    assert f32.dtype == F32
    return dict(P=P, var=var, ref=ref, bound=bound, f32=f32)


def _run_variance(ops, probs, vars_, C, want_label, want_score):
    npix = probs[0].shape[0]
    fused = _Out((npix, 1), torch.int64) if want_label else None
    score = _Out((npix, C)) if want_score else None
    rc = _lib().lib().xv_variance_fuse(ops._ptr_array(probs), ops._ptr_array(vars_), len(probs), C, npix,
                                       ops._ptr(fused.t if fused else None), ops._ptr(score.t if score else None), _stream())
    return rc, (fused.get()[:, 0] if fused and rc == 0 else None), (score.get() if score and rc == 0 else None)


def _check_variance(ops, name, case, C, misalign=False, limit=None):
    probs, vars_ = [_dev(p) for p in case['P']], [_dev(v) for v in case['var']]
    if misalign:
        probs[-1] = _offset_input(case['P'][-1])
    rc, label, score = _run_variance(ops, probs, vars_, C, True, True)
    assert rc == 0
    rk, rc32 = _report(name, case['bound'], np.abs(score - case['ref']), np.abs(case['f32'] - case['ref']))
    assert rc32 <= 1.0 and rk <= 1.0
    _check_labels(label, score, case['ref'], case['bound'], limit)
    assert np.array_equal(_run_variance(ops, probs, vars_, C, True, False)[1], label)
    assert _same_bits(_run_variance(ops, probs, vars_, C, False, True)[2], score)
    if case['P'].shape[1] > 7 and C > 1:                                # the tied rows: the lower of the two equal classes
        top = case['P'][0, 4:8].argmax(-1)
        assert np.array_equal(label[4:8], np.minimum(top, (top + 1) % C))
    return label, score


@pytest.mark.parametrize('C', FUSE_C)
@pytest.mark.parametrize('E', [1, 2, 3, 4])
def test_variance_fuse_against_float64(ops, E, C):
    for npix in NPIX:
        case = _variance_case(E, C, npix)
        limit = LEFT_OUT if npix == 4099 else None
        label, score = _check_variance(ops, 'variance_fuse E=%d C=%d npix=%d' % (E, C, npix), case, C, limit=limit)
        label_u, score_u = _check_variance(ops, 'variance_fuse E=%d C=%d npix=%d offset' % (E, C, npix), case, C, misalign=True)
        assert np.array_equal(label_u, label) and _same_bits(score_u, score)


def test_variance_fuse_grid_stride_loop(ops):
    case = _variance_case(1, 2, GRID_CAP * 256 + 3)
    _check_variance(ops, 'variance_fuse past the capped grid', case, 2, limit=LEFT_OUT)


def test_variance_fuse_without_an_output_is_refused(ops):
    case = _variance_case(2, 3, 255)
    rc, _, _ = _run_variance(ops, [_dev(p) for p in case['P']], [_dev(v) for v in case['var']], 3, False, False)
    assert rc == _code('XV_EINVAL')


# ---- the random-valued cases above, for the companion that checks the references without a GPU -------------------------------

def reference_cases():
    """(name, float64 reference, bound, float32 evaluation on the CPU, whether check (2) must leave out at most LEFT_OUT)."""
    for U in (8, 24, 64, 256):
        c = _score_lowres_case(U)
        yield 'score_lowres U=%d' % U, c['ref'], c['bound'], c['f32'], False
    heads = [('from_scores C=%d' % C, _head_random_case(C)) for C in HEAD_RANDOM_C]
    heads += [('head_fwd U=%d C=%d' % (U, C), _head_chain_case(U, C)) for U, C in CHAIN]
    heads += [('affine U=%d' % U, _affine_random_case(U)) for U in AFFINE_U]
    heads += [('affine identity U=%d' % U, _affine_random_case(U, identity=True)) for U in (8, 64)]
    for name, c in heads:
        yield name + ' score', c['z'], c['dz'], c['z32'], False
        yield name + ' prob', c['ref'], c['bound'], c['f32'], not name.startswith('affine identity')
    for C in SOFTMAX_C:
        for npix in (255, 257):
            z = _softmax_rows(C, npix)[0]
            yield ('softmax rows C=%d npix=%d' % (C, npix),) + _softmax_ref(z) + (_softmax_f32(z), False)
        z = (np.random.default_rng(C).standard_normal((4099, C)) * 3.5).astype(F32)
        yield ('softmax random C=%d' % C,) + _softmax_ref(z) + (_softmax_f32(z), True)
    for E in (1, 2, 3, 4):
        for C in (1, 2, 12, 16, 17, 32):
            c = _bayes_case(E, C, 4099)
            yield 'bayes E=%d C=%d' % (E, C), c['ref'], c['bound'], c['f32'], True
        for C in FUSE_C:
            c = _variance_case(E, C, 4099)
            yield 'variance E=%d C=%d' % (E, C), c['ref'], c['bound'], c['f32'], True
    for branch, C, E, _ in DIRICHLET_BRANCHES:
        for npix in NPIX:
            c = _dirichlet_case(E, C, npix)
            yield 'dirichlet %s C=%d E=%d npix=%d' % (branch, C, E, npix), c['ref'], c['bound'], c['f32'], npix == 4099
