"""The inference-side pointwise and data-movement kernels at their edges: max-pool, x2 bilinear upsample, concat, add, subsample,
dropout (all six forms), the 7x7-stride-2 gather and the dilated im2col pair (row and flat forms), the phase shuffles of the
dense transposed convs and the bf16 -> float32 map copy.

Conventions of test_training_kernels_edges_gpu.py, whose helpers are imported: operands are built from bf16 bit patterns, the
whole padded buffer is compared (interior and zero border), outputs are prefilled with a non-zero pattern so that an unwritten
element shows, and every reference is numpy / torch-CPU and calls no kernel.  Everything is compared bit for bit except (i) the
pool window that holds +0 and -0.0 only as its maximum, whose sign IEEE leaves open, and (ii) the random-valued upsample and
depth-to-space cases, which are held to a per-element bound counted from the roundings of the arithmetic; the same formulas in
float32 on the CPU are held to the same bound first, and each such test prints the bound and both error-to-bound ratios."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import fcn_oracle as fo
from test_training_kernels_edges_gpu import BF16, EPS, MAPS, NEG0, NEGSUB, POS0, SUB
from test_training_kernels_edges_gpu import _act_bits, _act_from_bits, _bf16_bits, _bits_to_f64, _border_is_zero, _dev, _padded
from test_training_kernels_edges_gpu import ops  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

CHANNELS = [8, 24, 64, 192]          # one 16-byte group, not a power of two, the usual count, three times 64
CAP = 8192 * 256                     # threads of the capped grid (xv_grid_for): one 16-byte group of eight each per pass


def _rand_bits(rng, shape):
    """Random bf16 bit patterns without NaN / inf (exponent 255 -> 191): subnormals 1 in 128, both zeros now and then."""
    b = rng.integers(0, 1 << 16, shape, dtype=np.uint16)
    b[(b & 0x7f80) == 0x7f80] &= 0xbfff
    return b.view(np.int16)


def _ints(rng, lo, hi, shape, step=1):
    return _bf16_bits((rng.integers(lo // step, hi // step + 1, shape) * step).astype(np.float32))


def _bits_to_f32(bits):
    return (bits.astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def _prefilled(ops, n, h, w, c, whole=False):
    """An output whose interior (whole=True: border too, for the kernels that walk the whole padded buffer) holds 3.0."""
    a = ops.Act(n, h, w, c)
    (a.t if whole else a.interior()).fill_(3.0)
    return a


def _f32_bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _report(name, bound, err, err32):
    """Print the bound and the largest error / bound of the kernel and of the float32 evaluation on the CPU; return both."""
    def ratio(e):
        e = np.asarray(e, np.float64)
        assert np.isfinite(e).all(), name
        with np.errstate(divide='ignore', invalid='ignore'):
            return float(np.max(np.where(e == 0, 0.0, e / bound)))
    rk, rc = ratio(err), ratio(err32)
    print('%s: bound max %.3e median %.3e; kernel err/bound %.4f; CPU float32 err/bound %.4f'
          % (name, float(np.max(bound)), float(np.median(bound)), rk, rc))
    return rk, rc


# ---- a. max-pool forward ------------------------------------------------------------------------------------------------------

def _order_key(bits):
    """int16 whose integer order is the value order of the (non-NaN) bf16 patterns; +0 and -0.0 both map to 0."""
    return np.where(bits < 0, -(bits & 0x7fff), bits).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _order_key_is_the_value_order():
    b = np.arange(-32768, 32768).astype(np.int16)
    b = b[(b & 0x7f80) != 0x7f80]
    v, k = _bits_to_f64(b), _order_key(b).astype(np.int64)
    o = np.argsort(v, kind='stable')
    assert (np.diff(k[o]) >= 0).all() and ((np.diff(v[o]) > 0) == (np.diff(k[o]) > 0)).all()
    return True


def _pool_ref(bits, zero_signs=True):
    """(bits of the window maximum, mask of the windows whose maximum is a zero with both signs present)."""
    assert _order_key_is_the_value_order()
    n, h, w, c = bits.shape
    win = [bits[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    best, kbest = win[0], _order_key(win[0])
    for v in win[1:]:
        k = _order_key(v)
        best, kbest = np.where(k > kbest, v, best), np.maximum(k, kbest)
    tie = np.zeros(best.shape, bool)
    if zero_signs:
        tie = (kbest == 0) & np.any([v == POS0 for v in win], 0) & np.any([v == NEG0 for v in win], 0)
    return best.astype(np.int16), tie


def _check_pool(got, want, tie):
    """Bits over the whole padded buffer; a window of +0 against -0.0 by value (either zero)."""
    tie = np.pad(tie, ((0, 0), (1, 1), (1, 1), (0, 0)))
    want = _padded(want)
    assert np.array_equal(np.where(tie, got & 0x7fff, got), np.where(tie, 0, want))


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('n,h,w', MAPS)
def test_maxpool_forward_bits(ops, n, h, w, c):
    rng = np.random.default_rng(n * h * w + c)
    x = _rand_bits(rng, (n, h, w, c))
    x[..., c // 2:] = _ints(rng, -3, 3, (n, h, w, c - c // 2))          # half the channels: many ties, all of them +0 or equal
    v = lambda *a: _bf16_bits(np.array(a, np.float32)).reshape(2, 2)    # noqa: E731
    x[0, 0:2, 0:2, 0] = v(-1.0, -2.0, -3.0, -0.5)                       # all negative: a maximum that starts at 0 fails
    x[0, 0:2, 0:2, 1] = v(-1.0, 2.0, -3.0, 0.5)                         # mixed signs
    x[0, 0:2, 0:2, 2] = v(-2.0, -2.0, -2.0, -2.0)                       # four equal
    x[0, 0:2, 0:2, 3] = [[POS0, POS0], [SUB, POS0]]                     # a subnormal, the only positive value
    x[0, 0:2, 0:2, 4] = [[POS0, NEG0], [NEG0, POS0]]                    # +0 against -0.0
    x[0, 0:2, 0:2, 5] = [[NEG0, NEG0], [NEG0, NEG0]]                    # -0.0 alone keeps its sign
    x[0, 0:2, 0:2, 6] = [[NEGSUB, NEG0], [NEGSUB, NEGSUB]]              # -0.0 above the negative subnormal
    want, tie = _pool_ref(x)
    neg_half, neg_two = _bf16_bits(np.array([-0.5, -2.0], np.float32))
    assert list(want[0, 0, 0, :4]) == [neg_half, _bf16_bits(np.array([2.0], np.float32))[0], neg_two, SUB]
    assert tie[0, 0, 0, 4] and not tie[0, 0, 0, 5] and want[0, 0, 0, 5] == NEG0 and want[0, 0, 0, 6] == NEG0
    y = _prefilled(ops, n, h // 2, w // 2, c)
    ops.maxpool2x2_fwd(_act_from_bits(ops, x), y)
    torch.cuda.synchronize()
    _check_pool(_act_bits(y), want, tie)


def test_maxpool_forward_grid_stride_loop(ops):
    n, h, w, c = 1, 2 * 1449, 2 * 1449, 8
    assert n * (h // 2) * (w // 2) * c // 8 > CAP
    x = _rand_bits(np.random.default_rng(0), (n, h, w, c))
    x[x == NEG0] = POS0                                                 # (the zero-sign window is the small test's)
    want, tie = _pool_ref(x, zero_signs=False)
    y = _prefilled(ops, n, h // 2, w // 2, c)
    ops.maxpool2x2_fwd(_act_from_bits(ops, x), y)
    torch.cuda.synchronize()
    _check_pool(_act_bits(y), want, tie)


# ---- b. x2 bilinear upsample --------------------------------------------------------------------------------------------------

def _up2(x, dt):
    """bilinear x2 of custom_layers.py:8-25 written out: out[2i] = .25 x[i-1] + .75 x[i], out[2i+1] = .75 x[i] + .25 x[i+1] per
    axis, zero outside the map; the four products summed in the kernel's order (lower row first, lower column first).  Returns
    the sum and the sum of the magnitudes of its terms, both in dt."""
    n, h, w, c = x.shape
    xp = np.pad(x.astype(dt), ((0, 0), (1, 1), (1, 1), (0, 0)))
    out, A = np.empty((n, 2 * h, 2 * w, c), dt), np.empty((n, 2 * h, 2 * w, c), dt)
    taps = {0: (dt(0.25), dt(0.75)), 1: (dt(0.75), dt(0.25))}           # (weight of the lower source, of the upper) per parity
    for py in (0, 1):
        for px in (0, 1):
            t = [xp[:, py + a:py + a + h, px + b:px + b + w] * (taps[py][a] * taps[px][b]) for a in (0, 1) for b in (0, 1)]
            out[:, py::2, px::2] = ((t[0] + t[1]) + t[2]) + t[3]
            A[:, py::2, px::2] = ((np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])) + np.abs(t[3])
    assert out.dtype == dt
    return out, A


@functools.lru_cache(maxsize=None)
def _up2_is_the_oracles_deconv():
    x = np.random.default_rng(5).integers(-8, 9, (2, 5, 7, 3)).astype(np.float64)
    want = fo.deconv_same(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), fo.bilinear_kernel(4, 3), 2)
    assert np.array_equal(_up2(x, np.float64)[0], want.permute(0, 2, 3, 1).numpy().astype(np.float64))     # multiples of 1/16
    return True


def _upsample_ref(x, scale, shift, res, relu):
    """y = act(up2(x) [* scale + shift]) [+ res] in float64 and the per-element bound of a float32 evaluation stored as bf16:
    the four products are exact (8 bits x 4 bits), then three roundings of the four-term sum, one of the affine (a fused
    multiply-add), one of the residual add, and the bf16 store -- each of size (unit roundoff) x (|exact value| + error so far)."""
    u, A = _up2(x, np.float64)
    e = ((1 + EPS) ** 3 - 1) * A
    if scale is not None:
        u, e = u * scale + shift, np.abs(scale) * e
        e = e + EPS * (np.abs(u) + e)
    if relu:
        u = np.maximum(u, 0.0)                                          # |max(a, 0) - max(b, 0)| <= |a - b|
    if res is not None:
        u = u + res
        e = e + EPS * (np.abs(u) + e)
    return u, e + BF16 * (np.abs(u) + e) + 2.0 ** -134                  # (+ half the spacing of the bf16 subnormals)


def _upsample_f32(x, scale, shift, res, relu):
    """The same formulas in float32 on the CPU, stored as bf16 (the affine as one rounding of the float64 value)."""
    u = _up2(x.astype(np.float32), np.float32)[0]
    if scale is not None:
        u = (u.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
    if relu:
        u = np.maximum(u, np.float32(0))
    if res is not None:
        u = u + res.astype(np.float32)
    assert u.dtype == np.float32
    return fo.round_bf16(u)


COMBOS = [(relu, affine, residual) for relu in (True, False) for affine in (True, False) for residual in (True, False)]


def _run_upsample(ops, xb, scale, shift, resb, relu, entry='general'):
    n, h, w, c = xb.shape
    x = _act_from_bits(ops, xb)
    res = _act_from_bits(ops, resb) if resb is not None else None
    y = _prefilled(ops, n, 2 * h, 2 * w, c)
    sc, sh = (_dev(scale), _dev(shift)) if scale is not None else (None, None)
    if entry == 'general':
        ops.upsample2x_relu_add(x, res, y, scale=sc, shift=sh, relu=relu)
    else:
        from modular_semantic_segmentation_amd import _lib
        rp = res.xv() if res is not None else ops._NULL_ACT
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if entry == 'relu_add':
            _lib.check(_lib.lib().xv_upsample2x_relu_add(x.xv(), rp, y.xv(), stream), entry)
        else:
            _lib.check(_lib.lib().xv_upsample2x_affine_relu_add(x.xv(), ops._ptr(sc), ops._ptr(sh), rp, y.xv(), stream), entry)
    torch.cuda.synchronize()
    return _act_bits(y)


def _exact_upsample_case(rng, n, h, w, c, affine, residual):
    """x multiples of 4 in [-8, 8], residual integers in [-8, 8], scale in {+-0.5, 1, 2}, shift integers in [-3, 3]: up2(x) is a
    multiple of 1/4 up to 8, the affine a multiple of 1/8 up to 19, the result a multiple of 1/8 below 32 -- 8 bits, a bf16."""
    xb = _ints(rng, -8, 8, (n, h, w, c), step=4)
    resb = _ints(rng, -8, 8, (n, 2 * h, 2 * w, c)) if residual else None
    scale = rng.choice(np.array([0.5, -0.5, 1.0, 2.0], np.float32), c) if affine else None
    shift = rng.integers(-3, 4, c).astype(np.float32) if affine else None
    return xb, scale, shift, resb


def _check_exact_upsample(ops, xb, scale, shift, resb, relu):
    assert _up2_is_the_oracles_deconv()
    ref, _ = _upsample_ref(_bits_to_f64(xb), scale, shift, _bits_to_f64(resb) if resb is not None else None, relu)
    assert np.array_equal(fo.round_bf16(ref.astype(np.float32)).astype(np.float64), ref)       # every output is a bf16
    want = _padded(_bf16_bits(ref.astype(np.float32)))
    got = _run_upsample(ops, xb, scale, shift, resb, relu)
    assert np.array_equal(got, want), (relu, scale is not None, resb is not None)
    if relu:                                                            # the thin entry points: the same bytes
        entry = 'affine_relu_add' if scale is not None else 'relu_add'
        assert np.array_equal(_run_upsample(ops, xb, scale, shift, resb, relu, entry), got), entry
    return ref


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('n,h,w', MAPS + [(1, 1, 1), (1, 1, 7), (1, 7, 1)])
def test_upsample2x_exact_all_combinations(ops, n, h, w, c):
    rng = np.random.default_rng(n * h * w + c)
    for relu, affine, residual in COMBOS:
        xb, scale, shift, resb = _exact_upsample_case(rng, n, h, w, c, affine, residual)
        ref = _check_exact_upsample(ops, xb, scale, shift, resb, relu)
        assert h * w * c < 100 or relu == (ref.min() >= 0) or residual      # the relu cuts something when it is on


@pytest.mark.parametrize('relu,affine,residual', COMBOS)
def test_upsample2x_random_within_the_rounding_bound(ops, relu, affine, residual):
    n, h, w, c = 2, 12, 20, 24
    rng = np.random.default_rng(100 + 4 * relu + 2 * affine + residual)
    xb = _bf16_bits(rng.standard_normal((n, h, w, c)).astype(np.float32))
    resb = _bf16_bits(rng.standard_normal((n, 2 * h, 2 * w, c)).astype(np.float32)) if residual else None
    scale = rng.standard_normal(c).astype(np.float32) if affine else None
    shift = rng.standard_normal(c).astype(np.float32) if affine else None
    x64, r64 = _bits_to_f64(xb), (_bits_to_f64(resb) if residual else None)
    s64, t64 = (scale.astype(np.float64), shift.astype(np.float64)) if affine else (None, None)
    ref, bound = _upsample_ref(x64, s64, t64, r64, relu)
    cpu = _upsample_f32(x64, scale, shift, r64, relu)
    got = _run_upsample(ops, xb, scale, shift, resb, relu)
    assert not (got[:, 0].any() or got[:, -1].any() or got[:, :, 0].any() or got[:, :, -1].any())
    if relu:
        entry = 'affine_relu_add' if affine else 'relu_add'
        assert np.array_equal(_run_upsample(ops, xb, scale, shift, resb, relu, entry), got), entry
    rk, rc = _report('upsample2x relu=%d affine=%d residual=%d' % (relu, affine, residual), bound,
                     np.abs(_bits_to_f64(got[:, 1:-1, 1:-1]) - ref), np.abs(cpu.astype(np.float64) - ref))
    assert rc <= 1.0, 'float32 on the host misses the bound'
    assert rk <= 1.0


def test_upsample2x_grid_stride_loop(ops):
    n, h, w, c = 1, 725, 724, 8
    assert n * (2 * h) * (2 * w) * c // 8 > CAP
    xb, scale, shift, resb = _exact_upsample_case(np.random.default_rng(1), n, h, w, c, True, True)
    _check_exact_upsample(ops, xb, scale, shift, resb, True)


# ---- c. concat, add, subsample ------------------------------------------------------------------------------------------------

def _check_concat(ops, n, h, w, ca, cb, seed):
    rng = np.random.default_rng(seed)
    a, b = _rand_bits(rng, (n, h, w, ca)), _rand_bits(rng, (n, h, w, cb))
    y = _prefilled(ops, n, h, w, ca + cb, whole=True)                   # the kernel copies the whole padded buffers
    ops.concat_channels(_act_from_bits(ops, a), _act_from_bits(ops, b), y)
    torch.cuda.synchronize()
    assert np.array_equal(_act_bits(y), _padded(np.concatenate([a, b], -1)))


@pytest.mark.parametrize('ca,cb', [(8, 8), (8, 24), (64, 8), (192, 64)])
@pytest.mark.parametrize('n,h,w', MAPS)
def test_concat_channels_bits(ops, n, h, w, ca, cb):
    _check_concat(ops, n, h, w, ca, cb, n * h * w + ca + cb)


def test_concat_channels_grid_stride_loop(ops):
    n, h, w, ca, cb = 1, 724, 722, 8, 24
    assert n * (h + 2) * (w + 2) * (ca + cb) // 8 > CAP
    _check_concat(ops, n, h, w, ca, cb, 2)


@pytest.mark.parametrize('kind', ['integers', 'random'])
@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('n,h,w', MAPS)
def test_add_bits(ops, n, h, w, c, kind):
    rng = np.random.default_rng(n * h * w + c)
    if kind == 'integers':
        a, b = _ints(rng, -8, 8, (n, h, w, c)), _ints(rng, -8, 8, (n, h, w, c))
    else:
        a, b = _rand_bits(rng, (n, h, w, c)), _rand_bits(rng, (n, h, w, c))
    # the kernel's own IEEE operations on the CPU: two exact conversions, one float32 addition, one rounding to bf16
    ta, tb = (torch.from_numpy(v).view(torch.bfloat16) for v in (a, b))
    want = (ta.float() + tb.float()).bfloat16().view(torch.int16).numpy()
    y = _prefilled(ops, n, h, w, c, whole=True)
    ops.add(_act_from_bits(ops, a), _act_from_bits(ops, b), y)
    torch.cuda.synchronize()
    assert np.array_equal(_act_bits(y), _padded(want))


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('n,h,w', MAPS)
def test_subsample2_bits(ops, n, h, w, c):
    x = _rand_bits(np.random.default_rng(n * h * w + c), (n, h, w, c))
    y = _prefilled(ops, n, h // 2, w // 2, c)
    ops.subsample2(_act_from_bits(ops, x), y)
    torch.cuda.synchronize()
    assert np.array_equal(_act_bits(y), _padded(x[:, ::2, ::2]))


# ---- d. dropout against its documented definition -----------------------------------------------------------------------------

def _mix32(z):
    """xv_mix32 of pointwise.hip: the splitmix64 finaliser, upper 32 bits (uint64 arrays wrap modulo 2^64)."""
    z = z + np.uint64(0x9e3779b97f4a7c15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return (z ^ (z >> np.uint64(31))) >> np.uint64(32)


def _dropout_model(padded_bits, rate, seed):
    """The documented dropout of one padded buffer (a slot): element i of the WHOLE padded buffer survives when
    mix32(seed ^ i * 0xd1342543de82ef95) >= floor(float32(rate) * 2^32) (clamped to 2^32 - 1); a survivor is
    bf16(float32(x) * float32(1 / (1 - rate))), everything else +0."""
    rate = np.float32(rate)
    idx = np.arange(padded_bits.size, dtype=np.uint64)
    r = _mix32(np.full(1, seed % (1 << 64), np.uint64) ^ (idx * np.uint64(0xd1342543de82ef95)))
    keep = (r >= np.uint64(min(int(float(rate) * 4294967296.0), 4294967295))).reshape(padded_bits.shape)
    scale = np.float32(1) / (np.float32(1) - rate)
    assert scale.dtype == np.float32
    kept = torch.from_numpy(_bits_to_f32(padded_bits) * scale).bfloat16().view(torch.int16).numpy()
    return np.where(keep, kept, np.int16(0)), keep


def _dropout_input(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    x[np.abs(x) < 2.0 ** -10] = 1.0                                     # no zero inside: a kept element is visible as non-zero
    b = _bf16_bits(x)
    assert (b & 0x7fff).all()
    return b


RATES = [0.0, 0.2, 0.5, 0.75, float(np.nextafter(np.float32(1), np.float32(0)))]
SEEDS = [0, 1, 1 << 32, (1 << 63) + 5]


def _check_dropout(ops, xb, rate, seeds):
    n, h, w, c = xb.shape
    x, outs = _act_from_bits(ops, xb), []
    for seed in seeds:
        y = _prefilled(ops, n, h, w, c, whole=True)
        ops.dropout(x, rate, seed, y)
        torch.cuda.synchronize()
        got = _act_bits(y)
        want, _ = _dropout_model(_padded(xb), rate, seed)
        assert np.array_equal(got, want), seed                          # bits, the whole padded buffer
        assert _border_is_zero(y)
        # the hash, not the kernel: the kept share of the N interior elements within five binomial standard deviations
        N, kept = xb.size, int((got[:, 1:-1, 1:-1] != 0).sum())
        p = 1.0 - float(np.float32(rate))
        assert abs(kept - N * p) <= 5.0 * np.sqrt(N * p * (1.0 - p)), (seed, kept, N * p)
        if rate == 0.0:
            assert np.array_equal(got, _padded(xb))
        outs.append(got)
    return outs


@pytest.mark.parametrize('rate', RATES)
@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('n,h,w', MAPS)
def test_dropout_is_the_documented_hash(ops, n, h, w, c, rate):
    xb = _dropout_input(np.random.default_rng(n * h * w + c), (n, h, w, c))
    outs = _check_dropout(ops, xb, rate, SEEDS)
    if rate in (0.2, 0.5, 0.75) and xb.size >= 1000:
        # seeds 0 and 2^32 differ only above bit 31, 0 and 1 only in bit 0: other masks
        assert not np.array_equal(outs[0] != 0, outs[2] != 0) and not np.array_equal(outs[0] != 0, outs[1] != 0)


def test_dropout_grid_stride_loop(ops):
    n, h, w, c = 1, 1448, 1446, 8
    assert n * (h + 2) * (w + 2) * c // 8 > CAP
    _check_dropout(ops, _dropout_input(np.random.default_rng(3), (n, h, w, c)), 0.5, [(1 << 63) + 5])


def _check_dropout_samples(ops, xb, T, rate, seed0, stride):
    """All four multi-slot forms against the host model of every slot (slot-major; seeds wrap modulo 2^64)."""
    from modular_semantic_segmentation_amd import _lib
    n, h, w, c = xb.shape
    x, px = _act_from_bits(ops, xb), _padded(xb)
    drop = lambda k: _dropout_model(px, rate, seed0 + k * stride)[0]    # noqa: E731
    with_plain = np.concatenate([px] + [drop(t) for t in range(T)])
    only = np.concatenate([drop(t) for t in range(T)])
    assert (with_plain[n:] != 0).any() and not np.array_equal(only[:n], only[n:2 * n])
    y = _prefilled(ops, (T + 1) * n, h, w, c, whole=True)
    ops.dropout_samples(x, T, rate, seed0, stride, y=y)
    assert np.array_equal(_act_bits(y), with_plain)
    y = _prefilled(ops, T * n, h, w, c, whole=True)
    ops.dropout_samples(x, T, rate, seed0, stride, y=y, sample_only=True)
    assert np.array_equal(_act_bits(y), only)
    # the in-place forms (nothing in the package calls them): every slot starts as a copy of x
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = _act_from_bits(ops, np.concatenate([xb] * (T + 1)))
    _lib.check(_lib.lib().xv_dropout_samples_inplace(y.xv(), T, rate, seed0 % (1 << 64), stride % (1 << 64), stream), 'inplace')
    assert np.array_equal(_act_bits(y), with_plain)
    y = _act_from_bits(ops, np.concatenate([xb] * T))
    _lib.check(_lib.lib().xv_dropout_samples_only_inplace(y.xv(), T, rate, seed0 % (1 << 64), stride % (1 << 64), stream),
               'only_inplace')
    assert np.array_equal(_act_bits(y), only)


@pytest.mark.parametrize('rate', [0.2, 0.5])
@pytest.mark.parametrize('n,h,w,c', [(1, 2, 2, 8), (2, 12, 20, 24), (1, 6, 34, 192)])
def test_dropout_samples_every_slot_is_the_documented_hash(ops, n, h, w, c, rate):
    xb = _dropout_input(np.random.default_rng(n * h * w + c), (n, h, w, c))
    _check_dropout_samples(ops, xb, 3, rate, (1 << 63) + 5, (1 << 63) + (1 << 32) + 1)


def test_dropout_samples_grid_stride_loop(ops):
    n, h, w, c = 1, 724, 722, 8
    assert n * (h + 2) * (w + 2) * c // 8 > 2048 * 256                  # the multi-slot grid is capped at 2 048 workgroups a slot
    _check_dropout_samples(ops, _dropout_input(np.random.default_rng(4), (n, h, w, c)), 2, 0.5, 1 << 32, 3)


# ---- e. the two gathers, element by element -----------------------------------------------------------------------------------

def _gather7s2_ref(x):
    """include/xview_hip.h: z[j][i][3 rv + cv] = x[2 (j + sr) + pr][2 (i + sc) + pc], variants (p, s) = (0,0), (0,1), (1,0) per
    axis -- source offsets 0, 2, 1 --, zero where there is no source."""
    n, hi, wi, c = x.shape
    xz = np.zeros((n, hi + 2, wi + 2, c), x.dtype)
    xz[:, :hi, :wi] = x
    off = np.array([0, 2, 1])
    sy, sx = 2 * np.arange(hi // 2)[:, None] + off, 2 * np.arange(wi // 2)[:, None] + off
    return xz[:, sy[:, None, :, None], sx[None, :, None, :]].reshape(n, hi // 2, wi // 2, 9 * c)


def _im2col_ref(x, d1, d2):
    """z[y][x][t] = x[y + ty d][x + tx d], t = 3 (ty + 1) + (tx + 1) at d1, then the same nine at d2; zero outside the map."""
    n, h, w, c = x.shape
    xz = np.zeros((n, h + 1, w + 1, c), x.dtype)
    xz[:, :h, :w] = x
    parts = []
    for d in (d1, d2):
        k = (np.arange(3) - 1) * d
        sy, sx = np.arange(h)[:, None] + k, np.arange(w)[:, None] + k
        sy, sx = np.where((sy >= 0) & (sy < h), sy, h), np.where((sx >= 0) & (sx < w), sx, w)
        parts.append(xz[:, sy[:, None, :, None], sx[None, :, None, :]].reshape(n, h, w, 9 * c))
    return np.concatenate(parts, -1)


def _row_widths(per):
    """Output widths whose destination row of w * per 16-byte groups: is the shortest there is (below 256 groups wherever per
    is); the longest inside one 1 024-group block; the shortest that needs a second block; spans three blocks and more.  (per is
    a multiple of 9: no row is exactly 1 024 or 1 025 groups long -- these are the nearest lengths on either side.)"""
    ws = [1, 1024 // per, 1024 // per + 1, 2048 // per + 2]
    assert ws[1] * per <= 1024 < ws[2] * per and ws[3] * per > 2048
    return sorted(set(ws))


def _run_gather7s2(ops, xb):
    n, hi, wi, c = xb.shape
    z = _prefilled(ops, n, hi // 2, wi // 2, 9 * c)
    ops.gather_conv7s2(_act_from_bits(ops, xb), z)
    torch.cuda.synchronize()
    return _act_bits(z)


def _run_im2col(ops, xb, d1, d2):
    n, h, w, c = xb.shape
    z = _prefilled(ops, n, h, w, 18 * c)
    ops.im2col_dilated_pair(_act_from_bits(ops, xb), d1, d2, z)
    torch.cuda.synchronize()
    return _act_bits(z)


GATHER_C = [8, 24, 64, 136]                                             # C = 8: the flat kernels (no reciprocal of C / 8 = 1)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('c', GATHER_C)
def test_gather_conv7s2_element_by_element(ops, c, n):
    rng = np.random.default_rng(c + n)
    for wo in _row_widths(9 * c // 8):
        xb = _rand_bits(rng, (n, 6, 2 * wo, c))
        want = _gather7s2_ref(xb)
        assert not want[:, -1, :, 3 * c:6 * c].any() and not want[:, :, -1, c:2 * c].any()      # variant 1 of the last row / column
        assert np.array_equal(_run_gather7s2(ops, xb), _padded(want)), wo


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('c', GATHER_C)
def test_im2col_dilated_pair_element_by_element(ops, c, n):
    rng = np.random.default_rng(c + n)
    h = 5
    for w in _row_widths(18 * c // 8):
        xb = _rand_bits(rng, (n, h, w, c))
        big = max(h, w)
        for d1, d2 in [(1, 2), (2, 2), (1, 16), (big, big + 3)]:        # the last: only the centre taps have a source
            want = _im2col_ref(xb, d1, d2)
            assert (d1, d2) != (big, big + 3) or not want[..., :4 * c].any()
            assert np.array_equal(_run_im2col(ops, xb, d1, d2), _padded(want)), (w, d1, d2)


def test_gathers_flat_kernels_past_65535_rows(ops):
    """More destination rows than a grid's y dimension holds: the flat kernels, whatever the environment says."""
    rng = np.random.default_rng(6)
    xb = _rand_bits(rng, (1, 65536, 1, 8))
    assert xb.shape[0] * xb.shape[1] > 65535
    assert np.array_equal(_run_im2col(ops, xb, 1, 2), _padded(_im2col_ref(xb, 1, 2)))
    xb = _rand_bits(rng, (1, 131072, 2, 8))
    assert xb.shape[0] * xb.shape[1] // 2 > 65535
    assert np.array_equal(_run_gather7s2(ops, xb), _padded(_gather7s2_ref(xb)))


FLAT_CASES = [(c, n, kind) for c in (24, 64, 136) for n, kind in ((1, 1), (3, 2), (1, 3))]      # kind: index into _row_widths


def _either_form_outputs(ops):
    """Both gathers at shapes the row forms take (C / 8 >= 2, few rows); the same inputs in whichever process runs this."""
    out = {}
    for c, n, kind in FLAT_CASES:
        rng = np.random.default_rng(1000 * c + 10 * n + kind)
        xb = _rand_bits(rng, (n, 6, 2 * _row_widths(9 * c // 8)[kind], c))
        out['g_%d_%d_%d' % (c, n, kind)] = _run_gather7s2(ops, xb)
        xb = _rand_bits(rng, (n, 5, _row_widths(18 * c // 8)[kind], c))
        out['i_%d_%d_%d' % (c, n, kind)] = _run_im2col(ops, xb, 2, 16)
    return out


def _flat_child(path):
    """Runs in a fresh process started with XV_GATHER_FLAT=1 (the switch is read once per process)."""
    from modular_semantic_segmentation_amd import ops as _ops
    np.savez(path, **_either_form_outputs(_ops))


def test_gathers_row_and_flat_forms_give_equal_bytes(ops, tmp_path):
    assert os.environ.get('XV_GATHER_FLAT', '0') == '0'
    rows = _either_form_outputs(ops)
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [os.path.dirname(here), here] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]
    env = dict(os.environ, XV_GATHER_FLAT='1', PYTHONPATH=os.pathsep.join(paths))
    path = str(tmp_path / 'flat.npz')
    subprocess.run([sys.executable] + (['-s'] if sys.flags.no_user_site else []) +
                   ['-c', 'import test_inference_pointwise_edges_gpu as t; t._flat_child(%r)' % path],
                   env=env, check=True, timeout=300)
    flat = np.load(path)
    assert sorted(flat.files) == sorted(rows)
    for k in rows:
        assert np.array_equal(rows[k], flat[k]), k


# ---- f. phase shuffles --------------------------------------------------------------------------------------------------------

STRIDES = [1, 2, 3, 8]


def _to_phases(g, s):
    """[n, s H, s W, C] -> [n, H, W, s s C], phase channel (py s + px) C + c  <->  pixel (s qy + py, s qx + px)."""
    n, hs, ws, c = g.shape
    return g.reshape(n, hs // s, s, ws // s, s, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, hs // s, ws // s, s * s * c)


def _from_phases(z, s, cp, classes):
    n, h, w, _ = z.shape
    return z.reshape(n, h, w, s, s, cp)[..., :classes].transpose(0, 1, 3, 2, 4, 5).reshape(n, h * s, w * s, classes)


def _check_space_to_depth(ops, n, h, w, c, s, seed):
    g = _rand_bits(np.random.default_rng(seed), (n, s * h, s * w, c))
    out = _prefilled(ops, n, h, w, s * s * c)
    ops.space_to_depth(_act_from_bits(ops, g), s, out)
    torch.cuda.synchronize()
    assert np.array_equal(_act_bits(out), _padded(_to_phases(g, s)))


@pytest.mark.parametrize('s', STRIDES)
@pytest.mark.parametrize('c', [8, 24])
@pytest.mark.parametrize('n,h,w', MAPS)
def test_space_to_depth_bits(ops, n, h, w, c, s):
    _check_space_to_depth(ops, n, h, w, c, s, n * h * w + c + s)


def test_space_to_depth_grid_stride_loop(ops):
    n, h, w, c, s = 1, 725, 724, 8, 2
    assert n * h * w * s * s * c // 8 > CAP
    _check_space_to_depth(ops, n, h, w, c, s, 7)


DENSE_CLASSES = [(1, 8), (1, 16), (12, 16), (14, 16)]                   # (classes, Cp): Cp a multiple of 8 that holds them
F32_CLASSES = [(3, 4), (3, 12), (3, 16), (12, 12), (12, 16), (14, 16)]  # (classes, cp): cp a multiple of 4 that holds them


@pytest.mark.parametrize('s', STRIDES)
@pytest.mark.parametrize('classes,cp', DENSE_CLASSES)
@pytest.mark.parametrize('n,h,w', MAPS)
def test_space_to_depth_dense_bits_and_zero_padding_channels(ops, n, h, w, classes, cp, s):
    rng = np.random.default_rng(n * h * w + classes + cp + s)
    g = rng.standard_normal((n, s * h, s * w, classes)).astype(np.float32)          # rounded to bf16 (nearest even) on the way
    g[0, 0, 0, 0], g[0, -1, -1, -1] = -0.0, 1.0 + 2.0 ** -8                         # a tie: rounds to even, 1.0
    padded = np.zeros((n, s * h, s * w, cp), np.int16)
    padded[..., :classes] = torch.from_numpy(g).bfloat16().view(torch.int16).numpy()
    out = _prefilled(ops, n, h, w, s * s * cp)
    ops.space_to_depth_dense(_dev(g), s, out)
    torch.cuda.synchronize()
    assert np.array_equal(_act_bits(out), _padded(_to_phases(padded, s)))


def _affine_cases(rng, classes):
    """None; an exact one (powers of two, integers); a random one."""
    return [('none', None, None),
            ('exact', 2.0 ** rng.integers(-2, 3, classes).astype(np.float32) * rng.choice(np.float32([-1, 1]), classes),
             rng.integers(-3, 4, classes).astype(np.float32)),
            ('random', rng.standard_normal(classes).astype(np.float32), rng.standard_normal(classes).astype(np.float32))]


def _check_depth_to_space(name, run, z32, s, cp, classes, rng):
    """z32: the phase map's values as float32 [n, h, w, s s cp].  Without an affine and with the exact one (z holds integers in
    [-8, 8]: |z| * 4 + 3 < 2^6) the float32 bits; with the random one a single rounding -- the kernel's expression is one fused
    multiply-add -- of the float64 value."""
    src = _from_phases(z32, s, cp, classes)
    for kind, scale, shift in _affine_cases(rng, classes):
        got = run(scale, shift)
        if kind == 'none':
            assert np.array_equal(got.view(np.int32), src.view(np.int32))
        else:
            ref = src.astype(np.float64) * scale + shift
            if kind == 'exact':
                assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
                assert np.array_equal(got, ref.astype(np.float32))
            else:
                bound = EPS * np.abs(ref) + 2.0 ** -150
                rk, rc = _report('%s s=%d cp=%d classes=%d' % (name, s, cp, classes), bound,
                                 np.abs(got.astype(np.float64) - ref), np.abs(ref.astype(np.float32).astype(np.float64) - ref))
                assert rc <= 1.0 and rk <= 1.0


@pytest.mark.parametrize('s', STRIDES)
@pytest.mark.parametrize('classes,cp', DENSE_CLASSES)
@pytest.mark.parametrize('n,h,w', MAPS)
def test_depth_to_space_dense(ops, n, h, w, classes, cp, s):
    rng = np.random.default_rng(n * h * w + classes + cp + s)
    zb = _ints(rng, -8, 8, (n, h, w, s * s * cp))                       # padding channels hold values too: they are not read

    def run(scale, shift):
        out = torch.full((n, s * h, s * w, classes), 3.0, dtype=torch.float32, device='cuda')
        ops.depth_to_space_dense(_act_from_bits(ops, zb), s, classes, out, scale=None if scale is None else _dev(scale),
                                 shift=None if shift is None else _dev(shift))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    _check_depth_to_space('depth_to_space_dense', run, _bits_to_f32(zb), s, cp, classes, rng)


@pytest.mark.parametrize('s', STRIDES)
@pytest.mark.parametrize('classes,cp', F32_CLASSES)
@pytest.mark.parametrize('n,h,w', MAPS)
def test_depth_to_space_dense_f32(ops, n, h, w, classes, cp, s):
    from modular_semantic_segmentation_amd import _lib
    rng = np.random.default_rng(n * h * w + classes + cp + s)
    z = rng.integers(-8, 9, (n, h, w, s * s * cp)).astype(np.float32)
    z[0, 0, 0, 0] = -0.0
    zd = _dev(z)

    def run(scale, shift):
        out = torch.full((n, s * h, s * w, classes), 3.0, dtype=torch.float32, device='cuda')
        sc, sh = (None, None) if scale is None else (_dev(scale), _dev(shift))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = _lib.lib().xv_depth_to_space_dense_f32(ops._ptr(zd), n, h, w, s, cp, classes, ops._ptr(sc), ops._ptr(sh),
                                                    ops._ptr(out), stream)
        _lib.check(rc, 'xv_depth_to_space_dense_f32')
        torch.cuda.synchronize()
        return out.cpu().numpy()
    _check_depth_to_space('depth_to_space_dense_f32', run, z, s, cp, classes, rng)


@pytest.mark.parametrize('c', CHANNELS)
@pytest.mark.parametrize('n,h,w', MAPS)
def test_act_to_dense_f32_is_exact(ops, n, h, w, c):
    """Every bf16 is a float32: the 16 bits shifted up, subnormals and -0.0 included."""
    from modular_semantic_segmentation_amd import _lib
    xb = _rand_bits(np.random.default_rng(n * h * w + c), (n, h, w, c))
    xb[0, 0, 0, :4] = [NEG0, SUB, NEGSUB, POS0]
    out = torch.full((n, h, w, c), 3.0, dtype=torch.float32, device='cuda')
    rc = _lib.lib().xv_act_to_dense_f32(_act_from_bits(ops, xb).xv(), ops._ptr(out),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'xv_act_to_dense_f32')
    torch.cuda.synchronize()
    assert np.array_equal(_f32_bits(out), (xb.astype(np.int32) << 16))
