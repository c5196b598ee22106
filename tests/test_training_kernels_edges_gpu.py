"""The training-side pointwise kernels past one workgroup, past C = 12 and off the aligned fast paths: softmax-CE head backward,
valid-label count, pool / relu / x2-upsample gradients, the three optimizers, confusion matrix and Dirichlet sufficient statistics.

Every reference below restates the operation in float64 (numpy / torch-CPU) and calls no kernel.  Every tolerance is derived per
element from the reference: A is the reference's own sum with every term replaced by its absolute value, EPS = 2^-24 the unit
roundoff of fp32, and each K is written next to the count of additions it comes from.  Where a bound carries arithmetic error (head,
optimizers, sufficient statistics) the same formulas are first evaluated in float32 on the CPU and held to the same bound against
float64: the bound is one that a correct fp32 evaluation meets, not one fitted to the kernel."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo

EPS = 2.0 ** -24          # unit roundoff of fp32
BF16 = 2.0 ** -8          # unit roundoff of bf16 (8 significant bits): a store of a value just above a power of two uses all of it


def _ratio(kernel, err, bound):
    """Largest err / bound over the elements (0 / 0 = 0: exact where nothing is allowed)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(err).all(), kernel
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops as _ops
    return _ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _bf16_bits(x):
    """float32 array of bf16-representable (or to-be-rounded) values -> their bf16 bit patterns, int16."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().view(torch.int16).numpy().copy()


def _bits_to_f64(bits):
    """bf16 bit patterns -> float64, exactly (subnormals and signed zeros included: no flush on the host)."""
    return (bits.astype(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _act_from_bits(ops, bits):
    """Padded activation whose interior holds exactly these bf16 bit patterns (Act.from_dense converts from float32 on the
    device, which need not carry -0.0 or a subnormal)."""
    n, h, w, c = bits.shape
    a = ops.Act(n, h, w, c)
    a.interior().copy_(torch.from_numpy(np.ascontiguousarray(bits, np.int16)).view(torch.bfloat16).cuda())
    return a


def _act_bits(a):
    return a.t.view(torch.int16).cpu().numpy()


def _padded(bits):
    n, h, w, c = bits.shape
    p = np.zeros((n, h + 2, w + 2, c), np.int16)
    p[:, 1:-1, 1:-1] = bits
    return p


def _border_is_zero(a):
    t = a.t.view(torch.int16)
    return not (t[:, 0].any() or t[:, -1].any() or t[:, :, 0].any() or t[:, :, -1].any())


@functools.lru_cache(maxsize=None)
def _deconv_matrix(size, s):
    """[s * size, size] matrix of the bilinear `conv2d_transpose` with stride s, kernel 2 s, 'same' (custom_layers.py:8-25):
    out[o] = sum_i in[i] w1[o + s / 2 - s i], w1[t] = 1 - |t - (s - 0.5)| / s for even s.  float64; checked once against the
    oracle's kernel through torch's transposed convolution."""
    t = np.arange(2 * s, dtype=np.float64)
    w1 = 1.0 - np.abs(t - (s - 0.5)) / s
    B = np.zeros((s * size, size))
    for o in range(s * size):
        for i in range(size):
            k = o + s // 2 - s * i
            if 0 <= k < 2 * s:
                B[o, i] = w1[k]
    wk = torch.from_numpy(fo.bilinear_kernel(2 * s, 1)).permute(3, 2, 0, 1).double()
    x = torch.from_numpy(np.random.default_rng(size).standard_normal((1, 1, size, size)))
    want = F.conv_transpose2d(x, wk, stride=s, padding=s // 2)[0, 0].numpy()
    assert np.allclose(B @ x[0, 0].numpy() @ B.T, want, rtol=0, atol=1e-12)
    return B


# ---- 1. head backward ---------------------------------------------------------------------------------------------------------

def _head_formulas(f, ws, bs, lab, C, dtype):
    """The kernel's stated contract (include/xview_hip.h, backward.hip): score = bilinear_x8(fused . Ws) + bs -- no relu on the
    deconv --, softmax cross-entropy over the pixels with 0 <= label < C, denominator 1e-20 + count.  Closed-form gradients, all
    in `dtype`; with float64 also the absolute-value sums A of every output."""
    n, h, w, U = f.shape
    ft, wt, bt = (torch.from_numpy(a).to(dtype) for a in (f, ws, bs))
    By = torch.from_numpy(_deconv_matrix(h, 8)).to(dtype)
    Bx = torch.from_numpy(_deconv_matrix(w, 8)).to(dtype)
    labt = torch.from_numpy(lab.astype(np.int64))
    valid = (labt >= 0) & (labt < C)
    inv = torch.tensor(1.0, dtype=dtype) / (torch.tensor(1e-20, dtype=dtype) + valid.sum().to(dtype))
    S = ft @ wt
    score = torch.einsum('oi,nijc,pj->nopc', By, S, Bx) + bt
    z = score - score.max(-1, keepdim=True)[0]
    e = z.exp()
    se = e.sum(-1, keepdim=True)
    onehot = F.one_hot(torch.where(valid, labt, torch.zeros_like(labt)), C).to(dtype) * valid[..., None].to(dtype)
    terms = -(onehot * (z - se.log())).sum(-1) * inv                     # one per output pixel, 0 where unlabelled
    dscore = (e / se - onehot) * valid[..., None].to(dtype) * inv
    dS = torch.einsum('oi,nopc,pj->nijc', By, dscore, Bx)
    out = {'loss': terms.sum(), 'dbs': dscore.sum((0, 1, 2)), 'dws': torch.einsum('nijc,niju->uc', dS, ft), 'df': dS @ wt.T}
    if dtype == torch.float64:
        AdS = torch.einsum('oi,nopc,pj->nijc', By, dscore.abs(), Bx)
        out['A'] = {'loss': terms.abs().sum(), 'dbs': dscore.abs().sum((0, 1, 2)),
                    'dws': torch.einsum('nijc,niju->uc', AdS, ft.abs()), 'df': AdS @ wt.abs().T}
    return out


def _head_labels(rng, n, h, w, C, kind):
    lab = rng.integers(-1, C, (n, 8 * h, 8 * w)).astype(np.int32)          # uniform in [-1, C)
    if kind == 'edges':
        CM = (C + 3) // 4 * 4
        odd = [C, 255, -7] + ([CM - 1] if CM - 1 > C else [])
        pick = rng.random(lab.shape)
        for i, v in enumerate(odd):
            lab[(pick >= 0.05 * i) & (pick < 0.05 * (i + 1))] = v
        assert all((lab == v).any() for v in odd)                 # (only used at maps of thousands of pixels)
    elif kind == 'none':
        lab[:] = -1
    return lab


@functools.lru_cache(maxsize=None)
def _head_case(n, h, w, U, C, kind):
    """Inputs, float64 reference and per-element bounds of one case; computed once, shared, never modified."""
    rng = np.random.default_rng(1000 * U + 10 * C + n * h * w)
    f = fo.round_bf16(np.abs(rng.standard_normal((n, h, w, U))).astype(np.float32))       # fused >= 0, bf16
    f[..., 7 % U] = 0                                                                  # a dead channel
    f[0, h // 2, w // 2, :] = 0                                                        # a dead pixel
    ws = (rng.standard_normal((U, C)) * (2.4 / np.sqrt(U))).astype(np.float32)         # scores of a few units whatever U is
    bs = rng.standard_normal(C).astype(np.float32)
    lab = _head_labels(rng, n, h, w, C, kind)
    ref = _head_formulas(f, ws, bs, lab, C, torch.float64)
    A = ref.pop('A')
    npix, lowres = n * 64 * h * w, n * h * w
    ncols = 8 * lowres
    g1 = min((ncols + 255) // 256, 4096)
    cpt = -(-ncols // (g1 * 256))                # columns of eight pixels per thread of head_loss_kernel
    nslabs = (lowres + 255) // 256
    # K = twice the fp32 additions on the longest chain into one output.
    #   loss, dbs: 8 rows x cpt columns in the thread, 6 butterfly steps over the wave, 3 adds over the four waves, then the
    #   double-precision reduce over the workgroups rounds once to fp32 and once more in `out +=`: 8 cpt + 6 + 3 + 2
    K_sum = 2 * (8 * cpt + 6 + 3 + 2)
    #   dWs: the 256-pixel chain of a slab, ceil(nslabs / 16) slabs per lane + 4 butterfly steps + `dws +=` in the slab reduce
    K_dws = 2 * (256 + -(-nslabs // 16) + 4 + 1)
    # second term: the ~1e-7 relative error of the hardware exp / log / rcp on the average term (N_terms = terms of the sum)
    bound = {'loss': K_sum * EPS * A['loss'] + 2.0 ** -20 * A['loss'] / npix,
             'dbs': K_sum * EPS * A['dbs'] + 2.0 ** -20 * A['dbs'] / npix,
             'dws': K_dws * EPS * A['dws'] + 2.0 ** -20 * A['dws'] / (256 * lowres),
             'df': BF16 * ref['df'].abs() + 8 * EPS * A['df']}
    # the float32 evaluation of the same formulas on the host sits inside these bounds (df stored as bf16, like the kernel's)
    f32 = _head_formulas(f, ws, bs, lab, C, torch.float32)
    f32['df'] = f32['df'].bfloat16().float()
    for k in bound:
        err = (f32[k].double() - ref[k]).abs()
        assert bool((err <= bound[k]).all()), ('float32 on the host misses the bound', k, float((err / bound[k]).max()))
    return {'f': f, 'ws': ws, 'bs': bs, 'lab': lab, 'count': int(((lab >= 0) & (lab < C)).sum()), 'ref': ref, 'bound': bound}


def _run_head(ops, case, C, prefill):
    f, ws = case['f'], case['ws']
    n, h, w, U = f.shape
    rng = np.random.default_rng(7)
    pre = {'loss': 3.25 if prefill else 0.0,
           'dws': (rng.standard_normal((U, C)) if prefill else np.zeros((U, C))).astype(np.float32),
           'dbs': (rng.standard_normal(C) if prefill else np.zeros(C)).astype(np.float32)}
    loss = torch.full((1,), pre['loss'], dtype=torch.float64, device='cuda')
    dws, dbs = _dev(pre['dws']), _dev(pre['dbs'])
    df = ops.Act(n, h, w, U)
    df.interior().fill_(3.0)                                 # every interior value is written
    count = torch.tensor([case['count']], dtype=torch.int64, device='cuda')
    ops.decoder_head_bwd(ops.Act.from_dense(_dev(f)), _dev(ws), _dev(case['bs']), _dev(case['lab']), count, C, loss, dws, dbs, df)
    torch.cuda.synchronize()
    return pre, {'loss': loss, 'dws': dws, 'dbs': dbs, 'df': df}


HEAD_CASES = [
    # n, h, w, U, C, labels, prefill
    (1, 16, 16, 64, 12, 'basic', False),      # exactly one full slab of 256; 2048 columns = 8 loss workgroups
    (2, 12, 16, 64, 12, 'basic', True),       # 384 px: two slabs, the second half dead
    (2, 12, 16, 64, 12, 'edges', True),       # labels C, 255, -7 among them
    (1, 17, 31, 64, 14, 'basic', True),       # 527 px: three slabs, odd sizes, CM = 16 non-FULL
    (1, 17, 31, 64, 14, 'edges', False),      # ... with labels 14 and 15 = CM - 1 inside the padded class lanes
    (3, 9, 11, 128, 5, 'basic', False),       # slab boundary mid-image and mid-row
    (1, 1, 1, 64, 12, 'basic', False),        # every footprint clipped on both sides
    (1, 1, 9, 64, 12, 'basic', False),
    (1, 9, 1, 64, 12, 'basic', False),
    (2, 12, 16, 192, 19, 'basic', False),     # CM = 20
    (1, 6, 8, 64, 1, 'basic', False),         # class-count edges, FULL (4, 32) and not
    (1, 6, 8, 64, 2, 'basic', False),
    (1, 6, 8, 64, 3, 'basic', False),
    (1, 6, 8, 64, 4, 'basic', False),
    (1, 6, 8, 64, 32, 'basic', False),
    (2, 12, 16, 256, 12, 'basic', False),     # largest U that fits LDS at this C
    (2, 12, 16, 256, 16, 'basic', False),     # CM = 16: 163 840 bytes, exactly the 160 KB limit
    (2, 12, 16, 192, 32, 'basic', False),     # 155 648 bytes, fits
]


@pytest.mark.parametrize('n,h,w,U,C,kind,prefill', HEAD_CASES)
def test_head_backward_against_float64(ops, n, h, w, U, C, kind, prefill):
    case = _head_case(n, h, w, U, C, kind)
    ref, bound = case['ref'], case['bound']
    pre, got = _run_head(ops, case, C, prefill)
    assert _border_is_zero(got['df'])
    # accumulation: got - prefill against the reference; `out += sum` rounds once more at the size of the prefilled value
    for k in ('dws', 'dbs'):
        delta = got[k].cpu().double() - torch.from_numpy(pre[k]).double()
        err = (delta - ref[k]).abs()
        lim = bound[k] + EPS * torch.from_numpy(pre[k]).double().abs()
        assert _ratio('head_bwd ' + k, err.numpy(), lim.numpy()) <= 1.0, (k, float(err.max()))
    err = abs(got['loss'].item() - pre['loss'] - ref['loss'].item())
    assert _ratio('head_bwd loss', err, bound['loss'].item() + 2.0 ** -52 * abs(pre['loss'])) <= 1.0, (err, ref['loss'].item())
    # d loss / d fused: the same (commuted, linear) operation, so EVERY element is compared
    err = (got['df'].interior().float().cpu().double() - ref['df']).abs()
    assert _ratio('head_bwd dfused', err.numpy(), bound['df'].numpy()) <= 1.0, float(err.max())


def test_head_backward_without_a_valid_label(ops):
    """All labels -1: count = 0, 1 / (1e-20 + 0) = 1e20 multiplies exact zeros.  Nothing may move."""
    case = _head_case(2, 12, 16, 64, 12, 'none')
    assert case['count'] == 0
    pre, got = _run_head(ops, case, 12, True)
    assert got['loss'].item() == pre['loss']
    assert np.array_equal(got['dws'].cpu().numpy(), pre['dws']) and np.array_equal(got['dbs'].cpu().numpy(), pre['dbs'])
    assert not got['df'].t.view(torch.int16).bitwise_and(0x7fff).any()                   # interior and border all zero


def test_head_backward_same_bits_from_run_to_run(ops):
    """Three slabs, seventeen loss workgroups' rows (4 216 columns): the fixed-order reductions give the same bits every time."""
    case = _head_case(1, 17, 31, 64, 14, 'basic')
    runs = [_run_head(ops, case, 14, False)[1] for _ in range(2)]
    assert torch.equal(runs[0]['loss'], runs[1]['loss'])
    assert torch.equal(runs[0]['dws'], runs[1]['dws']) and torch.equal(runs[0]['dbs'], runs[1]['dbs'])
    assert torch.equal(runs[0]['df'].t.view(torch.int16), runs[1]['df'].t.view(torch.int16))


@pytest.mark.parametrize('U,C', [(256, 17), (256, 32)])
def test_head_backward_refuses_what_its_slab_kernel_cannot_hold(ops, U, C):
    """(U CM + 256 CM) 4 + 512 U bytes of LDS per slab: 172 032 at U = 256, CM = 20 and 196 608 at CM = 32, over the 160 KB of
    a workgroup.  XV_ESHAPE before the first launch: the loss kernel and its reduce, which run first, must not have added
    into loss or db_score."""
    from modular_semantic_segmentation_amd._lib import XvError
    n, h, w = 2, 12, 16
    rng = np.random.default_rng(U + C)
    fa = ops.Act.from_dense(_dev(np.abs(rng.standard_normal((n, h, w, U))).astype(np.float32)))
    lab = _dev(rng.integers(0, C, (n, 8 * h, 8 * w)).astype(np.int32))
    loss = torch.full((1,), 3.25, dtype=torch.float64, device='cuda')
    dws, dbs = _dev(rng.standard_normal((U, C)).astype(np.float32)), _dev(rng.standard_normal(C).astype(np.float32))
    df = ops.Act(n, h, w, U)
    df.interior().fill_(3.0)
    before = [t.clone() for t in (loss, dws, dbs, df.t)]
    count = torch.tensor([lab.numel()], dtype=torch.int64, device='cuda')
    with pytest.raises(XvError, match='XV_ESHAPE'):
        ops.decoder_head_bwd(fa, _dev((rng.standard_normal((U, C)) * 0.1).astype(np.float32)), _dev(np.zeros(C, np.float32)), lab,
                             count, C, loss, dws, dbs, df)
    torch.cuda.synchronize()
    for b, t in zip(before, (loss, dws, dbs, df.t)):
        assert torch.equal(b.view(torch.int16), t.view(torch.int16))


# ---- 2. count_valid_labels ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [1, 12, 14])
# The grid is capped at 256 x 1 024 threads.  262 147 labels are the first size past one pass of the element loop (the unaligned
# view); the 16-byte loop takes four labels a thread, so only 4 x 262 144 + 4 099 labels send it (the aligned tensor) round again.
@pytest.mark.parametrize('npix', [1, 3, 4, 5, 1023, 1025, 4099, 262144 + 3, 4 * 262144 + 4099])
def test_count_valid_labels_tail_unaligned_and_grid_stride(ops, npix, C):
    rng = np.random.default_rng(npix + C)
    odd = np.array([-7, -1, 0, C - 1, C, 255, 2 ** 31 - 1], np.int64)
    lab = np.where(rng.random(npix + 1) < 0.5, odd[rng.integers(0, len(odd), npix + 1)], rng.integers(-1, C + 1, npix + 1))
    lab = lab.astype(np.int32)
    aligned, shifted = _dev(lab[:npix]), _dev(lab)[1:]       # 16-byte loads + the npix % 4 tail; a 4-byte offset: scalar path
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    for view, host in ((aligned, lab[:npix]), (shifted, lab[1:])):
        count = torch.full((1,), 5, dtype=torch.int64, device='cuda')
        ops.count_valid_labels(view, C, count)
        assert count.item() == 5 + int(((host >= 0) & (host < C)).sum())


# ---- 3. pool / relu / x2-upsample gradients -----------------------------------------------------------------------------------

POS0, NEG0, SUB, NEGSUB = 0x0000, -0x8000, 0x0001, -0x7fff       # bf16 bits as int16: +0, -0.0, smallest subnormal, its negative

MAPS = [(1, 2, 2), (2, 12, 20), (1, 6, 34)]


@pytest.mark.parametrize('c', [8, 24, 64, 192])
@pytest.mark.parametrize('n,h,w', MAPS)
def test_maxpool_backward_exact(ops, n, h, w, c):
    rng = np.random.default_rng(n * h * w + c)
    y = _bf16_bits(rng.integers(0, 3, (n, h, w, c)).astype(np.float32))           # many ties, many zeros
    neg, two = _bf16_bits(np.array([-1.0, 2.0], np.float32))
    # the first window of channels 0-3: maximum +0 / -0.0 among negatives / the subnormal (> 0: passes) / four equal positives
    y[0, 0:2, 0:2, 0] = [[POS0, NEG0], [NEG0, POS0]]
    y[0, 0:2, 0:2, 1] = [[neg, NEG0], [neg, neg]]
    y[0, 0:2, 0:2, 2] = [[POS0, SUB], [POS0, NEG0]]
    y[0, 0:2, 0:2, 3] = [[two, two], [two, two]]
    dp = _bf16_bits(rng.integers(-4, 5, (n, h // 2, w // 2, c)).astype(np.float32))
    dp[0, 0, 0, :4] = _bf16_bits(np.array([3.0, -2.0, 4.0, -3.0], np.float32))
    dy = ops.Act(n, h, w, c)
    dy.interior().fill_(3.0)
    ops.maxpool2x2_bwd(_act_from_bits(ops, y), _act_from_bits(ops, dp), dy)
    torch.cuda.synchronize()
    # MaxPoolGrad + ReluGrad: the FIRST maximum in row-major order takes the gradient, and only if it is > 0
    win = _bits_to_f64(y).reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    assert _bits_to_f64(np.array([SUB], np.int16))[0] > 0
    take = (np.arange(4) == win.argmax(-1)[..., None]) & (win.max(-1) > 0)[..., None]     # (numpy's argmax: the first maximum)
    out = np.where(take, dp[..., None], np.int16(0)).reshape(n, h // 2, w // 2, c, 2, 2).transpose(0, 1, 4, 2, 5, 3)
    want = _padded(out.reshape(n, h, w, c))
    assert want[0, 1, 2, 2] == dp[0, 0, 0, 2] and want[0, 1, 1, 3] == dp[0, 0, 0, 3] and not want[0, 1:3, 1:3, :2].any()
    assert np.array_equal(_act_bits(dy), want)                                   # bits, interior and zero border


def _relu_case(rng, shape):
    """g: random bf16; ref: -1 / 0 / 1 with +0, -0.0 and both subnormals planted.  As int16, bf16 bits are > 0 exactly where
    the value is > 0 (no NaN here): the expected output is an integer select."""
    g = _bf16_bits(rng.standard_normal(shape).astype(np.float32))
    ref = _bf16_bits(rng.integers(-1, 2, shape).astype(np.float32))
    pick = rng.random(shape)
    for i, v in enumerate((POS0, NEG0, SUB, NEGSUB)):
        ref[(pick >= 0.05 * i) & (pick < 0.05 * (i + 1))] = v
    return g, ref, np.where(ref > 0, g, np.int16(0))


@pytest.mark.parametrize('c', [8, 24, 64, 192])
@pytest.mark.parametrize('n,h,w', MAPS)
def test_relu_backward_exact(ops, n, h, w, c):
    g, ref, want = _relu_case(np.random.default_rng(n * h * w + c), (n, h, w, c))
    if ref.size >= 100:                                       # 5 % of the elements each: the 2 x 2 map may miss one
        assert (ref == SUB).any() and (ref == NEG0).any()
    out = ops.Act(n, h, w, c)
    out.interior().fill_(3.0)
    ops.relu_bwd(_act_from_bits(ops, g), _act_from_bits(ops, ref), out)
    torch.cuda.synchronize()
    assert np.array_equal(_act_bits(out), _padded(want))


def test_relu_backward_grid_stride_loop(ops):
    """5 x 128 x 256 x 128 padded elements = 2 621 440 groups of eight, more than the 8 192 x 256 threads of the capped grid."""
    n, h, w, c = 5, 126, 254, 128
    assert n * (h + 2) * (w + 2) * c // 8 > 8192 * 256
    g, ref, want = _relu_case(np.random.default_rng(0), (n, h, w, c))
    out = ops.Act(n, h, w, c)
    out.t.fill_(3.0)                                          # the kernel walks the whole padded buffer: border of ref is 0
    ops.relu_bwd(_act_from_bits(ops, g), _act_from_bits(ops, ref), out)
    torch.cuda.synchronize()
    assert np.array_equal(_act_bits(out), _padded(want))


@pytest.mark.parametrize('c', [8, 64, 192])
@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 5, 7), (1, 24, 48)])
def test_upsample2x_backward_against_float64(ops, n, h, w, c):
    """ds5 = (s5 > 0) * sum over the 4 x 4 footprint of wy wx dfused (up2(s5) > 0).  s5 >= 0, so up2(s5) > 0 is the same set in
    any precision (positive weights); 70 % of s5 is exactly 0 in 2 x 2 blocks, so the inner mask really cuts."""
    rng = np.random.default_rng(n * h * w + c)
    keep = rng.random((n, (h + 1) // 2, (w + 1) // 2, c)) >= 0.7
    keep = keep.repeat(2, 1).repeat(2, 2)[:, :h, :w]
    s5 = fo.round_bf16(np.abs(rng.standard_normal((n, h, w, c))).astype(np.float32)) * keep
    df = fo.round_bf16(rng.standard_normal((n, 2 * h, 2 * w, c)).astype(np.float32))
    By, Bx = _deconv_matrix(h, 2), _deconv_matrix(w, 2)
    s64, d64 = s5.astype(np.float64), df.astype(np.float64)
    ein = lambda spec, x: torch.einsum(spec, torch.from_numpy(By), torch.from_numpy(x), torch.from_numpy(Bx)).numpy()  # noqa: E731
    mask = ein('oi,nijc,pj->nopc', s64) > 0
    assert 0.1 <= 1.0 - mask.mean() <= 0.9, mask.mean()                       # a condition on the input
    live = s64 > 0
    ref = ein('oi,nopc,pj->nijc', d64 * mask) * live
    A = ein('oi,nopc,pj->nijc', np.abs(d64) * mask) * live
    ds5 = ops.Act(n, h, w, c)
    ds5.interior().fill_(3.0)
    ops.upsample2x_bwd(ops.Act.from_dense(_dev(df)), ops.Act.from_dense(_dev(s5.astype(np.float32))), ds5)
    torch.cuda.synchronize()
    assert _border_is_zero(ds5)
    err = np.abs(ds5.interior().float().cpu().numpy().astype(np.float64) - ref)
    # bf16 store + 16 footprint terms, each a product of two roundings and one addition: 16 EPS A is generous and fixed
    assert _ratio('upsample2x_bwd', err, BF16 * np.abs(ref) + 16 * EPS * A) <= 1.0, err.max()


# ---- 4. optimizers ------------------------------------------------------------------------------------------------------------

STEPS = 3
HP = {'lr': 1e-2, 'beta1': 0.8, 'beta2': 0.99, 'eps': 1e-6, 'decay': 0.8, 'grad_scale': 0.5}
HP = {k: float(np.float32(v)) for k, v in HP.items()}      # the kernels take floats: the reference uses the same values


def _adam_lr_t(t):
    return float(np.float32(HP['lr'] * np.sqrt(1 - HP['beta2'] ** t) / (1 - HP['beta1'] ** t)))


def _opt_formulas(kind, p, grads, state, dt):
    """[TF1] update rules (include/xview_hip.h) in dtype dt; returns p, the state buffers and per step (|p|, |update|)."""
    c = lambda v: dt(v)                                      # noqa: E731
    p = p.astype(dt)
    state = [s.astype(dt) for s in state]
    trace = []
    for t, g in enumerate(grads, 1):
        gi = g.astype(dt) * c(HP['grad_scale'])
        if kind == 'adam':
            m = c(HP['beta1']) * state[0] + (c(1) - c(HP['beta1'])) * gi
            v = c(HP['beta2']) * state[1] + (c(1) - c(HP['beta2'])) * gi * gi
            state = [m, v]
            upd = c(_adam_lr_t(t)) * m / (np.sqrt(v) + c(HP['eps']))
        elif kind == 'rmsprop':
            ms = c(HP['decay']) * state[0] + (c(1) - c(HP['decay'])) * gi * gi
            state = [ms]
            upd = c(HP['lr']) * gi / np.sqrt(ms + c(HP['eps']))
        else:
            acc = state[0] + gi * gi
            state = [acc]
            upd = c(HP['lr']) * gi / np.sqrt(acc)
        p = p - upd
        assert p.dtype == dt and upd.dtype == dt
        trace.append((np.abs(p), np.abs(upd)))
    return p, state, trace


@pytest.mark.parametrize('n', [1, 255, 257, 1000, 2097152 + 5])          # 2 097 157: past the 8 192 x 256 threads of the grid
@pytest.mark.parametrize('kind', ['adam', 'rmsprop', 'adagrad'])
def test_optimizers_three_steps_parameters_and_state(ops, kind, n):
    """A fresh gradient per step, signs included.  v, ms and accum are sums of non-negative terms and are held to (4 STEPS) EPS
    relative to the float64 result.  Adam's m is a signed sum: its bound is the same (4 STEPS) EPS times A, the sum of the
    magnitudes of its beta-weighted terms -- equal to |m|, the relative bound, wherever the element's three gradients share a
    sign (a quarter of them), and the only meaningful one where they cancel; Adam's |update| in the bound on p carries A in
    place of |m| likewise.  One element in ten has g = 0 throughout: m = v = 0 and Adam's update is exactly 0."""
    rng = np.random.default_rng(n)
    p0 = rng.standard_normal(n).astype(np.float32)
    live = rng.random(n) >= 0.1
    live[0] = n == 1
    grads = [(live * rng.standard_normal(n)).astype(np.float32) for _ in range(STEPS)]
    # TF's initial values (include/xview_hip.h): Adam m = v = 0, RMSProp ms = 1, Adagrad accum = 0.1 (never 0: 0 / 0 at g = 0)
    state0 = {'adam': [np.zeros(n), np.zeros(n)], 'rmsprop': [np.ones(n)], 'adagrad': [np.full(n, 0.1)]}[kind]
    state0 = [s.astype(np.float32) for s in state0]
    ref_p, ref_state, trace = _opt_formulas(kind, p0, grads, state0, np.float64)
    # state buffers: at most 4 roundings a step (g * scale, the two products, the sum), relative to the float64 result
    state_bound = [(4 * STEPS) * EPS * np.abs(s) for s in ref_state]
    if kind == 'adam':
        _, (A_m, _), trace_A = _opt_formulas(kind, p0, [np.abs(g) for g in grads], state0, np.float64)   # same v, m -> A
        like = np.all([g >= 0 for g in grads], 0) | np.all([g <= 0 for g in grads], 0)
        assert np.array_equal(A_m[like], np.abs(ref_state[0])[like]) and (n < 255 or (like & live).any() and not like.all())
        state_bound[0] = (4 * STEPS) * EPS * A_m
        trace = [(ap, au) for (ap, _), (_, au) in zip(trace, trace_A)]
    # p: per step one rounding of the subtraction at |p| and (8 * STEPS) roundings' worth of the update (state error 4 * STEPS,
    # half of it through the square root, plus sqrt, + eps, the division and the product with lr), summed over the steps
    p_bound = sum(EPS * ap + (8 * STEPS) * EPS * au for ap, au in trace)
    # float32 on the host meets the same bounds
    h_p, h_state, _ = _opt_formulas(kind, p0, grads, state0, np.float32)
    assert (np.abs(h_p - ref_p) <= p_bound).all()
    assert all((np.abs(h - r) <= b).all() for h, r, b in zip(h_state, ref_state, state_bound))
    p, state = _dev(p0), [_dev(s) for s in state0]
    for t, g in enumerate(grads, 1):
        if kind == 'adam':
            ops.adam_step(p, _dev(g), state[0], state[1], _adam_lr_t(t), beta1=HP['beta1'], beta2=HP['beta2'], eps=HP['eps'],
                          grad_scale=HP['grad_scale'])
        elif kind == 'rmsprop':
            ops.rmsprop_step(p, _dev(g), state[0], HP['lr'], decay=HP['decay'], eps=HP['eps'], grad_scale=HP['grad_scale'])
        else:
            ops.adagrad_step(p, _dev(g), state[0], HP['lr'], grad_scale=HP['grad_scale'])
    torch.cuda.synchronize()
    assert _ratio(kind + ' p', np.abs(p.cpu().numpy().astype(np.float64) - ref_p), p_bound) <= 1.0
    for name, s, r, b in zip({'adam': 'mv', 'rmsprop': ['ms'], 'adagrad': ['accum']}[kind], state, ref_state, state_bound):
        assert _ratio('%s %s' % (kind, name), np.abs(s.cpu().numpy().astype(np.float64) - r), b) <= 1.0, name
    if kind == 'adam':
        zero = ~live
        assert np.array_equal(p.cpu().numpy()[zero], p0[zero]) and not state[0].cpu().numpy()[zero].any()


# ---- 5. confusion matrix, Dirichlet sufficient statistics ---------------------------------------------------------------------

def _offset_view(host, offset):
    """The array on the device, starting `offset` elements into a fresh (16-byte aligned) allocation."""
    flat = torch.empty(host.size + offset, dtype=torch.from_numpy(host[:0]).dtype, device='cuda')
    assert flat.data_ptr() % 16 == 0
    v = flat[offset:].view(host.shape)
    v.copy_(torch.from_numpy(host))
    assert offset == 0 or v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize('npix', [1, 7, 8, 9, 4653, 256 * 1024 * 8 + 13])          # the last: past one pass of the capped grid
@pytest.mark.parametrize('C', [1, 2, 12, 14, 33, 64])
def test_confusion_matrix_exact(ops, C, npix):
    """cm[label][pred] += 1 where 0 <= label < C and 0 <= pred < C, everything else skipped; 16-byte loads where both maps are
    aligned, element loads from element 1 of either; two calls accumulate into one matrix."""
    rng = np.random.default_rng(C * 100003 + npix)
    sets = []
    for _ in range(2):
        lab = rng.integers(-1, C + 1, npix)
        lab[rng.random(npix) < 0.05] = 255
        pred = rng.integers(-1, C + 1, npix).astype(np.int64)
        pred[rng.random(npix) < 0.05] = 2 ** 40
        sets.append((lab.astype(np.int32), pred))
    want = np.full((C, C), 3, np.int64)
    for lab, pred in sets:
        ok = (lab >= 0) & (lab < C) & (pred >= 0) & (pred < C)
        want += np.bincount(lab[ok].astype(np.int64) * C + pred[ok], minlength=C * C).reshape(C, C)
    assert npix < 100 or want.sum() > 3 * C * C
    for offset in (0, 1):
        cm = torch.full((C, C), 3, dtype=torch.int64, device='cuda')
        for lab, pred in sets:
            ops.confusion_matrix(_offset_view(lab, offset), _offset_view(pred, offset), cm)
        assert np.array_equal(cm.cpu().numpy(), want), offset


def _suffstats_inputs(rng, npix, C):
    prob = rng.random((npix, C)).astype(np.float32) ** 4
    prob[rng.random((npix, C)) < 0.2] = 0.0                                  # exact zeros
    hot = rng.random(npix) < 0.2                                             # one-hot rows: exact ones and zeros
    prob[hot] = np.eye(C, dtype=np.float32)[rng.integers(0, C, int(hot.sum()))]
    lab = rng.integers(-1, C + 1, npix)
    lab[rng.random(npix) < 0.05] = 255
    return prob, lab.astype(np.int32)


@pytest.mark.parametrize('C,npix', [(C, npix) for C in (1, 2, 12, 14, 20, 32, 33, 64) for npix in (1, 5, 4653)] +
                         [(12, 256 * 1024 + 77)])                            # the last: past one pass of the capped grid
def test_dirichlet_suffstats_against_float64(ops, C, npix):
    """S[label][k] += log(1e-10 + p[k]) with the sum 1e-10 + p made in float32 (kernel and reference graph alike), counts[label]
    += 1, over the pixels with 0 <= label < C.  C % 4 == 0 and C <= 32 take the 16-byte row loads when `prob` is aligned; other
    class counts and a 4-byte-offset `prob` the element loads; the number of LDS table copies goes 16 -> 4 -> 1 with C."""
    rng = np.random.default_rng(C * 100003 + npix)
    prob, lab = _suffstats_inputs(rng, npix, C)
    ok = (lab >= 0) & (lab < C)
    onehot = np.zeros((npix, C))
    onehot[ok, lab[ok]] = 1.0
    x32 = np.float32(1e-10) + prob
    assert x32.dtype == np.float32
    term = np.log(x32.astype(np.float64))
    S_ref = onehot.T @ term
    counts_ref = onehot.sum(0).astype(np.int64)
    # per pixel: the hardware logarithm to 1 ulp of log2 x, times ln 2 (two roundings), converted: 4 EPS |term|; + EPS absolute
    # for terms near 0, where an ulp of the result means nothing
    bound = onehot.T @ (4 * EPS * np.abs(term) + EPS)
    # float32 on the host (libm logf) meets the same bound
    assert (np.abs(onehot.T @ np.log(x32).astype(np.float64) - S_ref) <= bound).all()
    rs = np.random.default_rng(1)
    S0, c0 = rs.standard_normal((C, C)), rs.integers(0, 9, C).astype(np.int64)
    for offset in ((0, 1) if C % 4 == 0 else (0,)):
        S, counts = _dev(S0), _dev(c0)
        for _ in range(2):                                                   # two calls accumulate
            ops.dirichlet_suffstats(_offset_view(prob, offset), _dev(lab), S, counts)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), c0 + 2 * counts_ref)
        # (the double additions onto the prefilled cell: 2^-52 relative each, two calls of at most 256 workgroups)
        lim = 2 * bound + 2.0 ** -52 * 512 * (np.abs(S0) + 2 * np.abs(S_ref))
        assert _ratio('dirichlet_suffstats', np.abs(S.cpu().numpy() - S0 - 2 * S_ref), lim) <= 1.0, offset
