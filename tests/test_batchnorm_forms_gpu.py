"""Every form of the training-mode batch norm (csrc/batchnorm.hip) against a float64 reference of the same operation.

The inputs are bf16 values; the reference is float64 torch-CPU on the exact tensors the kernel read.  Where a relu mask or a
max-pool route matters, the reference takes it from the GPU's own stored bf16 output, so no error compounds and every bound
below follows from the kernel's own arithmetic (fp32 chains of a few tens of additions per thread, an LDS reduction, fp64
after that: a few tens of units of 2^-24 relative to the sum of the magnitudes of the terms).

The statistics and gradient reductions walk their positions with a grid chosen by bn_reduce_grid; the walk cases state the
regime they land in (positions per thread, grid stride against a row and an image, idle threads, the grid cap) and assert it
through a copy of that rule, so that a later change to the grid cannot quietly turn a case into a trivial one."""
import itertools
import types

import numpy as np
import pytest
import torch

from oracle import fcn_oracle as fo

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.99
U24 = 2.0 ** -24
CHUNK_ELEMS = 1 << 22       # values per chunk of the float64 reference (the largest map has 2^26)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops as o
    return o


def _lib():
    from modular_semantic_segmentation_amd import _lib as lb
    return lb


# ---- the walk of bn_reduce_kernel ----------------------------------------------------------------------------------
def reduce_grid(total):
    """bn_reduce_grid (csrc/batchnorm.hip): at least 16 elements per thread and 64 workgroups, at most one workgroup per 256
    elements and BN_MAX_GRID = 2048 workgroups."""
    g = max(64, -(-total // 4096))
    cap = min(2048, max(1, -(-total // 256)))
    return min(g, cap)


def walk(n, h, w, c):
    total = n * h * w * c // 8
    g = reduce_grid(total)
    stride_px = g * 256 * 8 // c                       # the grid stride in pixels (a thread keeps its 8-channel group)
    return dict(grid=g, per_thread=-(-total // (g * 256)), idle=total < g * 256, stride_px=stride_px,
                below_row=stride_px < w, images=stride_px // (h * w), capped=g == 2048)


# (N, H, W, C), the regime claimed: per_thread = most positions a thread visits; MODE 0 runs its 4-way loop from 4 on, the
# backward reductions their 2-way loop from 2 on
WALK = {
    'one_pixel': ((1, 1, 1, 64), dict(idle=True, per_thread=1)),
    'one_row': ((1, 1, 7, 64), dict(idle=True, per_thread=1)),
    'column': ((3, 5, 1, 64), dict(idle=True, per_thread=1, images=6)),          # stride 32 px: six 5-pixel images
    'row_pair': ((2, 1, 33, 64), dict(idle=True, per_thread=1)),
    'trunk_small': ((2, 12, 20, 64), dict(idle=False, per_thread=1)),
    'trunk_small_512': ((2, 12, 20, 512), dict(idle=False, per_thread=2)),
    'below_row': ((1, 3, 100, 2048), dict(grid=64, stride_px=64, below_row=True, images=0, per_thread=5)),
    'many_images': ((160, 7, 9, 64), dict(grid=64, stride_px=2048, images=32, per_thread=5)),
    'quad_twice': ((2, 96, 96, 64), dict(grid=64, stride_px=2048, per_thread=9)),
    'conv5_b16': ((16, 24, 48, 512), dict(grid=288, stride_px=1152, images=1, per_thread=16)),
    'capped': ((2, 512, 1024, 64), dict(grid=2048, capped=True, per_thread=16, stride_px=65536)),
}
BIG = ('below_row', 'many_images', 'quad_twice', 'conv5_b16', 'capped')


def _check_regime(name):
    shape, claim = WALK[name]
    got = walk(*shape)
    for k, v in claim.items():
        assert got[k] == v, (name, k, got)
    return shape


def test_walk_cases_land_in_the_regimes_they_claim():
    for name in WALK:
        _check_regime(name)
    assert walk(*WALK['many_images'][0])['images'] > 0 and not walk(*WALK['many_images'][0])['capped']


# ---- inputs and the float64 reference ---------------------------------------------------------------------------------
def _bf16_map(shape, seed, mean=0.3, std=1.5):
    """A bf16 NHWC map on the GPU (drawn there: the largest map has 67 M values)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    return (torch.randn(shape, device='cuda', generator=g) * std + mean).bfloat16()


def _params(c, seed):
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
    beta = (0.3 * rng.standard_normal(c)).astype(np.float32)
    mm0 = (0.1 * rng.standard_normal(c)).astype(np.float32)
    mv0 = rng.uniform(0.5, 1.5, c).astype(np.float32)
    return [torch.from_numpy(a).cuda() for a in (gamma, beta, mm0, mv0)]


def _rows(c):
    return max(1, CHUNK_ELEMS // c)


def _chunks(t):
    """Float64 CPU chunks of rows of pixels of a tensor [..., C] (chunk i holds pixels i * _rows(C) ...)."""
    c = t.shape[-1]
    flat = t.reshape(-1, c)
    r = _rows(c)
    for i in range(0, flat.shape[0], r):
        yield flat[i:i + r].cpu().double()


def _sl(i, c):
    return slice(i * _rows(c), (i + 1) * _rows(c))


def _ref_stats(z):
    """Per channel: sum z, sum z^2, sum |z| in float64 over the exact values; mean and biased variance from them (two-pass
    variance: no cancellation in the reference)."""
    c = z.shape[-1]
    s1, s2, sa = (torch.zeros(c, dtype=torch.float64) for _ in range(3))
    M = 0
    for ch in _chunks(z):
        s1 += ch.sum(0)
        s2 += (ch * ch).sum(0)
        sa += ch.abs().sum(0)
        M += ch.shape[0]
    mean = s1 / M
    var = torch.zeros(c, dtype=torch.float64)
    for ch in _chunks(z):
        var += ((ch - mean) ** 2).sum(0)
    return dict(s1=s1, s2=s2, sa=sa, M=M, mean=mean, var=var / M, invstd=1.0 / torch.sqrt(var / M + EPS))


def _ref_grad_sums(dy, mask, z, mean, invstd):
    """sum g, sum g * zhat and the sums of their magnitudes, g = dy * mask (mask None: no relu)."""
    c = z.shape[-1]
    sg, sgz, ag, agz = (torch.zeros(c, dtype=torch.float64) for _ in range(4))
    for g, m, zz in zip(_chunks(dy), _chunks(mask) if mask is not None else itertools.repeat(None), _chunks(z)):
        if m is not None:
            g = g * (m > 0)
        zh = (zz - mean) * invstd
        sg += g.sum(0)
        sgz += (g * zh).sum(0)
        ag += g.abs().sum(0)
        agz += (g * zh).abs().sum(0)
    return dict(sg=sg, sgz=sgz, ag=ag, agz=agz)


def _cpu(t):
    return t.detach().cpu().double()


def _assert_bf16_close(got, ref_fn, what):
    """got (GPU bf16 [..., C]) against the float64 values ref_fn(chunk index) in chunks: within one bf16 ulp -- the output
    rounding (half an ulp) plus the fp32 arithmetic before it, which is below 1e-6 of the largest value --, and fewer than 1 % of
    the elements off the correctly rounded value in their bits."""
    worst, off, n, mx = 0.0, 0, 0, 0.0
    refs = []
    for i, g in enumerate(_chunks(got)):
        r = ref_fn(i)
        refs.append((g, r))
        mx = max(mx, float(r.abs().max()))
    for i, (g, r) in enumerate(refs):
        tol = 2.0 ** -8 * r.abs() + 1e-6 * mx
        err = (g - r).abs()
        assert bool((err <= tol).all()), '%s: worst %.3g of its bound' % (what, float((err / tol).max()))
        worst = max(worst, float((err / tol).max()))
        off += int((g != r.float().bfloat16().double()).sum())
        n += g.numel()
    # (a map of under a hundred values may hold one element at a rounding edge)
    assert off < max(0.01 * n, 2), '%s: %d of %d elements are not the rounded reference' % (what, off, n)
    return worst, off / n


def _check_sums(sums, ref, what):
    c = sums.numel() // 2
    s = _cpu(sums)
    # fp32 chains: <= 16 positions per thread + <= 32 rows of the LDS column sum, then fp64: well inside 2e-6 of sum |terms|
    e1 = float(((s[:c] - ref['s1']).abs() / ref['sa']).max())
    e2 = float(((s[c:] - ref['s2']).abs() / ref['s2']).max())
    assert e1 <= 2e-6 and e2 <= 2e-6, (what, e1, e2)
    return max(e1, e2)


def _check_stats(st, mm, mv, mm0, mv0, ref, gamma, what, rel_inv=1e-5):
    mean, inv = _cpu(st.mean), _cpu(st.invstd)
    std = torch.sqrt(ref['var'])
    # mean = (fp64 sum of fp32 partials) / M, rounded to fp32: the relative error of the sums, scaled by sum|z| / M
    assert bool(((mean - ref['mean']).abs() <= 1e-5 * (ref['mean'].abs() + std) + 1e-30).all()), what
    # invstd: E[z^2] - E[z]^2 in fp64 from fp32 partial sums -- their relative error times (mean^2 + var) / (var + eps)
    e_inv = float(((inv - ref['invstd']).abs() / ref['invstd']).max())
    assert e_inv <= rel_inv, (what, 'invstd', e_inv)
    sc = _cpu(st.scale)
    want_sc = _cpu(gamma) * ref['invstd']
    assert bool(((sc - want_sc).abs() <= (rel_inv + 2 * U24) * want_sc.abs()).all()), what
    # moving statistics: fp32 momentum update of fp32-rounded batch values; unbiased variance M / (M - 1) (M > 1)
    M = ref['M']
    unb = ref['var'] * (M / (M - 1.0) if M > 1 else 1.0)
    want_mm = MOM * _cpu(mm0) + (1 - MOM) * ref['mean']
    want_mv = MOM * _cpu(mv0) + (1 - MOM) * unb
    assert bool(((_cpu(mm) - want_mm).abs() <= 4 * U24 * (MOM * _cpu(mm0).abs() + (1 - MOM) * ref['mean'].abs())
                 + (1 - MOM) * 1e-5 * (ref['mean'].abs() + std)).all()), (what, 'moving mean')
    # (the variance carries twice the relative error of invstd, times (var + eps) / var <= 1.3 at std >= 2^-4)
    e_mv = float(((_cpu(mv) - want_mv).abs() / want_mv).max())
    assert e_mv <= 3 * rel_inv + 4 * U24, (what, 'moving variance', e_mv)
    return e_inv


def _forward(ops, z, c, seed, deterministic=True, relu=True):
    gamma, beta, mm0, mv0 = _params(c, seed)
    n, h, w, _ = z.shape
    za = ops.Act.from_dense(z)
    ya = ops.Act(n, h, w, c)
    st = ops.BnState(c, 'cuda', deterministic=deterministic)
    mm, mv = mm0.clone(), mv0.clone()
    ops.bn_forward(za, gamma, beta, mm, mv, st, ya, relu=relu)
    torch.cuda.synchronize()
    return dict(za=za, ya=ya, st=st, gamma=gamma, beta=beta, mm0=mm0, mv0=mv0, mm=mm, mv=mv)


def _y_ref(z, ref, gamma, beta, relu):
    zz = z.reshape(-1, z.shape[-1])
    g, b = _cpu(gamma), _cpu(beta)

    def f(i):
        y = (zz[_sl(i, zz.shape[1])].cpu().double() - ref['mean']) * ref['invstd'] * g + b
        return y.clamp_min(0) if relu else y
    return f


# ---- statistics + finalize + apply --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(WALK))
def test_statistics_and_apply_with_a_workspace(ops, case):
    n, h, w, c = _check_regime(case)
    z = _bf16_map((n, h, w, c), seed=len(case) * 7 + c)
    ref = _ref_stats(z)
    f = _forward(ops, z, c, seed=c + n)
    st = f['st']
    e_sum = _check_sums(st.sums, ref, case)
    e_inv = _check_stats(st, f['mm'], f['mv'], f['mm0'], f['mv0'], ref, f['gamma'], case)
    worst, off = _assert_bf16_close(f['ya'].interior(), _y_ref(z, ref, f['gamma'], f['beta'], True), case + ' y')
    # the workspace path is bitwise reproducible: a second run leaves the same bits everywhere
    f2 = _forward(ops, z, c, seed=c + n)
    for name in ('sums', 'mean', 'invstd', 'scale', 'shift'):
        assert torch.equal(getattr(st, name), getattr(f2['st'], name)), name
    assert torch.equal(f['mm'], f2['mm']) and torch.equal(f['mv'], f2['mv']) and torch.equal(f['ya'].t, f2['ya'].t)
    print('%s: sums %.2e (bound 2e-6), invstd %.2e (1e-5), y %.2f of its bound, %.3f%% off the rounded value'
          % (case, e_sum, e_inv, worst, 100 * off))


@pytest.mark.parametrize('case', ['one_row', 'column', 'trunk_small_512', 'below_row', 'many_images', 'capped'])
def test_statistics_with_atomics(ops, case):
    """BnState(deterministic=False): a memset, f64 atomics per workgroup, then xv_bn_finalize (bn_finalize_kernel)."""
    n, h, w, c = _check_regime(case)
    z = _bf16_map((n, h, w, c), seed=len(case) * 7 + c)
    ref = _ref_stats(z)
    fa = _forward(ops, z, c, seed=c + n, deterministic=False)
    st = fa['st']
    e_sum = _check_sums(st.sums, ref, case)
    e_inv = _check_stats(st, fa['mm'], fa['mv'], fa['mm0'], fa['mv0'], ref, fa['gamma'], case)
    _assert_bf16_close(fa['ya'].interior(), _y_ref(z, ref, fa['gamma'], fa['beta'], True), case + ' y')
    # against the workspace path: the same partial sums added in another order -- within the same bound of each other
    fw = _forward(ops, z, c, seed=c + n)
    s_a, s_w = _cpu(st.sums), _cpu(fw['st'].sums)
    assert bool(((s_a[:c] - s_w[:c]).abs() <= 2e-6 * ref['sa']).all())
    assert bool(((s_a[c:] - s_w[c:]).abs() <= 2e-6 * ref['s2']).all())
    print('%s atomics: sums %.2e, invstd %.2e' % (case, e_sum, e_inv))


@pytest.mark.parametrize('case', ['quad_twice', 'conv5_b16'])
def test_statistics_with_large_offsets(ops, case):
    """Per-channel mean / std of 0, 4 and 16 with std from 2^-4 to 2^4: E[z^2] - E[z]^2 loses log2(1 + ratio^2) bits of
    the fp32 partial sums.  invstd, scale and the moving variance within 1e-5 up to ratio 4 and 1e-3 at ratio 16."""
    n, h, w, c = _check_regime(case)
    ratio = torch.tensor([0.0, 4.0, 16.0], device='cuda').repeat(c // 3 + 1)[:c]
    std = 2.0 ** torch.linspace(-4, 4, c, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(c)
    z = (torch.randn((n, h, w, c), device='cuda', generator=g) * std + ratio * std).bfloat16()
    ref = _ref_stats(z)
    f = _forward(ops, z, c, seed=c + 1)
    st = f['st']
    _check_sums(st.sums, ref, case)
    r = ratio.cpu().double()
    inv_err = (_cpu(st.invstd) - ref['invstd']).abs() / ref['invstd']
    worst = {float(q): float(inv_err[r == q].max()) for q in (0.0, 4.0, 16.0)}
    print('%s: worst relative invstd error by mean/std ratio %s (bounds 1e-5, 1e-5, 1e-3)' % (case, worst))
    assert worst[0.0] <= 1e-5 and worst[4.0] <= 1e-5 and worst[16.0] <= 1e-3, worst
    for sel, bound in (((r < 8), 1e-5), ((r > 8), 1e-3)):
        idx = torch.nonzero(sel).ravel()
        sub = dict(ref)
        for k in ('s1', 's2', 'sa', 'mean', 'var', 'invstd'):
            sub[k] = ref[k][idx]
        s = types.SimpleNamespace(**{k: getattr(st, k)[idx.cuda()] for k in ('mean', 'invstd', 'scale')})
        _check_stats(s, f['mm'][idx.cuda()], f['mv'][idx.cuda()], f['mm0'][idx.cuda()], f['mv0'][idx.cuda()], sub,
                     f['gamma'][idx.cuda()], case, rel_inv=bound)
    # y: one bf16 ulp plus what the invstd and mean bounds allow (|gamma zhat| 1e-3, |mean| + std 1e-5 in units of std)
    gam, inv_b = _cpu(f['gamma']), torch.where(r > 8, 1e-3, 1e-5)
    zz = z.reshape(-1, c)

    def extra(i):
        zh = ((zz[_sl(i, c)].cpu().double() - ref['mean']) * ref['invstd']).abs()
        return gam * (inv_b * zh + 1e-5 * (ref['mean'].abs() + torch.sqrt(ref['var'])) * ref['invstd'])
    yref = _y_ref(z, ref, f['gamma'], f['beta'], True)
    # (the count of differently rounded elements is not asserted at ratio 16: the 1e-3 of the scale moves most of them)
    worst_y = 0.0
    for i, gch in enumerate(_chunks(f['ya'].interior())):
        rr = yref(i)
        tol = 2.0 ** -8 * rr.abs() + 1e-6 * float(rr.abs().max()) + extra(i)
        assert bool(((gch - rr).abs() <= tol).all())
        worst_y = max(worst_y, float(((gch - rr).abs() / tol).max()))
    print('%s: y %.2f of its bound' % (case, worst_y))


@pytest.mark.parametrize('c', [8, 24, 64, 96, 256, 320, 2048])
@pytest.mark.parametrize('relu', [True, False])
def test_apply_fast_and_generic(ops, c, relu):
    """xv_bn_apply: bn_apply_fast_kernel where C / 8 divides 256 (64 .. 2048), bn_apply_kernel otherwise (8, 24, 96, 320):
    y = bf16([relu](fmaf(z, scale, shift))) -- at most one ulp from the float64 value, nearly always its rounding."""
    n, h, w = (2, 5, 7) if c <= 320 else (1, 3, 5)
    z = _bf16_map((n, h, w, c), seed=c)
    rng = np.random.default_rng(c)
    scale = torch.from_numpy(rng.uniform(-2, 2, c).astype(np.float32)).cuda()
    shift = torch.from_numpy(rng.uniform(-1, 1, c).astype(np.float32)).cuda()
    za, ya = ops.Act.from_dense(z), ops.Act(n, h, w, c)
    ya.t.fill_(7.0)                                 # the border must stay as it was: apply writes the interior only
    lb = _lib()
    lb.check(lb.lib().xv_bn_apply(za.xv(), scale.data_ptr(), shift.data_ptr(), int(relu), ya.xv(), None), 'xv_bn_apply')
    torch.cuda.synchronize()
    ref = _cpu(z) * _cpu(scale) + _cpu(shift)
    ref = ref.clamp_min(0) if relu else ref
    _assert_bf16_close(ya.interior(), lambda i: ref.reshape(-1, c), 'apply C=%d' % c)
    border = ya.t.clone()
    border[:, 1:-1, 1:-1] = 7.0
    assert bool((border == 7.0).all())


@pytest.mark.parametrize('c,shape', [(64, (2, 12, 20)), (256, (3, 6, 34)), (2048, (1, 4, 2))])
def test_apply_with_fused_pool(ops, c, shape):
    """xv_bn_apply_pool with and without the full-resolution output: bit-equal to xv_bn_apply + xv_maxpool2x2_fwd, exact ties
    inside windows included; both within the float64 bounds."""
    n, h, w = shape
    z = _bf16_map((n, h, w, c), seed=c + 5)
    z[:, ::2, ::2] = z[:, 1::2, 1::2]                     # exact ties between two positions of every window
    ref = _ref_stats(z)
    gamma, beta, mm0, mv0 = _params(c, c)
    za = ops.Act.from_dense(z)

    def fwd(y, pooled):
        st = ops.BnState(c, 'cuda')
        ops.bn_forward(za, gamma, beta, mm0.clone(), mv0.clone(), st, y, relu=True, pooled=pooled)
        return y
    y1 = fwd(ops.Act(n, h, w, c), None)
    q1 = ops.maxpool2x2_fwd(y1, ops.Act(n, h // 2, w // 2, c))
    y2, q2, q3 = ops.Act(n, h, w, c), ops.Act(n, h // 2, w // 2, c), ops.Act(n, h // 2, w // 2, c)
    fwd(y2, q2)
    fwd(None, q3)
    torch.cuda.synchronize()
    assert torch.equal(y1.t, y2.t) and torch.equal(q1.t, q2.t) and torch.equal(q1.t, q3.t)
    _assert_bf16_close(y2.interior(), _y_ref(z, ref, gamma, beta, True), 'y')
    yr = _y_ref(z, ref, gamma, beta, True)(0).reshape(n, h, w, c).permute(0, 3, 1, 2)
    qr = torch.nn.functional.max_pool2d(yr, 2).permute(0, 2, 3, 1).contiguous()
    _assert_bf16_close(q2.interior(), lambda i: qr.reshape(-1, c), 'pooled')


# ---- backward -----------------------------------------------------------------------------------------------------------
def _check_grads(dg, db, dg0, db0, sums_ref, what):
    """dgamma / dbeta accumulate INTO the buffers: got - start within 4e-6 of the channel's sum |g zhat| / sum |g| (the fp32
    chains of the reduction, fp32-rounded mean and invstd in zhat) plus the rounding of the fp32 addition into the buffer."""
    out = []
    for got, start, want, mag in ((dg, dg0, sums_ref['sgz'], sums_ref['agz']), (db, db0, sums_ref['sg'], sums_ref['ag'])):
        got, start = _cpu(got), _cpu(start)
        err = (got - (start + want)).abs()
        tol = 4e-6 * mag + U24 * (start + want).abs() + 1e-30
        assert bool((err <= tol).all()), '%s: worst %.3g of its bound' % (what, float((err / tol).max()))
        out.append(float((err / tol).max()))
    return max(out)


def _dz_ref(dy, mask, z, gamma, ref, sums_ref):
    """dz = gamma invstd (g - sum g / M - zhat sum g zhat / M) in float64, g = dy * mask."""
    M = ref['M']
    c = z.shape[-1]
    fl = [t.reshape(-1, c) if t is not None else None for t in (dy, mask, z)]
    gk = _cpu(gamma) * ref['invstd']

    def f(i):
        sl = _sl(i, c)
        g = fl[0][sl].cpu().double()
        if fl[1] is not None:
            g = g * (fl[1][sl].cpu().double() > 0)
        zh = (fl[2][sl].cpu().double() - ref['mean']) * ref['invstd']
        return gk * (g - sums_ref['sg'] / M - zh * sums_ref['sgz'] / M)
    return f


BWD = [(name, 'ymask') for name in ('one_row', 'column', 'trunk_small', 'trunk_small_512') + BIG] + \
      [(name, 'zmask') for name in ('one_pixel', 'row_pair', 'trunk_small', 'trunk_small_512') + BIG] + \
      [(name, 'norelu') for name in ('column', 'trunk_small', 'below_row', 'many_images', 'quad_twice', 'conv5_b16')] + \
      [(name, 'zmask_128') for name in ('trunk_small',)]


@pytest.mark.parametrize('case,variant', BWD)
def test_backward(ops, case, variant):
    """bn_backward: the relu mask read from y (MODE 1, bn_bwd_apply_fast_kernel<false>), recomputed from z (MODE 2,
    <true>), or no relu (MODE 1 without y); gradients added into non-zero dgamma / dbeta; the workspace and atomic paths
    against the reference and each other; two workspace runs bit-identical."""
    n, h, w, c = _check_regime(case)
    if variant == 'zmask_128':
        c = 128
    relu = variant != 'norelu'
    z = _bf16_map((n, h, w, c), seed=c + 11 * n)
    dy = _bf16_map((n, h, w, c), seed=c + 13 * n, mean=0.0, std=1.0)
    ref = _ref_stats(z)
    f = _forward(ops, z, c, seed=c + 3, relu=relu)
    st, ya = f['st'], f['ya']
    mask = ya.interior() if relu else None                     # the GPU's own stored activations: y > 0
    sums_ref = _ref_grad_sums(dy, mask, z, ref['mean'], ref['invstd'])
    dya = ops.Act.from_dense(dy)
    rng = np.random.default_rng(c)
    dg0 = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).cuda() * float(sums_ref['agz'].mean() / 16)
    db0 = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).cuda() * float(sums_ref['ag'].mean() / 16)
    kw = dict(mask_from_z=False) if variant == 'ymask' else {}

    def run(state):
        dg, db, dza = dg0.clone(), db0.clone(), ops.Act(n, h, w, c)
        ops.bn_backward(dya, ya if relu else None, f['za'], f['gamma'], state, dg, db, dza, **kw)
        torch.cuda.synchronize()
        return dg, db, dza
    dg, db, dza = run(st)
    what = '%s %s C=%d' % (case, variant, c)
    e_g = _check_grads(dg, db, dg0, db0, sums_ref, what)
    worst, off = _assert_bf16_close(dza.interior(), _dz_ref(dy, mask, z, f['gamma'], ref, sums_ref), what + ' dz')
    dg2, db2, dz2 = run(st)
    assert torch.equal(dg, dg2) and torch.equal(db, db2) and torch.equal(dza.t, dz2.t)
    if case in ('column', 'trunk_small', 'many_images', 'capped'):
        # the atomic path (a memset, f64 atomics, bn_grads_kernel) with the forward pass's statistics
        sa = ops.BnState(c, 'cuda', deterministic=False)
        for name in ('mean', 'invstd', 'scale', 'shift'):
            getattr(sa, name).copy_(getattr(st, name))
        dga, dba, dza_a = run(sa)
        _check_grads(dga, dba, dg0, db0, sums_ref, what + ' atomics')
        gz = (_cpu(dga) - _cpu(dg)).abs()
        assert bool((gz <= 4e-6 * sums_ref['agz'] + U24 * _cpu(dg).abs() * 2).all())
        _assert_bf16_close(dza_a.interior(), _dz_ref(dy, mask, z, f['gamma'], ref, sums_ref), what + ' dz atomics')
    print('%s: dgamma/dbeta %.2f of their bound, dz %.2f of its bound, %.3f%% off the rounded value'
          % (what, e_g, worst, 100 * off))


@pytest.mark.parametrize('c', [24, 96])
@pytest.mark.parametrize('masked', [True, False])
def test_generic_backward_apply(ops, c, masked):
    """xv_bn_bwd_apply at a channel count the fast kernel does not take: bn_bwd_apply_kernel, with st filled from the float64
    finalize (mean, invstd rounded to fp32; the sums as float64) and the mask from the GPU's y of xv_bn_apply."""
    n, h, w = 2, 9, 11
    z = _bf16_map((n, h, w, c), seed=c)
    dy = _bf16_map((n, h, w, c), seed=c + 1, mean=0.0, std=1.0)
    ref = _ref_stats(z)
    gamma, beta, _, _ = _params(c, c)
    st = ops.BnState(c, 'cuda')
    st.mean.copy_(ref['mean'].float())
    st.invstd.copy_(ref['invstd'].float())
    st.scale.copy_((_cpu(gamma) * ref['invstd']).float())
    st.shift.copy_((_cpu(beta) - ref['mean'] * _cpu(gamma) * ref['invstd']).float())
    za, ya, dya, dza = ops.Act.from_dense(z), ops.Act(n, h, w, c), ops.Act.from_dense(dy), ops.Act(n, h, w, c)
    lb = _lib()
    lb.check(lb.lib().xv_bn_apply(za.xv(), st.scale.data_ptr(), st.shift.data_ptr(), 1, ya.xv(), None), 'xv_bn_apply')
    torch.cuda.synchronize()
    mask = ya.interior() if masked else None
    sums_ref = _ref_grad_sums(dy, mask, z, ref['mean'], ref['invstd'])
    st.sums.copy_(torch.cat([sums_ref['sg'], sums_ref['sgz']]))
    lb.check(lb.lib().xv_bn_bwd_apply(dya.xv(), ya.xv() if masked else ops._NULL_ACT, za.xv(), st.mean.data_ptr(),
                                      st.invstd.data_ptr(), gamma.data_ptr(), st.sums.data_ptr(), n * h * w, dza.xv(), None),
             'xv_bn_bwd_apply')
    torch.cuda.synchronize()
    _assert_bf16_close(dza.interior(), _dz_ref(dy, mask, z, gamma, ref, sums_ref), 'generic bwd apply C=%d' % c)


@pytest.mark.parametrize('c', [64, 256])
def test_pool_backward(ops, c):
    """bn_pool_backward against float64 MaxPoolGrad (to the first maximum of the GPU's y in window order, if positive), ReluGrad
    and the batch-norm gradient; ties inside windows; gradients added into non-zero buffers."""
    n, h, w = 2, 12, 20
    z = _bf16_map((n, h, w, c), seed=c + 21)
    z[:, ::4, ::4] = z[:, 1::4, 1::4]
    z[:, 2::4, 1::4] = z[:, 3::4, 1::4]
    dp = _bf16_map((n, h // 2, w // 2, c), seed=c + 22, mean=0.0, std=1.0)
    ref = _ref_stats(z)
    f = _forward(ops, z, c, seed=c + 23)
    y = _cpu(f['ya'].interior())
    win = y.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c)
    best = win.argmax(3)                                      # torch.argmax: the first maximal index
    first = torch.zeros_like(win)
    first.scatter_(3, best.unsqueeze(3), 1.0)
    ties = int(((win == win.max(3, keepdim=True).values).sum(3) > 1).sum())
    assert ties > 0
    pos = (win.max(3).values > 0).double()
    route = first * (_cpu(dp) * pos).unsqueeze(3)
    dyf = route.reshape(n, h // 2, w // 2, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, c)
    sums_ref = _ref_grad_sums(dyf, None, z, ref['mean'], ref['invstd'])
    dg0 = torch.full((c,), 0.5, device='cuda')
    db0 = torch.full((c,), -0.25, device='cuda')
    dg, db, dza = dg0.clone(), db0.clone(), ops.Act(n, h, w, c)
    ops.bn_pool_backward(ops.Act.from_dense(dp), f['za'], f['gamma'], f['st'], dg, db, dza)
    torch.cuda.synchronize()
    _check_grads(dg, db, dg0, db0, sums_ref, 'pool backward')
    _assert_bf16_close(dza.interior(), _dz_ref(dyf, None, z, f['gamma'], ref, sums_ref), 'pool backward dz')


# ---- the batch norm behind the x8 deconv --------------------------------------------------------------------------------
def _interp(n_out, n_in, s=8):
    """The 1-D weights of the bilinear x s transposed conv (custom_layers.py:8-25; 'same' padding): A[o, i]."""
    center = (2.0 * s - 1 - (s % 2)) / (2.0 * s)
    a = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        for i in range(n_in):
            p = o + s // 2 - i * s
            if 0 <= p < 2 * s:
                a[o, i] = 1.0 - abs(p / s - center)
    return a


LOW = [(1, 3, 5, 64), (2, 4, 6, 128), (1, 2, 3, 2048)]


@pytest.mark.parametrize('low_shape', LOW)
def test_x8_head_forward_and_backward(ops, low_shape):
    """bn_forward(ups8_of=low) (statistics + finalize + apply on the recomputed map), bn_apply_ups8 and
    bn_backward(ups8_of=low) against float64 on z = upsample_raw_fwd(low, 8): the stored map, the same bits by contract."""
    n, hl, wl, c = low_shape
    h, w = 8 * hl, 8 * wl
    low = _bf16_map(low_shape, seed=c + hl)
    la = ops.Act.from_dense(low)
    zmap = ops.upsample_raw_fwd(la, 8)
    torch.cuda.synchronize()
    z = zmap.interior().contiguous()
    # the stored map is the bilinear interpolation to bf16 rounding
    zr = torch.einsum('oh,nhwc,pw->nopc', _interp(h, hl), _cpu(low), _interp(w, wl))
    _assert_bf16_close(z, lambda i: zr.reshape(-1, c), 'x8 map')
    ref = _ref_stats(z)
    gamma, beta, mm0, mv0 = _params(c, c + 1)
    st = ops.BnState(c, 'cuda')
    mm, mv = mm0.clone(), mv0.clone()
    ya = ops.Act(n, h, w, c)
    ops.bn_forward(None, gamma, beta, mm, mv, st, ya, relu=True, ups8_of=la)
    y2 = ops.bn_apply_ups8(la, st, ops.Act(n, h, w, c))
    torch.cuda.synchronize()
    _check_sums(st.sums, ref, 'x8')
    _check_stats(st, mm, mv, mm0, mv0, ref, gamma, 'x8')
    _assert_bf16_close(ya.interior(), _y_ref(z, ref, gamma, beta, True), 'x8 y')
    assert torch.equal(ya.t, y2.t)
    dy = _bf16_map((n, h, w, c), seed=c + 2, mean=0.0, std=1.0)
    sums_ref = _ref_grad_sums(dy, ya.interior(), z, ref['mean'], ref['invstd'])
    dg0, db0 = torch.full((c,), 0.125, device='cuda'), torch.full((c,), -1.0, device='cuda')
    dg, db, dza = dg0.clone(), db0.clone(), ops.Act(n, h, w, c)
    ops.bn_backward(ops.Act.from_dense(dy), None, None, gamma, st, dg, db, dza, ups8_of=la)
    torch.cuda.synchronize()
    _check_grads(dg, db, dg0, db0, sums_ref, 'x8 backward')
    _assert_bf16_close(dza.interior(), _dz_ref(dy, ya.interior(), z, gamma, ref, sums_ref), 'x8 dz')


@pytest.mark.parametrize('classes', [5, 12, 32])
def test_fused_x8_score(ops, classes):
    """score_dense_fwd_ups8: y bit-equal to bn_apply_ups8, score = y . W + b against float64 on the GPU's y (the weights enter
    as three bf16 parts: fp32 accuracy, 64 products added in fp32); more than 16 classes are refused (nothing launched)."""
    n, hl, wl, c = 1, 3, 5, 64
    low = _bf16_map((n, hl, wl, c), seed=classes)
    la = ops.Act.from_dense(low)
    gamma, beta, mm0, mv0 = _params(c, classes)
    st = ops.BnState(c, 'cuda')
    ops.bn_forward(None, gamma, beta, mm0.clone(), mv0.clone(), st, None, relu=True, ups8_of=la)
    rng = np.random.default_rng(classes)
    wsc = torch.from_numpy((0.3 * rng.standard_normal((c, classes))).astype(np.float32)).cuda()
    bsc = torch.from_numpy(rng.standard_normal(classes).astype(np.float32)).cuda()
    y1 = ops.bn_apply_ups8(la, st, ops.Act(n, 8 * hl, 8 * wl, c))
    y2 = ops.Act(n, 8 * hl, 8 * wl, c)
    score = torch.full((n, 8 * hl, 8 * wl, classes), float('nan'), device='cuda')
    fused = ops.score_dense_fwd_ups8(la, st, wsc, bsc, classes, y2, score)
    assert fused == (classes <= 16)
    if not fused:
        y2 = y1
        ops.score_dense_fwd(y1, wsc, bsc, classes, score)
    torch.cuda.synchronize()
    assert torch.equal(y1.t, y2.t)
    yd = _cpu(y2.interior()).reshape(-1, c)
    ref = yd @ _cpu(wsc) + _cpu(bsc)
    mag = yd.abs() @ _cpu(wsc).abs() + _cpu(bsc).abs()
    err = (_cpu(score).reshape(-1, classes) - ref).abs()
    # (the matrix-core form adds 3 x 64 products of y with the weights' three bf16 parts in fp32; the FMA form 64)
    assert bool((err <= 3 * 64 * U24 * mag).all()), float((err / mag).max())


@pytest.mark.parametrize('low_shape', LOW)
@pytest.mark.parametrize('block_sums', [True, False])
def test_x8_transpose(ops, monkeypatch, low_shape, block_sums):
    """upsample_raw_bwd(., 8) -- per-block sums in a workspace, or the 256-tap gather -- against the float64 adjoint."""
    monkeypatch.setattr(ops, 'UPS8_BLOCK_SUMS', block_sums)
    n, hl, wl, c = low_shape
    dy = _bf16_map((n, 8 * hl, 8 * wl, c), seed=c + 7, mean=0.0, std=1.0)
    dx = ops.upsample_raw_bwd(ops.Act.from_dense(dy), 8, ops.Act(n, hl, wl, c))
    torch.cuda.synchronize()
    ay, ax = _interp(8 * hl, hl), _interp(8 * wl, wl)
    ref = torch.einsum('oh,nopc,pw->nhwc', ay, _cpu(dy), ax)
    # up to 256 products of exact weights (multiples of 1/256) added in fp32 before the bf16 rounding: 1e-6 of the largest
    # value covers the chains at these magnitudes
    mag = torch.einsum('oh,nopc,pw->nhwc', ay, _cpu(dy).abs(), ax)
    got = _cpu(dx.interior())
    err = (got - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 256 * U24 * mag
    assert bool((err <= tol).all()), float((err / tol).max())
    assert int((got != ref.float().bfloat16().double()).sum()) < 0.01 * got.numel()
    assert not bool(dx.t[:, 0].float().any()) and not bool(dx.t[:, :, 0].float().any())     # the zero border untouched


# ---- dense float32 [rows][C] forms (the batch norm on `score`) ---------------------------------------------------------
@pytest.mark.parametrize('c', [1, 4, 5, 8, 12, 16, 31, 32])
@pytest.mark.parametrize('rows', [1, 7, 3000, 200003])
@pytest.mark.parametrize('offset', [0, 1])
def test_dense(ops, c, rows, offset):
    """bn_dense_forward / bn_dense_backward: statistics (row-vector loads where C % 4 == 0), xv_bn_finalize, apply; gradient
    sums and bn_dense_bwd_apply_rows_kernel (C in 4, 8, 12, 16 on 16-byte aligned rows) or bn_dense_bwd_apply_kernel (every
    other C, and views one float off that alignment)."""
    g = torch.Generator(device='cuda').manual_seed(c * 1000 + rows)
    buf = (torch.randn(rows * c + 4, device='cuda', generator=g) * 1.5 + 0.3).bfloat16().float()
    dbuf = torch.randn(rows * c + 4, device='cuda', generator=g).bfloat16().float()
    z = buf[offset:offset + rows * c].view(rows, c)
    dy = dbuf[offset:offset + rows * c].view(rows, c)
    y = torch.full((rows * c + 4,), float('nan'), device='cuda')[offset:offset + rows * c].view(rows, c)
    dz = torch.full((rows * c + 4,), float('nan'), device='cuda')[offset:offset + rows * c].view(rows, c)
    assert (z.data_ptr() % 16 == 0) == (offset == 0)
    gamma, beta, mm0, mv0 = _params(c, c + rows)
    st = ops.BnState(c, 'cuda')
    mm, mv = mm0.clone(), mv0.clone()
    ops.bn_dense_forward(z, gamma, beta, mm, mv, st, y)
    dg0 = torch.full((c,), 0.75, device='cuda')
    db0 = torch.full((c,), -0.5, device='cuda')
    dg, db = dg0.clone(), db0.clone()
    ops.bn_dense_backward(dy, z, gamma, st, dg, db, dz)
    torch.cuda.synchronize()
    zc, dyc = _cpu(z), _cpu(dy)
    ref = dict(s1=zc.sum(0), s2=(zc * zc).sum(0), sa=zc.abs().sum(0), M=rows, mean=zc.mean(0))
    ref['var'] = ((zc - ref['mean']) ** 2).mean(0)
    ref['invstd'] = 1.0 / torch.sqrt(ref['var'] + EPS)
    what = 'dense C=%d rows=%d offset=%d' % (c, rows, offset)
    # (the statistics were overwritten by the backward reductions: check them through the moving averages and y)
    _check_stats(st, mm, mv, mm0, mv0, ref, gamma, what)
    zh = (zc - ref['mean']) * ref['invstd']
    gam, bet = _cpu(gamma), _cpu(beta)
    y_ref = zh * gam + bet
    # y = z * scale + shift in fp32: the invstd and mean bounds (1e-5) plus a few fp32 roundings of |z scale| + |shift|
    tol = 1e-5 * gam * (zh.abs() + (ref['mean'].abs() + torch.sqrt(ref['var'])) * ref['invstd']) + \
        4 * U24 * (zc.abs() * _cpu(st.scale).abs() + _cpu(st.shift).abs())
    assert bool(((_cpu(y) - y_ref).abs() <= tol).all()), what + ' y'
    sums_ref = _ref_grad_sums(dy, None, z, ref['mean'], ref['invstd'])
    _check_grads(dg, db, dg0, db0, sums_ref, what)
    dz_ref = gam * ref['invstd'] * (dyc - sums_ref['sg'] / rows - zh * sums_ref['sgz'] / rows)
    # fp32: a few roundings of each term, the sums' own bound (4e-6 of their magnitudes), the invstd bound on the whole
    tol = gam * ref['invstd'] * (8 * U24 * (dyc.abs() + sums_ref['ag'] / rows + zh.abs() * sums_ref['agz'] / rows)
                                 + 1e-5 * (sums_ref['ag'] / rows + zh.abs() * sums_ref['agz'] / rows)) + 2e-5 * dz_ref.abs()
    err = (_cpu(dz) - dz_ref).abs()
    assert bool((err <= tol).all()), '%s dz: worst %.3g of its bound' % (what, float((err / tol).max()))


@pytest.mark.parametrize('c', [5, 12])
def test_dense_cross_entropy_with_the_batch_norm_affine(ops, c):
    """softmax_ce_dense(affine=st): logits = scores * scale + shift inside the kernel, ignored labels (-1) out of the loss and
    with zero gradient; against float64 softmax cross-entropy (the kernel's exp / log approximations: 1e-6 relative)."""
    npix = 5000
    rng = np.random.default_rng(c)
    scores = torch.from_numpy(fo.round_bf16((2 * rng.standard_normal((npix, c))).astype(np.float32))).cuda()
    labels = torch.from_numpy(rng.integers(-1, c, npix).astype(np.int32)).cuda()
    st = ops.BnState(c, 'cuda')
    st.scale.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, c).astype(np.float32)))
    st.shift.copy_(torch.from_numpy(rng.uniform(-1.0, 1.0, c).astype(np.float32)))
    valid = labels >= 0
    count = valid.sum().reshape(1).to(torch.int64)
    loss = torch.zeros(1, dtype=torch.float64, device='cuda')
    dlog = torch.full((npix, c), float('nan'), device='cuda')
    ops.softmax_ce_dense(scores, labels, count, c, loss, dlog, affine=st)
    torch.cuda.synchronize()
    lg = _cpu(scores) * _cpu(st.scale) + _cpu(st.shift)
    lab = labels.cpu().long()
    v = valid.cpu()
    logp = torch.log_softmax(lg, 1)
    k = int(v.sum())
    want = float(-(logp[v, lab[v]]).sum() / k)
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    d = torch.softmax(lg, 1)
    d[v, lab[v]] -= 1.0
    d = d / k
    d[~v] = 0.0
    err = (_cpu(dlog) - d).abs()
    assert bool((err <= 1e-5 / k).all()), float(err.max() * k)
    assert bool((_cpu(dlog)[~v] == 0).all())
