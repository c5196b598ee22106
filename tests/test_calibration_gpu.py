"""The reliability tables of csrc/calibration.hip on small maps: xv_calibration_table against the float64 definition
(calibration.table_reference) and xv_fused_head_multi_calibration_fwd against xv_calibration_table on the maps the existing
route materialises.

Bounds, derived: every term exp(x), x <= 0, of z carries at most (|x| e^x + 2 ulp) <= ~2^-23 absolute error, so for scores
given exactly |conf32 - conf64| <= DELTA = (C + 8) 2^-23.  A pixel whose float64 confidence lies within DELTA of a bin edge at
ANY tested temperature may fall on either side: it is made void before the run, and the share left out must stay below 1 %.
The bin count of a case is lowered (never the cap) until the uniform estimate 2 DELTA NB T-count is below 0.8 %."""
import ctypes
import math

import numpy as np
import pytest
import torch

from modular_semantic_segmentation_amd.calibration import Q_ONE, table_reference

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LEFT_OUT = 0.01
SENTINEL = -7
N, H, W = 2, 24, 40                                     # low resolution 3 x 5
TEMPS = {'one': [1.0], 'three': [0.5, 1.0, 2.5], 'long': [float(t) for t in np.geomspace(0.4, 3.0, 17)]}   # 17 > any capacity


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops
    return ops


def delta(c):
    return (c + 8) * 2.0 ** -23


def case_bits(c, bits, num_t, d=None):
    """the case's bin bits: the requested ones, lowered until the uniform estimate of the left-out share is below 0.8 %"""
    d = delta(c) if d is None else d
    while bits > 4 and 2 * d * (1 << bits) * num_t > 0.008:
        bits -= 1
    return bits


def void_near_edges(conf, labels, bits, d):
    """labels with every pixel within d of an inner bin edge (at any temperature) made void; the share that was left out"""
    nb = 1 << bits
    frac = conf * nb
    near = (np.abs(frac - np.round(frac)) <= d * nb) & (np.round(frac) >= 1) & (np.round(frac) <= nb - 1)
    near = near.any(0)
    valid = labels >= 0
    out = np.where(near, -1, labels).astype(np.int32)
    return out, float((near & valid).sum()) / max(1, int(valid.sum()))


def prepare(values, labels, temps, bits, d, kind=0):
    """(labels with the pixels near an edge made void, the case's bin bits, the share left out).  The confidences are not
    uniform, so where the share measured on the float64 confidences still passes the cap the bin bits of the case are lowered
    further -- a property of the inputs and the reference alone, decided before anything runs on the GPU."""
    bits = case_bits(values.shape[-1], bits, len(temps), d)
    while True:
        conf = table_reference(values, labels, temps, bits, kind=kind)[2]
        out, left_out = void_near_edges(conf, labels, bits, d)
        if left_out <= LEFT_OUT or bits == 4:
            return out, bits, left_out
        bits -= 1


def random_scores(c, seed, n=N, h=H, w=W):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, h, w, c), generator=g) * 3.5).numpy()


def random_labels(values, seed, void=0.1, right=0.5):
    """half the pixels carry the winner, a tenth is void, the rest is uniform"""
    rng = np.random.default_rng(seed)
    c = values.shape[-1]
    u = rng.random(values.shape[:-1])
    return np.where(u < right, values.argmax(-1), np.where(u < right + void, -1, rng.integers(0, c, u.shape))).astype(np.int32)


def check_against_reference(got, got_nll, values, labels, temps, bits, kind, d, groups=None, num_groups=1):
    c = values.shape[-1]
    want, want_nll, conf = table_reference(values, labels, temps, bits, kind=kind, groups=groups, num_groups=num_groups)
    got, got_nll = got.cpu().numpy(), got_nll.cpu().numpy()
    assert got.shape == want.shape and got_nll.shape == want_nll.shape
    assert np.array_equal(got[..., :2], want[..., :2])                          # count and correct: equal
    # the q column against the float64 confidences summed per bin
    ids = np.zeros(len(labels), np.int64) if groups is None else np.asarray(groups)
    grp = np.broadcast_to(ids.reshape((-1,) + (1,) * (labels.ndim - 1)), labels.shape)
    counted = (labels >= 0) & (labels < c) & (grp >= 0) & (grp < num_groups)
    sums = np.zeros(want.shape[:-1] if groups is not None else (1,) + want.shape[:-1])
    spread = float((values.max(-1) - values.min(-1)).max()) if kind == 0 else None
    for t in range(len(temps)):
        b = np.minimum(np.floor(conf[t] * Q_ONE).astype(np.int64) >> (24 - bits), (1 << bits) - 1)
        np.add.at(sums[:, t], (grp[counted], b[counted]), conf[t][counted])
    if groups is None:
        sums = sums[0]
    count = want[..., 0]
    err = np.abs(got[..., 2] / Q_ONE - sums)
    assert (err <= count * (d + 2.0 ** -24)).all(), (err.max(), d)
    if spread is not None:
        for t, T in enumerate(temps):
            bound = count[..., t, :].sum(-1) * (c + 8) * 2.0 ** -23 * max(1.0, spread / T)
            assert (np.abs(got_nll[..., t] - want_nll[..., t]) <= bound).all(), (t, got_nll[..., t], want_nll[..., t], bound)
    worst = float((err[count > 0] / count[count > 0]).max()) if (count > 0).any() else 0.0
    print('C=%d bits=%d T=%d: worst per-bin mean |conf32 - conf64| %.3e (delta %.3e)' % (c, bits, len(temps), worst, d))
    return want


@pytest.mark.parametrize('temps', list(TEMPS), ids=list(TEMPS))
@pytest.mark.parametrize('bits', [4, 10])
@pytest.mark.parametrize('c', [2, 3, 12, 13, 32])
def test_table_against_the_reference(ops, c, bits, temps):
    temps = TEMPS[temps]
    values = random_scores(c, 100 + c)
    labels = random_labels(values, 200 + c)
    labels[0, 0, :3] = (c, 255, -1)                                             # three kinds of void
    labels, bits, left_out = prepare(values, labels, temps, bits, delta(c))
    assert left_out <= LEFT_OUT, left_out
    assert (len(temps) > ops.calibration_capacity(bits)) == (len(temps) == 17)      # the long list goes in several launches
    table, nll = ops.calibration_table(torch.from_numpy(values).to(DEV), torch.from_numpy(labels).to(DEV), temps, bits)
    want = check_against_reference(table, nll, values, labels, temps, bits, 0, delta(c))
    assert int(want[0, :, 0].sum()) == int(((labels >= 0) & (labels < c)).sum()) > 1000


def test_every_pixels_confidence_is_within_delta(ops):
    """one pixel per image and one group per pixel: the q column of a group IS its pixel's fixed-point confidence"""
    worst = {}
    for c in (2, 12, 32):
        values = random_scores(c, 300 + c).reshape(-1, 1, c)
        labels = np.zeros(values.shape[:2], np.int32)
        for T in (0.5, 1.0, 2.5):
            conf = table_reference(values, labels, [T], 4)[2][0, :, 0]
            table, _ = ops.calibration_table(torch.from_numpy(values).to(DEV), torch.from_numpy(labels).to(DEV), [T], 4,
                                             groups=np.arange(len(values)), num_groups=len(values))
            table = table.cpu().numpy()
            assert (table[:, 0, :, 0].sum(-1) == 1).all()
            q = table[:, 0, :, 2].sum(-1)
            err = np.maximum(q / Q_ONE - conf, conf - (q + 1) / Q_ONE)                # q is a truncation: conf32 in [q, q + 1)
            worst[c, T] = float(err.max())
            assert err.max() <= delta(c), (c, T, err.max(), delta(c))
    print('worst |conf32 - conf64| per pixel beyond the truncation:', worst)


def test_void_labels_count_nothing(ops):
    c = 12
    values = torch.from_numpy(random_scores(c, 1)).to(DEV)
    labels = torch.from_numpy(np.random.default_rng(2).choice([-1, c, 255], (N, H, W)).astype(np.int32)).to(DEV)
    table, nll = ops.calibration_table(values, labels, [0.5, 1.0], 10)
    assert not bool(table.any()) and not bool(nll.any())


def test_probability_maps(ops):
    """kind 1: s = ln(1e-20 + p) is rounded to float32 (about 1 ulp of |s| from v_log_f32) before it enters x = (s[k] - s[win])
    / T: with |s[win]| <= ln C the argument moves by at most (2 ln C + |x| T) 2^-23 / T and the term by e^x times that, so
    DELTA grows by C (2 ln C / T + 1 / e) 2^-23 at the smallest temperature."""
    c, temps = 12, [0.5, 1.0, 2.5]
    d = delta(c) + c * (2 * math.log(c) / min(temps) + 1 / math.e) * 2.0 ** -23
    probs = torch.softmax(torch.from_numpy(random_scores(c, 5)), -1).numpy()
    labels, bits, left_out = prepare(probs, random_labels(probs, 6), temps, 10, d, kind=1)
    assert left_out <= LEFT_OUT, left_out
    table, nll = ops.calibration_table(torch.from_numpy(probs).to(DEV), torch.from_numpy(labels).to(DEV), temps, bits, kind=1)
    want = check_against_reference(table, nll, probs, labels, temps, bits, 1, d)
    want_nll = table_reference(probs, labels, temps, bits, kind=1)[1]
    count = want[0, :, 0].sum()
    logs = np.log(np.float64(np.float32(1e-20)) + probs.astype(np.float64))
    spread = float((logs.max(-1) - logs.min(-1)).max())
    for t, T in enumerate(temps):
        # the bound of the score maps with d for DELTA, and the float32 rounding of the two logarithms the term subtracts
        # (|ln(1e-20 + p)| <= 46.06)
        assert abs(float(nll[t]) - want_nll[t]) <= count * (d * max(1.0, spread / T) + 2 * 46.06 * 2.0 ** -23 / T)


def test_two_calls_are_twice_one_call(ops):
    c = 12
    values = torch.from_numpy(random_scores(c, 7)).to(DEV)
    labels = torch.from_numpy(random_labels(values.cpu().numpy(), 8)).to(DEV)
    table, nll = ops.calibration_table(values, labels, [0.5, 1.0, 2.5], 10)
    once, once_nll = table.clone(), nll.clone()
    ops.calibration_table(values, labels, [0.5, 1.0, 2.5], 10, table=table, nll=nll)
    assert torch.equal(table, 2 * once) and torch.allclose(nll, 2 * once_nll, rtol=1e-12)


def test_groups(ops):
    c, temps, bits = 12, [0.5, 1.0], 8
    values = random_scores(c, 9, n=4)
    labels = random_labels(values, 10)
    host_ids = [2, 0, 5, 2]                                                     # 5: counted nowhere
    labels, bits, left_out = prepare(values, labels, temps, bits, delta(c))
    assert left_out <= LEFT_OUT
    v, l = torch.from_numpy(values).to(DEV), torch.from_numpy(labels).to(DEV)
    ids = torch.tensor(host_ids, dtype=torch.int32, device=DEV)
    table, nll = ops.calibration_table(v, l, temps, bits, groups=ids, num_groups=3)
    check_against_reference(table, nll, values, labels, temps, bits, 0, delta(c), groups=host_ids, num_groups=3)
    assert not bool(table[1].any())
    for g in (0, 2):                                                            # a group's slice: the ungrouped call on its images
        imgs = [i for i, x in enumerate(host_ids) if x == g]
        one, one_nll = ops.calibration_table(v[imgs].contiguous(), l[imgs].contiguous(), temps, bits)
        assert torch.equal(table[g], one) and torch.allclose(nll[g], one_nll, rtol=1e-12)
    with pytest.raises(ValueError):
        ops.calibration_table(v, l, temps, bits, groups=host_ids, num_groups=3)   # (host ids are checked before a launch)


def test_confidence_one_passes_32_bits(ops):
    """960 pixels of one image, each at confidence 1: the top bin's q sum is 960 2^24, beyond 32 bits"""
    c = 12
    values = torch.full((1, H, W, c), -200.0)
    win = torch.arange(H * W).reshape(1, H, W) % c
    values.scatter_(-1, win[..., None], 0.0)
    labels = torch.where(torch.arange(H * W).reshape(1, H, W) % 2 == 0, win, (win + 1) % c).int()
    for bits in (4, 10):
        table, nll = ops.calibration_table(values.to(DEV), labels.to(DEV), [1.0, 2.5], bits)
        table = table.cpu().numpy()
        for t in range(2):
            assert table[t, -1].tolist() == [960, 480, 960 * Q_ONE] and not table[t, :-1].any()
        assert 960 * Q_ONE > 1 << 32
        assert float(nll[0]) == pytest.approx(480 * -math.log(1e-10), rel=1e-6)   # the wrong half, clipped


# ---- the fused launch against the materialised route --------------------------------------------------------------------

def _scores(c, geo, seed, experts):
    """zero-bordered low-resolution scores [n][hi+2][wi+2][CP] of every expert -- a shared field plus its own noise -- and
    biases, as tests/test_agreement_gpu.py builds them"""
    n, hi, wi = geo
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    shared = torch.randn((n, hi, wi, c), generator=g) * 3.0
    S = [torch.zeros((n, hi + 2, wi + 2, cp)) for _ in range(experts)]
    for t in S:
        t[:, 1:-1, 1:-1, :c] = shared + torch.randn((n, hi, wi, c), generator=g) * 1.5
    bias = [torch.randn(c, generator=g) for _ in range(experts)]
    return [t.to(DEV) for t in S], [b.to(DEV) for b in bias]


def _tables(c, experts, mode, seed):
    if mode == 2:
        return {}
    g = torch.Generator().manual_seed(1000 + seed)
    cond = torch.rand((experts, c, c), generator=g) + 0.05 + 2.0 * torch.eye(c)
    loglik = torch.log(1e-20 + cond / cond.sum(1, keepdim=True))
    prior = torch.exp(torch.randn(c, generator=g))
    logprior = torch.log(prior / prior.sum()).contiguous()
    if mode == 0:
        return dict(tab=loglik.contiguous().to(DEV), logprior=logprior.to(DEV))
    # (small alpha - 1: the fused Dirichlet scores stay a few nats apart, so the confidences spread over the bins)
    am1 = (torch.rand((experts, c, c), generator=g) * 0.3 + 0.5 * torch.eye(c)).contiguous()
    lognorm = torch.randn((experts, c), generator=g)
    return dict(tab=am1.to(DEV), lognorm=lognorm.contiguous().to(DEV), logprior=logprior.to(DEV))


def _materialised(ops, S, bias, geo, c, mode, tables):
    """(fused values, kind, every expert's score map) as the existing route writes them"""
    n, hi, wi = geo
    score, prob, label = [], [], []
    for s, b in zip(S, bias):
        sc = torch.empty((n, 8 * hi, 8 * wi, c), dtype=torch.float32, device=DEV)
        pr, lab = torch.empty_like(sc), torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=DEV)
        ops.decoder_head_from_scores(s, b, n, hi, wi, c, score=sc, prob=pr, label=lab)
        score.append(sc), prob.append(pr), label.append(lab)
    if mode == 0:
        return ops.bayes_fuse(label, tables['tab'], tables['logprior'], want_score=True)[1], 0, score
    if mode == 1:
        return ops.dirichlet_fuse(prob, tables['tab'], tables['lognorm'], tables['logprior'], want_score=True)[1], 0, score
    total = prob[0]
    for p in prob[1:]:
        total = total + p
    return total / torch.tensor(float(len(prob)), device=DEV), 1, score


FUSED_CASES = [(e, m, 12) for e in (2, 3, 4) for m in (0, 1, 2)] + [(3, 1, 13), (2, 0, 32), (4, 2, 5)]


@pytest.mark.parametrize('experts,mode,c', FUSED_CASES, ids=['E%d-%s-C%d' % (e, 'bdm'[m], c) for e, m, c in FUSED_CASES])
def test_fused_launch_against_the_materialised_route(ops, experts, mode, c):
    geo, bits = (N, H // 8, W // 8), 10
    n, hi, wi = geo
    S, bias = _scores(c, geo, 40 + c + experts, experts)
    tables = _tables(c, experts, mode, c + experts)
    values, kind, expert_scores = _materialised(ops, S, bias, geo, c, mode, tables)
    host = values.cpu().numpy()
    labels_h = random_labels(host, 50 + c)
    labels = torch.from_numpy(labels_h).to(DEV)
    pixels = int(((labels_h >= 0) & (labels_h < c)).sum())
    logs = np.log(np.float64(np.float32(1e-20)) + host) if kind == 1 else host
    spread = float((logs.max(-1) - logs.min(-1)).max())
    for temps in ([1.0], [0.5, 1.0, 2.5]):
        want, want_nll = ops.calibration_table(values, labels, temps, bits, kind=kind)
        want_e = [ops.calibration_table(sc, labels, temps, bits) for sc in expert_scores]
        for with_experts in (False, True):
            for bound in (0, 1):
                got = ops.fused_head_multi_calibration(S, bias, n, hi, wi, c, mode, labels, temps, bits, experts=with_experts,
                                                       max_workgroups=bound, **tables)
                assert len(got) == (4 if with_experts else 2)
                pairs = [(got[0], got[1], want, want_nll, 'fused')]
                if with_experts:
                    assert tuple(got[2].shape) == (experts, len(temps), 1 << bits, 3)
                    pairs += [(got[2][e], got[3][e], want_e[e][0], want_e[e][1], 'expert %d' % e) for e in range(experts)]
                for tab, nl, wt, wn, name in pairs:
                    tab, wt = tab.cpu().numpy(), wt.cpu().numpy()
                    assert np.array_equal(tab[..., :2].sum(1), wt[..., :2].sum(1)), name       # the diagonal and the total
                    assert (tab[..., 0].sum(1) == pixels).all()
                    moved = np.abs(tab[..., 0] - wt[..., 0]).sum(1) / 2
                    assert (moved <= LEFT_OUT * pixels).all(), (name, moved)
                    for t, T in enumerate(temps):
                        d = delta(c) + (experts * c + 2) * 2.0 ** -23 * spread / T
                        assert abs(int(tab[t, :, 2].sum()) - int(wt[t, :, 2].sum())) / Q_ONE <= pixels * (d + 2.0 ** -24), name
                        assert abs(float(nl[t]) - float(wn[t])) <= pixels * d * max(1.0, spread / T), name
                    if bound == 0:
                        print('E=%d mode=%d C=%d T=%s %s: pixels that moved bin %s of %d' % (experts, mode, c, temps, name,
                                                                                            moved.tolist(), pixels))


def _guard(shape, dtype):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def test_table_refusals_leave_the_outputs_untouched(ops):
    from modular_semantic_segmentation_amd import _lib
    from modular_semantic_segmentation_amd.ops import _ptr
    c = 12
    values = torch.from_numpy(random_scores(c, 3)).to(DEV)
    labels = torch.zeros((N, H, W), dtype=torch.int32, device=DEV)
    table, nll = _guard((3, 1024, 3), torch.int64), _guard((3,), torch.float64)
    ids = torch.zeros(N, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(0)

    def arr(*t):
        return ctypes.cast((ctypes.c_float * len(t))(*t), ctypes.c_void_p)
    keep = [arr(1.0, 2.0, 0.5), arr(1.0, 0.0), arr(-1.0), arr(float('nan')), arr(float('inf'))]
    good = dict(values=_ptr(values), kind=0, labels=_ptr(labels), group=null, n=N, ppi=H * W, num_classes=c, temperatures=keep[0],
                num_temperatures=3, bin_bits=10, num_groups=1, table=_ptr(table), nll=_ptr(nll), stream=null)
    bad = [dict(bin_bits=3), dict(bin_bits=11), dict(num_temperatures=0), dict(num_temperatures=9), dict(bin_bits=4, num_temperatures=17),
           dict(temperatures=keep[1], num_temperatures=2), dict(temperatures=keep[2], num_temperatures=1),
           dict(temperatures=keep[3], num_temperatures=1), dict(temperatures=keep[4], num_temperatures=1), dict(temperatures=null),
           dict(num_classes=1), dict(num_classes=33), dict(kind=2), dict(kind=-1), dict(n=0), dict(ppi=0), dict(num_groups=0),
           dict(num_groups=2), dict(group=_ptr(ids), num_groups=0), dict(values=null), dict(labels=null), dict(table=null),
           dict(nll=null), dict(values=ctypes.c_void_p(values.data_ptr() + 2)), dict(labels=ctypes.c_void_p(labels.data_ptr() + 2)),
           dict(table=ctypes.c_void_p(table.data_ptr() + 4)), dict(nll=ctypes.c_void_p(nll.data_ptr() + 4)),
           dict(group=ctypes.c_void_p(ids.data_ptr() + 2))]
    for change in bad:
        assert _lib.lib().xv_calibration_table(*dict(good, **change).values()) == -1, change
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all()) and bool((nll == SENTINEL).all())
    for kwargs in (dict(temperatures=[0.0]), dict(temperatures=[]), dict(bin_bits=11), dict(kind=2), dict(num_groups=2)):
        with pytest.raises(ValueError):
            ops.calibration_table(values, labels, **dict(dict(temperatures=[1.0], bin_bits=10), **kwargs))
    with pytest.raises(TypeError):
        ops.calibration_table(values, labels.long(), [1.0], 10)
    with pytest.raises(ValueError):
        ops.calibration_table(values, labels[:, :8].contiguous(), [1.0], 10)


def test_fused_refusals_leave_the_outputs_untouched(ops):
    from modular_semantic_segmentation_amd import _lib
    from modular_semantic_segmentation_amd.ops import _ptr, _ptr_array
    c, experts, geo = 12, 3, (N, H // 8, W // 8)
    n, hi, wi = geo
    S, bias = _scores(c, geo, 3, experts)
    t = _tables(c, experts, 1, 3)
    labels = torch.zeros((N, H, W), dtype=torch.int32, device=DEV)
    table, nll = _guard((2, 1024, 3), torch.int64), _guard((2,), torch.float64)
    etab, enll = _guard((experts, 2, 1024, 3), torch.int64), _guard((experts, 2), torch.float64)
    ids = torch.zeros(n, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(0)
    temps = ctypes.cast((ctypes.c_float * 3)(1.0, 2.0, -1.0), ctypes.c_void_p)
    good = dict(S=_ptr_array(S), bias=_ptr_array(bias), num_experts=experts, n=n, hi=hi, wi=wi, num_classes=c, mode=1,
                tab=_ptr(t['tab']), lognorm=_ptr(t['lognorm']), logprior=_ptr(t['logprior']), labels=_ptr(labels), group=null,
                num_groups=1, temperatures=temps, num_temperatures=2, bin_bits=10, table=_ptr(table), nll=_ptr(nll),
                expert_table=_ptr(etab), expert_nll=_ptr(enll), max_workgroups=0, stream=null)
    bad = [dict(bin_bits=3), dict(bin_bits=11), dict(num_temperatures=0), dict(num_temperatures=3),          # (the third is -1)
           dict(expert_table=null, expert_nll=null, num_temperatures=3), dict(temperatures=null),
           dict(expert_table=null), dict(expert_nll=null),                                                    # one without the other
           dict(num_experts=1), dict(num_experts=5), dict(num_classes=1), dict(num_classes=33), dict(mode=3), dict(mode=-1),
           dict(n=0), dict(hi=0), dict(wi=-1), dict(max_workgroups=-1), dict(num_groups=0), dict(num_groups=2),
           dict(group=_ptr(ids), num_groups=0), dict(tab=null), dict(lognorm=null), dict(logprior=null), dict(labels=null),
           dict(table=null), dict(nll=null), dict(S=None), dict(bias=None), dict(mode=0, tab=null), dict(mode=0, logprior=null),
           dict(tab=ctypes.c_void_p(t['tab'].data_ptr() + 2)), dict(labels=ctypes.c_void_p(labels.data_ptr() + 2)),
           dict(table=ctypes.c_void_p(table.data_ptr() + 4)), dict(nll=ctypes.c_void_p(nll.data_ptr() + 4)),
           dict(expert_table=ctypes.c_void_p(etab.data_ptr() + 4)), dict(expert_nll=ctypes.c_void_p(enll.data_ptr() + 4)),
           dict(group=ctypes.c_void_p(ids.data_ptr() + 2))]
    for e in range(experts):
        for name, tensors, offsets in (('S', S, (None, 4)), ('bias', bias, (None, 2))):
            for off in offsets:
                ptrs = [x.data_ptr() for x in tensors]
                ptrs[e] = 0 if off is None else ptrs[e] + off
                bad.append({name: (ctypes.c_void_p * experts)(*ptrs)})
    # three temperatures with the experts' tables: above the capacity of four tables at ten bin bits (2)
    assert ops.calibration_capacity(10, 1 + experts) == 2
    three = ctypes.cast((ctypes.c_float * 3)(1.0, 2.0, 0.5), ctypes.c_void_p)
    bad.append(dict(temperatures=three, num_temperatures=3))
    for change in bad:
        assert _lib.lib().xv_fused_head_multi_calibration_fwd(*dict(good, **change).values()) == -1, change
    torch.cuda.synchronize()
    for buf in (table, nll, etab, enll):
        assert bool((buf == SENTINEL).all())
    args = (S, bias, n, hi, wi, c)
    with pytest.raises(ValueError):
        ops.fused_head_multi_calibration(*args, 2, labels, tab=t['tab'])
    with pytest.raises(ValueError):
        ops.fused_head_multi_calibration(*args, 1, labels, tab=t['tab'], logprior=t['logprior'])
    with pytest.raises(ValueError):
        ops.fused_head_multi_calibration(*args, 1, labels, [1.0, -2.0], **t)
    with pytest.raises(ValueError):
        ops.fused_head_multi_calibration(S[:1], bias[:1], n, hi, wi, c, 2, labels)
    with pytest.raises(TypeError):
        ops.fused_head_multi_calibration(*args, 1, labels.long(), **t)
