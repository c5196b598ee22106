"""The label-tuple heads (csrc/tuple_lut.hip): ops.fused_head_multi_tuple_hist, ops.fused_head_multi_lut and
ops.fused_head_multi_lut_count from the experts' low-resolution scores, on small maps.

The oracle is built on the host from maps that existing kernels write on the same GPU, as tests/test_agreement_gpu.py does:
ops.decoder_head_from_scores per expert for the labels, the tuple index t = ((l_0 C + l_1) C + ...) from them, np.bincount
of it for the histogram, lut[t] for the fused labels and np.add.at for the confusion matrices.  Every comparison is integer
equality.

Scores as that file's _scores: one shared field plus every expert's own noise, so that the experts neither always agree nor
never agree; the oracle of every case is asserted to hit unanimous tuples, non-unanimous tuples and at least min(T, 50)
distinct tuples, summed over its geometries.  The lookup table is random uint8 in [0, C) from a seeded generator: a wrong
index cannot hide behind a diagonal table.  Labels include -1."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EXPERTS = [2, 3, 4]
CLASSES = [2, 5, 12, 13, 32]                           # CM 4, 8 padded, 12 full, 16 padded, 32
MAX_TUPLES = 160 * 1024 // 4                           # u32 counters in one workgroup's LDS: what xv_tuple_capacity serves
CASES = [(e, c) for e in EXPERTS for c in CLASSES if c ** e <= MAX_TUPLES]
GEOMETRIES = [(1, 3, 5), (3, 5, 4), (2, 7, 9)]         # under one workgroup; several images; several workgroups, one partial
SCALE = 3.0                                            # of the field the experts share
SIGMA = {2: 3.0, 5: 2.0, 12: 1.5, 13: 1.5, 14: 1.5, 32: 1.0}    # of each expert's own noise
SENTINEL = -7


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops
    return ops


def _scores(c, geo, seed, experts):
    """zero-bordered scores [n][hi+2][wi+2][CP] of every expert -- a shared field plus the expert's own noise -- and biases"""
    n, hi, wi = geo
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    shared = torch.randn((n, hi, wi, c), generator=g) * SCALE
    S = [torch.zeros((n, hi + 2, wi + 2, cp)) for _ in range(experts)]
    for t in S:
        t[:, 1:-1, 1:-1, :c] = shared + torch.randn((n, hi, wi, c), generator=g) * SIGMA[c]
    bias = [torch.randn(c, generator=g) for _ in range(experts)]
    return [t.to(DEV) for t in S], [b.to(DEV) for b in bias]


def numpy_hist(t, num_tuples, groups=None, num_groups=1):
    """int64 [num_groups, T] from the tuple indices t [n, H, W] on the host"""
    ids = np.zeros(len(t), np.int64) if groups is None else np.asarray(groups, np.int64)
    hist = np.zeros((num_groups, num_tuples), np.int64)
    for i, g in enumerate(ids):
        if 0 <= g < num_groups:
            hist[g] += np.bincount(t[i].reshape(-1), minlength=num_tuples)
    return hist


def numpy_cm(labels, fused, c, groups=None, num_groups=1):
    """int64 [num_groups, C, C] (rows = ground truth) from host maps [n, H, W]"""
    ids = np.zeros(len(labels), np.int64) if groups is None else np.asarray(groups, np.int64)
    grp = np.broadcast_to(ids.reshape(-1, 1, 1), labels.shape)
    valid = (labels >= 0) & (labels < c) & (grp >= 0) & (grp < num_groups)
    cm = np.zeros((num_groups, c, c), np.int64)
    np.add.at(cm, (grp[valid], labels[valid], fused[valid]), 1)
    return cm


_CACHE = {}


def case(ops, c, geo, experts, seed):
    """one input and its oracle, computed once and shared (never written to): S, bias, lut (device uint8 [T]), labels (device
    int32), and on the host maps (int64 per expert), t, fused, hist [T], cm [C, C]"""
    key = (c, geo, experts, seed)
    if key not in _CACHE:
        n, hi, wi = geo
        S, bias = _scores(c, geo, seed, experts)
        maps = []
        for s, b in zip(S, bias):
            lab = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=DEV)
            ops.decoder_head_from_scores(s, b, n, hi, wi, c, label=lab)
            maps.append(lab.cpu().numpy())
        t = np.zeros_like(maps[0])
        for m in maps:
            t = t * c + m
        rng = np.random.default_rng(1000 + seed)
        lut = rng.integers(0, c, c ** experts).astype(np.uint8)
        u = rng.random(t.shape)
        labels = np.where(u < 0.1, -1, np.where(u < 0.5, maps[0], rng.integers(0, c, t.shape))).astype(np.int32)
        fused = lut[t].astype(np.int64)
        _CACHE[key] = dict(S=S, bias=bias, lut=torch.from_numpy(lut).to(DEV), labels=torch.from_numpy(labels).to(DEV),
                           host_labels=labels, maps=maps, t=t, fused=fused, hist=numpy_hist(t, c ** experts)[0],
                           cm=numpy_cm(labels, fused, c)[0])
    return _CACHE[key]


def _guarded(shape):
    """a zeroed tensor between two sentinel rows: (whole buffer, the tensor)"""
    buf = torch.full((3,) + tuple(shape), SENTINEL, dtype=torch.int64, device=DEV)
    buf[1] = 0
    return buf, buf[1]


def _clean(buf):
    return bool((buf[0] == SENTINEL).all()) and bool((buf[2] == SENTINEL).all())


def test_capacity_query(ops):
    for c, e in ((12, 4), (13, 3), (32, 2)):
        assert ops.tuple_capacity(c, e), (c, e)
    for e in range(0, 7):
        for c in range(0, 35):
            served = 2 <= e <= 4 and 2 <= c <= 32 and c ** e <= MAX_TUPLES
            assert ops.tuple_capacity(c, e) == served, (c, e)
    # every pair below the three the feature is built for
    assert all(ops.tuple_capacity(c, 4) for c in range(2, 13)) and all(ops.tuple_capacity(c, 3) for c in range(2, 14))
    assert all(ops.tuple_capacity(c, 2) for c in range(2, 33))
    assert (4, 12) in CASES and (3, 13) in CASES and (2, 32) in CASES and (4, 32) not in CASES


@pytest.mark.parametrize('experts,c', CASES)
def test_the_three_heads_equal_the_oracle(ops, experts, c):
    T = c ** experts
    total = np.zeros(T, np.int64)
    for gi, geo in enumerate(GEOMETRIES):
        n, hi, wi = geo
        k = case(ops, c, geo, experts, 7 * c + gi)
        total += k['hist']
        assert int(k['hist'].sum()) == n * hi * wi * 64           # every output pixel, whatever its label
        buf, hist = _guarded((T,))
        ops.fused_head_multi_tuple_hist(k['S'], k['bias'], n, hi, wi, c, hist=hist)
        assert np.array_equal(hist.cpu().numpy(), k['hist']), geo
        assert _clean(buf)
        buf, out = _guarded((n, 8 * hi, 8 * wi))
        out.fill_(SENTINEL)
        ops.fused_head_multi_lut(k['S'], k['bias'], n, hi, wi, c, k['lut'], out=out)
        assert np.array_equal(out.cpu().numpy(), k['fused']), geo
        assert _clean(buf)
        buf, cm = _guarded((c, c))
        ops.fused_head_multi_lut_count(k['S'], k['bias'], n, hi, wi, c, k['lut'], k['labels'], cm=cm)
        assert np.array_equal(cm.cpu().numpy(), k['cm']), geo
        assert _clean(buf)
        assert int(k['cm'].sum()) == int((k['host_labels'] >= 0).sum()) < k['host_labels'].size
    # the input conditions, so that a degenerate input fails loudly
    digits = np.stack(np.unravel_index(np.arange(T), (c,) * experts))
    unanimous = np.all(digits == digits[0], 0)
    assert int(total[unanimous].sum()) > 0 and int(total[~unanimous].sum()) > 0
    assert int((total > 0).sum()) >= min(T, 50), int((total > 0).sum())


def test_the_largest_pair_the_capacity_query_serves(ops):
    """Four experts at 14 classes: 38 416 tuples, 150 KB of counters, the last pair under the 160 KB the query promises (15
    classes are refused).  The histogram takes almost a whole CU's LDS there; the table of the lookup heads is 38 KB."""
    experts, c = 4, 14
    T = c ** experts
    assert 4 * T <= 160 * 1024 < 4 * 15 ** experts and ops.tuple_capacity(c, experts) and not ops.tuple_capacity(15, experts)
    for gi, geo in enumerate(GEOMETRIES[1:]):
        n, hi, wi = geo
        k = case(ops, c, geo, experts, 300 + gi)
        assert int((k['hist'] > 0).sum()) >= 50 and int(k['t'].max()) > T // 2       # tuples far up the table are hit
        buf, hist = _guarded((T,))
        ops.fused_head_multi_tuple_hist(k['S'], k['bias'], n, hi, wi, c, hist=hist)
        assert np.array_equal(hist.cpu().numpy(), k['hist']) and _clean(buf), geo
        out = ops.fused_head_multi_lut(k['S'], k['bias'], n, hi, wi, c, k['lut'])
        assert np.array_equal(out.cpu().numpy(), k['fused']), geo
        buf, cm = _guarded((c, c))
        ops.fused_head_multi_lut_count(k['S'], k['bias'], n, hi, wi, c, k['lut'], k['labels'], cm=cm, max_workgroups=3)
        assert np.array_equal(cm.cpu().numpy(), k['cm']) and _clean(buf), geo


@pytest.mark.parametrize('experts,c', [(2, 12), (3, 5), (4, 12), (2, 32), (4, 13)])
def test_bounded_grids_and_accumulation(ops, experts, c):
    geo = (2, 7, 9)
    k = case(ops, c, geo, experts, 11)
    args = (k['S'], k['bias']) + geo + (c,)
    want_hist, want_cm = torch.from_numpy(k['hist']).to(DEV), torch.from_numpy(k['cm']).to(DEV)
    for bound in (1, 3):
        assert torch.equal(ops.fused_head_multi_tuple_hist(*args, max_workgroups=bound), want_hist), bound
        assert torch.equal(ops.fused_head_multi_lut_count(*args, k['lut'], k['labels'], max_workgroups=bound), want_cm), bound
    assert torch.equal(ops.fused_head_multi_tuple_hist(*args, hist=want_hist.clone()), 2 * want_hist)
    assert torch.equal(ops.fused_head_multi_lut_count(*args, k['lut'], k['labels'], cm=want_cm.clone()), 2 * want_cm)


@pytest.mark.parametrize('experts,c', [(2, 12), (3, 13), (4, 5)])
def test_groups(ops, experts, c):
    geo = (5, 3, 5)
    n, hi, wi = geo
    T = c ** experts
    host_ids = [2, 0, 7, -1, 2]                                               # 7 and -1: counted nowhere
    ids = torch.tensor(host_ids, dtype=torch.int32, device=DEV)
    k = case(ops, c, geo, experts, 13)
    hist = ops.fused_head_multi_tuple_hist(k['S'], k['bias'], n, hi, wi, c, groups=ids, num_groups=3)
    cm = ops.fused_head_multi_lut_count(k['S'], k['bias'], n, hi, wi, c, k['lut'], k['labels'], groups=ids, num_groups=3)
    assert tuple(hist.shape) == (3, T) and tuple(cm.shape) == (3, c, c)
    assert np.array_equal(hist.cpu().numpy(), numpy_hist(k['t'], T, host_ids, 3))
    assert np.array_equal(cm.cpu().numpy(), numpy_cm(k['host_labels'], k['fused'], c, host_ids, 3))
    for g in range(3):                                                        # a group's slice: the ungrouped call on its images
        imgs = [i for i, v in enumerate(host_ids) if v == g]
        if not imgs:
            assert int(hist[g].sum()) == 0 and int(cm[g].sum()) == 0
            continue
        S = [s[imgs].contiguous() for s in k['S']]
        assert torch.equal(hist[g], ops.fused_head_multi_tuple_hist(S, k['bias'], len(imgs), hi, wi, c)), g
        assert torch.equal(cm[g], ops.fused_head_multi_lut_count(S, k['bias'], len(imgs), hi, wi, c, k['lut'],
                                                                 k['labels'][imgs].contiguous())), g
    assert int(hist.sum()) == 3 * hi * wi * 64                                # the other two images are missing
    with pytest.raises(ValueError):                                           # ids from the host are checked before any launch
        ops.fused_head_multi_tuple_hist(k['S'], k['bias'], n, hi, wi, c, groups=host_ids, num_groups=3)


def test_refusals_leave_the_outputs_untouched(ops):
    from modular_semantic_segmentation_amd import _lib
    from modular_semantic_segmentation_amd.ops import _ptr, _ptr_array
    c, experts, geo = 12, 3, (1, 3, 5)
    n, hi, wi = geo
    k = case(ops, c, geo, experts, 19)
    S, bias, lut, labels = k['S'], k['bias'], k['lut'], k['labels']
    hist = torch.full((c ** experts,), SENTINEL, dtype=torch.int64, device=DEV)
    cm = torch.full((c, c), SENTINEL, dtype=torch.int64, device=DEV)
    out = torch.full((n, 8 * hi, 8 * wi), SENTINEL, dtype=torch.int64, device=DEV)
    ids = torch.zeros(n, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(0)
    lib = _lib.lib()
    experts_args = dict(S=_ptr_array(S), bias=_ptr_array(bias), num_experts=experts, n=n, hi=hi, wi=wi, num_classes=c)
    bad_experts = [dict(num_experts=1), dict(num_experts=5), dict(num_classes=1), dict(num_classes=33), dict(n=0), dict(hi=0),
                   dict(wi=-1), dict(S=None), dict(bias=None)]
    for e in range(experts):                # an entry of the host pointer arrays: null, or not aligned to its loads
        for name, tensors, offsets in (('S', S, (None, 4)), ('bias', bias, (None, 2))):
            for off in offsets:
                ptrs = [x.data_ptr() for x in tensors]
                ptrs[e] = 0 if off is None else ptrs[e] + off
                bad_experts.append({name: (ctypes.c_void_p * experts)(*ptrs)})
    bad_groups = [dict(max_workgroups=-1), dict(num_groups=0), dict(num_groups=2), dict(group=_ptr(ids), num_groups=0),
                  dict(group=ctypes.c_void_p(ids.data_ptr() + 2))]
    entries = [
        (lib.xv_fused_head_multi_tuple_hist_fwd,
         dict(experts_args, group=null, num_groups=1, hist=_ptr(hist), max_workgroups=0, stream=null),
         bad_groups + [dict(hist=null), dict(hist=ctypes.c_void_p(hist.data_ptr() + 4))]),
        (lib.xv_fused_head_multi_lut_fwd, dict(experts_args, lut=_ptr(lut), fused_label=_ptr(out), stream=null),
         [dict(lut=null), dict(fused_label=null), dict(lut=ctypes.c_void_p(lut.data_ptr() + 1)),
          dict(fused_label=ctypes.c_void_p(out.data_ptr() + 8))]),
        (lib.xv_fused_head_multi_lut_count_fwd,
         dict(experts_args, lut=_ptr(lut), labels=_ptr(labels), group=null, num_groups=1, cm=_ptr(cm), max_workgroups=0,
              stream=null),
         bad_groups + [dict(lut=null), dict(labels=null), dict(cm=null), dict(lut=ctypes.c_void_p(lut.data_ptr() + 1)),
                       dict(labels=ctypes.c_void_p(labels.data_ptr() + 2)), dict(cm=ctypes.c_void_p(cm.data_ptr() + 4))]),
    ]
    for fn, good, bad in entries:
        for change in bad_experts + bad:
            assert fn(*dict(good, **change).values()) == -1, (fn.__name__, change)           # XV_EINVAL
        # pairs whose counters do not fit one workgroup's LDS: XV_ESHAPE (the pointers are not read before the refusal)
        for change in (dict(num_experts=4, num_classes=15), dict(num_experts=4, num_classes=32)):
            four = dict(S=_ptr_array(S + S[:1]), bias=_ptr_array(bias + bias[:1]))
            assert fn(*dict(good, **four, **change).values()) == ops.XV_ESHAPE, (fn.__name__, change)
    torch.cuda.synchronize()
    for t in (hist, cm, out):
        assert bool((t == SENTINEL).all())
    args = (S, bias, n, hi, wi, c)
    with pytest.raises(ValueError):
        ops.fused_head_multi_tuple_hist(S[:1], bias[:1], n, hi, wi, c)
    with pytest.raises(ValueError):
        ops.fused_head_multi_tuple_hist(*args, num_groups=2)
    with pytest.raises(ValueError):
        ops.fused_head_multi_tuple_hist(*args, hist=torch.zeros(c ** 2, dtype=torch.int64, device=DEV))
    with pytest.raises(TypeError):
        ops.fused_head_multi_lut(*args, lut.long())
    with pytest.raises(ValueError):
        ops.fused_head_multi_lut(*args, lut[:c * c].contiguous())
    with pytest.raises(TypeError):
        ops.fused_head_multi_lut_count(*args, lut, labels.long())
    with pytest.raises(ValueError):
        ops.fused_head_multi_lut_count(*args, lut, labels, cm=torch.zeros((c, c + 1), dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    for t in (hist, cm, out):
        assert bool((t == SENTINEL).all())
