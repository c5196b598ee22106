"""The expert-agreement table (csrc/agreement.hip): xv_fused_head_multi_agreement_fwd / ops.fused_head_multi_agreement from the
experts' low-resolution scores and xv_agreement_table / ops.agreement_table from materialised maps, on small maps.

The oracle is built on the host straight from the definition -- table[label][mask][unanimous][outcome] += 1 with np.add.at --
from maps the existing kernels write on the same GPU: ops.decoder_head_from_scores per expert, ops.fused_head_multi for the
fused labels.  Every comparison is integer equality.

Inputs as tests/test_multi_count_gpu.py::_case with one change: independent scores make the experts agree on 1/C of the pixels
and random labels make "all experts right" vanish, so each expert's interior scores are one shared N(0, 3^2) field plus its own
N(0, sigma^2) noise, and the labels are drawn FROM the experts' maps (40 % a random expert's label, 10 % -1, the rest uniform).
The conditions that make the comparison mean something -- every mask, both unanimous values, outcomes 0 and 1, and outcome 2
under Bayes and Dirichlet -- are asserted on the oracle table of every case (summed over its geometries)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EXPERTS = [2, 3, 4]
MODES = [0, 1, 2]                                      # Bayes, Dirichlet, mean
CLASSES = [2, 5, 12, 13, 32]                           # CM 4, 8 padded, 12 full, 16 padded, 32: the widest table
GEOMETRIES = [(1, 3, 5), (3, 5, 4), (2, 7, 9)]         # under one workgroup; several images; several workgroups, one partial
SCALE = 3.0                                            # of the field the experts share
SIGMA = {2: 3.0, 5: 2.0, 12: 1.5, 13: 1.5, 32: 1.0}    # of each expert's own noise: see _case
SENTINEL = -7


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops
    return ops


def _scores(c, geo, seed, experts, sigma=None):
    """zero-bordered scores [n][hi+2][wi+2][CP] of every expert -- a shared field plus the expert's own noise -- and biases"""
    n, hi, wi = geo
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    shared = torch.randn((n, hi, wi, c), generator=g) * SCALE
    S = [torch.zeros((n, hi + 2, wi + 2, cp)) for _ in range(experts)]
    for t in S:
        t[:, 1:-1, 1:-1, :c] = shared + torch.randn((n, hi, wi, c), generator=g) * (SIGMA[c] if sigma is None else sigma)
    bias = [torch.randn(c, generator=g) for _ in range(experts)]
    return [t.to(DEV) for t in S], [b.to(DEV) for b in bias]


def _tables(c, experts, mode, seed):
    """keyword tables of ops.fused_head_multi for one parameter set, as tests/test_multi_count_gpu.py::_tables builds them
    (priors a few nats apart) with class 0 made a weak claim and class 1 the likeliest a priori, so that unanimous experts are
    overruled on some pixels (outcome 2): Bayes -- an expert saying 0 says little (that row of the conditionals weighs classes
    0 and 1 alike, so the prior decides between them); Dirichlet -- class 0's normaliser is large"""
    if mode == 2:
        return {}
    g = torch.Generator().manual_seed(1000 + seed)
    eye = torch.eye(c)
    eye[0, 0] = 0.0
    cond = torch.rand((experts, c, c), generator=g) + 0.05 + 2.0 * eye
    cond[:, 0, 1] += 2.0                                   # (an expert says 0 as often where the truth is 1)
    loglik = torch.log(1e-20 + cond / cond.sum(1, keepdim=True))
    prior = torch.exp(torch.randn(c, generator=g) * 1.0)
    prior[1] = prior[1] + 3.0 * prior.max()
    logprior = torch.log(prior / prior.sum()).contiguous()
    if mode == 0:
        return dict(tab=loglik.contiguous().to(DEV), logprior=logprior.to(DEV))
    am1 = (torch.rand((experts, c, c), generator=g) * 3.0 - 0.5 + 4.0 * torch.eye(c)).contiguous()
    lognorm = torch.randn((experts, c), generator=g)
    lognorm[:, 0] += 8.0
    return dict(tab=am1.to(DEV), lognorm=lognorm.contiguous().to(DEV), logprior=logprior.to(DEV))


def _expert_maps(ops, S, bias, geo, c):
    n, hi, wi = geo
    maps = []
    for s, b in zip(S, bias):
        lab = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=DEV)
        ops.decoder_head_from_scores(s, b, n, hi, wi, c, label=lab)
        maps.append(lab)
    return maps


def _labels(maps, c, seed):
    """int32 labels drawn from the experts' own maps (host arrays): 40 % a random expert's label, 10 % -1, the rest uniform"""
    rng = np.random.default_rng(seed)
    shape = maps[0].shape
    u = rng.random(shape)
    pick = np.choose(rng.integers(0, len(maps), shape), maps)
    labels = np.where(u < 0.4, pick, np.where(u < 0.5, -1, rng.integers(0, c, shape)))
    return labels.astype(np.int32)


def numpy_table(labels, maps, fused, c, groups=None, num_groups=1):
    """the definition, on host arrays [n, ...]: int64 [num_groups, C, 2^E, 2, 3]"""
    E = len(maps)
    table = np.zeros((num_groups, c, 1 << E, 2, 3), np.int64)
    ids = np.zeros(len(labels), np.int64) if groups is None else np.asarray(groups, np.int64)
    grp = np.broadcast_to(ids.reshape((-1,) + (1,) * (labels.ndim - 1)), labels.shape)
    valid = (labels >= 0) & (labels < c) & (grp >= 0) & (grp < num_groups)
    mask = sum(((m == labels).astype(np.int64) << e) for e, m in enumerate(maps))
    unanimous = np.all([m == maps[0] for m in maps], 0).astype(np.int64)
    hit = np.any([m == fused for m in maps], 0)
    outcome = np.where(fused == labels, 0, np.where(hit, 1, 2))
    np.add.at(table, (grp[valid], labels[valid], mask[valid], unanimous[valid], outcome[valid]), 1)
    return table


_CACHE = {}


def case(ops, c, geo, experts, mode, seed, sigma=None):
    """one input and its oracle, computed once and shared: dict of S, bias, tables, labels (device int32), maps (device int64
    per expert), fused (device int64), want (host int64 [C, 2^E, 2, 3])"""
    key = (c, geo, experts, mode, seed, sigma)
    if key not in _CACHE:
        n, hi, wi = geo
        S, bias = _scores(c, geo, seed, experts, sigma)
        tables = _tables(c, experts, mode, c + experts)
        maps = _expert_maps(ops, S, bias, geo, c)
        fused = ops.fused_head_multi(S, bias, n, hi, wi, c, mode, **tables)
        host = [m.cpu().numpy() for m in maps]
        labels = _labels(host, c, seed + 1)
        want = numpy_table(labels, host, fused.cpu().numpy(), c)[0]
        _CACHE[key] = dict(S=S, bias=bias, tables=tables, labels=torch.from_numpy(labels).to(DEV), maps=maps, fused=fused,
                           want=want)
    return _CACHE[key]


def input_conditions(table, mode):
    """what the oracle table of a case has to show for the comparison to mean something: {condition: holds}"""
    masks, unanimous, outcomes = table.sum((0, 2, 3)), table.sum((0, 1, 3)), table.sum((0, 1, 2))
    return {'every mask occurs': bool((masks > 0).all()), 'both unanimous values occur': bool((unanimous > 0).all()),
            'outcomes 0 and 1 occur': bool((outcomes[:2] > 0).all()), 'outcome 2 occurs': mode == 2 or bool(outcomes[2] > 0)}


def _guarded(shape):
    """a zeroed table between two sentinel rows: (whole buffer, the table)"""
    buf = torch.full((3,) + tuple(shape), SENTINEL, dtype=torch.int64, device=DEV)
    buf[1] = 0
    return buf, buf[1]


def _count_tables(tables, mode):
    """the tables of ops.fused_head_multi_count for the one parameter set of `tables`"""
    if mode == 2:
        return {}
    out = {k: v[None].contiguous() for k, v in tables.items()}
    if mode == 0:
        out['tab'] = tables['tab']
    return out


@pytest.mark.parametrize('c', CLASSES)
@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
@pytest.mark.parametrize('experts', EXPERTS)
def test_both_routes_equal_the_oracle(ops, experts, mode, c):
    total = np.zeros((c, 1 << experts, 2, 3), np.int64)
    for gi, geo in enumerate(GEOMETRIES):
        n, hi, wi = geo
        k = case(ops, c, geo, experts, mode, 7 * c + gi)
        want = torch.from_numpy(k['want']).to(DEV)
        total += k['want']
        assert int(k['want'].sum()) == int(((k['labels'] >= 0) & (k['labels'] < c)).sum())
        # the fused kernel
        buf, table = _guarded(want.shape)
        ops.fused_head_multi_agreement(k['S'], k['bias'], n, hi, wi, c, mode, k['labels'], table=table, **k['tables'])
        assert torch.equal(table, want), geo
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[2] == SENTINEL).all())
        # the same table from the materialised maps
        buf, table = _guarded(want.shape)
        ops.agreement_table(k['labels'], k['maps'], k['fused'], c, table=table)
        assert torch.equal(table, want), geo
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[2] == SENTINEL).all())
        # margins: what the counting head counts on the same inputs
        expert_cm = torch.zeros((experts, c, c), dtype=torch.int64, device=DEV)
        cm = ops.fused_head_multi_count(k['S'], k['bias'], n, hi, wi, c, mode, k['labels'], expert_cm=expert_cm,
                                        **_count_tables(k['tables'], mode))[0].cpu().numpy()
        expert_cm = expert_cm.cpu().numpy()
        assert np.array_equal(k['want'].sum((1, 2, 3)), cm.sum(1))
        assert np.array_equal(k['want'][..., 0].sum((1, 2)), np.diag(cm))
        for e in range(experts):
            with_e = [m for m in range(1 << experts) if (m >> e) & 1]
            assert np.array_equal(k['want'][:, with_e].sum((1, 2, 3)), np.diag(expert_cm[e])), e
    # the input conditions, so that a degenerate input fails loudly
    for name, holds in input_conditions(total, mode).items():
        assert holds, (name, total.sum((0, 2, 3)), total.sum((0, 1, 3)), total.sum((0, 1, 2)))
    # cells that cannot occur
    full = (1 << experts) - 1
    assert int(total[:, 1:full, 1].sum()) == 0 and int(total[:, full, 0].sum()) == 0


@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
def test_bounded_grids_and_accumulation(ops, mode):
    c, experts, geo = 5, 3, (2, 7, 9)
    k = case(ops, c, geo, experts, mode, 11)
    args = (k['S'], k['bias']) + geo + (c, mode, k['labels'])
    want = torch.from_numpy(k['want']).to(DEV)
    for bound in (1, 2, 7):
        assert torch.equal(ops.fused_head_multi_agreement(*args, max_workgroups=bound, **k['tables']), want), bound
    again = ops.fused_head_multi_agreement(*args, table=want.clone(), **k['tables'])
    assert torch.equal(again, 2 * want)
    again = ops.agreement_table(k['labels'], k['maps'], k['fused'], c, table=want.clone())
    assert torch.equal(again, 2 * want)


@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
def test_groups(ops, mode):
    c, experts, geo = 12, 3, (5, 3, 5)
    n, hi, wi = geo
    host_ids = [2, 0, 7, -1, 1]                                               # 7 and -1: counted nowhere
    ids = torch.tensor(host_ids, dtype=torch.int32, device=DEV)
    k = case(ops, c, geo, experts, mode, 13)
    want = numpy_table(k['labels'].cpu().numpy(), [m.cpu().numpy() for m in k['maps']], k['fused'].cpu().numpy(), c,
                       groups=host_ids, num_groups=3)
    fused = ops.fused_head_multi_agreement(k['S'], k['bias'], n, hi, wi, c, mode, k['labels'], groups=ids, num_groups=3,
                                           **k['tables'])
    mat = ops.agreement_table(k['labels'], k['maps'], k['fused'], c, groups=ids, num_groups=3)
    assert tuple(fused.shape) == (3, c, 8, 2, 3)
    assert np.array_equal(fused.cpu().numpy(), want) and np.array_equal(mat.cpu().numpy(), want)
    for g in range(3):                                                        # a group's slice: the ungrouped call on its images
        imgs = [i for i, v in enumerate(host_ids) if v == g]
        one = ops.fused_head_multi_agreement([s[imgs].contiguous() for s in k['S']], k['bias'], len(imgs), hi, wi, c, mode,
                                             k['labels'][imgs].contiguous(), **k['tables'])
        assert torch.equal(fused[g], one), g
        one = ops.agreement_table(k['labels'][imgs].contiguous(), [m[imgs].contiguous() for m in k['maps']],
                                  k['fused'][imgs].contiguous(), c)
        assert torch.equal(mat[g], one), g
    inrange = [i for i, v in enumerate(host_ids) if 0 <= v < 3]
    counted = int(((k['labels'][inrange] >= 0) & (k['labels'][inrange] < c)).sum())
    assert int(fused.sum()) == counted < int((k['labels'] >= 0).sum())        # the other two images are missing


def test_fused_refusals_leave_the_table_untouched(ops):
    from modular_semantic_segmentation_amd import _lib
    from modular_semantic_segmentation_amd.ops import _ptr, _ptr_array
    c, experts, geo = 12, 3, (1, 3, 5)
    n, hi, wi = geo
    k = case(ops, c, geo, experts, 1, 19)
    S, bias, t, labels = k['S'], k['bias'], k['tables'], k['labels']
    table = torch.full((c, 8, 2, 3), SENTINEL, dtype=torch.int64, device=DEV)
    ids = torch.zeros(n, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(0)
    good = dict(S=_ptr_array(S), bias=_ptr_array(bias), num_experts=experts, n=n, hi=hi, wi=wi, num_classes=c, mode=1,
                tab=_ptr(t['tab']), lognorm=_ptr(t['lognorm']), logprior=_ptr(t['logprior']), labels=_ptr(labels), group=null,
                num_groups=1, table=_ptr(table), max_workgroups=0, stream=null)
    bad = [dict(num_experts=1), dict(num_experts=5), dict(num_classes=1), dict(num_classes=33), dict(mode=3), dict(mode=-1),
           dict(n=0), dict(hi=0), dict(wi=-1), dict(max_workgroups=-1), dict(num_groups=0), dict(num_groups=2),
           dict(group=_ptr(ids), num_groups=0), dict(tab=null), dict(lognorm=null), dict(logprior=null), dict(labels=null),
           dict(table=null), dict(S=None), dict(bias=None), dict(mode=0, tab=null), dict(mode=0, logprior=null),
           dict(tab=ctypes.c_void_p(t['tab'].data_ptr() + 2)), dict(lognorm=ctypes.c_void_p(t['lognorm'].data_ptr() + 2)),
           dict(logprior=ctypes.c_void_p(t['logprior'].data_ptr() + 2)), dict(labels=ctypes.c_void_p(labels.data_ptr() + 2)),
           dict(table=ctypes.c_void_p(table.data_ptr() + 4)), dict(group=ctypes.c_void_p(ids.data_ptr() + 2))]
    # an entry of the host pointer arrays: null, or not aligned to its loads (16 bytes for scores, 4 for biases)
    for e in range(experts):
        for name, tensors, offsets in (('S', S, (None, 4)), ('bias', bias, (None, 2))):
            for off in offsets:
                ptrs = [x.data_ptr() for x in tensors]
                ptrs[e] = 0 if off is None else ptrs[e] + off
                bad.append({name: (ctypes.c_void_p * experts)(*ptrs)})
    for change in bad:
        rc = _lib.lib().xv_fused_head_multi_agreement_fwd(*dict(good, **change).values())
        assert rc == -1, change
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all())
    args = (S, bias, n, hi, wi, c)
    with pytest.raises(ValueError):
        ops.fused_head_multi_agreement(*args, 2, labels, tab=t['tab'])
    with pytest.raises(ValueError):
        ops.fused_head_multi_agreement(*args, 1, labels, tab=t['tab'], logprior=t['logprior'])
    with pytest.raises(ValueError):
        ops.fused_head_multi_agreement(*args, 1, labels, num_groups=2, **t)
    with pytest.raises(TypeError):
        ops.fused_head_multi_agreement(*args, 1, labels.long(), **t)
    with pytest.raises(ValueError):
        ops.fused_head_multi_agreement(*args, 1, labels, table=torch.zeros((c, 4, 2, 3), dtype=torch.int64, device=DEV), **t)
    with pytest.raises(ValueError):
        ops.fused_head_multi_agreement(S[:1], bias[:1], n, hi, wi, c, 2, labels)
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all())


def test_materialised_refusals_leave_the_table_untouched(ops):
    from modular_semantic_segmentation_amd import _lib
    from modular_semantic_segmentation_amd.ops import _ptr, _ptr_array
    c, experts, geo = 12, 3, (1, 3, 5)
    k = case(ops, c, geo, experts, 1, 19)
    labels, maps, fused = k['labels'], k['maps'], k['fused']
    n, ppi = labels.shape[0], labels.numel() // labels.shape[0]
    table = torch.full((c, 8, 2, 3), SENTINEL, dtype=torch.int64, device=DEV)
    ids = torch.zeros(n, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(0)
    good = dict(labels=_ptr(labels), expert_labels=_ptr_array(maps), num_experts=experts, fused=_ptr(fused), group=null, n=n,
                ppi=ppi, num_classes=c, num_groups=1, table=_ptr(table), stream=null)
    bad = [dict(num_experts=1), dict(num_experts=5), dict(num_classes=1), dict(num_classes=33), dict(n=0), dict(ppi=0),
           dict(ppi=-4), dict(num_groups=0), dict(num_groups=2), dict(group=_ptr(ids), num_groups=0), dict(labels=null),
           dict(expert_labels=None), dict(fused=null), dict(table=null),
           dict(labels=ctypes.c_void_p(labels.data_ptr() + 2)), dict(fused=ctypes.c_void_p(fused.data_ptr() + 4)),
           dict(table=ctypes.c_void_p(table.data_ptr() + 4)), dict(group=ctypes.c_void_p(ids.data_ptr() + 2))]
    for e in range(experts):
        for off in (None, 4):
            ptrs = [m.data_ptr() for m in maps]
            ptrs[e] = 0 if off is None else ptrs[e] + off
            bad.append(dict(expert_labels=(ctypes.c_void_p * experts)(*ptrs)))
    for change in bad:
        rc = _lib.lib().xv_agreement_table(*dict(good, **change).values())
        assert rc == -1, change
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all())
    with pytest.raises(TypeError):
        ops.agreement_table(labels.long(), maps, fused, c)
    with pytest.raises(TypeError):
        ops.agreement_table(labels, [m.int() for m in maps], fused, c)
    with pytest.raises(ValueError):
        ops.agreement_table(labels, maps[:1], fused, c)
    with pytest.raises(ValueError):
        ops.agreement_table(labels, maps, fused[:, :8].contiguous(), c)
    with pytest.raises(ValueError):
        ops.agreement_table(labels, maps, fused, c, num_groups=3)
