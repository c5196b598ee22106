"""The counting head for two to four experts (xv_fused_head_multi_count_fwd / ops.fused_head_multi_count) on small maps.

The oracle is the map-writing route on the same GPU: ops.fused_head_multi with one point's tables, counted by
ops.confusion_matrix; an expert's own matrix is that of ops.decoder_head_from_scores' label map.  Every comparison is integer
equality.  Inputs as tests/test_multi_head_gpu.py: N(0, 3^2) low-resolution scores, random tables, labels from [-1, C)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EXPERTS = [2, 3, 4]
MODES = [0, 1, 2]                                      # Bayes, Dirichlet, mean
CLASSES = [2, 5, 12, 13, 32]                           # CM 4, 8 padded, 12 full, 16 padded, 32 (capacity 1 with four experts)
GEOMETRIES = [(1, 3, 5), (3, 5, 4), (2, 7, 9)]         # under one workgroup; several images; several workgroups, one partial
SIGMAS = [0.2, 1.0, 5.0]                               # the points of a Dirichlet grid scale alpha - 1 by 1 / sigma
SCALE = 3.0
SENTINEL = -7


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops
    return ops


def _case(c, geo, seed, experts):
    """zero-bordered scores [n][hi+2][wi+2][CP] of every expert, their biases, labels in [-1, C)"""
    n, hi, wi = geo
    g = torch.Generator().manual_seed(seed)
    cp = (c + 3) // 4 * 4
    S = [torch.zeros((n, hi + 2, wi + 2, cp)) for _ in range(experts)]
    for t in S:
        t[:, 1:-1, 1:-1, :c] = torch.randn((n, hi, wi, c), generator=g) * SCALE
    bias = [torch.randn(c, generator=g) for _ in range(experts)]
    labels = torch.randint(-1, c, (n, 8 * hi, 8 * wi), generator=g, dtype=torch.int32)
    return [t.to(DEV) for t in S], [b.to(DEV) for b in bias], labels.to(DEV)


def _tables(c, experts, points, mode, seed):
    """keyword tables of ops.fused_head_multi_count for `points` parameter sets; priors a few nats apart"""
    if mode == 2:
        return {}
    g = torch.Generator().manual_seed(1000 + seed)
    cond = torch.rand((experts, c, c), generator=g) + 0.05 + 2.0 * torch.eye(c)
    loglik = torch.log(1e-20 + cond / cond.sum(1, keepdim=True))
    prior = torch.exp(torch.randn((points, c), generator=g) * 1.0)
    logprior = torch.log(prior / prior.sum(1, keepdim=True)).contiguous()
    if mode == 0:
        return dict(tab=loglik.contiguous().to(DEV), logprior=logprior.to(DEV))
    am1 = torch.rand((experts, c, c), generator=g) * 3.0 - 0.5 + 4.0 * torch.eye(c)
    am1 = torch.stack([am1 / SIGMAS[p % 3] for p in range(points)]).contiguous()
    lognorm = torch.randn((points, experts, c), generator=g).contiguous()
    return dict(tab=am1.to(DEV), lognorm=lognorm.to(DEV), logprior=logprior.to(DEV))


def _point(tables, mode, p):
    """the tables ops.fused_head_multi takes for point p"""
    if mode == 0:
        return dict(tab=tables['tab'], logprior=tables['logprior'][p].contiguous())
    if mode == 1:
        return dict(tab=tables['tab'][p].contiguous(), lognorm=tables['lognorm'][p].contiguous(),
                    logprior=tables['logprior'][p].contiguous())
    return {}


def _oracle(ops, S, bias, geo, c, mode, tables, labels, points):
    n, hi, wi = geo
    cm = torch.zeros((points, c, c), dtype=torch.int64, device=DEV)
    for p in range(points):
        fused = ops.fused_head_multi(S, bias, n, hi, wi, c, mode, **_point(tables, mode, p))
        ops.confusion_matrix(labels, fused, cm[p])
    return cm


def _expert_oracle(ops, S, bias, geo, c, labels):
    n, hi, wi = geo
    cm = torch.zeros((len(S), c, c), dtype=torch.int64, device=DEV)
    for e, (s, b) in enumerate(zip(S, bias)):
        lab = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=DEV)
        ops.decoder_head_from_scores(s, b, n, hi, wi, c, label=lab)
        ops.confusion_matrix(labels, lab, cm[e])
    return cm


@pytest.mark.parametrize('c', CLASSES)
@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
@pytest.mark.parametrize('experts', EXPERTS)
def test_counts_equal_the_map_writing_route(ops, experts, mode, c):
    for gi, geo in enumerate(GEOMETRIES):
        n, hi, wi = geo
        S, bias, labels = _case(c, geo, 7 * c + gi, experts)
        want_experts = _expert_oracle(ops, S, bias, geo, c, labels)
        for points in ([1] if mode == 2 else [1, 3]):
            tables = _tables(c, experts, points, mode, c + experts)
            want = _oracle(ops, S, bias, geo, c, mode, tables, labels, points)
            # input conditions: the fused labels take at least two values; with three points two matrices differ
            assert all(int((want[p].sum(0) > 0).sum()) >= 2 for p in range(points))
            if points == 3:
                assert not (torch.equal(want[0], want[1]) and torch.equal(want[1], want[2]))
            buf = torch.full((points + 2, c, c), SENTINEL, dtype=torch.int64, device=DEV)
            buf[1:-1] = 0
            expert_cm = torch.zeros((experts, c, c), dtype=torch.int64, device=DEV)
            ops.fused_head_multi_count(S, bias, n, hi, wi, c, mode, labels, cm=buf[1:-1], expert_cm=expert_cm, **tables)
            assert torch.equal(buf[1:-1], want), (geo, points)
            assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
            assert torch.equal(expert_cm, want_experts), (geo, points)


def test_more_points_than_the_capacity(ops):
    c, experts, geo = 12, 4, (2, 7, 9)
    cap = ops.fused_head_multi_count_capacity(c, experts, 'dirichlet')
    assert cap >= 8
    points = cap + 3
    S, bias, labels = _case(c, geo, 5, experts)
    tables = _tables(c, experts, points, 1, 3)
    expert_cm = torch.zeros((experts, c, c), dtype=torch.int64, device=DEV)
    got = ops.fused_head_multi_count(S, bias, *geo, c, 1, labels, expert_cm=expert_cm, **tables)
    for p in range(points):
        one = ops.fused_head_multi_count(S, bias, *geo, c, 1, labels, **{k: v[p:p + 1].contiguous() for k, v in tables.items()})
        assert torch.equal(got[p], one[0]), p
    assert torch.equal(expert_cm, _expert_oracle(ops, S, bias, geo, c, labels))      # counted once


def test_capacities(ops):
    assert ops.fused_head_multi_count_capacity(12, 4, 1) >= 8
    for mode in MODES:
        assert ops.fused_head_multi_count_capacity(32, 4, mode) >= 1
    assert ops.fused_head_multi_count_capacity(12, 3, 2) == 1
    for bad in ((1, 3, 0), (33, 3, 0), (12, 1, 0), (12, 5, 0), (12, 3, 3), (12, 3, -1)):
        assert ops.fused_head_multi_count_capacity(*bad) == 0


@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
def test_bounded_grids_and_accumulation(ops, mode):
    c, experts, geo = 5, 3, (2, 7, 9)
    S, bias, labels = _case(c, geo, 11, experts)
    tables = _tables(c, experts, 1 if mode == 2 else 3, mode, 2)
    want = ops.fused_head_multi_count(S, bias, *geo, c, mode, labels, **tables)
    for bound in (1, 3):
        assert torch.equal(ops.fused_head_multi_count(S, bias, *geo, c, mode, labels, max_workgroups=bound, **tables), want)
    again = ops.fused_head_multi_count(S, bias, *geo, c, mode, labels, cm=want.clone(), **tables)
    assert torch.equal(again, 2 * want)


@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
def test_groups(ops, mode):
    c, experts, geo = 12, 3, (5, 3, 5)
    n, hi, wi = geo
    ids = torch.tensor([2, 0, 2, 7, 1], dtype=torch.int32, device=DEV)        # 7 is out of range: counted nowhere
    S, bias, labels = _case(c, geo, 13, experts)
    points = 1 if mode == 2 else 3
    tables = _tables(c, experts, points, mode, 4)
    cm = torch.zeros((3, points, c, c), dtype=torch.int64, device=DEV)
    expert_cm = torch.zeros((3, experts, c, c), dtype=torch.int64, device=DEV)
    ops.fused_head_multi_count(S, bias, n, hi, wi, c, mode, labels, groups=ids, num_groups=3, cm=cm, expert_cm=expert_cm,
                               **tables)
    total, total_e = torch.zeros_like(cm[0]), torch.zeros_like(expert_cm[0])
    for g in range(3):
        imgs = [i for i, v in enumerate(ids.tolist()) if v == g]
        sub = [s[imgs].contiguous() for s in S]
        e_one = torch.zeros((experts, c, c), dtype=torch.int64, device=DEV)
        one = ops.fused_head_multi_count(sub, bias, len(imgs), hi, wi, c, mode, labels[imgs].contiguous(), expert_cm=e_one,
                                         **tables)
        assert torch.equal(cm[g], one) and torch.equal(expert_cm[g], e_one), g
        total += one
        total_e += e_one
    inrange = [i for i, v in enumerate(ids.tolist()) if 0 <= v < 3]
    sub = [s[inrange].contiguous() for s in S]
    ungrouped = ops.fused_head_multi_count(sub, bias, len(inrange), hi, wi, c, mode, labels[inrange].contiguous(), **tables)
    assert torch.equal(cm.sum(0), ungrouped) and torch.equal(total, ungrouped)
    assert int(cm.sum()) < points * int((labels >= 0).sum())                  # the fourth image is missing


def test_two_experts_equal_the_two_expert_heads(ops):
    from modular_semantic_segmentation_amd.bayes_mix import confusion_from_joint_hist, fused_decision_table
    c, geo = 12, (2, 7, 9)
    n, hi, wi = geo
    S, bias, labels = _case(c, geo, 17, 2)
    pair = (S[0], S[1], bias[0], bias[1], n, hi, wi, c)
    t = _tables(c, 2, 3, 1, 6)
    assert torch.equal(ops.fused_head_multi_count(S, bias, n, hi, wi, c, 1, labels, **t),
                       ops.fused_head_grid_score(*pair, t['tab'], t['lognorm'], t['logprior'], labels))
    assert torch.equal(ops.fused_head_multi_count(S, bias, n, hi, wi, c, 2, labels)[0],
                       ops.fused_head_average_count(*pair, labels))
    t = _tables(c, 2, 1, 0, 6)
    expert_cm = torch.zeros((2, c, c), dtype=torch.int64, device=DEV)
    got = ops.fused_head_multi_count(S, bias, n, hi, wi, c, 0, labels, expert_cm=expert_cm, **t)
    hist = ops.fused_head_joint_hist(*pair, labels).cpu().numpy()
    decision = fused_decision_table(t['tab'].cpu().numpy(), t['logprior'][0].cpu().numpy())
    assert (got[0].cpu().numpy() == confusion_from_joint_hist(hist, decision)).all()
    assert (expert_cm[0].cpu().numpy() == hist.sum(2)).all() and (expert_cm[1].cpu().numpy() == hist.sum(1)).all()


def test_refusals_leave_cm_untouched(ops):
    import ctypes
    from modular_semantic_segmentation_amd import _lib
    from modular_semantic_segmentation_amd.ops import _ptr, _ptr_array
    c, experts, geo = 12, 3, (1, 3, 5)
    n, hi, wi = geo
    S, bias, labels = _case(c, geo, 19, experts)
    t = _tables(c, experts, 1, 1, 8)
    cm = torch.full((1, c, c), SENTINEL, dtype=torch.int64, device=DEV)
    ids = torch.zeros(n, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(0)
    good = dict(S=_ptr_array(S), bias=_ptr_array(bias), num_experts=experts, n=n, hi=hi, wi=wi, num_classes=c, mode=1,
                num_points=1, tab=_ptr(t['tab']), lognorm=_ptr(t['lognorm']), logprior=_ptr(t['logprior']), labels=_ptr(labels),
                group=null, num_groups=1, cm=_ptr(cm), expert_cm=null, max_workgroups=0, stream=null)
    cap = ops.fused_head_multi_count_capacity(c, experts, 1)
    bad = [dict(num_experts=1), dict(num_experts=5), dict(num_classes=1), dict(num_classes=33), dict(mode=3), dict(mode=-1),
           dict(num_points=0), dict(num_points=cap + 1), dict(mode=2, num_points=2), dict(n=0), dict(hi=0), dict(wi=-1),
           dict(max_workgroups=-1), dict(num_groups=0), dict(num_groups=2), dict(group=_ptr(ids), num_groups=0),
           dict(tab=null), dict(lognorm=null), dict(logprior=null), dict(labels=null), dict(S=None), dict(bias=None),
           dict(tab=ctypes.c_void_p(t['tab'].data_ptr() + 2)), dict(labels=ctypes.c_void_p(labels.data_ptr() + 2)),
           dict(expert_cm=ctypes.c_void_p(cm.data_ptr() + 4)), dict(cm=ctypes.c_void_p(cm.data_ptr() + 4)),
           dict(group=ctypes.c_void_p(ids.data_ptr() + 2))]
    # an entry of the host pointer arrays: null, or not aligned to its loads (16 bytes for scores, 4 for biases)
    for e in range(experts):
        for name, tensors, offsets in (('S', S, (None, 4)), ('bias', bias, (None, 2))):
            for off in offsets:
                ptrs = [t.data_ptr() for t in tensors]
                ptrs[e] = 0 if off is None else ptrs[e] + off
                bad.append({name: (ctypes.c_void_p * experts)(*ptrs)})
    for change in bad:
        rc = _lib.lib().xv_fused_head_multi_count_fwd(*dict(good, **change).values())
        assert rc == -1, change
    torch.cuda.synchronize()
    assert bool((cm == SENTINEL).all())
    with pytest.raises(ValueError):
        ops.fused_head_multi_count(S, bias, n, hi, wi, c, 2, labels, tab=t['tab'])
    with pytest.raises(ValueError):
        ops.fused_head_multi_count(S, bias, n, hi, wi, c, 1, labels, num_groups=2, **t)
    with pytest.raises(TypeError):
        ops.fused_head_multi_count(S, bias, n, hi, wi, c, 1, labels.long(), **t)
    with pytest.raises(ValueError):
        ops.fused_head_multi_count(S, bias, n, hi, wi, c, 1, labels, cm=torch.zeros((2, c, c), dtype=torch.int64, device=DEV), **t)


@pytest.mark.parametrize('c', [21, 26])                 # CM 24 and 28: the class steps the issue's list leaves out
@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
@pytest.mark.parametrize('experts', [3, 4])
def test_wide_class_steps(ops, experts, mode, c):
    """four experts, Dirichlet: the forms that evaluate the taps a class quad at a time"""
    geo = (2, 7, 9)
    S, bias, labels = _case(c, geo, 3 * c, experts)
    points = 1 if mode == 2 else 3
    tables = _tables(c, experts, points, mode, c + experts)
    want = _oracle(ops, S, bias, geo, c, mode, tables, labels, points)
    assert all(int((want[p].sum(0) > 0).sum()) >= 2 for p in range(points))
    expert_cm = torch.zeros((experts, c, c), dtype=torch.int64, device=DEV)
    got = ops.fused_head_multi_count(S, bias, *geo, c, mode, labels, expert_cm=expert_cm, **tables)
    assert torch.equal(got, want)
    assert torch.equal(expert_cm, _expert_oracle(ops, S, bias, geo, c, labels))


@pytest.mark.parametrize('mode', [0, 1], ids=['bayes', 'dirichlet'])
def test_more_points_than_the_capacity_with_groups(ops, mode):
    """32 classes, four experts hold one point per launch: three points in groups go in three launches (Bayes on its shared
    log-likelihoods), each counted apart and added to its slice; the experts' matrices are counted once"""
    c, experts, geo = 32, 4, (5, 3, 5)
    n, hi, wi = geo
    assert ops.fused_head_multi_count_capacity(c, experts, mode) == 1
    ids = torch.tensor([2, 0, 2, 7, 1], dtype=torch.int32, device=DEV)
    S, bias, labels = _case(c, geo, 23, experts)
    tables = _tables(c, experts, 3, mode, 9)
    expert_cm = torch.zeros((3, experts, c, c), dtype=torch.int64, device=DEV)
    got = ops.fused_head_multi_count(S, bias, n, hi, wi, c, mode, labels, groups=ids, num_groups=3, expert_cm=expert_cm, **tables)
    assert tuple(got.shape) == (3, 3, c, c)
    for p in range(3):
        point = {k: (v if (mode == 0 and k == 'tab') else v[p:p + 1].contiguous()) for k, v in tables.items()}
        one = ops.fused_head_multi_count(S, bias, n, hi, wi, c, mode, labels, groups=ids, num_groups=3, **point)
        assert torch.equal(got[:, p], one[:, 0]), p
    assert not (torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 1], got[:, 2]))
    inrange = [i for i, v in enumerate(ids.tolist()) if 0 <= v < 3]
    sub = [s[inrange].contiguous() for s in S]
    assert torch.equal(expert_cm.sum(0), _expert_oracle(ops, sub, bias, (len(inrange), hi, wi), c, labels[inrange].contiguous()))
